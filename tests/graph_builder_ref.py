"""A vectorised NumPy restatement of the graph builder, for batches too large for ``batch([from_obs_dicts(...)])`` (0.23 ms per environment
on the host).  Written from the contract in uav_bs_ctrl_amd/graph.py (``from_obs_dicts`` + ``batch``) and include/uavgnn.h:

    offsets            cumulative counts of ``flag == 1`` over the agent rows a = b n + i
    kept rows          ``x[mask][:, 1:]``: row-major order, flag column dropped
    talk               edge i -> j of environment b iff ``d_u2u[b, i, j] <= r_comm`` (self loops included), in-edges grouped by destination
                       (ascending source inside a destination)
    reference edge id  position of (i, j) in the i-major list of the environment's edges, plus the edges of the environments before it

tests/test_graph_builder_ref.py pins it, array for array, to ``batch([from_obs_dicts(...)])``."""
import numpy as np

KEYS = ("x_a", "x_gt", "seen_off", "x_ubs", "near_off", "talk_off", "talk_src", "talk_eid", "graph_off")


def _offsets(count_per_row):
    off = np.zeros(count_per_row.size + 1, dtype=np.int64)
    np.cumsum(count_per_row.reshape(-1), out=off[1:])
    assert off[-1] < 2 ** 31
    return off.astype(np.int32)


def build(gt, ubs, agent, d_u2u=None, r_comm=np.inf):
    """gt [B, n, M, 5], ubs [B, n, U, 3] (column 0 = visibility flag), agent [B, n, 2], d_u2u [B, n, n] -> dict of the arrays of KEYS
    (the talk arrays only with d_u2u)."""
    gt, ubs, agent = (np.asarray(a, dtype=np.float32) for a in (gt, ubs, agent))
    B, n = gt.shape[:2]
    N = B * n
    mg, mu = gt[..., 0] == 1, ubs[..., 0] == 1
    out = dict(x_a=agent.reshape(N, -1), x_gt=gt[mg][:, 1:], seen_off=_offsets(mg.sum(-1)), x_ubs=ubs[mu][:, 1:], near_off=_offsets(mu.sum(-1)),
               graph_off=np.arange(0, N + 1, n, dtype=np.int32))
    if d_u2u is not None:
        adj = np.asarray(d_u2u) <= r_comm                                              # adj[b, i, j]: edge i -> j
        b, j, i = np.nonzero(adj.transpose(0, 2, 1))                                   # grouped by (b, destination j), ascending source i
        env_base = np.concatenate([[0], np.cumsum(adj.reshape(B, -1).sum(1))])[:-1]     # edges of the environments before b
        eid_of = np.cumsum(adj.reshape(B, -1), 1).reshape(B, n, n) - 1 + env_base[:, None, None]
        out.update(talk_off=_offsets(adj.sum(1)), talk_src=(b * n + i).astype(np.int32), talk_eid=eid_of[b, i, j].astype(np.int32))
    return out


def transpose(talk_off, talk_src):
    """(t_off, t_dst, t_pos) of a CSC: the out-edges of every source in CSC position order - ``HeteroBatch.talk_transpose`` on the host."""
    N = talk_off.size - 1
    dst = np.repeat(np.arange(N), np.diff(talk_off.astype(np.int64)))
    order = np.argsort(talk_src, kind="stable")
    return _offsets(np.bincount(talk_src, minlength=N)), dst[order].astype(np.int32), order.astype(np.int32)


def random_obs(rng, B, n, M, p_seen=0.3, p_near=0.5, r_comm=1.0, exact=0):
    """Random padded observations: (gt, ubs, agent, d_u2u) as float32.  Flags are 0 / 1; the first agent sees nothing and the last one
    everything; distances are symmetric with a zero diagonal, and in about a quarter of the environments ``exact`` off-diagonal pairs are set to
    exactly float32(r_comm) (the edge is kept: the rule is <=)."""
    U = max(n - 1, 0)
    gt = rng.uniform(-1, 1, (B, n, M, 5)).astype(np.float32)
    gt[..., 0] = rng.uniform(size=(B, n, M)) < p_seen
    gt[0, 0, :, 0] = 0
    gt[-1, -1, :, 0] = 1
    ubs = rng.uniform(-1, 1, (B, n, U, 3)).astype(np.float32)
    ubs[..., 0] = rng.uniform(size=(B, n, U)) < p_near
    agent = rng.uniform(0, 1, (B, n, 2)).astype(np.float32)
    d = rng.uniform(0, 2 * r_comm, (B, n, n)).astype(np.float32)
    d = (d + d.transpose(0, 2, 1)) / np.float32(2)
    if exact and n > 1:
        for _ in range(exact):
            b = np.flatnonzero(rng.uniform(size=B) < 0.25) if B > 1 else np.arange(1)
            i = rng.integers(0, n, b.size)
            j = (i + rng.integers(1, n, b.size)) % n
            d[b, i, j] = np.float32(r_comm)
            d[b, j, i] = np.float32(r_comm)
    d[:, np.arange(n), np.arange(n)] = 0
    return gt, ubs, agent, d

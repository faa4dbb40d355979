"""The vectorised NumPy restatement of the graph builder (tests/graph_builder_ref.py: the reference of the large device-builder cases in
tests/test_grid_caps_gpu.py) equals ``batch([from_obs_dicts(...)])`` array for array.  Index and byte work: every comparison is exact."""
import numpy as np
import pytest
import torch as th

from tests import graph_builder_ref as G
from uav_bs_ctrl_amd import batch, from_obs_dicts


def _host(gt, ubs, agent, d, r_comm):
    B, n = gt.shape[:2]
    g = batch([from_obs_dicts([dict(agent=agent[b, i], ubs=ubs[b, i], gt=gt[b, i]) for i in range(n)], d[b], r_comm) for b in range(B)])
    out = dict(x_a=g.agent_feat(), graph_off=g.graph_off, talk_eid=g.talk_eid())
    out["x_gt"], out["seen_off"] = g.relation_segments("seen")
    out["x_ubs"], out["near_off"] = g.relation_segments("near")
    out["talk_off"], out["talk_src"] = g.talk_csc()
    return g, {k: v.numpy() for k, v in out.items()}


def _same(got, want, what):
    assert set(got) == set(want) == set(G.KEYS)
    for k in G.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} {got[k].dtype}{got[k].shape} vs {want[k].dtype}{want[k].shape}"
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs"


# (B, n, M, r_comm, distances set exactly to r_comm per environment): 371 environments in all
CASES = [(120, 8, 20, 1.0, 2), (150, 2, 5, 0.4, 1), (60, 1, 7, 1.0, 0), (40, 5, 70, np.inf, 0), (1, 3, 4, 0.75, 1)]


@pytest.mark.parametrize("B,n,M,r_comm,exact", CASES)
def test_restatement_equals_batch_of_from_obs_dicts(B, n, M, r_comm, exact):
    rng = np.random.default_rng(1000 * B + n)
    gt, ubs, agent, d = G.random_obs(rng, B, n, M, r_comm=1.0 if np.isinf(r_comm) else r_comm, exact=exact)
    if B > 2 and n > 1:
        d[1] = 0.0                                    # a complete environment ...
        d[2] = np.float32(r_comm if np.isfinite(r_comm) else 1.0) * 3
        d[2][np.arange(n), np.arange(n)] = 0          # ... and one with self loops only
    # what the cases are for is really in them
    assert not gt[0, 0, :, 0].any() and gt[-1, -1, :, 0].all(), "an agent that sees nothing, one that sees everything"
    if exact:
        off_diag = ~np.eye(n, dtype=bool)
        assert (d[:, off_diag] == np.float32(r_comm)).any(), "no distance equal to r_comm"
    g, want = _host(gt, ubs, agent, d, r_comm)
    got = G.build(gt, ubs, agent, d, r_comm)
    _same(got, want, f"B={B} n={n} M={M} r={r_comm}")
    if exact:                                         # the tie is an edge: (i, j) with d == r_comm is among the sources of j
        b, i, j = (a[0] for a in np.nonzero((d == np.float32(r_comm)) & ~np.eye(n, dtype=bool)[None]))
        lo, hi = got["talk_off"][b * n + j], got["talk_off"][b * n + j + 1]
        assert b * n + i in got["talk_src"][lo:hi]
    t_off, t_dst, t_pos = (t.numpy() for t in g.talk_transpose())
    r_off, r_dst, r_pos = G.transpose(got["talk_off"], got["talk_src"])
    assert np.array_equal(r_off, t_off) and np.array_equal(r_dst, t_dst) and np.array_equal(r_pos, t_pos)
    assert r_off.dtype == r_dst.dtype == r_pos.dtype == np.int32


def test_restatement_without_the_talk_relation():
    gt, ubs, agent, _ = G.random_obs(np.random.default_rng(5), 3, 4, 6)
    out = G.build(gt, ubs, agent)
    assert "talk_off" not in out and out["seen_off"][-1] == int((gt[..., 0] == 1).sum()) and th.equal(
        th.as_tensor(out["x_gt"]), th.as_tensor(gt[gt[..., 0] == 1][:, 1:]))

"""NumPy restatement of the three rules of the prioritised replay (include/uavgnn.h, uavgnn_replay_prio_commit / _prio_sample /
_prio_update), written from the header text - not from csrc/replay_prio.hip: Python integers for every sum and product that decides a
slot, ``np.searchsorted`` on the exclusive prefix sums for the slot, float64 for the weights and the priorities."""
import numpy as np

from tests.map_sampler_ref import philox4x32_10

PRIO_ONE = 1 << 20
PRIO_TOP = (1 << 32) - 1
_M64 = (1 << 64) - 1


def strata(S, B):
    """[(lo_k, hi_k)] for k < B: lo_k = k qB + (k rB) // B with S = qB B + rB, hi_k = lo_{k+1}."""
    qB, rB = divmod(int(S), int(B))
    lo = [k * qB + (k * rB) // B for k in range(B + 1)]
    assert lo[B] == S
    return list(zip(lo[:-1], lo[1:]))


def words(seed, draws, B):
    """r_k for k < B: words 0 (low) and 1 (high) of Philox4x32-10 at counter (k, 1, draws_lo, draws_hi) under key seed, as Python ints."""
    seed, draws = int(seed) & _M64, int(draws) & _M64
    w = philox4x32_10(np.arange(B), 1, draws & 0xFFFFFFFF, draws >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return [(int(hi) << 32) | int(lo) for lo, hi in zip(w[0], w[1])]


def targets(seed, draws, S, B):
    return [lo + (r % (hi - lo) if hi > lo else 0) for (lo, hi), r in zip(strata(S, B), words(seed, draws, B))]


def sample(seed, draws, prio, size, B, beta):
    """(idx [B] int64, weights [B] float32, weights in float64, status bit) of one draw on ``prio[:size]`` (whatever lies beyond is not read)."""
    size = int(size)
    p = np.asarray(prio)[:size].astype(np.uint64)
    inc = np.cumsum(p, dtype=np.uint64)                 # exact: size <= 2^30 words below 2^32 stay below 2^62
    S = int(inc[-1]) if size else 0
    if size == 0 or S == 0:
        return np.zeros(B, dtype=np.int64), np.ones(B, dtype=np.float32), np.ones(B), 1
    tg = targets(seed, draws, S, B)
    idx = np.array([int(np.searchsorted(inc, np.uint64(t), side="right")) for t in tg], dtype=np.int64)
    for k, t in zip(idx, tg):                           # the defining inequality, on Python integers
        assert int(inc[k]) - int(p[k]) <= t < int(inc[k])
    w = np.power(np.float64(size) * p[idx].astype(np.float64) / np.float64(S), -np.float64(beta))
    w64 = w / w.max()
    return idx, w64.astype(np.float32), w64, 0


def priority(td, alpha, eta, eps):
    """q [B] (Python-int valued uint64 array) and ``finite`` [B] for td [T, B, C] float32: a = eta max|td| + (1 - eta) mean|td| in double,
    q = clamp(rint(pow(a + eps, alpha) 2^20), 1, 2^32 - 1); alpha == 1: a + eps itself."""
    a_td = np.abs(np.asarray(td, dtype=np.float32).astype(np.float64))
    T, B, C = a_td.shape
    rows = a_td.transpose(1, 0, 2).reshape(B, T * C)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.float64(eta) * rows.max(1) + (1.0 - np.float64(eta)) * (rows.sum(1) / np.float64(T * C))
        finite = np.isfinite(a)
        x = np.where(finite, a, 0.0) + np.float64(eps)
        v = (x if alpha == 1 else np.power(x, np.float64(alpha))) * 1048576.0
    q = np.where(v >= 1.0, np.where(v >= float(PRIO_TOP), float(PRIO_TOP), np.rint(np.minimum(v, float(PRIO_TOP)))), 1.0)
    return q.astype(np.uint64), finite


def update(td, idx, capacity, alpha, eta, eps, prio, prio_max):
    """(prio', prio_max', status bit) after uavgnn_replay_prio_update; ``within`` one unit of q is the caller's tolerance."""
    q, finite = priority(td, alpha, eta, eps)
    out, top, skipped = np.array(prio, dtype=np.uint64), int(prio_max), 0
    B = len(idx)
    for b in range(B):
        s = int(idx[b])
        if not finite[b] or s < 0 or s >= capacity:
            skipped = 2
            continue
        top = max(top, int(q[b]))
        if b + 1 == B or int(idx[b + 1]) != s:
            out[s] = q[b]
    return out, top, skipped


def commit(prio, head, E, capacity, prio_max):
    out = np.array(prio, dtype=np.uint64)
    for e in range(E):
        out[(int(head) + e) % capacity] = int(prio_max)
    return out


def slots96():
    """The 96-slot case the host and the GPU tests share: |N(0,1)| x {8 with probability 0.1, else 0.3} under default_rng(0) as TD errors,
    alpha = 0.9, eps = 1e-3 -> 96 fixed-point priorities."""
    rng = np.random.default_rng(0)
    a = np.abs(rng.standard_normal(96)) * np.where(rng.random(96) < 0.1, 8.0, 0.3)
    q, finite = priority(a.astype(np.float32).reshape(1, 96, 1), 0.9, 0.5, 1e-3)
    assert finite.all()
    return q

"""NumPy restatement of uavgnn_eps_greedy_philox and uavgnn_stats_push, written from their contract in include/uavgnn.h - not from
csrc/eval_stats.hip.

Selection: w(index, lane) = first Philox4x32-10 word at counter (index, lane, step_lo, step_hi) under the key (seed_lo, seed_hi);
u = (w >> 8) * 2^-24 (exact in float32); team t explores when u(t, 0) <= eps (a float32 comparison); an exploring row a takes
min((int)(u(a, 1) * A), A - 1) with the product rounded to float32; every other row its first maximum.

Statistics: an accumulator row is {count, mean, M2, min, max, non-finite count}, empty {0, 0, 0, +inf, -inf, 0}; a push of n values
merges their finite part (mean_b, M2_b about mean_b, in float64) by the pairwise rule.  The header fixes no summation order inside a
push, so this restatement agrees with the kernel to the bound of ``moment_tolerances``, not bit for bit; counts, min and max are exact."""
import numpy as np

from tests.map_sampler_ref import philox4x32_10

_M64 = 2 ** 64 - 1
EMPTY = np.array([0.0, 0.0, 0.0, np.inf, -np.inf, 0.0])


def uniforms(seed, step, index, lane):
    """float32 u(index, lane) at {seed, step}; index and step: integers or integer arrays that broadcast against each other."""
    seed, step = int(seed) & _M64, np.asarray(step).astype(np.uint64)
    w = philox4x32_10(np.asarray(index).astype(np.uint64), np.uint64(lane), step & np.uint64(0xFFFFFFFF), step >> np.uint64(32),
                      seed & 0xFFFFFFFF, seed >> 32)[0]
    return ((w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def draws(seed, step, N, n_agents):
    """(u_team float32 [ceil(N / n_agents)], u_agent float32 [N]): what a caller of uavgnn_eps_greedy would pass to get the same actions."""
    teams = (N + n_agents - 1) // n_agents
    return uniforms(seed, step, np.arange(teams), 0), uniforms(seed, step, np.arange(N), 1)


def eps_greedy_philox(q, A, n_agents, seed, step, eps):
    """int64 [N]: the actions the kernel writes for q [N, >= A] (float32; columns beyond A are padding) at {seed, step}."""
    q = np.asarray(q, dtype=np.float32)[:, :A]
    N = q.shape[0]
    u_team, u_agent = draws(seed, step, N, n_agents)
    greedy = np.argmax(q, axis=1).astype(np.int64) if N else np.zeros(0, dtype=np.int64)       # np.argmax: the first maximum
    explore = (u_team <= np.float32(eps))[np.arange(N) // n_agents]
    r = np.minimum((u_agent * np.float32(A)).astype(np.float32).astype(np.int64), A - 1)
    return np.where(explore, r, greedy).astype(np.int64)


def stats_empty(n_keys):
    return np.tile(EMPTY, (n_keys, 1))


def stats_push(acc, vals):
    """acc [K, 6] float64 after pushing vals [K, n] (in place, returned)."""
    vals = np.asarray(vals, dtype=np.float64).reshape(acc.shape[0], -1)
    for a, row in zip(acc, vals):
        ok = np.isfinite(row)
        v, nb = row[ok], float(ok.sum())
        a[5] += float((~ok).sum())
        if nb == 0:
            continue
        mean_b = v.sum() / nb
        m2_b = ((v - mean_b) ** 2).sum()
        count, mean = a[0], a[1]
        d, n2 = mean_b - mean, count + nb
        a[0] = n2
        a[1] = mean + d * nb / n2
        a[2] = a[2] + (m2_b + d * d * count * nb / n2)
        a[3], a[4] = min(a[3], v.min()), max(a[4], v.max())
    return acc


def two_pass(values):
    """(mean, M2) of the finite values in np.longdouble: the yardstick of the merge."""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[np.isfinite(v)].astype(np.longdouble)
    mean = v.sum() / v.size
    return mean, ((v - mean) ** 2).sum()


def moment_tolerances(values):
    """(tol_mean, tol_m2) = 4 n 2^-53 of the data's scale.  Mean: a sum of n terms in ANY order is off by at most (n - 1) u sum|v|
    (u = 2^-53), so the mean by at most n u max|v|; the merges add a few u each.  M2: a sum of n non-negative squares, each carrying a few
    u relative, in any order: at most ~ n u M2 relative to M2 itself.  The factor 4 covers the constants; the scales are max|v| and M2."""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    n = v.size
    _, m2 = two_pass(v)
    return 4.0 * n * 2.0 ** -53 * float(np.abs(v).max()), 4.0 * n * 2.0 ** -53 * float(m2)


def logger_mean_std(values):
    """utils/mpi_tools.py:87-92 on one process: float32 sums, population std."""
    x = np.asarray(values, dtype=np.float32)
    mean = np.sum(x) / len(x)
    return mean, np.sqrt(np.sum((x - mean) ** 2) / len(x))

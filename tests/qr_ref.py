"""NumPy float64 restatement of include/uavgnn_qr.h (the quantile-regression head's mean fold, the select on quantile rows and the
pairwise quantile-Huber loss with n-step targets), written from the header alone: explicit loops over rows, nothing vectorised over the
pair index that the header does not write as a sum.  The tests hold the torch arms (float64, 1e-12) and the kernels (fp32, the project's
parity rule) to it."""
import numpy as np


def taus(K):
    return (2.0 * np.arange(K) + 1.0) / (2.0 * K)


def mean_fold(W, b, A, K):
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    H = W.shape[1]
    W_bar, b_bar = np.zeros((A, H)), np.zeros(A)
    for a in range(A):
        for k in range(K):
            W_bar[a] += W[a * K + k]
            b_bar[a] += b[a * K + k]
    return W_bar / K, b_bar / K


def _argmax_first(v):
    """First maximum; a NaN counts as the maximum (the first one wins)."""
    best = 0
    for j in range(1, len(v)):
        if v[j] > v[best] or (np.isnan(v[j]) and not np.isnan(v[best])):
            best = j
    return best


def select(theta_pol, theta_tgt, acts, double_q):
    """-> theta_a [T, N, K], theta_next [T, N, K], next_acts [T, N], q_pol [T+1, N, A]."""
    theta_pol, theta_tgt = np.asarray(theta_pol, np.float64), np.asarray(theta_tgt, np.float64)
    T, N, A, K = theta_tgt.shape
    acts = np.asarray(acts).reshape(T, N)
    theta_a, theta_next = np.full((T, N, K), np.nan), np.full((T, N, K), np.nan)
    next_acts = np.zeros((T, N), np.int64)
    q_pol = theta_pol.sum(-1) / K
    for t in range(T):
        for n in range(N):
            a = int(acts[t, n])
            if 0 <= a < A:
                theta_a[t, n] = theta_pol[t, n, a]
            pick = theta_pol[t + 1, n] if double_q else theta_tgt[t, n]
            best = _argmax_first(pick.sum(-1))
            next_acts[t, n] = best
            theta_next[t, n] = theta_tgt[t, n, best]
    return theta_a, theta_next, next_acts, q_pol


def select_bwd(d_theta_a, acts, A):
    d_theta_a = np.asarray(d_theta_a, np.float64)
    T, N, K = d_theta_a.shape
    acts = np.asarray(acts).reshape(T, N)
    out = np.zeros((T + 1, N, A, K))
    for t in range(T):
        for n in range(N):
            if 0 <= acts[t, n] < A:
                out[t, n, int(acts[t, n])] = d_theta_a[t, n]
    return out


def targets(theta_next, rews, dones, gamma, n_step):
    """y [T, B, C, K]: y_j = sum_{k<m} (prod_{l<k} c_{t+l}) r_{t+k} + (prod_{l<m} c_{t+l}) theta_next[t+m-1, j], m = min(n_step, T - t)."""
    theta_next = np.asarray(theta_next, np.float64)
    T, B, C, K = theta_next.shape
    rews = np.broadcast_to(np.asarray(rews, np.float64).reshape(T, B, -1), (T, B, C))
    c = gamma * (1.0 - np.asarray(dones, np.float64).reshape(T, B))
    y = np.zeros((T, B, C, K))
    for t in range(T):
        m = min(int(n_step), T - t)
        for b in range(B):
            for ch in range(C):
                acc, prod = 0.0, 1.0
                for k in range(m):
                    acc += prod * rews[t + k, b, ch]
                    prod *= c[t + k, b]
                y[t, b, ch] = acc + prod * theta_next[t + m - 1, b, ch]
    return y


def huber(u, kappa):
    au = np.abs(u)
    return np.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa))


def loss(theta_a, theta_next, rews, dones, weights, gamma, n_step, kappa):
    """-> loss (a float), g [T, B, C, K], td [T, B, C], row losses l [T, B, C], y [T, B, C, K]."""
    theta_a = np.asarray(theta_a, np.float64)
    T, B, C, K = theta_a.shape
    y = targets(theta_next, rews, dones, gamma, n_step)
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64).reshape(B)
    tau = taus(K)
    l, g, td = np.zeros((T, B, C)), np.zeros((T, B, C, K)), np.zeros((T, B, C))
    count = T * B * C
    for t in range(T):
        for b in range(B):
            for ch in range(C):
                th = theta_a[t, b, ch]
                for i in range(K):
                    u = y[t, b, ch] - th[i]                                # u_ij over j
                    wt = np.abs(tau[i] - (u < 0))
                    l[t, b, ch] += (wt * huber(u, kappa)).sum() / kappa / K
                    g[t, b, ch, i] = -(w[b] / count) * (wt * np.clip(u, -kappa, kappa)).sum() / kappa / K
                td[t, b, ch] = th.mean() - y[t, b, ch].mean()
    total = (w.reshape(1, B, 1) * l).sum() / count
    return total, g, td, l, y

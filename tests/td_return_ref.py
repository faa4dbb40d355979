"""NumPy float64 restatement of the TD tail with multi-step targets, written from the definitions of DESIGN ("Multi-step TD targets"),
not from the kernel: the select, both targets, the weighted loss and d_agent_out.

A sequence has T transitions.  q [T, B, C] is the chosen-action value, V [T, B, C] the bootstrap value of the state after transition t,
c_t = gamma (1 - done_t) with done [T, B, 1], r [T, B, C] or [T, B, 1] (broadcast).
  n-step:  y_t = sum_{k<m} (prod_{j<k} c_{t+j}) r_{t+k} + (prod_{j<m} c_{t+j}) V_{t+m-1},  m = min(n, T - t)
  lambda:  G_{T-1} = r_{T-1} + c_{T-1} V_{T-1},  G_t = r_t + c_t ((1 - lam) V_t + lam G_{t+1}),  y_t = G_t
  loss  =  sum w_b (q - y)^2 / (T B C)
"""
import numpy as np


def select(agent_out, target_out, acts, double_q):
    """agent_out [T+1, N, A], target_out [T, N, A], acts [T, N] -> (qvals, next_vals, next_acts), each [T, N].  np.argmax takes the
    first maximum."""
    agent_out, target_out = np.asarray(agent_out, np.float64), np.asarray(target_out, np.float64)
    acts = np.asarray(acts).reshape(target_out.shape[:2])
    qvals = np.take_along_axis(agent_out[:-1], acts[..., None], 2)[..., 0]
    next_acts = np.argmax(agent_out[1:] if double_q else target_out, axis=2)
    next_vals = np.take_along_axis(target_out, next_acts[..., None], 2)[..., 0]
    return qvals, next_vals, next_acts


def one_step(V, r, done, gamma):
    V = np.asarray(V, np.float64)
    return np.broadcast_to(np.asarray(r, np.float64), V.shape) + gamma * (1.0 - np.asarray(done, np.float64)) * V


def nstep(V, r, done, gamma, n):
    V = np.asarray(V, np.float64)
    T = V.shape[0]
    r = np.broadcast_to(np.asarray(r, np.float64), V.shape)
    c = np.broadcast_to(gamma * (1.0 - np.asarray(done, np.float64)), V.shape)
    y = np.zeros_like(V)
    for t in range(T):
        m = min(n, T - t)
        disc = np.ones_like(V[0])
        for k in range(m):
            y[t] += disc * r[t + k]
            disc = disc * c[t + k]
        y[t] += disc * V[t + m - 1]
    return y


def lam_return(V, r, done, gamma, lam):
    V = np.asarray(V, np.float64)
    T = V.shape[0]
    r = np.broadcast_to(np.asarray(r, np.float64), V.shape)
    c = np.broadcast_to(gamma * (1.0 - np.asarray(done, np.float64)), V.shape)
    G = np.zeros_like(V)
    G[T - 1] = r[T - 1] + c[T - 1] * V[T - 1]
    for t in range(T - 2, -1, -1):
        G[t] = r[t] + c[t] * ((1.0 - lam) * V[t] + lam * G[t + 1])
    return G


def targets(V, r, done, gamma, returns):
    kind, p = returns
    return nstep(V, r, done, gamma, int(p)) if kind == "nstep" else lam_return(V, r, done, gamma, float(p))


def loss_and_td(q, y, weights=None):
    """(loss, td [T, B, C], g = d loss / d q [T, B, C])."""
    td = np.asarray(q, np.float64) - y
    w = np.ones(td.shape[1]) if weights is None else np.asarray(weights, np.float64)
    wb = w.reshape(1, -1, 1)
    return float((wb * td * td).sum() / td.size), td, 2.0 * wb * td / td.size


def d_agent_out(g_flat, acts, A):
    """d loss / d agent_out [T+1, N, A] from g [T, N] (no mixer: q is the gathered value): g at the chosen action, zero elsewhere and in
    row T."""
    T, N = g_flat.shape
    out = np.zeros((T + 1, N, A))
    np.put_along_axis(out[:-1], np.asarray(acts).reshape(T, N, 1), g_flat[..., None], 2)
    return out

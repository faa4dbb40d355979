"""NumPy restatement of the noisy-net Q head, written from include/uavgnn_ext.h: the noise stream (Philox4x32-10 of
tests/map_sampler_ref.py, float64 Box-Muller), f, the shared fold and its transpose.  Nothing here imports the package."""
import numpy as np

from tests.map_sampler_ref import philox4x32_10

OUT_BLOCK0 = 0x10000


def _pair(seed, step):
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return step & 0xFFFFFFFF, step >> 32, seed & 0xFFFFFFFF, seed >> 32


def uniforms(seed, step, rows, blocks):
    """u [len(rows), len(blocks), 4] float64 of block(row, b): ((w >> 9) + 0.5) 2^-23 - exact in float32 as well."""
    s_lo, s_hi, k0, k1 = _pair(seed, step)
    rows, blocks = np.asarray(rows, dtype=np.uint64)[:, None], np.asarray(blocks, dtype=np.uint64)[None, :]
    w = philox4x32_10(rows, blocks, np.uint64(s_lo), np.uint64(s_hi), k0, k1)
    return np.stack([((x >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23 for x in w], -1)


def box_muller(u, dtype=np.float64):
    """z [..., 4] from u [..., 4]: (z0, z1) = r (cos, sin)(2 pi u1), r = sqrt(-2 ln u0); (z2, z3) likewise from (u2, u3)."""
    u = u.astype(dtype)
    two, tau = dtype(2.0), dtype(2.0 * np.pi)
    r0, r1 = np.sqrt(-two * np.log(u[..., 0])), np.sqrt(-two * np.log(u[..., 2]))
    a0, a1 = tau * u[..., 1], tau * u[..., 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], -1).astype(dtype)


def xi(seed, step, rows, n_cols, block0=0):
    """xi [len(rows), n_cols] float64: column 4 b + k is z_k of block(row, block0 + b)."""
    nb = (n_cols + 3) // 4
    z = box_muller(uniforms(seed, step, rows, block0 + np.arange(nb)))
    return z.reshape(len(rows), 4 * nb)[:, :n_cols]


def xi_in(seed, step, rows, H):
    return xi(seed, step, rows, H, 0)


def xi_out(seed, step, rows, A):
    return xi(seed, step, rows, A, OUT_BLOCK0)


def f(z):
    return np.sign(z) * np.sqrt(np.abs(z))


def fold(W_mu, W_sigma, b_mu, b_sigma, f_in, f_out):
    """(W_eff, b_eff) in the header's order of operations, in the dtype of the inputs."""
    return W_mu + W_sigma * (f_out[:, None] * f_in[None, :]), b_mu + b_sigma * f_out


def fold_transpose(dW_eff, db_eff, f_in, f_out):
    """(d W_mu, d W_sigma, d b_mu, d b_sigma)."""
    return dW_eff, dW_eff * (f_out[:, None] * f_in[None, :]), db_eff, db_eff * f_out


def head_rows(h, W_mu, W_sigma, b_mu, b_sigma, f_in, f_out):
    """q [N, A] of mode "rows" and the scale S of its rounding bound, in float64, from per-row f_in [N, H], f_out [N, A]."""
    h, W_mu, W_sigma, b_mu, b_sigma, f_in, f_out = (np.asarray(t, dtype=np.float64) for t in (h, W_mu, W_sigma, b_mu, b_sigma, f_in, f_out))
    hf = h * f_in
    q = (h @ W_mu.T + b_mu) + f_out * (hf @ W_sigma.T + b_sigma)
    S = np.abs(h) @ np.abs(W_mu).T + np.abs(b_mu) + np.abs(f_out) * (np.abs(hf) @ np.abs(W_sigma).T + np.abs(b_sigma))
    return q, S

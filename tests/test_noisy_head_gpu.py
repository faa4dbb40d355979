"""The kernels of csrc/ext/noisy_head.hip on the GPU against the NumPy restatement (tests/noisy_ref.py) and float64.

Bounds.  Noise: rtol = atol = 2e-5 on g = f |f| against the float64 xi - the tolerance test_disc_comm_in_kernel_gumbel_noise holds the
Gumbel stream to; float32 Box-Muller of the same uniforms stays within 5e-6 (tests/test_noisy_head_host.py).  Head: |q - q64| <= 6e-7 S
with S = |h||mu|^T + |b_mu| + |f_out| (|h (.) f_in||sigma|^T + |b_sigma|): 4e-7 is test_head_kernel_vs_float64's bound for one K = H
accumulation, and the kernel adds three single fp32 roundings (h f_in, the multiply by f_out, the final add): 3 * 2^-24 = 1.8e-7.
The float64 value is formed from the DUMPED f values (uavgnn_noisy_noise), which part (a) ties to the stream."""
import numpy as np
import pytest
import torch as th

from tests import noisy_ref as R

pytestmark = pytest.mark.gpu

SEED = 2 ** 41 + 977
HEAD_BOUND = 6e-7
GRID_CAP, TILES_PER_BLOCK, TILE_ROWS = 4096, 4, 16       # uavgnn_noisy_head_fwd's launch (csrc/ext/noisy_head.hip)


def _ext():
    from uav_bs_ctrl_amd import _lib as L
    return L, L.ext()


def _pair(seed=SEED, step=0):
    return th.tensor([seed, step], dtype=th.int64, device="cuda")


def _noise(rng, N, H, A):
    from uav_bs_ctrl_amd import ops
    return ops.noisy_noise(rng, N, H, A)


# ---- (a) the stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("A", [1, 9, 16])
def test_noise_dump_is_the_restated_stream(H, A):
    N, step = 5000, 2 ** 32 + 5            # both words of the step are in the counter
    rng = _pair(SEED, step)
    f_in, f_out = _noise(rng, N, H, A)
    th.cuda.synchronize()
    rows = np.r_[np.arange(40), N - 1]
    for name, f, want in (("xi_in", f_in, R.xi_in(SEED, step, rows, H)), ("xi_out", f_out, R.xi_out(SEED, step, rows, A))):
        g = (f * f.abs())[rows].double().cpu().numpy()
        err = np.abs(g - want) - 2e-5 * np.abs(want)
        print(f"{name} H={H} A={A}: max |g - xi| = {np.abs(g - want).max():.3g}")
        assert (err <= 2e-5).all(), (name, float(err.max()))
        assert np.array_equal(np.sign(f[rows].cpu().numpy()), np.sign(want)), name
    # moments over everything drawn (n = 5000 (H + A) >= 325 000: sd of the variance estimate <= 0.0025, the Gumbel test's bounds hold)
    g = th.cat(((f_in * f_in.abs()).flatten(), (f_out * f_out.abs()).flatten())).double()
    n = g.numel()
    mean, var = float(g.mean()), float(g.var())
    print(f"H={H} A={A}: n = {n}, mean {mean:.3g} (bound {5 / np.sqrt(n):.3g}), var {var:.5f}")
    assert abs(mean) < 5 / np.sqrt(n) and abs(var - 1) < 0.02
    again = _noise(rng, N, H, A)
    assert th.equal(again[0], f_in) and th.equal(again[1], f_out), "the same pair gives the same bits"
    for other in (_pair(SEED, step + 1), _pair(SEED + 1, step)):
        o_in, o_out = _noise(other, N, H, A)
        assert float((o_in == f_in).float().mean()) < 1e-3 and float((o_out == f_out).float().mean()) < 1e-2
    L, E = _ext()
    only_out = th.full((N, A), 7.0, device="cuda")
    L.check(E.uavgnn_noisy_noise(rng.data_ptr(), N, H, A, None, only_out.data_ptr(), L.stream()), "f_out alone")
    assert th.equal(only_out, f_out), "a NULL output is skipped, the other one is the same"


# ---- (b), (c) the per-row head -------------------------------------------------------------------------------------------------------
def _head_case(N, H, A, gen, pad=True, sigma_scale=0.3):
    """Operands with padded row strides (h: H + 4, both weights: H + 8, q: A + 3)."""
    ph, pw = (4, 8) if pad else (0, 0)
    h = th.randn(N, H + ph, generator=gen).cuda()[:, :H]
    W_mu = (0.2 * th.randn(A, H + pw, generator=gen)).cuda()[:, :H]
    W_sigma = (sigma_scale * th.rand(A, H + pw, generator=gen)).cuda()[:, :H]
    b_mu, b_sigma = th.randn(A, generator=gen).cuda(), (sigma_scale * th.rand(A, generator=gen)).cuda()
    return h, W_mu, W_sigma, b_mu, b_sigma


def _launch(h, W_mu, W_sigma, b_mu, b_sigma, rng, q, N=None):
    L, E = _ext()
    N = h.shape[0] if N is None else N
    A, H = W_mu.shape
    L.check(E.uavgnn_noisy_head_fwd(h.data_ptr(), h.stride(0), N, H, W_mu.data_ptr(), W_sigma.data_ptr(), W_mu.stride(0), b_mu.data_ptr(),
                                    b_sigma.data_ptr(), A, rng.data_ptr(), q.data_ptr(), q.stride(0), L.stream()), "uavgnn_noisy_head_fwd")


def _rel_err(q, rows, h, W_mu, W_sigma, b_mu, b_sigma, f_in, f_out):
    c = lambda t: t.double().cpu().numpy()          # noqa: E731
    want, S = R.head_rows(c(h[rows]), c(W_mu), c(W_sigma), c(b_mu), c(b_sigma), c(f_in[rows]), c(f_out[rows]))
    return float((np.abs(c(q[rows]) - want) / S).max())


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("A", [1, 9, 16])
def test_noisy_head_kernel_vs_float64(H, A):
    L, E = _ext()
    assert E.uavgnn_noisy_head_supported(H, A) == 1
    for N in (1, 15, 16, 17, 1000):
        gen = th.Generator().manual_seed(1000 * N + H + A)
        ops_ = _head_case(N, H, A, gen)
        rng = _pair(SEED + N, 7)
        q = th.full((N + 2, A + 3), 7.0, device="cuda")
        _launch(*ops_, rng, q, N)
        f_in, f_out = _noise(rng, N, H, A)
        th.cuda.synchronize()
        err = _rel_err(q[:N, :A], slice(None), *ops_, f_in, f_out)
        print(f"N={N} H={H} A={A}: max |q - q64| / S = {err:.3g}")
        assert err <= HEAD_BOUND, (N, err)
        # (c) neighbours, reproducibility
        assert bool((q[:N, A:] == 7.0).all()) and bool((q[N:] == 7.0).all()), "columns past A or rows past N were written"
        q2 = th.empty(N, A, device="cuda")
        _launch(*ops_, rng, q2)
        assert th.equal(q2, q[:N, :A]), "a second launch at the same pair is not bit-identical"
        q3 = th.empty(N, A, device="cuda")
        _launch(*ops_, _pair(SEED + N, 8), q3)
        assert not th.equal(q3, q2), "the next step draws other noise"


@pytest.mark.parametrize("N,H,A", [(17, 64, 1), (1000, 128, 9), (33, 256, 16)])
def test_zero_sigmas_give_the_plain_head_bit_for_bit(N, H, A):
    L, E = _ext()
    h, W_mu, W_sigma, b_mu, b_sigma = _head_case(N, H, A, th.Generator().manual_seed(N))
    W_sigma.zero_()
    b_sigma.zero_()
    q, plain = th.empty(N, A, device="cuda"), th.empty(N, A, device="cuda")
    _launch(h, W_mu, W_sigma, b_mu, b_sigma, _pair(), q)
    L.check(L.lib().uavgnn_head_fwd(h.data_ptr(), h.stride(0), N, H, W_mu.data_ptr(), W_mu.stride(0), b_mu.data_ptr(), A, plain.data_ptr(), A,
                                    L.stream()), "uavgnn_head_fwd")
    assert th.equal(q, plain)


def test_misaligned_operands_are_refused():
    L, E = _ext()
    N, H, A = 16, 64, 9
    h, W_mu, W_sigma, b_mu, b_sigma = _head_case(N, H, A, th.Generator().manual_seed(0))
    rng, q = _pair(), th.empty(N, A, device="cuda")
    args = lambda hp, wm, ws: (hp, h.stride(0), N - 1, H, wm, ws, W_mu.stride(0), b_mu.data_ptr(), b_sigma.data_ptr(), A, rng.data_ptr(),   # noqa: E731
                               q.data_ptr(), A, L.stream())
    ptrs = (h.data_ptr(), W_mu.data_ptr(), W_sigma.data_ptr())
    for i in range(3):
        shifted = tuple(p + 4 if k == i else p for k, p in enumerate(ptrs))
        assert E.uavgnn_noisy_head_fwd(*args(*shifted)) == L.UAVGNN_EUNSUPPORTED, i
    assert E.uavgnn_noisy_head_fwd(*args(*ptrs)) == 0


# ---- (d) past the grid cap -----------------------------------------------------------------------------------------------------------
def test_noisy_head_past_the_grid_cap():
    """cap * 4 tiles + one full and one ragged tile: the first workgroup's first wavefront walks a second tile.  The same bound on the first
    tile, the last two tiles and 1000 random rows; rows equal those of launches over a prefix alone (1, 65 and 4096 workgroups)."""
    H, A = 64, 9
    per_wg = TILES_PER_BLOCK * TILE_ROWS
    N = GRID_CAP * per_wg + 17
    assert (N + TILE_ROWS - 1) // TILE_ROWS >= GRID_CAP * TILES_PER_BLOCK + 2
    gen = th.Generator().manual_seed(5)
    h, W_mu, W_sigma, b_mu, b_sigma = _head_case(N, H, A, gen, pad=False)
    rng = _pair(SEED, 11)
    q = th.full((N, A), 7.0, device="cuda")
    _launch(h, W_mu, W_sigma, b_mu, b_sigma, rng, q)
    f_in, f_out = _noise(rng, N, H, A)
    th.cuda.synchronize()
    pick = th.randperm(N, generator=gen)[:1000].sort().values
    rows = th.cat((th.arange(16), th.arange(N - 33, N), pick)).cuda()
    err = _rel_err(q, rows, h, W_mu, W_sigma, b_mu, b_sigma, f_in, f_out)
    print(f"N={N}: max |q - q64| / S = {err:.3g}")
    assert err <= HEAD_BOUND
    assert not bool((q == 7.0).all(1).any()), "a row was left unwritten"
    for n in (33, 65 * per_wg - 3, GRID_CAP * per_wg):
        part = th.empty(n, A, device="cuda")
        _launch(h, W_mu, W_sigma, b_mu, b_sigma, rng, part, n)
        assert th.equal(part, q[:n]), f"rows depend on the launch geometry (prefix of {n} rows)"


# ---- (e) the fold --------------------------------------------------------------------------------------------------------------------
FOLD_SHAPES = [(1, 1), (9, 32), (9, 256), (16, 250)]


@pytest.mark.parametrize("A,H", FOLD_SHAPES)
def test_fold_and_its_transpose_bit_for_bit(A, H):
    L, E = _ext()
    gen = th.Generator().manual_seed(A * 1000 + H)
    ld = H + 3              # no alignment is asked of the fold
    W_mu, W_sigma = th.randn(A, ld, generator=gen).cuda()[:, :H], th.rand(A, ld, generator=gen).cuda()[:, :H]
    b_mu, b_sigma = th.randn(A, generator=gen).cuda(), th.rand(A, generator=gen).cuda()
    rng = _pair(SEED, 3)
    W_eff, b_eff = th.full((A, H), 7.0, device="cuda"), th.full((A,), 7.0, device="cuda")
    f_in, f_out = th.full((H,), 7.0, device="cuda"), th.full((A,), 7.0, device="cuda")
    L.check(E.uavgnn_noisy_fold(W_mu.data_ptr(), W_sigma.data_ptr(), ld, b_mu.data_ptr(), b_sigma.data_ptr(), A, H, rng.data_ptr(),
                                W_eff.data_ptr(), b_eff.data_ptr(), f_in.data_ptr(), f_out.data_ptr(), L.stream()), "uavgnn_noisy_fold")
    n_in, n_out = _noise(rng, 3, H, A)
    assert th.equal(f_in, n_in[0]) and th.equal(f_out, n_out[0]), "the fold's draw is row 0 of the stream at that step"
    c = lambda t: t.cpu().numpy()           # noqa: E731  (NumPy float32: every operation rounded once, no fused multiply-add)
    W_want, b_want = R.fold(c(W_mu), c(W_sigma), c(b_mu), c(b_sigma), c(f_in), c(f_out))
    assert W_want.dtype == np.float32 and np.array_equal(c(W_eff), W_want) and np.array_equal(c(b_eff), b_want)
    # through ops, with autograd: the same bits, and the backward launch equals the fp32 products
    from uav_bs_ctrl_amd import ops
    params = [t.clone().contiguous().requires_grad_(True) for t in (W_mu, W_sigma, b_mu, b_sigma)]
    out = ops.noisy_fold(*params, rng=rng)
    assert th.equal(out[0], W_eff) and th.equal(out[1], b_eff) and th.equal(out[2], f_in) and th.equal(out[3], f_out)
    assert int(rng[1]) == 3, "nothing advances the step but the caller"
    dW, db = th.randn(A, ld, generator=gen).cuda()[:, :H], th.randn(A, generator=gen).cuda()
    th.autograd.backward([out[0], out[1]], [dW, db])
    _, dWs, _, dbs = R.fold_transpose(c(dW), c(db), c(f_in), c(f_out))
    assert th.equal(params[0].grad, dW) and th.equal(params[2].grad, db), "the means' gradients are d W_eff / d b_eff themselves"
    assert np.array_equal(c(params[1].grad), dWs) and np.array_equal(c(params[3].grad), dbs)
    got = ops.noisy_fold_bwd(dW, db, f_in, f_out)          # a padded row stride of d W_eff
    assert np.array_equal(c(got[0]), dWs) and np.array_equal(c(got[1]), dbs)


# ---- (f) capture ---------------------------------------------------------------------------------------------------------------------
def test_fold_and_step_advance_replay_under_capture():
    from uav_bs_ctrl_amd import ops
    A, H, s = 9, 256, 40
    gen = th.Generator().manual_seed(1)
    params = [th.randn(A, H, generator=gen).cuda(), th.rand(A, H, generator=gen).cuda(), th.randn(A, generator=gen).cuda(),
              th.rand(A, generator=gen).cuda()]
    eager = []
    for k in range(2):
        eager.append([t.clone() for t in ops.noisy_fold(*params, rng=_pair(SEED, s + k))])
    rng = _pair(SEED, s - 1)

    def body():
        out = ops.noisy_fold(*params, rng=rng)
        rng[1:].add_(1)
        return out

    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side), th.no_grad():
        body()                                  # warm-up: step s - 1 -> s
    th.cuda.current_stream().wait_stream(side)
    graph = th.cuda.CUDAGraph()
    with th.cuda.graph(graph), th.no_grad():
        held = body()
    th.cuda.synchronize()
    assert int(rng[1]) == s, "a capture executes nothing"
    for k in range(2):
        graph.replay()
        th.cuda.synchronize()
        assert int(rng[1]) == s + k + 1
        for got, want in zip(held, eager[k]):
            assert th.equal(got, want), f"replay {k}: not the fold of step {s + k}"


# ---- ops.head_fwd --------------------------------------------------------------------------------------------------------------------
def test_ops_head_fwd_takes_the_launch_where_it_has_the_shape_and_the_stream_elsewhere():
    from uav_bs_ctrl_amd import ops
    N, A = 100, 9
    for H, fused in ((256, True), (96, False)):
        h, W_mu, W_sigma, b_mu, b_sigma = (t.contiguous() for t in _head_case(N, H, A, th.Generator().manual_seed(H), pad=False))
        rng = _pair(SEED, 1)
        assert ops.noisy_supported(h, W_mu, W_sigma, b_mu, b_sigma) == fused
        q = ops.head_fwd(h, W_mu, b_mu, noisy=(W_sigma, b_sigma, rng))
        assert int(rng[1]) == 1
        f_in, f_out = _noise(rng, N, H, A)
        # elsewhere: a vendor GEMM in an order of its own - the worst case of an fp32 sum of H + 1 terms and the three further roundings
        assert _rel_err(q, slice(None), h, W_mu, W_sigma, b_mu, b_sigma, f_in, f_out) <= (HEAD_BOUND if fused else (H + 4) * 2.0 ** -24)
        if fused:
            direct = th.empty(N, A, device="cuda")
            _launch(h, W_mu, W_sigma, b_mu, b_sigma, rng, direct)
            assert th.equal(q, direct)

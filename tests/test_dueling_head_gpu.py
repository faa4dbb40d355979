"""`-m gpu`: the dueling form of the Q head kernel (csrc/head.hip: uavgnn_head_fwd_duel) and ``ops.dueling_head`` against float64 of the
reference's formula q = v + (adv - mean_a adv) (algos/madrqn/agents/dueling.py:13-16)."""
import pytest
import torch as th

from tests.gpu_util import _LibSpy
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EUNSUPPORTED = -1000, -1001


def _params(H, A, seed, dtype=th.float32, device=DEV):
    gen = th.Generator().manual_seed(seed)
    Wa, wv = 0.3 * th.randn(A, H, generator=gen), 0.3 * th.randn(1, H, generator=gen)
    ba, bv = 0.2 * th.randn(A, generator=gen), 0.2 * th.randn(1, generator=gen)
    return [t.to(dtype).to(device) for t in (Wa, ba, wv, bv)]


def _ref64(h, Wa, ba, wv, bv):
    """dueling.py:14-16 in float64"""
    h, Wa, ba, wv, bv = (t.double() for t in (h, Wa, ba, wv, bv))
    vals = th.nn.functional.linear(h, wv, bv)
    advs = th.nn.functional.linear(h, Wa, ba)
    return vals + (advs - advs.mean(-1, keepdim=True))


def _launch(h, N, H, Wa, ba, wv, bv, A, q, ld_h=None, ld_q=None):
    from uav_bs_ctrl_amd import _lib as L
    return L.lib().uavgnn_head_fwd_duel(L.ptr(h), h.stride(0) if ld_h is None else ld_h, N, H, L.ptr(Wa), H, L.ptr(wv), L.ptr(ba), L.ptr(bv), A,
                                        L.ptr(q), (q.stride(0) if q is not None else A) if ld_q is None else ld_q, L.stream())


@pytest.mark.parametrize("N,H,A", [(1, 64, 1), (7, 64, 2), (16, 128, 9), (17, 256, 9), (333, 128, 5), (1000, 256, 15)])
def test_kernel_against_float64(N, H, A):
    from uav_bs_ctrl_amd import _lib as L
    assert L.lib().uavgnn_head_duel_supported(H, A) == 1
    Wa, ba, wv, bv = _params(H, A, seed=N + A)
    h = th.randn(N, H, generator=th.Generator().manual_seed(N)).to(DEV)
    q = th.full((N, A), float("nan"), device=DEV)
    assert _launch(h, N, H, Wa, ba, wv, bv, A, q) == 0
    th.cuda.synchronize()
    assert_close(q, _ref64(h, Wa, ba, wv, bv), 1e-5, f"q ({N}, {H}, {A})")
    if A == 1:      # adv - mean is exactly 0: q is the value column, bit for bit the plain head kernel's on the value head
        v = th.empty((N, 1), device=DEV)
        assert L.lib().uavgnn_head_fwd(h.data_ptr(), H, N, H, wv.data_ptr(), H, bv.data_ptr(), 1, v.data_ptr(), 1, L.stream()) == 0
        assert th.equal(q, v)


def test_kernel_past_the_grid_cap():
    """More 16-row tiles than the capped grid has wavefronts: every wavefront walks a second tile, the last one a partial tile."""
    N, H, A = 4096 * 4 * 16 + 21, 64, 9
    tiles = (N + 15) // 16
    grid = min((tiles + 3) // 4, 4096)
    assert grid * 64 < N
    Wa, ba, wv, bv = _params(H, A, seed=1)
    h = th.randn(N, H, device=DEV, generator=th.Generator(device=DEV).manual_seed(2))
    q = th.full((N, A), float("nan"), device=DEV)
    assert _launch(h, N, H, Wa, ba, wv, bv, A, q) == 0
    th.cuda.synchronize()
    assert_close(q, _ref64(h, Wa, ba, wv, bv), 1e-5, "q past the grid cap")


def test_kernel_respects_row_strides_and_writes_nothing_else():
    N, H, A = 37, 128, 9
    ld_h, ld_q = H + 4, A + 3
    Wa, ba, wv, bv = _params(H, A, seed=3)
    hbuf = th.randn(4 + N * ld_h, generator=th.Generator().manual_seed(4)).to(DEV)
    h = hbuf[4:].view(N, ld_h)[:, :H]                  # base one float4 into the allocation
    qbuf = th.full((4 + N * ld_q + 8,), float("nan"), device=DEV)
    q = qbuf[4:4 + N * ld_q].view(N, ld_q)
    assert _launch(h, N, H, Wa, ba, wv, bv, A, q, ld_h=ld_h, ld_q=ld_q) == 0
    th.cuda.synchronize()
    assert_close(q[:, :A], _ref64(h, Wa, ba, wv, bv), 1e-5, "q, padded rows")
    written = ~th.isnan(qbuf)
    expect = th.zeros_like(written)
    expect[4:4 + N * ld_q].view(N, ld_q)[:, :A] = True
    assert th.equal(written, expect), "the kernel wrote outside [N, A]"


def test_a_nan_row_poisons_its_own_q_row_only():
    """Row N - 1 is also what the lanes past the end of the last tile read (min(row0 + j, N - 1)): their products stay in rows that are
    never stored."""
    N, H, A = 21, 64, 9
    Wa, ba, wv, bv = _params(H, A, seed=5)
    h = th.randn(N, H, generator=th.Generator().manual_seed(6)).to(DEV)
    ref = _ref64(h, Wa, ba, wv, bv)
    for bad in (3, N - 1):
        hb = h.clone()
        hb[bad, 7] = float("nan")
        q = th.zeros((N, A), device=DEV)
        assert _launch(hb, N, H, Wa, ba, wv, bv, A, q) == 0
        th.cuda.synchronize()
        assert bool(th.isnan(q[bad]).all())
        keep = th.arange(N, device=DEV) != bad
        assert_close(q[keep], ref[keep], 1e-5, f"q with a NaN in row {bad}")


def test_two_launches_are_bit_identical():
    N, H, A = 1000, 256, 9
    Wa, ba, wv, bv = _params(H, A, seed=7)
    h = th.randn(N, H, generator=th.Generator().manual_seed(8)).to(DEV)
    q1, q2 = th.empty((N, A), device=DEV), th.empty((N, A), device=DEV)
    assert _launch(h, N, H, Wa, ba, wv, bv, A, q1) == 0 and _launch(h, N, H, Wa, ba, wv, bv, A, q2) == 0
    th.cuda.synchronize()
    assert th.equal(q1, q2)


def test_argument_codes():
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    assert lib.uavgnn_head_duel_supported(64, 16) == 0 and lib.uavgnn_head_duel_supported(32, 9) == 0
    assert lib.uavgnn_head_duel_supported(64, 0) == 0 and lib.uavgnn_head_duel_supported(256, 15) == 1
    N = 8
    q = th.full((N, 16), float("nan"), device=DEV)
    for H, A in ((64, 16), (32, 9)):
        Wa, ba, wv, bv = _params(H, A, seed=9)
        h = th.randn(N, H, device=DEV)
        assert _launch(h, N, H, Wa, ba, wv, bv, A, q) == EUNSUPPORTED
    H, A = 64, 9
    Wa, ba, wv, bv = _params(H, A, seed=10)
    h = th.randn(N, H, device=DEV)
    for k in range(6):
        a = [h, Wa, ba, wv, bv, q]
        a[k] = None
        assert _launch(a[0], N, H, a[1], a[2], a[3], a[4], A, a[5], ld_h=H, ld_q=16) == EINVAL, f"null pointer {k}"
    assert _launch(h, N, H, Wa, ba, wv, bv, A, q, ld_h=H - 4) == EINVAL and _launch(h, N, H, Wa, ba, wv, bv, A, q, ld_q=A - 1) == EINVAL
    assert _launch(h, N, H, Wa, ba, wv, bv, A, q, ld_h=H + 2) == EUNSUPPORTED
    assert _launch(h.view(-1)[1:], N - 1, H, Wa, ba, wv, bv, A, q, ld_h=H) == EUNSUPPORTED       # h off the 16-byte boundary
    assert _launch(h, 0, H, Wa, ba, wv, bv, A, q) == 0
    assert _launch(h, -1, H, Wa, ba, wv, bv, A, q) == EINVAL
    th.cuda.synchronize()
    assert bool(th.isnan(q).all()), "a refused or empty launch wrote to q"


def _layer(H, A, seed, dtype=th.float32, device=DEV):
    from uav_bs_ctrl_amd.agents.heads import DuelingLayer
    layer = DuelingLayer(H, A)
    with th.no_grad():
        for prm, t in zip((layer.adv_head.weight, layer.adv_head.bias, layer.v_head.weight, layer.v_head.bias),
                          _params(H, A, seed, device="cpu")):
            prm.copy_(t)
    return layer.to(dtype).to(device)


@pytest.mark.parametrize("N,H,A", [(1000, 256, 9), (37, 64, 2)])
def test_dueling_head_gradients_against_float64(N, H, A, monkeypatch):
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    layer = _layer(H, A, seed=11)
    gen = th.Generator().manual_seed(12 + N)
    h0, dq0 = th.randn(N, H, generator=gen), th.randn(N, A, generator=gen)

    def oracle(dtype):
        leaves = [h0.clone().to(dtype).requires_grad_(True)] + [p.detach().cpu().to(dtype).requires_grad_(True) for p in ops.dueling_params(layer)]
        vals = th.nn.functional.linear(leaves[0], leaves[3], leaves[4])
        advs = th.nn.functional.linear(leaves[0], leaves[1], leaves[2])
        q = vals + (advs - advs.mean(-1, keepdim=True))
        return q.detach(), th.autograd.grad(q, leaves, dq0.to(dtype))
    q64, g64 = oracle(th.float64)
    _, g32 = oracle(th.float32)
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    h = h0.to(DEV).requires_grad_(True)
    q = ops.dueling_head(h, layer)
    q.backward(dq0.to(DEV))
    monkeypatch.undo()
    assert "uavgnn_head_fwd_duel" in spy.names
    assert_close(q, q64, 1e-5, "ops.dueling_head: q")
    got = [h.grad] + [p.grad for p in ops.dueling_params(layer)]
    for name, a, r64, r32 in zip(("h", "adv_head.weight", "adv_head.bias", "v_head.weight", "v_head.bias"), got, g64, g32):
        grad_close(a, r64, f"ops.dueling_head ({N}, {H}, {A}): grad {name}", ref32=r32)
    # the module takes the same route
    with th.no_grad():
        assert th.equal(layer(h0.to(DEV)), q)


@pytest.mark.parametrize("what,H,A,dtype,device", [("cpu", 64, 9, th.float32, "cpu"), ("float64", 64, 9, th.float64, DEV),
                                                   ("A = 16", 64, 16, th.float32, DEV), ("H = 32", 32, 9, th.float32, DEV)])
def test_unsupported_calls_keep_the_torch_formulation(what, H, A, dtype, device, monkeypatch):
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    layer = _layer(H, A, seed=13, dtype=dtype, device=device)
    x = th.randn(50, H, generator=th.Generator().manual_seed(14)).to(dtype).to(device)
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    with th.no_grad():
        got = layer(x)
    monkeypatch.undo()
    assert "uavgnn_head_fwd_duel" not in spy.names, what
    with th.no_grad():      # the formulation the layer has had so far: one GEMM over the stacked weight, the combine in torch
        w = th.cat((layer.adv_head.weight, layer.v_head.weight), 0)
        b = th.cat((layer.adv_head.bias, layer.v_head.bias), 0)
        out = ops.linear(x, w, b)
        adv, val = out[:, :A], out[:, A:]
        ref = val + adv - adv.mean(-1, keepdim=True)
    assert th.equal(got, ref), what

"""The recurrent half of the GRU cell for few rows (csrc/gru_rec.hip: uavgnn_gru_rec_fwd / _bwd) and ``ops.gru_unroll`` on top of it,
against a float64 ``nn.GRUCell`` loop; the kernels' contract (strides, tails, row independence, determinism, argument errors).

Weights at H = 256 come from the modules' own initialisers (U(-1/sqrt(H), 1/sqrt(H))) under a fixed seed: with the fixtures' closed-form
fill (amplitude 0.25) float32 arithmetic ALONE is 2e-5 from float64 after 11 steps, with these it is below 1e-6."""
import copy
import functools

import pytest
import torch as th
import torch.nn as nn

from tests.util import assert_close, grad_close

gpu = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1000, -1001
N_ACTIONS = 9
# (T1, N, K, H): a single row, a ragged tile, exact tiles, every supported H granularity, more row tiles than column blocks
SHAPES = [(3, 1, 256, 256), (11, 37, 256, 256), (11, 32, 256, 256), (5, 16, 32, 32), (7, 17, 64, 64), (6, 130, 128, 128)]


def _modules(K, H, seed=0):
    th.manual_seed(seed)
    return nn.GRUCell(K, H), nn.Linear(H, N_ACTIONS)


def _inputs(T1, N, K, H, seed=1):
    gen = th.Generator().manual_seed(seed)
    return (th.randn(T1 * N, K, generator=gen), 0.5 * th.randn(N, H, generator=gen), th.randn(T1, N, N_ACTIONS, generator=gen))


@functools.lru_cache(maxsize=None)
def _reference(T1, N, K, H, dtype):
    """(h_all, q_all, gradients of x_all, h0, the cell's four parameters and the head's two) of the CPU loop in `dtype`; the loss weights
    every Q value of every step."""
    cell, head = _modules(K, H)
    cell, head = cell.to(dtype), head.to(dtype)
    x_all, h0, wq = (t.to(dtype) for t in _inputs(T1, N, K, H))
    x_all.requires_grad_(True)
    h0.requires_grad_(True)
    h, hs = h0, []
    for t in range(T1):
        h = cell(x_all[t * N:(t + 1) * N], h)
        hs.append(h)
    h_all = th.stack(hs)
    q = head(h_all)
    leaves = [x_all, h0, cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, head.weight, head.bias]
    grads = th.autograd.grad((q * wq).sum(), leaves)
    return h_all.detach(), q.detach(), [g.detach() for g in grads]


GRAD_NAMES = ("x_all", "h0", "weight_ih", "bias_ih", "weight_hh", "bias_hh", "f_out.weight", "f_out.bias")


def _device_run(T1, N, K, H, train=True, h0_edit=None):
    from uav_bs_ctrl_amd import ops
    cell, head = _modules(K, H)
    cell, head = copy.deepcopy(cell).cuda(), copy.deepcopy(head).cuda()
    x_all, h0, wq = (t.cuda() for t in _inputs(T1, N, K, H))
    if h0_edit is not None:
        h0_edit(h0)
    if not train:
        with th.no_grad():
            return ops.gru_unroll(x_all, h0, cell, T1), None, None
    x_all.requires_grad_(True)
    h0.requires_grad_(True)
    h_all = ops.gru_unroll(x_all, h0, cell, T1)
    q = ops.linear(h_all.reshape(T1 * N, H), head.weight, head.bias).view(T1, N, -1)
    leaves = [x_all, h0, cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, head.weight, head.bias]
    grads = th.autograd.grad((q * wq).sum(), leaves)
    return h_all.detach(), q.detach(), [g.detach() for g in grads]


@gpu
@pytest.mark.parametrize("T1,N,K,H", SHAPES)
def test_gru_unroll_forward_and_every_gradient_against_float64(T1, N, K, H):
    h64, q64, g64 = _reference(T1, N, K, H, th.float64)
    _, _, g32 = _reference(T1, N, K, H, th.float32)
    h_all, q, grads = _device_run(T1, N, K, H)
    assert h_all.shape == (T1, N, H)
    assert_close(h_all, h64, 1e-5, "h_all")
    assert_close(q, q64, 1e-5, "Q")
    for name, g, r64, r32 in zip(GRAD_NAMES, grads, g64, g32):
        grad_close(g, r64, f"gru_unroll ({T1}, {N}, {K}, {H}): grad {name}", ref32=r32)


def _step_inputs(N, H, seed=3):
    gen = th.Generator(device="cuda").manual_seed(seed)
    r = lambda *s, a=1.0: a * th.randn(*s, device="cuda", generator=gen)  # noqa: E731
    return dict(gi=r(N, 3 * H), h=r(N, H, a=0.5), W=r(3 * H, H, a=H ** -0.5), b=r(3 * H, a=0.1), pre=r(N, 4 * H), d_hout=r(N, H), d_carry=r(N, H))


def _rec_fwd(gi, h, W, b, N, H, h_out, pre):
    from uav_bs_ctrl_amd import _lib as L
    rc = L.lib().uavgnn_gru_rec_fwd(gi.data_ptr(), gi.stride(0), h.data_ptr(), h.stride(0), N, H, W.data_ptr(), b.data_ptr(), h_out.data_ptr(),
                                    h_out.stride(0), L.ptr(pre), L.stream())
    assert rc == 0, rc


def _rec_bwd(pre, h, d_hout, d_carry, W, N, H, d_gi, d_gh, dh_prev):
    from uav_bs_ctrl_amd import _lib as L
    rc = L.lib().uavgnn_gru_rec_bwd(pre.data_ptr(), h.data_ptr(), h.stride(0), L.ptr(d_hout), L.ptr(d_carry), N, H, W.data_ptr(),
                                    d_gi.data_ptr(), d_gh.data_ptr(), dh_prev.data_ptr(), L.stream())
    assert rc == 0, rc


@gpu
@pytest.mark.parametrize("which", ["d_hout", "d_carry", "both"])
def test_one_backward_step_against_the_gate_kernel_and_a_float64_product(which):
    """d_gi / d_gh are a handful of fp32-rounded factors of the same saved values in both kernels (1e-6: ten roundings of 2^-24, the compiler's
    choice of fused multiply-adds included); dh_prev is a 3H-term fp32 sum against float64 (the parity rule, 1e-5)."""
    from uav_bs_ctrl_amd import _lib as L
    N, H = 17, 64
    s = _step_inputs(N, H)
    d_hout = s["d_hout"] if which != "d_carry" else None
    d_carry = s["d_carry"] if which != "d_hout" else None
    total = s["d_hout"] + s["d_carry"] if which == "both" else (d_hout if d_hout is not None else d_carry)
    new = lambda *shape: th.full(shape, float("nan"), device="cuda")  # noqa: E731
    gi_ref, gh_ref, dh_ref = new(N, 3 * H), new(N, 3 * H), new(N, H)
    rc = L.lib().uavgnn_gru_gates_bwd_fused(s["pre"].data_ptr(), s["h"].data_ptr(), total.data_ptr(), N, H, gi_ref.data_ptr(), gh_ref.data_ptr(),
                                            dh_ref.data_ptr(), L.stream())
    assert rc == 0
    d_gi, d_gh, dh_prev = new(N, 3 * H), new(N, 3 * H), new(N, H)
    _rec_bwd(s["pre"], s["h"], d_hout, d_carry, s["W"], N, H, d_gi, d_gh, dh_prev)
    assert_close(d_gi, gi_ref, 1e-6, f"{which}: d_gi")
    assert_close(d_gh, gh_ref, 1e-6, f"{which}: d_gh")
    assert_close(dh_prev, dh_ref.double() + gh_ref.double() @ s["W"].double(), 1e-5, f"{which}: dh_prev")


@gpu
def test_strided_operands_give_the_contiguous_result_bit_for_bit():
    N, H = 17, 64
    s = _step_inputs(N, H)
    h_out, pre = th.empty(N, H, device="cuda"), th.empty(N, 4 * H, device="cuda")
    _rec_fwd(s["gi"], s["h"], s["W"], s["b"], N, H, h_out, pre)
    gi_w, h_w, ho_w = th.zeros(N, 3 * H + 16, device="cuda"), th.zeros(N, H + 4, device="cuda"), th.zeros(N, 2 * H, device="cuda")
    gi_v, h_v, ho_v = gi_w[:, 8:8 + 3 * H], h_w[:, 4:], ho_w[:, H:]
    gi_v.copy_(s["gi"])
    h_v.copy_(s["h"])
    pre2 = th.empty_like(pre)
    _rec_fwd(gi_v, h_v, s["W"], s["b"], N, H, ho_v, pre2)
    assert th.equal(ho_v, h_out) and th.equal(pre2, pre)
    assert not bool(ho_w[:, :H].any()), "columns outside the h_out view were written"
    # the backward kernel's h
    outs = [th.empty(N, 3 * H, device="cuda"), th.empty(N, 3 * H, device="cuda"), th.empty(N, H, device="cuda")]
    outs2 = [th.empty_like(t) for t in outs]
    _rec_bwd(pre, s["h"], s["d_hout"], None, s["W"], N, H, *outs)
    _rec_bwd(pre, h_v, s["d_hout"], None, s["W"], N, H, *outs2)
    for a, b in zip(outs, outs2):
        assert th.equal(a, b)


@gpu
def test_tails_every_row_below_N_is_written_and_nothing_behind_it():
    N, H = 17, 64
    s = _step_inputs(N, H)
    nan = lambda *shape: th.full(shape, float("nan"), device="cuda")  # noqa: E731
    h_out, pre = nan(N + 1, H), nan(N + 1, 4 * H)
    _rec_fwd(s["gi"], s["h"], s["W"], s["b"], N, H, h_out, pre)
    d_gi, d_gh, dh_prev = nan(N + 1, 3 * H), nan(N + 1, 3 * H), nan(N + 1, H)
    _rec_bwd(s["pre"], s["h"], s["d_hout"], s["d_carry"], s["W"], N, H, d_gi, d_gh, dh_prev)
    for name, t in dict(h_out=h_out, pre=pre, d_gi=d_gi, d_gh=d_gh, dh_prev=dh_prev).items():
        assert bool(th.isfinite(t[:N]).all()), f"{name}: an element of rows < N was not written"
        assert bool(th.isnan(t[N]).all()), f"{name}: the guard row behind row N - 1 was written"


@gpu
def test_a_nan_row_stays_in_its_row():
    T1, N, K, H = 3, 37, 256, 256

    def poison(h0):
        h0[3] = float("nan")
    clean, _, _ = _device_run(T1, N, K, H, train=False)
    dirty, _, _ = _device_run(T1, N, K, H, train=False, h0_edit=poison)
    assert bool(th.isnan(dirty[:, 3]).all())
    keep = [i for i in range(N) if i != 3]
    assert th.equal(dirty[:, keep], clean[:, keep])


@gpu
def test_two_calls_are_bit_identical_and_no_grad_equals_training():
    T1, N, K, H = 11, 37, 256, 256
    h1, q1, g1 = _device_run(T1, N, K, H)
    h2, q2, g2 = _device_run(T1, N, K, H)
    assert th.equal(h1, h2) and th.equal(q1, q2)
    for name, a, b in zip(GRAD_NAMES, g1, g2):
        assert th.equal(a, b), f"grad {name}"
    h3, _, _ = _device_run(T1, N, K, H, train=False)        # pre_save NULL
    assert th.equal(h3, h1)


def test_argument_errors_are_codes_never_a_launch():
    """No GPU needed: every call returns before it would launch (the addresses are made up and never dereferenced)."""
    from uav_bs_ctrl_amd import _lib
    lib = _lib.lib()
    assert [lib.uavgnn_gru_rec_supported(H) for H in (16, 32, 64, 128, 256, 24, 512, 0, 8)] == [1, 1, 1, 1, 1, 0, 0, 0, 0]
    N, H = 17, 64
    gi, h, W, b, ho, pre = (0x100000 * (i + 1) for i in range(6))

    def fwd(gi=gi, ld_gi=3 * H, h=h, ld_h=H, N=N, H=H, W=W, b=b, ho=ho, ld_ho=H, pre=pre):
        return lib.uavgnn_gru_rec_fwd(gi, ld_gi, h, ld_h, N, H, W, b, ho, ld_ho, pre, None)
    for kw in (dict(gi=None), dict(h=None), dict(W=None), dict(b=None), dict(ho=None), dict(N=-1), dict(ld_gi=3 * H - 4), dict(ld_h=H - 4)):
        assert fwd(**kw) == EINVAL, kw
    assert fwd(ho=h) == EINVAL and fwd(ho=h + 4 * H * (N - 1)) == EINVAL and fwd(h=ho + 16, ld_h=H + 4) == EINVAL, "h_out overlapping h"
    for kw in (dict(H=24, ld_gi=72, ld_h=24, ld_ho=24), dict(H=512, ld_gi=1536, ld_h=512, ld_ho=512), dict(gi=gi + 4), dict(h=h + 8),
               dict(ho=ho + 4), dict(W=W + 4), dict(pre=pre + 4), dict(ld_h=H + 2), dict(ld_gi=3 * H + 1), dict(ld_ho=H + 3)):
        assert fwd(**kw) == EUNSUPPORTED, kw
    d_hout, d_carry, d_gi, d_gh, dh = (0x100000 * (i + 8) for i in range(5))

    def bwd(pre=pre, h=h, ld_h=H, d_hout=d_hout, d_carry=d_carry, N=N, H=H, W=W, d_gi=d_gi, d_gh=d_gh, dh=dh):
        return lib.uavgnn_gru_rec_bwd(pre, h, ld_h, d_hout, d_carry, N, H, W, d_gi, d_gh, dh, None)
    for kw in (dict(pre=None), dict(h=None), dict(W=None), dict(d_gi=None), dict(d_gh=None), dict(dh=None), dict(N=-1), dict(ld_h=H - 4)):
        assert bwd(**kw) == EINVAL, kw
    assert bwd(dh=d_hout) == EINVAL and bwd(dh=d_carry) == EINVAL and bwd(dh=d_carry + 4 * H * (N - 1), d_hout=None) == EINVAL
    for kw in (dict(H=24, ld_h=24), dict(H=512, ld_h=512), dict(pre=pre + 4), dict(d_hout=d_hout + 4), dict(d_carry=d_carry + 8),
               dict(dh=dh + 4), dict(d_gi=d_gi + 4), dict(ld_h=H + 2)):
        assert bwd(**kw) == EUNSUPPORTED, kw

"""`-m gpu`: the row bounds a K1 launch with row maxima hands to the f16x2 f_aggr product behind it (``ops.hetero_gatv2`` ->
``ops.linear_relu``, gnn_agents.py:106).  The bounds travel on the K1 output as ``_uavgnn_rowmax``; the f16x2 kernel scales every row
by them, so they must exist only where the launch wrote them, and hold only for the values they were taken from: a launch the library
declined leaves none, and an in-place edit of the output between the two calls retires them.  Each product is held to float64."""
import pytest
import torch as th

from tests.gpu_util import EXP3, _LibSpy, agent_from_params, default_init_params, synth_graph, to_batch
from tests.util import assert_close

pytestmark = pytest.mark.gpu

# 16 384 destinations: the fewest on which f_aggr's [N, 512] x [512, 256] product takes the f16x2 kernel (ops.gemm_h2_supported: 128
# output tiles of 256 x 128).  ops.K1_ROWMAX_MIN_ROWS (2^17) is lowered below it, so that the K1 launch leaves row maxima here.
B, N_AGENTS, M = 2048, 8, 20


def _encoder_inputs(monkeypatch):
    from uav_bs_ctrl_amd import ops
    monkeypatch.setattr(ops, "K1_ROWMAX_MIN_ROWS", 1024)
    net = agent_from_params(default_init_params(EXP3, seed=1), EXP3)
    g = to_batch(synth_graph(B, N_AGENTS, M, "env", seed=4))
    enc = net.enc
    rels = []
    for et in ("seen", "near"):
        x_src, off = g.relation_segments(et)
        rels.append((x_src, off, g.relation_order(et), enc.f_conv[et]))
    return enc, g.agent_feat(), rels


def _spied(monkeypatch, fn):
    """fn() under the library spy: (its value, the spy)."""
    from uav_bs_ctrl_amd import _lib as L
    spy = _LibSpy(L.lib())
    with monkeypatch.context() as mp:
        mp.setattr(L, "lib", lambda: spy)
        out = fn()
    return out, spy


def _rowmax_rcs(spy):
    return [rc for (nm, _), rc in zip(spy.calls, spy.results) if nm == "uavgnn_gatv2_hetero_fwd_rowmax"]


def _linear_relu64(x, W, b):
    f = lambda t: t.detach().double().cpu()   # noqa: E731
    return th.relu(f(x) @ f(W).t() + f(b))


def test_declined_k1_rowmax_launch_leaves_no_row_bound(monkeypatch):
    """The `seen` source at an address that is 8-byte but not 16-byte aligned: the fused K1 launch (16-byte loads of x_gt) declines with
    UAVGNN_EUNSUPPORTED, the per-relation kernels (8 bytes suffice) fill the output - and no row maxima may come with it: the launch that
    would have written them never ran (they used to be attached anyway, uninitialised, and scaled the f16x2 product behind)."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    enc, x_dst, rels = _encoder_inputs(monkeypatch)
    x_gt = rels[0][0]
    buf = th.empty(x_gt.numel() + 2, dtype=th.float32, device=x_gt.device)
    x_gt8 = buf[2:].view_as(x_gt)
    x_gt8.copy_(x_gt)
    assert x_gt8.data_ptr() % 16 == 8 and x_gt8.is_contiguous()
    moved = [(x_gt8,) + tuple(rels[0][1:]), rels[1]]
    with th.no_grad():
        x, spy = _spied(monkeypatch, lambda: ops.hetero_gatv2(x_dst, enc._n_heads, moved))
        x_ref, spy_ref = _spied(monkeypatch, lambda: ops.hetero_gatv2(x_dst, enc._n_heads, rels))
    assert _rowmax_rcs(spy) == [L.UAVGNN_EUNSUPPORTED], _rowmax_rcs(spy)
    assert [nm for nm, _ in spy.calls if nm == "uavgnn_gatv2_fwd"] == ["uavgnn_gatv2_fwd"] * 2, "the per-relation fallback did not run"
    assert _rowmax_rcs(spy_ref) == [0] and getattr(x_ref, "_uavgnn_rowmax", None) is not None
    assert getattr(x, "_uavgnn_rowmax", None) is None, "a declined K1 launch left row maxima on its output"
    assert_close(x, x_ref, 1e-5, "K1 output of the per-relation fallback vs the fused launch")
    lin = enc.f_aggr[0]
    with th.no_grad():
        y = ops.linear_relu(x, lin.weight, lin.bias)
    assert bool(th.isfinite(y).all()), "f_aggr behind a declined K1 launch: non-finite output"
    assert_close(y, _linear_relu64(x, lin.weight, lin.bias), 1e-5, "f_aggr behind a declined K1 launch vs float64")


@pytest.mark.parametrize("scale", [16.0, 2.0 ** -30], ids=["x16", "x2^-30"])
def test_in_place_edit_of_k1_output_retires_its_row_bound(scale, monkeypatch):
    """``x = hetero_gatv2(...)`` with row maxima, then ``x.mul_(scale)`` before ``linear_relu(x, W, b)``: the maxima no longer bound x.
    x16 puts rows above their bound (the f16 split overflows: half of the outputs came out 0 where float64 has up to 4.3); x2^-30
    leaves them 2^30 below it (the split keeps few significant bits of them: errors of 3e-3 of the output scale, silently).  The
    product must match float64 either way, and the UNEDITED output must still take the f16x2 kernel (the benchmark's path).  The bias
    is zero so that the product of the x2^-30 case is not hidden under it."""
    from uav_bs_ctrl_amd import ops
    enc, x_dst, rels = _encoder_inputs(monkeypatch)
    W = enc.f_aggr[0].weight
    b = th.zeros_like(enc.f_aggr[0].bias)
    with th.no_grad():
        x, spy = _spied(monkeypatch, lambda: ops.hetero_gatv2(x_dst, enc._n_heads, rels))
        assert _rowmax_rcs(spy) == [0] and getattr(x, "_uavgnn_rowmax", None) is not None
        y, spy = _spied(monkeypatch, lambda: ops.linear_relu(x, W, b))
        assert any(nm == "uavgnn_gemm_nt_h2" for nm, _ in spy.calls), "f_aggr behind a K1 launch with row maxima left the f16x2 kernel"
        assert_close(y, _linear_relu64(x, W, b), 1e-5, "f_aggr on the K1 output as the launch left it vs float64")
        x.mul_(scale)
        y = ops.linear_relu(x, W, b)
    assert not bool(th.isnan(y).any()), f"f_aggr after x.mul_({scale:g}): NaN"
    assert_close(y, _linear_relu64(x, W, b), 1e-5, f"f_aggr after x.mul_({scale:g}) vs float64")

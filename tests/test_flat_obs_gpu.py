"""`-m gpu`: the first encoder layer of the flattened-observation agents read straight from the padded observations
(csrc/flat_obs.hip through ops.flat_linear_relu): forward against float64, full coverage of the output, bit-reproducibility, strided
views, agreement with th.cat + linear_relu, the weight / bias gradients against float64 at the time-batched size, and the fallback
of an unsupported shape.  Parity rule: BASELINE.md section 4 (rtol 1e-5, atol 1e-5 max|ref|); gradients through grad_close."""
import pytest
import torch as th

from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fused(monkeypatch):
    """These tests are about the kernels: the fused path wherever the shape is supported (UAVGNN_FLAT_OBS_FUSED=1), whatever the
    measured default picks for the shape."""
    from uav_bs_ctrl_amd import ops
    monkeypatch.setattr(ops, "FLAT_OBS_FUSED", "1")

SHAPES = [(4, 4, 5), (4, 4, 4), (3, 4, 5), (8, 50, 5)]      # (n, M, Sg)
ROWS = [1, 17, 16384, 41 * 16384]
BIG = 41 * 16384


def _pieces(rows, n, M, Sg, seed, pad=0):
    """(agent [rows, 2], gt [rows, M Sg], ubs [rows, (n-1) 3]) in the simulator's value ranges; pad > 0: strided row views of wider
    buffers (what time-major views of the replay look like to the kernel)."""
    g = th.Generator(device="cuda").manual_seed(seed)
    out = []
    for k in (2, M * Sg, (n - 1) * 3):
        buf = th.rand(rows, k + pad, device="cuda", generator=g) * 2 - 1
        out.append(buf[:, :k])
    return tuple(out)


def _weights(H, F, seed):
    g = th.Generator(device="cuda").manual_seed(seed)
    return (th.randn(H, F, device="cuda", generator=g) / F ** 0.5, th.randn(H, device="cuda", generator=g) * 0.1)


def _ref64(parts, W, b):
    x = th.cat([p.double() for p in parts], 1)
    return th.relu(x @ W.double().t() + b.double())


def _fwd_raw(parts, W, b, y):
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.ops import _flat_src
    L.check(L.lib().uavgnn_flat_obs_fwd(*_flat_src(parts), parts[0].shape[0], W.data_ptr(), b.data_ptr(), W.shape[0], y.data_ptr(),
                                        y.stride(0), L.stream()), "uavgnn_flat_obs_fwd")
    return y


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_matches_float64_and_reproduces(shape, rows, H):
    from uav_bs_ctrl_amd import ops
    n, M, Sg = shape
    parts = _pieces(rows, n, M, Sg, seed=rows + 7 * n + M)
    F = sum(p.shape[1] for p in parts)
    W, b = _weights(H, F, seed=F + H)
    assert ops.flat_obs_supported(parts, W)
    y_nan = th.full((rows, H), float("nan"), device="cuda")
    y1 = _fwd_raw(parts, W, b, y_nan)
    assert bool(th.isfinite(y1).all()), "output rows / columns left unwritten"
    assert_close(y1, _ref64(parts, W, b), 1e-5, f"flat fwd {shape} rows={rows} H={H}")
    y2 = _fwd_raw(parts, W, b, th.empty_like(y1))
    assert th.equal(y1, y2), "two launches differ"
    # the autograd op = the raw launch; the th.cat + linear_relu path within the parity rule
    with th.no_grad():
        y_op = ops.flat_linear_relu(parts, W, b)
        y_cat = ops.linear_relu(th.cat(parts, 1), W, b)
    assert th.equal(y_op, y1)
    assert_close(y_op, y_cat.double(), 1e-5, f"flat fwd vs cat+linear_relu {shape} rows={rows} H={H}")


@pytest.mark.parametrize("shape", SHAPES)
def test_strided_views_give_the_bits_of_contiguous_copies(shape):
    from uav_bs_ctrl_amd import ops
    n, M, Sg = shape
    strided = _pieces(4099, n, M, Sg, seed=5, pad=3)
    assert strided[1].stride(0) > strided[1].shape[1]
    contig = tuple(p.contiguous() for p in strided)
    W, b = _weights(128, sum(p.shape[1] for p in contig), seed=9)
    with th.no_grad():
        assert th.equal(ops.flat_linear_relu(strided, W, b), ops.flat_linear_relu(contig, W, b))
    dy = th.randn(4099, 128, device="cuda")
    grads = []
    for parts in (strided, contig):
        Wg, bg = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        (ops.flat_linear_relu(parts, Wg, bg) * dy).sum().backward()
        grads.append((Wg.grad, bg.grad))
    assert th.equal(grads[0][0], grads[1][0]) and th.equal(grads[0][1], grads[1][1])


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("shape", SHAPES)
def test_weight_and_bias_gradients_match_float64_and_reproduce(shape, H):
    from uav_bs_ctrl_amd import ops
    n, M, Sg = shape
    parts = _pieces(BIG, n, M, Sg, seed=11 + n + M + Sg)
    F = sum(p.shape[1] for p in parts)
    W, b = _weights(H, F, seed=13 + F)
    wy = th.randn(BIG, H, device="cuda", generator=th.Generator(device="cuda").manual_seed(17)) / BIG ** 0.5
    runs = []
    for _ in range(2):
        Wg, bg = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        (ops.flat_linear_relu(parts, Wg, bg) * wy).sum().backward()
        runs.append((Wg.grad.clone(), bg.grad.clone()))
    assert th.equal(runs[0][0], runs[1][0]) and th.equal(runs[0][1], runs[1][1]), "gradients differ between two runs"
    x64 = th.cat([p.double() for p in parts], 1)
    # the ReLU mask is the one discontinuity: float64 is evaluated under the mask the fp32 forward took (a pre-activation within
    # rounding of 0 may fall on either side; each such row moves dW by |dy x|, far above the parity rule)
    with th.no_grad():
        mask = ops.flat_linear_relu(parts, W, b) > 0
    dym = wy.double() * mask
    grad_close(runs[0][0], dym.t() @ x64, f"flat dW {shape} H={H}")
    grad_close(runs[0][1], dym.sum(0), f"flat db {shape} H={H}")


def test_unsupported_shape_falls_back_and_agrees(monkeypatch):
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    parts = _pieces(1000, 4, 4, 5, seed=3)
    W, b = _weights(96, 31, seed=4)            # H_out = 96: no instantiation
    assert L.lib().uavgnn_flat_obs_supported(96, 31) == 0 and not ops.flat_obs_supported(parts, W)
    assert L.lib().uavgnn_flat_obs_supported(64, 1025) == 0
    called = []
    real = ops.linear_relu
    monkeypatch.setattr(ops, "linear_relu", lambda *a: called.append(1) or real(*a))
    Wg, bg = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.flat_linear_relu(parts, Wg, bg)
    assert called, "the unsupported shape did not take th.cat + linear_relu"
    assert_close(y, _ref64(parts, W, b), 1e-5, "fallback fwd")
    y.sum().backward()
    x64 = th.cat([p.double() for p in parts], 1)
    dym = (y > 0).double()          # the mask the fp32 forward took (see above)
    grad_close(Wg.grad, dym.t() @ x64, "fallback dW")
    # the switch: UAVGNN_FLAT_OBS_FUSED=0 sends a supported shape the same way
    monkeypatch.setattr(ops, "FLAT_OBS_FUSED", "0")
    W64, b64 = _weights(64, 31, seed=6)
    called.clear()
    with th.no_grad():
        y_off = ops.flat_linear_relu(parts, W64, b64)
    assert called
    assert_close(y_off, _ref64(parts, W64, b64), 1e-5, "switched-off fwd")


def test_auto_mode_takes_the_fused_forward_only_where_it_measured_faster(monkeypatch):
    from uav_bs_ctrl_amd import ops
    monkeypatch.setattr(ops, "FLAT_OBS_FUSED", "auto")
    small, big = _pieces(16384, 4, 4, 5, seed=1), _pieces(41 * 16384, 4, 4, 5, seed=2)
    wide = _pieces(16384, 8, 80, 5, seed=3)
    W = _weights(256, 31, seed=4)[0]
    assert ops.flat_obs_supported(small, W) and not ops.flat_obs_supported(small, W, needs_grad=True)
    assert not ops.flat_obs_supported(big, W) and not ops.flat_obs_supported(wide, _weights(256, 423, seed=5)[0])

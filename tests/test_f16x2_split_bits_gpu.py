"""`-m gpu`: the split helper of csrc/f16x2.h (four mixed-precision FMAs per element pair) through the weight-split kernels
uavgnn_split_h2 (both `transpose` values) and uavgnn_gru_split_weights_h2, on crafted rows: the planes and `winv` are bit-equal to
`split_f16x2` / `scale_exp` of tests/test_f16x2_emulation.py (multiply, convert, subtract, convert - the arithmetic the helper had
before), row by row under the row's own bound.  Rows: random normals; a ladder 2^-k below the row maximum, k = 0 .. 45 (lo subnormal,
then zero, then both terms zero), in both signs; exact ties after scaling (midpoints of neighbouring f16 values for hi, for lo and
among the f16 subnormals); -0.0, whose sign hi keeps; fp32 subnormal elements; row maxima near 3e38 and near 1e-38 (the clamped scale
exponents); an all-zero row; rows holding Inf or NaN, compared by class.

One input is outside bit-equality by construction and has a test of its own: an element whose scaled value lies below the fp32 range
(|v s| < 2^-150: |v| < 2^-164 of a row maximum above 2^15).  The separate multiply rounds that product to a zero and the subtraction
then gives lo = +0; the fused form keeps the product's sign, lo = -0 for a negative element.  hi is the same, both terms are zeros,
and every dot product is the same."""
import numpy as np
import pytest
import torch as th

from tests.test_f16x2_emulation import scale_exp, split_f16x2

pytestmark = pytest.mark.gpu

COLS = 64


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def crafted(cols=COLS, seed=0):
    """[16, cols] fp32: one kind of row each (module docstring); the first 64 columns carry the pattern, further columns stay below the bound."""
    rng = np.random.default_rng(seed)
    k = np.arange(46)
    rows = []
    rows.append(rng.standard_normal(cols))                                              # 0  random normals
    rows.append(np.concatenate([1.5 * np.exp2(-k[:1]), 1.2345 * np.exp2(-k[1:]), np.zeros(cols - 46)]))       # 1  ladder, positive
    rows.append(np.concatenate([-1.5 * np.exp2(-k[:1]), -1.7071 * np.exp2(-k[1:]), np.zeros(cols - 46)]))     # 2  ladder, negative
    s = 2.0 ** 14                                                                       # the scale of a row whose maximum is 1.5
    j = np.arange(20)
    ties_hi = (1024.5 + j) / s                                                          # midpoints of f16 values with ulp 1: to even
    ties_lo = (2048.5 + (2 * j + 1) * 2.0 ** -12) / s                                   # hi = 2048, the rest a midpoint of f16 values with ulp 2^-11
    ties_sub = (2 * j + 1) * 2.0 ** -25 / s                                             # midpoints of f16 subnormals
    t = np.concatenate([[1.5], ties_hi, ties_lo, ties_sub, np.zeros(cols - 61)])
    rows.append(t)                                                                      # 3  ties
    rows.append(np.concatenate([[-1.5], -ties_hi, -ties_lo, -ties_sub, np.zeros(cols - 61)]))                  # 4  ties, negative
    z = rng.standard_normal(cols)
    z[1::3] = -0.0
    z[2::3] = 0.0
    rows.append(z)                                                                      # 5  -0.0 and +0.0 among normals
    sub = rng.integers(1, 1 << 23, cols).astype(np.uint32).view(np.float32).astype(np.float64) * rng.choice([-1.0, 1.0], cols)
    r6 = sub.copy()
    r6[0] = 2.0 ** -100
    rows.append(r6)                                                                     # 6  fp32 subnormals under a normal maximum
    rows.append(sub)                                                                    # 7  only fp32 subnormals (scale exponent clamped to 126)
    big = np.concatenate([3.0e38 * np.exp2(-k[:1]), 2.9e38 * np.exp2(-k[1:]) * np.where(k[1:] & 1, -1.0, 1.0), np.zeros(cols - 46)])
    rows.append(big)                                                                    # 8  maximum near 3e38 (scale exponent -113)
    rows.append(np.concatenate([[1.0e-38], 0.9e-38 * np.exp2(-k[1:24]), np.zeros(cols - 24)]))                # 9  maximum near 1e-38, subnormal
    rows.append(np.concatenate([[-1.5e-38], 1.4e-38 * np.exp2(-k[1:24]), np.zeros(cols - 24)]))               # 10 maximum near 1e-38, normal
    rows.append(np.zeros(cols))                                                         # 11 all zero
    r = rng.standard_normal(cols)
    r[7] = np.inf
    rows.append(r)                                                                      # 12 +Inf
    r = rng.standard_normal(cols)
    r[8], r[20] = -np.inf, np.inf
    rows.append(r)                                                                      # 13 -Inf and +Inf
    r = rng.standard_normal(cols)
    r[9] = np.nan
    rows.append(r)                                                                      # 14 NaN (the row maximum drops it: the other elements split as usual)
    r = rng.standard_normal(cols) * 1e-3
    r[10], r[11] = np.nan, np.inf
    rows.append(r)                                                                      # 15 NaN and Inf
    return _f32(np.stack(rows))


def expected(a):
    """(hi, lo, winv) of every row of `a` under its own bound (fmaxf drops NaN, as the kernels' row maximum does)."""
    hi, lo, winv = np.empty(a.shape, np.float16), np.empty(a.shape, np.float16), np.empty(a.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for i, row in enumerate(a):
            bound = np.float32(np.fmax.reduce(np.abs(row)))
            if np.isnan(bound):
                bound = np.float32(0)
            hi[i], lo[i], _ = split_f16x2(row, bound)
            winv[i] = np.float32(2.0 ** float(-scale_exp(bound)))
    return hi, lo, winv


def assert_planes(got, want, what):
    """bit-equal, except that NaN is compared as a class (Inf has one encoding per sign and is compared bit for bit)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions"
    assert np.array_equal(np.isinf(got), np.isinf(want)), f"{what}: Inf positions"
    g, w = got.view(np.uint16), want.view(np.uint16)
    bad = (g != w) & ~nan
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{int(g[bad][0]):#06x} against {int(w[bad][0]):#06x}")


def _planes(buf, n_out, K):
    raw = buf.cpu().numpy()
    pl = raw[:4 * n_out * K].view(np.float16).reshape(2, n_out, K)
    return pl[0], pl[1], raw[4 * n_out * K:].view(np.float32)


@pytest.fixture(scope="module")
def reference():
    a = crafted()
    return (a,) + expected(a)


def test_the_crafted_rows_hold_what_they_claim(reference):
    a, hi, lo, winv = reference
    f = lambda t: t.astype(np.float64)   # noqa: E731
    sub16 = lambda t: (t != 0) & (np.abs(f(t)) < 2.0 ** -14)   # noqa: E731
    assert sub16(lo[1]).any() and (lo[1][:46] == 0).any() and ((hi[1][:46] == 0) & (a[1][:46] != 0)).any()     # the ladder reaches all three
    assert sub16(hi[3]).any() and (hi[3][1:21] % 2 == 0).all()                                                  # ties went to even
    assert np.signbit(hi[5][1::3]).all() and not np.signbit(hi[5][2::3]).any()
    assert (np.abs(a[6][1:]) < 2.0 ** -126).all() and (a[6][1:] != 0).all()
    assert winv[8] == np.float32(2.0 ** 113) and winv[7] == winv[9] == winv[10] == winv[11] == np.float32(2.0 ** -126)
    assert np.isnan(lo[12][7]) and np.isinf(hi[12][7]) and np.isnan(hi[14][9]) and not np.isnan(hi[14][:9]).any()


@pytest.mark.parametrize("transpose", [0, 1])
def test_split_h2_planes_and_winv(reference, transpose):
    from uav_bs_ctrl_amd import _lib as L
    a, hi, lo, winv = reference
    n_out, K = a.shape
    W = th.from_numpy(a.T.copy() if transpose else a).cuda()
    R, C = W.shape
    buf = th.zeros(L.lib().uavgnn_split_h2_bytes(n_out, K), dtype=th.uint8, device="cuda")
    L.check(L.lib().uavgnn_split_h2(W.data_ptr(), W.stride(0), R, C, transpose, buf.data_ptr(), L.stream()), "uavgnn_split_h2")
    th.cuda.synchronize()
    g_hi, g_lo, g_winv = _planes(buf, n_out, K)
    assert_planes(g_hi, hi, "hi")
    assert_planes(g_lo, lo, "lo")
    assert np.array_equal(g_winv.view(np.uint32), winv.view(np.uint32))


def test_gru_split_weights_h2_planes_and_winv():
    """[W_ih | W_hh] share the row's scale: the crafted rows, 80 columns wide, cut at column 64 (H = 16: 48 weight rows = the 16 rows three times)."""
    from uav_bs_ctrl_amd import _lib as L
    H, K_in = 16, 64
    a = np.tile(np.concatenate([crafted(), crafted(seed=1)[:, :H] * _f32(2.0 ** -3)], axis=1), (3, 1))
    a[:, K_in:][~np.isfinite(a[:, K_in:])] = 0.25                       # (keep the non-finite elements where the row kinds put them)
    a[11::16] = 0                                                        # the all-zero row stays all zero
    a[7::16, K_in:] = a[7::16, :H]                                       # ... and the subnormal-only row subnormal
    a[9::16, K_in:] = 0
    a[10::16, K_in:] = 0
    hi, lo, winv = expected(a)
    W_ih, W_hh = th.from_numpy(a[:, :K_in].copy()).cuda(), th.from_numpy(a[:, K_in:].copy()).cuda()
    buf = th.zeros(L.lib().uavgnn_gru_cell_h2_workspace_bytes(K_in, H), dtype=th.uint8, device="cuda")
    L.check(L.lib().uavgnn_gru_split_weights_h2(W_ih.data_ptr(), K_in, W_hh.data_ptr(), H, buf.data_ptr(), L.stream()), "gru split")
    th.cuda.synchronize()
    raw = buf.cpu().numpy()
    n_ih, n_hh = 2 * 3 * H * K_in * 2, 2 * 3 * H * H * 2
    p_ih = raw[:n_ih].view(np.float16).reshape(2, 3 * H, K_in)
    p_hh = raw[n_ih:n_ih + n_hh].view(np.float16).reshape(2, 3 * H, H)
    g_winv = raw[n_ih + n_hh:].view(np.float32)
    assert_planes(np.concatenate([p_ih[0], p_hh[0]], 1), hi, "hi")
    assert_planes(np.concatenate([p_ih[1], p_hh[1]], 1), lo, "lo")
    assert np.array_equal(g_winv.view(np.uint32), winv.view(np.uint32))


def test_product_below_fp32_range_keeps_hi_and_a_zero_lo():
    """|v s| < 2^-150 (module docstring): hi is bit-equal to the emulation (a zero with the element's sign), lo is a zero of the element's
    sign - the emulation's +0 for a negative element is the one bit that differs - and the rest of the row is bit-equal."""
    from uav_bs_ctrl_amd import _lib as L
    a = crafted()[8:9].copy()                                            # maximum 3e38: s = 2^-113
    tiny = _f32([-2.0 ** -40, 2.0 ** -40, -2.0 ** -149, 2.0 ** -149])    # |v s| = 2^-153, 2^-262
    a[0, 48:52] = tiny
    hi, lo, winv = expected(a)
    W = th.from_numpy(np.concatenate([a, a])).cuda()                     # (two rows: an even shape for both transposes is not needed here)
    buf = th.zeros(L.lib().uavgnn_split_h2_bytes(2, COLS), dtype=th.uint8, device="cuda")
    L.check(L.lib().uavgnn_split_h2(W.data_ptr(), W.stride(0), 2, COLS, 0, buf.data_ptr(), L.stream()), "uavgnn_split_h2")
    th.cuda.synchronize()
    g_hi, g_lo, g_winv = _planes(buf, 2, COLS)
    assert_planes(g_hi[:1], hi, "hi")
    keep = np.ones(COLS, bool)
    keep[48:52] = False
    assert_planes(g_lo[:1, keep], lo[:, keep], "lo away from the underflowing products")
    assert np.array_equal(g_lo[0, 48:52].view(np.uint16), np.array([0x8000, 0, 0x8000, 0], np.uint16))
    assert np.array_equal(lo[0, 48:52].view(np.uint16), np.zeros(4, np.uint16))
    assert np.array_equal(g_hi[0, 48:52].view(np.uint16), np.array([0x8000, 0, 0x8000, 0], np.uint16))

"""`-m gpu`: the f16x2 NT GEMMs of csrc/gemm_h2.hip (uavgnn_gemm_nt_h2, _rm2, _n64) at the smallest shapes that have their edges - a
clamped row tile (M = 1 .. 600), a partial column block and the per-element epilogue (N = 1 .. 320, ldy % 4 != 0, a misaligned Y),
contractions of one to three K slices, a view as the second source, the interleaved staging loop - against float64 ENTRY BY ENTRY under
the bound derived in tests/test_f16x2_nt_emulation.py, through the C ABI (no ops threshold is in the way, nothing is monkeypatched).

Every NT call goes through `_call`: X, X2 and the weight are views into wider buffers whose padding (and, for X, the rows behind M) holds
NaN; Y is a view into a buffer of a sentinel bit pattern with four guard rows in front and behind, and every word outside [M, N] - the
columns N .. ldy - 1 of the M rows included - must still hold the sentinel after the call.  No entry is exempt from the bound: the
float64 reference alone stays inside it on these operands.  The worst error / bound per case is appended to
f16x2_nt_edges.jsonl beside the gradient-error log of tests/util.py, against r = 1 and r = 4 roundings per MFMA step (profiles/f16x2_nt_edges.txt is the table made from it);
the assertion uses R_ASSERT of the emulation file.  The ragged shapes that tests/test_f16x2_kernels_golden_gpu.py pins bit for bit
(M = 257, N = 192, K1 = 32 of K = 64; the n64 kernel at M = 129) are among the cases."""
import json
import os

import numpy as np
import pytest
import torch as th

from tests.test_f16x2_nt_emulation import R_ASSERT, ladder, nt_bound, row_absmax, worst_ratio
from tests.util import _GRAD_LOG

pytestmark = pytest.mark.gpu

ACC, RELU, IL, TILE_128, TILE_64 = 1, 2, 4, 8, 16          # UAVGNN_GEMM_* (include/uavgnn.h)
EINVAL, EUNSUPPORTED = -1000, -1001
EPILOGUES = (0, RELU, ACC, ACC | RELU)
SENTINEL = 0x7FC5A5A5                                       # a NaN no kernel produces
GUARD = 4
M_MAX, N_MAX, K_MAX = 600, 320, 192

ONE_SOURCE = [(1, 1, 32), (1, 128, 64), (1, 192, 32), (1, 320, 96), (63, 9, 64), (63, 130, 32), (63, 192, 96), (256, 128, 32),
              (256, 130, 96), (256, 320, 64), (257, 192, 64), (257, 1, 96), (257, 9, 32), (257, 128, 96), (600, 9, 96), (600, 130, 64),
              (600, 192, 32), (600, 320, 96)]
TWO_SOURCE = [(M, N, K1, K2) for M in (1, 257) for N in (128, 192) for K1, K2 in ((32, 32), (32, 64), (64, 96))]
_LOG = os.path.join(os.path.dirname(_GRAD_LOG), "f16x2_nt_edges.jsonl")      # (the directory of the gradient-error log)


@pytest.fixture(scope="module")
def L():
    from uav_bs_ctrl_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def pool():
    """Ladder operands (normal x 2^-(0 .. 30) per element, x 2^(-6 .. 6) per row), drawn once; a case reads a leading block.  Never written."""
    rng = np.random.default_rng(9521)
    x = ladder(rng, M_MAX, K_MAX)
    x2 = ladder(rng, M_MAX, 96)      # the second source: each row 2^6 above the same row of the first (to within the rows' own elements)
    x2 = x2 * np.exp2(6 + np.floor(np.log2(row_absmax(x[:, :32]) / row_absmax(x2[:, :32]))))[:, None].astype(np.float32)
    return dict(x=x, x2=x2, w=ladder(rng, N_MAX, K_MAX),
                bias=rng.standard_normal(N_MAX).astype(np.float32), y0=rng.standard_normal((M_MAX, N_MAX)).astype(np.float32))


def _record(kernel, family, case, r1, r4):
    try:
        with open(_LOG, "a") as f:
            f.write(json.dumps(dict(kernel=kernel, family=family, case=case, ratio_r1=r1, ratio_r4=r4)) + "\n")
    except OSError:
        pass


def _view(a, pad_rows, pad_cols):
    """a [R, C] (host, fp32) as the leading block of a device buffer [R + pad_rows, C + pad_cols] of NaN."""
    R, C = a.shape
    buf = th.full((R + pad_rows, C + pad_cols), float("nan"), device="cuda")
    buf[:R, :C] = th.from_numpy(np.ascontiguousarray(a)).cuda()
    return buf[:R, :C]


def _planes(L, w, transpose):
    """uavgnn_split_h2 of the weight w [N, K], handed over as W = w (transpose 0) or W = w^T (transpose 1), either with ld > C."""
    N, K = w.shape
    W = _view(w.T if transpose else w, 1, 3)
    planes = th.empty(L.lib().uavgnn_split_h2_bytes(N, K), dtype=th.uint8, device="cuda")
    L.check(L.lib().uavgnn_split_h2(W.data_ptr(), W.stride(0), W.shape[0], W.shape[1], int(transpose), planes.data_ptr(), L.stream()), "split_h2")
    return planes


class _Y:
    """The output view [M, N] (row stride ldy, `off` floats behind a 16-byte boundary) inside a buffer of SENTINEL words with GUARD rows
    in front and behind."""

    def __init__(self, M, N, ldy, off=0, y0=None):
        self.M, self.N, self.ldy = M, N, ldy
        self.buf = th.full(((M + 2 * GUARD) * ldy + 4,), SENTINEL, dtype=th.int32, device="cuda")
        self.first = GUARD * ldy + off
        self.idx = (self.first + th.arange(M, device="cuda")[:, None] * ldy + th.arange(N, device="cuda")[None, :]).reshape(-1)
        if y0 is not None:
            self.buf[self.idx] = th.from_numpy(np.ascontiguousarray(y0[:M, :N])).cuda().view(th.int32).reshape(-1)
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 4 * self.first

    def result(self, what):
        """the int32 image [M, N] of the view, after checking that no word outside it changed."""
        th.cuda.synchronize()
        outside = th.ones_like(self.buf, dtype=th.bool)
        outside[self.idx] = False
        moved = (self.buf != self.before) & outside
        if bool(moved.any()):
            w = int(moved.nonzero()[0]) - self.first
            pytest.fail(f"{what}: {int(moved.sum())} words outside Y[{self.M}, {self.N}] were written, first at row {w // self.ldy} column {w % self.ldy}")
        return self.buf[self.idx].view(self.M, self.N).cpu().numpy()

    def untouched(self):
        th.cuda.synchronize()
        return bool((self.buf == self.before).all())


def _call(L, x, w, rm, *, x2=None, rm2=None, bias=None, y0=None, flags=0, transpose=0, ldy=None, off=0, rm2_out=None, what=""):
    """one uavgnn_gemm_nt_h2 (rm2_out: _rm2) launch on views; -> Y [M, N] as fp32 (host).  y0 is given exactly when flags has ACC."""
    M, K1 = x.shape
    N, K = w.shape
    assert (y0 is not None) == bool(flags & ACC) and K == K1 + (0 if x2 is None else x2.shape[1])
    ldy = (N + 3) // 4 * 4 + 4 if ldy is None else ldy
    X = _view(x, 3, 4)
    X2 = None if x2 is None else _view(x2, 3, 8)
    planes = _planes(L, w, transpose)
    y = _Y(M, N, ldy, off, y0)
    dev = lambda a: None if a is None else th.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    rm_d, rm2_d, bias_d = dev(rm), dev(rm2), dev(bias)
    args = (X.data_ptr(), X.stride(0), K1, L.ptr(X2), 0 if X2 is None else X2.stride(0), M, K, rm_d.data_ptr())
    tail = (planes.data_ptr(), N, L.ptr(bias_d), y.ptr, ldy, flags, L.stream())
    if rm2_out is None:
        code = L.lib().uavgnn_gemm_nt_h2(*args, L.ptr(rm2_d), *tail)
    else:
        code = L.lib().uavgnn_gemm_nt_h2_rm2(*args, rm2_out.data_ptr(), *tail)
    L.check(code, what)
    return y.result(what).view(np.float32)


def _reference(x, w, bias=None, y0=None):
    """float64, before the ReLU"""
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    if bias is not None:
        ref = ref + bias.astype(np.float64)[None, :]
    if y0 is not None:
        ref = ref + y0.astype(np.float64)
    return ref


def _check(got, x, w, bx, ref, flags, kernel, family, case, bias=None, y0=None, bw=None, rows=None):
    """every entry (of `rows`) inside the bound against float64; records the worst ratios against r = 1 and r = 4."""
    bw = row_absmax(w) if bw is None else bw
    want = np.maximum(ref, 0.0) if flags & RELU else ref
    sel = slice(None) if rows is None else rows
    with np.errstate(invalid="ignore", over="ignore"):
        ratios = {r: worst_ratio(got[sel], want[sel], nt_bound(x, w, bx, bw, r, ref, bias, y0)[sel]) for r in sorted({1, 4, R_ASSERT})}
    _record(kernel, family, case, ratios[1], ratios[4])
    print(f"{kernel} {family} {case}: worst error / bound {ratios[1]:.3f} (r = 1) {ratios[4]:.3f} (r = 4)")
    assert ratios[R_ASSERT] <= 1.0, f"{kernel} {family} {case}: {ratios[R_ASSERT]:.3f} x the bound (r = {R_ASSERT})"


def _epilogue_operands(pool, M, N, flags):
    bias = None if flags == ACC else pool["bias"][:N]           # bias with plain, ReLU and accumulate + ReLU (as the recorder)
    y0 = pool["y0"][:M, :N] if flags & ACC else None
    return bias, y0


@pytest.mark.parametrize("M,N,K", ONE_SOURCE)
def test_one_source_against_float64(L, pool, M, N, K):
    """uavgnn_gemm_nt_h2 with one source: M in {1, 63, 256, 257, 600} x N in {1, 9, 128, 130, 192, 320} x K in {32, 64, 96} (pruned), both
    uavgnn_split_h2 orientations (ld > C), all four epilogues (bias with plain and ReLU, a random Y0 when accumulating)."""
    x, w = pool["x"][:M, :K], pool["w"][:N, :K]
    bx = row_absmax(x)
    for flags in EPILOGUES:
        bias, y0 = _epilogue_operands(pool, M, N, flags)
        ref = _reference(x, w, bias, y0)
        outs = []
        for transpose in (0, 1):
            case = f"M {M} N {N} K {K} epilogue {flags} transpose {transpose}"
            outs.append(_call(L, x, w, bx, bias=bias, y0=y0, flags=flags, transpose=transpose, what=case))
            _check(outs[-1], x, w, bx, ref, flags, "gemm_nt_h2", "one source", case, bias, y0)
        assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), "the two orientations of uavgnn_split_h2 give different products"


@pytest.mark.parametrize("M,N,K1,K2", TWO_SOURCE)
def test_two_sources_against_float64(L, pool, M, N, K1, K2):
    """two sources, rowmax2 given, X2 a view (ldx2 = K2 + 8), the second source's rows 2^6 above the first's: the row's scale is that of
    max(rowmax, rowmax2), and a scale from rowmax alone would overflow f16."""
    x1, x2, w = pool["x"][:M, :K1], pool["x2"][:M, :K2], pool["w"][:N, :K1 + K2]
    x = np.concatenate([x1, x2], 1)
    rm, rm2 = row_absmax(x1), row_absmax(x2)
    assert np.mean(rm2 > 4.0 * rm) > 0.9
    for flags in EPILOGUES:
        bias, y0 = _epilogue_operands(pool, M, N, flags)
        case = f"M {M} N {N} K1 {K1} K2 {K2} epilogue {flags}"
        got = _call(L, x1, w, rm, x2=x2, rm2=rm2, bias=bias, y0=y0, flags=flags, transpose=flags & 1, what=case)
        _check(got, x, w, np.maximum(rm, rm2), _reference(x, w, bias, y0), flags, "gemm_nt_h2", "two sources", case, bias, y0)


@pytest.mark.parametrize("M,N,K", [(257, 256, 64), (300, 128, 96)])
def test_both_epilogue_paths_on_the_same_product(L, pool, M, N, K):
    """the LDS-tile epilogue (Y 16-byte aligned, ldy % 4 == 0) and the per-element epilogue (ldy = N + 1; Y one float behind a 16-byte
    boundary) evaluate acc * ci * sInv + bv, then + y0, then the ReLU: each inside the bound, the three bit-equal."""
    x, w = pool["x"][:M, :K], pool["w"][:N, :K]
    bx = row_absmax(x)
    for flags in EPILOGUES:
        bias, y0 = _epilogue_operands(pool, M, N, flags)
        ref = _reference(x, w, bias, y0)
        outs = {}
        for path, (ldy, off) in (("tile", (N + 4, 0)), ("ldy = N + 1", (N + 1, 0)), ("Y + 1 float", (N + 4, 1))):
            case = f"M {M} N {N} K {K} epilogue {flags} {path}"
            outs[path] = _call(L, x, w, bx, bias=bias, y0=y0, flags=flags, ldy=ldy, off=off, what=case)
            _check(outs[path], x, w, bx, ref, flags, "gemm_nt_h2", "epilogue paths", case, bias, y0)
        for path in ("ldy = N + 1", "Y + 1 float"):
            diff = outs[path].view(np.int32) != outs["tile"].view(np.int32)
            assert not diff.any(), (f"epilogue {flags}: {int(diff.sum())} entries of the per-element epilogue ({path}) differ from the LDS-tile "
                                    f"epilogue, first at {tuple(int(v) for v in np.argwhere(diff)[0])}")


@pytest.mark.parametrize("shape", ONE_SOURCE + TWO_SOURCE, ids=lambda s: "-".join(map(str, s)))
def test_interleaved_staging_is_bit_equal(L, pool, shape):
    """epilogue | UAVGNN_GEMM_STAGING_INTERLEAVED (the IL instantiation: the split's steps placed between the MFMAs by hand) == the default
    loop, bit for bit - the term order over K is the same: every case of the two lists at one epilogue each, (257, 192, 64) at all four."""
    if len(shape) == 3:
        M, N, K = shape
        x1, x2, rm2 = pool["x"][:M, :K], None, None
    else:
        M, N, K1, K2 = shape
        x1, x2, K = pool["x"][:M, :K1], pool["x2"][:M, :K2], K1 + K2
        rm2 = row_absmax(x2)
    w, rm = pool["w"][:N, :K], row_absmax(x1)
    n = (ONE_SOURCE + TWO_SOURCE).index(shape)
    for flags in (EPILOGUES if shape == (257, 192, 64) else (EPILOGUES[n % 4],)):
        bias, y0 = _epilogue_operands(pool, M, N, flags)
        outs = [_call(L, x1, w, rm, x2=x2, rm2=rm2, bias=bias, y0=y0, flags=flags | il, what=f"{shape} epilogue {flags | il}") for il in (0, IL)]
        if flags == 0 and x2 is None:      # (that the flag's launch computed the product, not only the same bits)
            _check(outs[1], x1, w, rm, _reference(x1, w, bias, y0), flags, "gemm_nt_h2", "interleaved staging", f"{shape}", bias, y0)
        diff = outs[0].view(np.int32) != outs[1].view(np.int32)
        assert not diff.any(), f"{shape} epilogue {flags}: {int(diff.sum())} entries differ, first at {tuple(int(v) for v in np.argwhere(diff)[0])}"


@pytest.mark.parametrize("M", [1, 257, 600])
@pytest.mark.parametrize("K2", [32, 96])
def test_rm2_takes_the_row_maxima_itself(L, pool, M, K2):
    """uavgnn_gemm_nt_h2_rm2: rowmax2_out == uavgnn_row_absmax(X2) bit for bit, rows at and behind M of a longer buffer keep the sentinel,
    Y is bit-equal to the call that is handed those maxima; a row of X2 holding Inf and one holding NaN get an Inf bound and a NaN row of
    Y - there and only there."""
    K1, N = 64, 192
    x1, w = pool["x"][:M, :K1], pool["w"][:N, :K1 + K2]
    x2 = pool["x2"][:M, :K2].copy()
    bad = np.array([r for r in (3, 200) if r < M], dtype=np.int64)
    if M > 3:
        x2[3, K2 - 1] = np.inf
    if M > 200:
        x2[200, 0] = np.nan
    rm, bias = row_absmax(x1), pool["bias"][:N]
    X2 = _view(x2, 3, 8)
    want = th.full((M,), -1.0, device="cuda")
    L.check(L.lib().uavgnn_row_absmax(X2.data_ptr(), X2.stride(0), K2, None, 0, 0, None, 0, 0, M, want.data_ptr(), L.stream()), "row_absmax")
    out = th.full((M + 5,), SENTINEL, dtype=th.int32, device="cuda").view(th.float32)
    got = _call(L, x1, w, rm, x2=x2, bias=bias, rm2_out=out, what=f"rm2 M {M} K2 {K2}")
    assert th.equal(out.view(th.int32)[M:], th.full((5,), SENTINEL, dtype=th.int32, device="cuda")), "rowmax2_out was written behind row M"
    assert th.equal(out.view(th.int32)[:M], want.view(th.int32)), "rowmax2_out differs from uavgnn_row_absmax(X2)"
    rm2 = want.cpu().numpy()
    assert np.all(np.isinf(rm2[bad])) and np.isfinite(np.delete(rm2, bad)).all()
    handed = _call(L, x1, w, rm, x2=x2, rm2=rm2, bias=bias, what=f"nt with the maxima, M {M} K2 {K2}")
    assert np.array_equal(got.view(np.int32), handed.view(np.int32)), "Y differs from the call that is handed the maxima"
    clean = np.setdiff1d(np.arange(M), bad)
    assert np.isnan(got[bad]).all() and np.isfinite(got[clean]).all()
    x, bx = np.concatenate([x1, x2], 1), np.maximum(rm, rm2)
    x[bad], bx[bad] = 0.0, 0.0             # (left out of the bound below)
    _check(got, x, w, bx, _reference(x, w, bias), 0, "gemm_nt_h2_rm2", "own row maxima", f"M {M} K2 {K2}", bias, rows=clean)


def test_contract_rows(L, pool):
    """M = 257, N = 192, K = 64, bias.  A row of X holding Inf and one holding NaN under an Inf bound: all NaN, every other row finite and
    inside the bound - with the plain epilogue and behind the ReLU on both epilogue paths (a ReLU that is fmaxf(v, 0) alone answers a NaN
    with 0: the kernel had it so, and a poisoned row left a ReLU layer as zeros).  A bound 2^-8 too small on one row (f16 overflow): NaN in that row, none of its entries a
    finite wrong number, the other rows bit-equal to the clean call.  A bound 2^5 too large on every row: inside the bound computed with
    that bound.  An all-zero row with bound 0: exactly the bias."""
    M, N, K = 257, 192, 64
    x, w, bias = pool["x"][:M, :K].copy(), pool["w"][:N, :K], pool["bias"][:N]
    bx = row_absmax(x)
    ref = _reference(x, w, bias)
    clean = _call(L, x, w, bx, bias=bias, what="contract: clean")
    # non-finite rows (row 256 is the clamped row tile's only row)
    xn, bn = x.copy(), bx.copy()
    xn[7, 11], xn[256, 63] = np.inf, np.nan
    bn[[7, 256]] = np.inf
    got = _call(L, xn, w, bn, bias=bias, what="contract: non-finite rows")
    rest = np.setdiff1d(np.arange(M), [7, 256])
    assert np.isnan(got[[7, 256]]).all() and np.isfinite(got[rest]).all()
    assert np.array_equal(got[rest].view(np.int32), clean[rest].view(np.int32))
    _check(got, x, w, bx, ref, 0, "gemm_nt_h2", "contract", "non-finite rows: the others", bias, rows=rest)
    for flags, path in ((RELU, dict()), (RELU, dict(ldy=N + 1)), (ACC | RELU, dict(y0=pool["y0"][:M, :N]))):      # the ReLU keeps the NaN
        got = _call(L, xn, w, bn, bias=bias, flags=flags, what=f"contract: non-finite rows, epilogue {flags}", **path)
        assert np.isnan(got[[7, 256]]).all(), f"epilogue {flags} {path.keys()}: the ReLU turned a NaN row into numbers"
        assert np.isfinite(got[rest]).all()
    # a bound too small
    bs = bx.copy()
    bs[100] *= np.float32(2.0 ** -8)
    got = _call(L, x, w, bs, bias=bias, what="contract: small bound")
    rest = np.setdiff1d(np.arange(M), [100])
    assert np.isnan(got[100]).any(), "a row bound 2^-8 too small gave no NaN"
    fin = np.isfinite(got[100])
    bound = nt_bound(x, w, bx, row_absmax(w), R_ASSERT, ref, bias)
    assert np.all(np.abs(got[100][fin] - ref[100][fin]) <= bound[100][fin]), "a finite wrong number under a row bound that is too small"
    print(f"contract, bound 2^-8 too small: {int((~fin).sum())} of {N} entries of the row are not finite, {int(np.isnan(got[100]).sum())} NaN")
    assert np.array_equal(got[rest].view(np.int32), clean[rest].view(np.int32))
    got = _call(L, x, w, bs, bias=bias, flags=RELU, what="contract: small bound, ReLU")
    assert np.isnan(got[100]).any() and np.isfinite(got[rest]).all(), "ReLU epilogue: a row bound 2^-8 too small gave no NaN"
    # a bound too large
    bl = bx * np.float32(32.0)
    got = _call(L, x, w, bl, bias=bias, what="contract: large bound")
    _check(got, x, w, bl, ref, 0, "gemm_nt_h2", "contract", "bound 2^5 too large", bias)
    # an all-zero row under the bound 0
    xz, bz = x.copy(), bx.copy()
    xz[[0, 130, 256]], bz[[0, 130, 256]] = 0.0, 0.0
    for flags in (0, RELU):
        got = _call(L, xz, w, bz, bias=bias, flags=flags, what="contract: zero rows")
        want = np.maximum(bias, 0.0) if flags else bias
        assert all(np.array_equal(got[r].view(np.int32), want.view(np.int32)) for r in (0, 130, 256))
        _check(got, xz, w, bz, _reference(xz, w, bias), flags, "gemm_nt_h2", "contract", f"zero rows, epilogue {flags}", bias)


@pytest.mark.parametrize("case", ["benign", "rows at 2^-100", "rows at 2^100", "in-row range 2^+-30", "weight rows 2^+-12 apart"])
def test_operand_ranges(L, case):
    """M = 300, N = 130, K = 96, no bias: whole rows near the ends of fp32's range (the scale exponent moves, nothing else), elements
    2^60 apart inside a row (the small ones live on the floor of the large), weight rows 2^24 apart (each has its own scale) - per entry;
    on plain normal operands additionally the project's aggregate bar, max < 4e-7 and mean < 4e-8 of |err| / sum |a b|."""
    M, N, K = 300, 130, 96
    rng = np.random.default_rng(9522)
    x, w = rng.standard_normal((M, K)), 0.1 * rng.standard_normal((N, K))
    if case == "rows at 2^-100":
        x = x * 2.0 ** -100
    elif case == "rows at 2^100":
        x = x * 2.0 ** 100
    elif case == "in-row range 2^+-30":
        x = x * np.exp2(rng.integers(-30, 31, (M, K)))
    elif case == "weight rows 2^+-12 apart":
        w = w * np.exp2(rng.integers(-12, 13, (N, 1)))
    x, w = x.astype(np.float32), w.astype(np.float32)
    bx = row_absmax(x)
    got = _call(L, x, w, bx, what=case)
    ref = _reference(x, w)
    assert np.isfinite(got).all()
    _check(got, x, w, bx, ref, 0, "gemm_nt_h2", "operand ranges", case)
    if case == "benign":
        e = np.abs(got.astype(np.float64) - ref) / (np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T)
        print(f"benign: |err| / sum |a b| max {e.max():.2e} mean {e.mean():.2e}")
        assert e.max() < 4e-7 and e.mean() < 4e-8


@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("K,N", [(64, 64), (64, 192), (128, 128), (128, 64), (192, 192), (192, 128)])
def test_n64_kernel_against_float64_and_the_wide_kernel(L, pool, M, K, N):
    """uavgnn_gemm_nt_h2_n64 (128 x 64 tiles): M in {1, 127, 128, 129, 300} x K in {64, 128, 192} x N in {64, 128, 192}; ldx = K + 4,
    ldy = N + 4, guard bands; per entry against float64, and every column bit-equal to uavgnn_gemm_nt_h2 on the same operands (the header's
    promise: the same accumulation order over K)."""
    x, w = pool["x"][:M, :K], pool["w"][:N, :K]
    bx = row_absmax(x)
    X, planes, y = _view(x, 3, 4), _planes(L, w, 0), _Y(M, N, N + 4)
    rm = th.from_numpy(bx).cuda()
    case = f"M {M} N {N} K {K}"
    L.check(L.lib().uavgnn_gemm_nt_h2_n64(X.data_ptr(), X.stride(0), M, K, rm.data_ptr(), planes.data_ptr(), N, y.ptr, N + 4, L.stream()), case)
    got = y.result("n64 " + case).view(np.float32)
    _check(got, x, w, bx, _reference(x, w), 0, "gemm_nt_h2_n64", "n64", case)
    wide = _call(L, x, w, bx, what="wide kernel " + case)
    diff = got.view(np.int32) != wide.view(np.int32)
    assert not diff.any(), f"{case}: {int(diff.sum())} entries differ from uavgnn_gemm_nt_h2, first at {tuple(int(v) for v in np.argwhere(diff)[0])}"


def test_argument_table(L, pool):
    """the return codes of include/uavgnn.h; a refused call and M == 0 write nothing to Y (nor to rowmax2_out)."""
    lib = L.lib()
    M, N, K = 8, 64, 64
    X = _view(pool["x"][:M, :128], 3, 4)                     # ldx = 132
    X2 = _view(pool["x2"][:M, :64], 3, 8)
    planes = _planes(L, pool["w"][:N, :K], 0)
    rm = th.from_numpy(row_absmax(pool["x"][:M, :128])).cuda()
    rm_out = th.full((M,), SENTINEL, dtype=th.int32, device="cuda")
    y = _Y(M, N, N + 4)
    st = L.stream()
    x, x2, r, p, ldx, ldx2, ldy = X.data_ptr(), X2.data_ptr(), rm.data_ptr(), planes.data_ptr(), X.stride(0), X2.stride(0), N + 4

    def nt(X_=x, ldx_=ldx, K1=K, X2_=None, ldx2_=0, M_=M, K_=K, rm_=r, rm2=None, N_=N, Y=y.ptr, ldy_=ldy, flags=0):
        return lib.uavgnn_gemm_nt_h2(X_, ldx_, K1, X2_, ldx2_, M_, K_, rm_, rm2, p, N_, None, Y, ldy_, flags, st)

    def rm2(X2_=x2, out=rm_out.data_ptr(), K1=32, M_=M):
        return lib.uavgnn_gemm_nt_h2_rm2(x, ldx, K1, X2_, ldx2, M_, K, r, out, p, N, None, y.ptr, ldy, 0, st)

    def n64(X_=x, ldx_=ldx, M_=M, K_=K, N_=N, Y=y.ptr, ldy_=ldy, rm_=r):
        return lib.uavgnn_gemm_nt_h2_n64(X_, ldx_, M_, K_, rm_, p, N_, Y, ldy_, st)
    unsupported = {"K % 32": nt(K1=48, K_=48), "K1 % 32 with a second source": nt(K1=16, X2_=x2, ldx2_=ldx2), "ldx % 4": nt(ldx_=ldx + 1),
                   "X misaligned": nt(X_=x + 4), "TILE_128": nt(flags=TILE_128), "TILE_64": nt(flags=RELU | TILE_64),
                   "ldx2 % 4": nt(K1=32, X2_=x2, ldx2_=ldx2 + 2), "X2 misaligned": nt(K1=32, X2_=x2 + 8, ldx2_=ldx2),
                   "n64: N % 64": n64(N_=32), "n64: K % 64": n64(K_=32), "n64: ldy % 4": n64(ldy_=ldy + 1), "n64: Y misaligned": n64(Y=y.ptr + 4),
                   "n64: ldx % 4": n64(ldx_=ldx + 2), "n64: X misaligned": n64(X_=x + 8)}
    invalid = {"rowmax NULL": nt(rm_=None), "X2 NULL with K1 < K": nt(K1=32), "X2 with K1 == K": nt(X2_=x2, ldx2_=ldx2), "ldy < N": nt(ldy_=N - 1),
               "ldx < K1": nt(ldx_=K - 4), "ldx2 < K2": nt(K1=32, X2_=x2, ldx2_=28), "M < 0": nt(M_=-1),
               "rm2: rowmax2_out NULL": rm2(out=None), "rm2: X2 NULL": rm2(X2_=None), "n64: rowmax NULL": n64(rm_=None), "n64: ldy < N": n64(ldy_=N - 4)}
    assert {k: v for k, v in unsupported.items() if v != EUNSUPPORTED} == {}
    assert {k: v for k, v in invalid.items() if v != EINVAL} == {}
    assert nt(M_=0) == 0 and rm2(M_=0) == 0 and n64(M_=0) == 0
    assert y.untouched() and bool((rm_out == SENTINEL).all())
    # ... and the same pointers and sizes are a valid call
    assert nt() == 0 and rm2() == 0 and n64() == 0
    y.result("the valid calls")

"""The f16x2 arithmetic of the NT products Y = X B^T (csrc/gemm_h2.hip: uavgnn_gemm_nt_h2, _rm2, _n64; the contractions of
csrc/gru_h2.hip) restated in NumPy (CPU, no GPU needed), and the per-entry error bound the GPU tests of
tests/test_f16x2_nt_edges_gpu.py and tests/test_gru_cell_h2_edges_gpu.py assert against float64.

Row i of the activation operand X is split under the caller's bound bx_i (scale s_i = 2^scale_exp(bx_i)), output row j of the weight B
under bw_j = max_k |b_jk| (split_h2_kernel): hi = f16(v s), lo = f16(v s - hi), f16 subnormals kept (`split_f16x2` of
tests/test_f16x2_emulation.py, whose derivation of the split terms this file uses).  The kernel forms x_hi b_lo + x_lo b_hi + x_hi b_hi
on v_mfma_f32_32x32x16_f16 (x_lo b_lo dropped), accumulates in fp32 and un-scales by two exact powers of two.  Per entry (i, j):

    |y - ref| <= A(K, r) sum_k |x_ik b_jk|  +  B_FLOOR (bx_i sum_k |b_jk| + bw_j sum_k |x_ik|)  +  E_epi

Derivation (u = x s_i, w = b s_j the scaled values; d = u - (hi + lo), |d| <= 2^-22 |u| + 2^-25, |lo| <= 2^-11 |u| + 2^-25):
  * the split, exactly as for the weight gradient (the roles of the two operands are symmetric): the three kept products differ from
    u w by -d_u w - u d_w + d_u d_w - lo_u lo_w, bounded by A_SPLIT |u w| + (2^-25 + 2^-36 + 2^-47)(|u| + |w|); un-scaled, with
    1 / s <= 2^-14 x bound, the absolute part is <= B_FLOOR per unit of (bx_i |b_jk| + bw_j |x_ik|).  A bound bx_i LARGER than the row's
    maximum (a producer's bound is tight only to within its power of two; the contract test passes one 2^5 too large) only moves the
    scale: the relative part is unchanged and the floor grows with bx_i - the same formula with the bound that was passed;
  * the fp32 accumulation: every f16 x f16 product is exact in fp32.  One 16-long MFMA step adds 16 products to the accumulator with r
    roundings (the instruction's internal order is not documented: r = 1, one rounding per step, is the model of the weight-gradient
    emulation; r = 4, a 16-long dot product in four groups of four, is the most the instruction can have); 3 K / 16 steps per entry,
    each rounding <= 2^-24 of a partial sum that is <= sum_k |u w| (1 + 2^-10):  A(K, r) = A_SPLIT + r (3 K / 16) 2^-24;
  * the epilogue: acc x 2^-e_col x 2^-e_row is exact unless the result leaves the normal range; the bias add and the accumulate round
    once each: <= 2^-24 (|ref| + |y0|) + 2^-24 |ref|, and one more 2^-24 |p| <= 2^-24 (|ref| + |bias| + |y0|) covers an un-scaling
    that rounds:  E_epi = 2^-23 (|ref| + |bias_j| + |y0_ij|), ref the float64 value before the ReLU (|relu(a) - relu(b)| <= |a - b|).

What the emulation shows on ladder operands (normal x 2^-(0 .. 30) per element, x 2^(-6 .. 6) per row - the recorder's pattern) at
(M, N, K) = (257, 192, 32), (257, 192, 64), (300, 130, 160), (300, 130, 768), seeded as below:
  * the exact model (the split alone) reaches 0.30 .. 0.48 of the r = 0 bound (A_SPLIT, floor, epilogue);
  * the in-order fp32 model (one rounding per term and step) reaches 0.08 .. 0.38 of the r = 1 bound, 0.02 .. 0.26 of the r = 4 bound;
  * dropping x_hi b_lo or x_lo b_hi exceeds the r = 4 bound 12 to 207 times; flushing f16 subnormals 30 to 216 times at K <= 64 (at
    larger K the accumulation's share of the bound grows past what the flushed elements carry: 0.7 at K = 160);
  * the project's aggregate bar max |err| / sum |a b| < 4e-7 is not a property of these operands: the exact model gives 2.5e-7 ..
    2.3e-5 on them (an entry of small products sits on the floor of its row's large elements), 7e-8 on plain normal operands - the
    floor term is needed here, and the aggregate bar belongs to benign operands.
R_ASSERT is the r the GPU tests assert with.  profiles/f16x2_nt_edges.txt holds what the MI355X gave against r = 1 and r = 4: every
case of every kernel stays inside the r = 1 bound (worst 0.47), so the one-rounding-per-step model of the weight-gradient emulation
also holds for v_mfma_f32_32x32x16_f16, and the asserted r is 2 - twice the model that was measured, not the measured value."""
import numpy as np
import pytest

from tests.test_f16x2_emulation import A_SPLIT, B_FLOOR, scale_exp, split_f16x2

R_ASSERT = 2          # roundings per 16-long MFMA step in the asserted bound (see profiles/f16x2_nt_edges.txt)
SHAPES = [(257, 192, 32), (257, 192, 64), (300, 130, 160), (300, 130, 768)]
TERMS = ((0, 1), (1, 0), (0, 0))      # UAVGNN_H2_TERM(ia, ib) in the kernel's order: x_hi b_lo, x_lo b_hi, x_hi b_hi


def ladder(rng, rows, cols):
    """[rows, cols] fp32: normal x 2^-(0 .. 30) per element, x 2^(-6 .. 6) per row (tools/record_f16x2_golden.py's pattern)."""
    v = rng.standard_normal((rows, cols)) * np.exp2(-rng.integers(0, 31, (rows, cols)))
    return (v * np.exp2(rng.integers(-6, 7, (rows, 1)))).astype(np.float32)


def row_absmax(a):
    return np.abs(a).max(1).astype(np.float32)


def split_rows(v, bounds, ftz=False):
    """planes [2][rows][cols] (f16 as float64: hi, lo) and the scales [rows] of a matrix whose row i is split under bounds[i]."""
    planes = np.empty((2,) + v.shape, dtype=np.float64)
    s = np.empty(v.shape[0], dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(v.shape[0]):
            planes[0, i], planes[1, i], s[i] = split_f16x2(v[i], bounds[i], ftz)
    return planes, s


def model_nt(x, w, bx, bw, ftz=False, drop=None):
    """x w^T by the kernel's split and three products, summed exactly (float64: every f16 x f16 product is exact) and un-scaled.
    drop: the index into TERMS of a product to leave out; ftz: f16 subnormals flushed - arithmetic the kernel must NOT have."""
    px, sx = split_rows(x, bx, ftz)
    pw, sw = split_rows(w, bw, ftz)
    with np.errstate(over="ignore", invalid="ignore"):
        P = sum(px[ia] @ pw[ib].T for t, (ia, ib) in enumerate(TERMS) if t != drop)
        return P / sx[:, None] / sw[None, :]


def model_nt_fp32(x, w, bx, bw):
    """... in the kernel's order: per 16-wide K step the terms x_hi b_lo, x_lo b_hi, x_hi b_hi, each step's 16 products summed exactly
    and rounded once into the fp32 accumulator (r = 1)."""
    px, sx = split_rows(x, bx)
    pw, sw = split_rows(w, bw)
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=np.float32)
    for k0 in range(0, x.shape[1], 16):
        k = slice(k0, k0 + 16)
        for ia, ib in TERMS:
            acc = (acc.astype(np.float64) + px[ia][:, k] @ pw[ib][:, k].T).astype(np.float32)
    return acc.astype(np.float64) / sx[:, None] / sw[None, :]


def nt_bound(x, w, bx, bw, r, ref, bias=None, y0=None):
    """[M, N] bound of the docstring; `ref`: the float64 result before the ReLU (bias and y0 included)."""
    ax, aw = np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64))
    a = A_SPLIT + r * (3 * x.shape[1] / 16) * 2.0 ** -24
    epi = np.abs(ref)
    if bias is not None:
        epi = epi + np.abs(bias.astype(np.float64))[None, :]
    if y0 is not None:
        epi = epi + np.abs(y0.astype(np.float64))
    floor = np.asarray(bx, dtype=np.float64)[:, None] * aw.sum(1)[None, :] + np.asarray(bw, dtype=np.float64)[None, :] * ax.sum(1)[:, None]
    return a * (ax @ aw.T) + B_FLOOR * floor + 2.0 ** -23 * epi


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an entry that is not a number, or wrong where the bound is zero, counts as infinite."""
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got.astype(np.float64) - ref)
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return float(ratio.max()) if ratio.size else 0.0


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    M, N, K = request.param
    rng = np.random.default_rng(M * 1000 + K)
    x, w = ladder(rng, M, K), ladder(rng, N, K)
    bx, bw = row_absmax(x), row_absmax(w)
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    return dict(K=K, x=x, w=w, bx=bx, bw=bw, ref=ref, bound={r: nt_bound(x, w, bx, bw, r, ref) for r in (0, 1, 4)})


def test_scale_puts_the_row_bound_into_the_f16_range(case):
    """2^scale_exp(b) b lies in [2^14, 2^15) for the bounds of both operands: the largest scaled magnitude is finite in f16."""
    for b in (case["bx"], case["bw"]):
        u = b.astype(np.float64) * np.exp2(scale_exp(b).astype(np.float64))
        assert np.all((u >= 2.0 ** 14) & (u < 2.0 ** 15))


def test_both_models_stay_inside_the_bound_with_room(case):
    """at least 2 x of room everywhere: the exact model against the r = 0 bound (0.30 .. 0.48: the split's share is a worst case of a
    few terms and is nearly attained) and the in-order fp32 model against r = 1 (0.08 .. 0.38) and r = 4 (0.02 .. 0.26)."""
    c = case
    exact = model_nt(c["x"], c["w"], c["bx"], c["bw"])
    fp32 = model_nt_fp32(c["x"], c["w"], c["bx"], c["bw"])
    e0, e4 = worst_ratio(exact, c["ref"], c["bound"][0]), worst_ratio(exact, c["ref"], c["bound"][4])
    f1, f4 = worst_ratio(fp32, c["ref"], c["bound"][1]), worst_ratio(fp32, c["ref"], c["bound"][4])
    print(f"K {c['K']}: exact / r0 {e0:.3f}  exact / r4 {e4:.3f}  fp32 / r1 {f1:.3f}  fp32 / r4 {f4:.3f}")
    assert e0 <= 0.5 and e4 <= 0.5
    assert f1 <= 0.5 and f4 <= 0.5
    assert worst_ratio(fp32, c["ref"], nt_bound(c["x"], c["w"], c["bx"], c["bw"], R_ASSERT, c["ref"])) <= 0.5      # the asserted r


@pytest.mark.parametrize("drop", [0, 1])
def test_a_dropped_cross_term_breaks_the_bound(case, drop):
    """without x_hi b_lo (drop = 0) or x_lo b_hi (drop = 1) the error is 2^-11 of the product: 10 to 225 times the r = 4 bound."""
    c = case
    ratio = worst_ratio(model_nt(c["x"], c["w"], c["bx"], c["bw"], drop=drop), c["ref"], c["bound"][4])
    print(f"K {c['K']} drop {drop}: {ratio:.1f} x the r = 4 bound")
    assert ratio >= 8.0            # (12 at K = 768, where the accumulation's share of the bound is largest)


def test_flushed_f16_subnormals_break_the_bound(case):
    """an f16 arithmetic without subnormals loses the elements below 2^-28 of their row bound: 30 to 216 times the r = 4 bound at
    K <= 64 (the contractions the GPU tests run); at K = 160 and 768 the accumulation's share of the bound has outgrown them."""
    c = case
    ratio = worst_ratio(model_nt(c["x"], c["w"], c["bx"], c["bw"], ftz=True), c["ref"], c["bound"][4])
    print(f"K {c['K']} ftz: {ratio:.1f} x the r = 4 bound")
    if c["K"] <= 64:
        assert ratio >= 20.0


def test_a_row_bound_too_small_gives_no_number(case):
    """one row's bound 2^-8 too small: its largest elements overflow f16, hi = Inf and lo = -Inf, and every entry of that row is NaN or
    Inf - outside any bound; the other rows are the clean model's."""
    c = case
    bx = c["bx"].copy()
    bx[5] *= np.float32(2.0 ** -8)
    got = model_nt(c["x"], c["w"], bx, c["bw"])
    assert not np.isfinite(got[5]).any()
    assert worst_ratio(got, c["ref"], c["bound"][4]) == np.inf
    clean = model_nt(c["x"], c["w"], c["bx"], c["bw"])
    keep = np.arange(len(bx)) != 5
    assert np.array_equal(got[keep], clean[keep])


def test_a_row_bound_too_large_moves_the_floor_only(case):
    """a bound 2^5 above the row maximum on every row: inside the bound computed with THAT bound, which the floor term carries."""
    c = case
    bx = c["bx"] * np.float32(32.0)
    got = model_nt(c["x"], c["w"], bx, c["bw"])
    assert worst_ratio(got, c["ref"], nt_bound(c["x"], c["w"], bx, c["bw"], 0, c["ref"])) <= 0.62


def test_the_aggregate_bar_belongs_to_benign_operands():
    """max |err| / sum |a b| < 4e-7 (tests/test_gpu_parity.py) holds for the exact model on plain normal operands with room (7e-8); on
    the ladder it does not (2.3e-5 at K = 32): there an entry of small products sits on the floor of its row's large elements."""
    rng = np.random.default_rng(7)

    def aggregate(x, w):
        ref = x.astype(np.float64) @ w.astype(np.float64).T
        den = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
        return float((np.abs(model_nt(x, w, row_absmax(x), row_absmax(w)) - ref) / den).max())
    benign = aggregate(rng.standard_normal((257, 64)).astype(np.float32), rng.standard_normal((192, 64)).astype(np.float32))
    worst = max(aggregate(ladder(rng, M, K), ladder(rng, N, K)) for M, N, K in SHAPES[:3])
    print(f"max |err| / sum |a b|: benign {benign:.2e}, ladder {worst:.2e}")
    assert benign < 2e-7 and worst > 4e-7

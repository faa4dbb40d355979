"""The f16x2 arithmetic of csrc/f16x2.h (`scale_exp`, `split_pair`), as csrc/gemm_tn_h2.hip uses it for the weight gradient
dW = dY^T X, restated in NumPy (CPU, no GPU needed), and the
error floor of its column bounds.  The kernel splits every element v of a column whose bound is B into two f16 terms at a power-of-two
scale s with B s in [2^14, 2^15) (`scale_exp`): hi = f16(v s), lo = f16(v s - hi), f16 subnormals kept; it forms hi hi + hi lo + lo hi
on the matrix cores (lo lo dropped) and accumulates in fp32.  The learner passes ONE bound per operand (WeightGradSink.end_sequence:
the maximum of the producers' row maxima), so a column far below that bound is held with fewer bits.  Per entry:

    |dW - ref| <= A sum_r |dy_r||x_r|  +  B_FLOOR (B_y sum_r |x_r| + B_x sum_r |dy_r|)

Derivation (u = v s, f16: 11 significant bits, smallest subnormal 2^-24, so a rounding error is <= 2^-11 |.| or <= 2^-25):
  * hi = f16(u): |u - hi| <= 2^-11 |u|  (|u| >= 2^-14)  or  <= 2^-25  (hi subnormal, |u| < 2^-14);  r = u - hi is exact in fp32;
  * lo = f16(r): |r - lo| <= 2^-11 |r| <= 2^-22 |u|  or  <= 2^-25;  so  d = u - (hi + lo)  has  |d| <= 2^-22 |u| + 2^-25,
    and |lo| <= 2^-11 |u| + 2^-25 (lo != 0 needs |u| >= 2^-14);
  * one row's products: yhat xhat - lo_y lo_x - u_y u_x = -d_y u_x - u_y d_x + d_y d_x - lo_y lo_x, bounded by
    3 (2^-22 + 2^-44) |u_y u_x|  +  (2^-25 + 2^-36 + 2^-47) (|u_y| + |u_x|)   (|d| <= |u| and |u| >= 2^-14 where lo != 0 absorb the rest);
  * unscaled (divide by s_y s_x, 1 / s <= 2^-14 B):  A_SPLIT = 3 (2^-22 + 2^-44) ~ 1.5 x 2^-21,  and the absolute term
    (2^-25 + 2^-35) 2^-14 = 2^-39 (1 + 2^-10) per unit of B |.|  <=  B_FLOOR = 2^-38 (a factor 2 of margin);
  * a value below 2^-25 / s ~ 2^-39 B flushes to 0 (both terms): its whole contribution is the B_FLOOR term.
The kernel then accumulates the three products in fp32 (MFMA chains over 512-row chunks, then a fixed-order sum of the chunk partials):
A_GPU = 2^-20 = A_SPLIT + 2^-22 for that rounding.  The fp32 share is not a worst-case bound; 2^-22 of sum |dy||x| is what the
accumulation reaches on these operands (emulated below in the kernel's order, and measured on the GPU by
test_gemm_tn_f16x2_weight_gradient_vs_float64: <= 4e-7 ~ 1.7 x 2^-22 for the split AND the accumulation together).
A caller that needs a small column exact passes its own bound (uavgnn_col_absmax) - INTEGRATION.md.
The GPU check of the kernel against this bound: tests/test_gpu_parity.py::test_gemm_tn_f16x2_global_bound_column_ladder."""
import numpy as np

A_SPLIT = 3 * (2.0 ** -22 + 2.0 ** -44)
A_GPU = 2.0 ** -20
B_FLOOR = 2.0 ** -38
LADDER = (17, 24, 30, 40)       # columns 2^-k below the operand's global bound


def scale_exp(amax):
    """csrc/f16x2.h scale_exp: 2^se * amax in [2^14, 2^15), clamped to the normal range (amax: fp32)."""
    e = ((np.asarray(amax, dtype=np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    return np.clip(14 - (e - 127), -126, 126)


def split_f16x2(v, bound, ftz=False):
    """(hi, lo, s) of fp32 values v under ONE bound: hi = f16(v s), lo = f16(v s - hi) (f16 subnormals kept; ftz=True flushes them,
    the arithmetic the kernel must NOT have)."""
    s = np.float32(2.0 ** float(scale_exp(np.float32(bound))))
    u = (np.asarray(v, dtype=np.float32) * s).astype(np.float32)
    hi = u.astype(np.float16)
    if ftz:
        hi = np.where(np.abs(hi) < 2.0 ** -14, np.float16(0), hi)
    r = (u - hi.astype(np.float32)).astype(np.float32)
    lo = r.astype(np.float16)
    if ftz:
        lo = np.where(np.abs(lo) < 2.0 ** -14, np.float16(0), lo)
    return hi, lo, s


def model_dw(dy, x, B_y, B_x, ftz=False):
    """dy^T x by the kernel's split and three products, summed exactly (float64: every f16 x f16 product is exact)."""
    hy, ly, sy = split_f16x2(dy, B_y, ftz)
    hx, lx, sx = split_f16x2(x, B_x, ftz)
    f = lambda t: t.astype(np.float64)   # noqa: E731
    P = f(hy).T @ f(hx) + f(hy).T @ f(lx) + f(ly).T @ f(hx)
    return P / (float(sy) * float(sx))


def model_dw_fp32(dy, x, B_y, B_x, chunk=512):
    """... with the kernel's fp32 accumulation: per 512-row chunk, per 16-row MFMA step the terms hi lo, lo hi, hi hi (each step's 16
    products summed, then one fp32 rounding into the accumulator), the chunk partials summed in fp32."""
    hy, ly, sy = split_f16x2(dy, B_y)
    hx, lx, sx = split_f16x2(x, B_x)
    f = lambda t: t.astype(np.float64)   # noqa: E731
    total = np.zeros((dy.shape[1], x.shape[1]), dtype=np.float32)
    for c0 in range(0, dy.shape[0], chunk):
        acc = np.zeros_like(total)
        for k0 in range(c0, min(c0 + chunk, dy.shape[0]), 16):
            k = slice(k0, k0 + 16)
            for a, b in ((hy, lx), (ly, hx), (hy, hx)):
                acc = (f(acc) + f(a[k]).T @ f(b[k])).astype(np.float32)
        total = (total + acc).astype(np.float32)
    return total.astype(np.float64) / (float(sy) * float(sx))


def ladder_operands(n, Mo, Ko, seed):
    """dY [n, Mo] (signed, row scales over 2^-14..1 as the gate gradients have) and X [n, Ko] (ReLU outputs) in fp32; columns
    1 + 5 j .. 4 + 5 j carry the LADDER (2^-17 .. 2^-40 below the column 0 + 5 j at full scale).  The bound is the global maximum."""
    rng = np.random.default_rng(seed)
    dy = (rng.standard_normal((n, Mo)) * np.exp2(rng.integers(-14, 1, (n, 1))) * 1e-3).astype(np.float32)
    x = np.maximum(rng.standard_normal((n, Ko)), 0).astype(np.float32)
    for i, k in enumerate(LADDER):
        dy[:, 1 + i::5] *= np.float32(2.0 ** -k)
        x[:, 1 + i::5] *= np.float32(2.0 ** -k)
    return dy, x


def derived_bound(dy, x, B_y, B_x, a):
    dy, x = np.abs(dy.astype(np.float64)), np.abs(x.astype(np.float64))
    return a * (dy.T @ x) + B_FLOOR * (B_y * x.sum(0)[None, :] + B_x * dy.sum(0)[:, None])


def test_split_terms_meet_the_derivation():
    """per element: |u - (hi + lo)| <= 2^-22 |u| + 2^-25, |lo| <= 2^-11 |u| + 2^-25, and the three kept products are exact in fp32."""
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(400000) * np.exp2(rng.integers(-45, 1, 400000))).astype(np.float32)
    B = np.float32(np.abs(v).max())
    hi, lo, s = split_f16x2(v, B)
    u = v.astype(np.float64) * float(s)
    assert 2.0 ** 14 <= float(B) * float(s) < 2.0 ** 15
    d = np.abs(u - (hi.astype(np.float64) + lo.astype(np.float64)))
    assert np.all(d <= 2.0 ** -22 * np.abs(u) + 2.0 ** -25)
    assert np.all(np.abs(lo.astype(np.float64)) <= 2.0 ** -11 * np.abs(u) + 2.0 ** -25)
    assert np.any((hi != 0) & (np.abs(hi.astype(np.float64)) < 2.0 ** -14))          # f16 subnormals occur and are kept
    h2 = hi[::-1]
    for p, q in ((hi, h2), (hi, lo[::-1]), (lo, h2)):
        assert np.array_equal((p.astype(np.float32) * q.astype(np.float32)).astype(np.float64), p.astype(np.float64) * q.astype(np.float64))


def test_global_bound_floor_on_the_column_ladder():
    """The split under ONE bound per operand meets |dW - ref| <= A_SPLIT sum|dy||x| + B_FLOOR (B_y sum|x| + B_x sum|dy|) entry by entry
    on columns 2^-17, 2^-24, 2^-30 and 2^-40 below the bound; from ~2^-39 a column flushes to 0; an f16 arithmetic without subnormals
    breaks the bound (the check has teeth); and the kernel's fp32 accumulation stays inside A_GPU."""
    n, Mo, Ko = 8192, 20, 20
    dy, x = ladder_operands(n, Mo, Ko, seed=1)
    B_y, B_x = np.float32(np.abs(dy).max()), np.float32(np.abs(x).max())
    ref = dy.astype(np.float64).T @ x.astype(np.float64)
    got = model_dw(dy, x, B_y, B_x)
    assert np.all(np.abs(got - ref) <= derived_bound(dy, x, B_y, B_x, A_SPLIT))
    # the floor is what the columns far below the bound see: the 2^-40 columns are gone, the 2^-30 columns are not
    flushed = 1 + LADDER.index(40)
    assert np.all(got[flushed::5, :] == 0) and np.all(got[:, flushed::5] == 0)
    assert np.all(got[1 + LADDER.index(30)::5, 0::5] != 0) and np.all(got[0::5, 1 + LADDER.index(30)::5] != 0)
    # ... and it is needed: without it (B_FLOOR -> 0) the 2^-30 / 2^-40 entries fail
    assert not np.all(np.abs(got - ref) <= A_SPLIT * (np.abs(dy.astype(np.float64)).T @ np.abs(x.astype(np.float64))))
    # flushing f16 subnormals (hi / lo below 2^-14 of the scaled range) would lose the 2^-30 columns: outside the derived bound
    ftz = model_dw(dy, x, B_y, B_x, ftz=True)
    assert not np.all(np.abs(ftz - ref) <= derived_bound(dy, x, B_y, B_x, A_SPLIT))
    # the kernel's fp32 accumulation (512-row chunks, 16-row MFMA steps) inside A_GPU
    acc = model_dw_fp32(dy[:4096], x[:4096], B_y, B_x)
    ref4 = dy[:4096].astype(np.float64).T @ x[:4096].astype(np.float64)
    assert np.all(np.abs(acc - ref4) <= derived_bound(dy[:4096], x[:4096], B_y, B_x, A_GPU))


def test_exact_column_bounds_keep_small_columns():
    """With per-column bounds (uavgnn_col_absmax) the same columns keep the full split: the error is inside A_SPLIT sum|dy||x| alone."""
    n, Mo, Ko = 4096, 10, 10
    dy, x = ladder_operands(n, Mo, Ko, seed=2)
    ref = dy.astype(np.float64).T @ x.astype(np.float64)
    got = np.zeros_like(ref)
    by, bx = np.abs(dy).max(0), np.abs(x).max(0)
    for i in range(Mo):
        for j in range(Ko):
            got[i, j] = model_dw(dy[:, i:i + 1], x[:, j:j + 1], by[i], bx[j])[0, 0]
    den = np.abs(dy.astype(np.float64)).T @ np.abs(x.astype(np.float64))
    assert np.all(np.abs(got - ref) <= A_SPLIT * den)

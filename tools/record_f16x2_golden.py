"""Records what the f16x2 kernels (csrc/gemm_h2.hip, csrc/gemm_tn_h2.hip, csrc/gru_h2.hip) compute on seeded operands, as raw fp32 bits,
into tests/golden/f16x2_mix/ - the fixtures of tests/test_f16x2_kernels_golden_gpu.py.  Needs the GPU.

    python tools/record_f16x2_golden.py             # writes the fixtures from the library that is loaded (UAVGNN_LIB: another build)

The fixtures are recorded ONCE, on the build whose results are to be kept (the commit before the split helper of csrc/f16x2.h moved to
mixed-precision FMAs), and a later build must reproduce them bit for bit: the test runs `compute()` of this file on its own build.

Operands: every element is a normal variate times 2^-j, j uniform in 0 .. 30, and every row (column, for the weight gradient) times
2^i, i in -6 .. 6 - magnitudes from 2^0 down to 2^-30 of the row / column bound, so that lo terms, f16 subnormals and flushed elements
all take part in the kernels' in-loop staging, and the rows have different scale exponents.

A fixture holds, per output: its shape, the SHA-256 of its int32 image (the whole array is checked through it) and the int32 image itself
- all of it up to 64 KB, every fourth row and the last two rows beyond (what a failing test can show; the repository keeps the set at a
few hundred KB)."""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "f16x2_mix")
ACCUMULATE, RELU = 1, 2          # UAVGNN_GEMM_ACCUMULATE, UAVGNN_GEMM_RELU (include/uavgnn.h)
FULL_BYTES = 64 * 1024


def ladder(gen, rows, cols, bound_axis):
    """[rows, cols] fp32 on the GPU: normal x 2^-(0 .. 30) per element, x 2^(-6 .. 6) per row (bound_axis = 1) or column (0)."""
    v = th.randn(rows, cols, generator=gen) * th.exp2(-th.randint(0, 31, (rows, cols), generator=gen).float())
    shape = (rows, 1) if bound_axis == 1 else (1, cols)
    return (v * th.exp2(th.randint(-6, 7, shape, generator=gen).float())).cuda()


def _split(L, W, transpose=0):
    R, C = W.shape
    n_out, K = (C, R) if transpose else (R, C)
    planes = th.empty(L.lib().uavgnn_split_h2_bytes(n_out, K), dtype=th.uint8, device="cuda")
    L.check(L.lib().uavgnn_split_h2(W.data_ptr(), W.stride(0), R, C, transpose, planes.data_ptr(), L.stream()), "uavgnn_split_h2")
    return planes


def compute():
    """{output name: fp32 tensor on the GPU} of every recorded call, on the library that is loaded."""
    from uav_bs_ctrl_amd import _lib as L
    lib, out = L.lib(), {}

    # ---- uavgnn_gemm_nt_h2 / _rm2: two sources (K1 = 32 of K = 64), M = 257 (a full 256-row tile and one clamped row), N = 192 (a full
    # 128-column block through the LDS tile, a partial one through the per-element epilogue)
    gen = th.Generator().manual_seed(9501)
    M, N, K1, K = 257, 192, 32, 64
    X, X2, W = ladder(gen, M, K1, 1), ladder(gen, M, K - K1, 1), ladder(gen, N, K, 1)
    bias, Y0 = th.randn(N, generator=gen).cuda(), th.randn(M, N, generator=gen).cuda()
    rm, rm2 = X.abs().amax(1), X2.abs().amax(1)
    planes = _split(L, W)
    for name, flags, b in (("nt_plain", 0, bias), ("nt_relu", RELU, bias), ("nt_acc", ACCUMULATE, None),
                           ("nt_acc_relu", ACCUMULATE | RELU, bias)):
        Y = Y0.clone()
        L.check(lib.uavgnn_gemm_nt_h2(X.data_ptr(), X.stride(0), K1, X2.data_ptr(), X2.stride(0), M, K, rm.data_ptr(), rm2.data_ptr(),
                                      planes.data_ptr(), N, L.ptr(b), Y.data_ptr(), Y.stride(0), flags, L.stream()), name)
        out[name] = Y
    Y, rm2_out = th.empty(M, N, device="cuda"), th.full((M,), -1.0, device="cuda")
    L.check(lib.uavgnn_gemm_nt_h2_rm2(X.data_ptr(), X.stride(0), K1, X2.data_ptr(), X2.stride(0), M, K, rm.data_ptr(), rm2_out.data_ptr(),
                                      planes.data_ptr(), N, bias.data_ptr(), Y.data_ptr(), Y.stride(0), 0, L.stream()), "nt_rm2")
    out["nt_rm2"], out["nt_rm2_rowmax2"] = Y, rm2_out

    # ---- uavgnn_gemm_nt_h2_n64: M = 129, K = 128, N = 64
    gen = th.Generator().manual_seed(9502)
    M, N, K = 129, 64, 128
    X, W = ladder(gen, M, K, 1), ladder(gen, N, K, 1)
    rm, planes, Y = X.abs().amax(1), _split(L, W), th.empty(M, N, device="cuda")
    L.check(lib.uavgnn_gemm_nt_h2_n64(X.data_ptr(), X.stride(0), M, K, rm.data_ptr(), planes.data_ptr(), N, Y.data_ptr(), Y.stride(0),
                                       L.stream()), "nt_n64")
    out["nt_n64"] = Y

    # ---- uavgnn_gemm_tn_h2: two chunks; 64 rows (the smallest count: one slice per chunk, staged by the prologue) and 256 rows (four
    # slices per chunk: the loop's staging), plain and accumulating; Mo = 260 (two row tiles, the second clamped), Ko = 20 (clamped)
    gen = th.Generator().manual_seed(9503)
    Mo, Ko, S = 260, 20, 2
    for name, n, acc in (("tn_64", 64, 0), ("tn_256", 256, 0), ("tn_256_acc", 256, 1)):
        dY, Xr = ladder(gen, n, Mo, 0), ladder(gen, n, Ko, 0)
        cy, cx = dY.abs().amax(0), Xr.abs().amax(0)
        P = th.randn(S, Mo, Ko, generator=gen).cuda()
        L.check(lib.uavgnn_gemm_tn_h2(dY.data_ptr(), dY.stride(0), Mo, Xr.data_ptr(), Xr.stride(0), Ko, n, cy.data_ptr(), cx.data_ptr(),
                                      P.data_ptr(), S, acc, L.stream()), name)
        out[name] = P.view(S * Mo, Ko)

    # ---- uavgnn_gru_cell_fwd_h2: N = 129, K_in = 256 + 64, H = 256; no-grad, then training (h' and the four saved pre-activation sets)
    gen = th.Generator().manual_seed(9504)
    N, K1, K2, H = 129, 256, 64, 256
    inp, inp2, h = ladder(gen, N, K1, 1), ladder(gen, N, K2, 1), ladder(gen, N, H, 1)
    W_ih, W_hh = ladder(gen, 3 * H, K1 + K2, 1), ladder(gen, 3 * H, H, 1)
    b_ih, b_hh = (0.1 * th.randn(3 * H, generator=gen)).cuda(), (0.1 * th.randn(3 * H, generator=gen)).cuda()
    rm = th.maximum(th.maximum(inp.abs().amax(1), inp2.abs().amax(1)), h.abs().amax(1))
    planes = th.empty(lib.uavgnn_gru_cell_h2_workspace_bytes(K1 + K2, H), dtype=th.uint8, device="cuda")
    L.check(lib.uavgnn_gru_split_weights_h2(W_ih.data_ptr(), K1 + K2, W_hh.data_ptr(), H, planes.data_ptr(), L.stream()), "gru split")
    for name, save in (("gru_nograd", False), ("gru_train", True)):
        h_out = th.empty(N, H, device="cuda")
        pre = th.empty(N, 4 * H, device="cuda") if save else None
        L.check(lib.uavgnn_gru_cell_fwd_h2(inp.data_ptr(), inp.stride(0), K1, inp2.data_ptr(), inp2.stride(0), K2, h.data_ptr(), N, H,
                                           rm.data_ptr(), planes.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), h_out.data_ptr(),
                                           L.ptr(pre), L.stream()), name)
        out[name + "_h"] = h_out
        if save:
            out[name + "_pre"] = pre
    th.cuda.synchronize()
    return out


def image(t):
    """int32 image [rows, columns] of an fp32 tensor, on the host."""
    a = t.detach().contiguous().view(th.int32).cpu().numpy()
    return a.reshape(a.shape[0], -1)


def kept_rows(bits):
    n = bits.shape[0]
    if bits.nbytes <= FULL_BYTES:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(0, n, 4), np.arange(n - 2, n)]))


def digest(bits):
    return hashlib.sha256(np.ascontiguousarray(bits).tobytes()).hexdigest()


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    total = 0
    for name, t in compute().items():
        bits = image(t)
        rows = kept_rows(bits)
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez(path, shape=np.asarray(bits.shape, dtype=np.int64), rows=rows.astype(np.int32), bits=bits[rows],
                 sha256=np.frombuffer(digest(bits).encode(), dtype=np.uint8))
        total += os.path.getsize(path)
        print(f"{name:16s} {tuple(bits.shape)}  rows kept {len(rows):4d}  {os.path.getsize(path):7d} bytes  sha256 {digest(bits)[:16]}")
    print(f"{total} bytes in {GOLDEN}")


if __name__ == "__main__":
    main()

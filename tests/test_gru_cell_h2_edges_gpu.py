"""`-m gpu`: uavgnn_gru_cell_fwd_h2 (csrc/gru_h2.hip) called directly at its edges - one row, a clamped row tile (N = 127, 129, 257),
one to ten input slices in one or two pieces, an odd slice count in front of the hidden contraction - against nn.GRUCell's math in
float64.  inp and inp2 are views (ld > K, NaN in the padding and behind row N), h_out and pre_save lie between guard rows of a
sentinel bit pattern that must survive the call.

What is held to what:
  * h' : assert_close(..., 1e-5), the parity rule (it lies behind two sigmoids and a tanh on the hardware transcendentals);
  * pre_save [N, 4 H] = (pr, pz, gin, ghn) - the four sets are what the kernel's epilogue has BEFORE any nonlinearity (gru_h2.hip:
    pr = r's pre-activation W_ir i + W_hr h + b_ir + b_hr, pz likewise, gin = W_in i + b_in, ghn = W_hn h + b_hn), so all four are
    linear in the products and get the per-entry bound of tests/test_f16x2_nt_emulation.py: pr and pz contract [inp || inp2 || h] with
    [W_ih | W_hh] (K = K_in + H), gin contracts the input only (K = K_in) and ghn the hidden state only (K = H); the row scale is the
    one bound passed for the whole row of [inp || inp2 || h], the column scale the maximum over the unit's rows of BOTH weight matrices
    (split_planes_h2_kernel), and both enter the floor term as such.  The epilogue term takes |b_ih| + |b_hh| for pr and pz: the two
    biases are added in fp32 first (one more rounding of at most 2^-24 |b_ih + b_hh|, inside the 2^-23 (|ref| + |bias|) of the bound);
  * the training call (pre_save given) and the no-grad call: bit-equal h'; the two-piece call and the call on the concatenated input:
    bit-equal h' and pre_save.
Operands are model-like, as in test_gru_cell_f16x2_vs_float64_and_the_other_cells.  The golden fixture's ragged cell (N = 129, K_in =
256 + 64, H = 256) is one of the cases."""
import numpy as np
import pytest
import torch as th

from tests.test_f16x2_nt_edges_gpu import EINVAL, EUNSUPPORTED, GUARD, SENTINEL, _record, _view
from tests.test_f16x2_nt_emulation import R_ASSERT, nt_bound, row_absmax, worst_ratio
from tests.util import assert_close

pytestmark = pytest.mark.gpu

ROWS = [1, 127, 128, 129, 257]
CONFIGS = [(256, 64, 256), (32, 0, 64), (32, 32, 64), (64, 32, 128)]          # (K1, K2, H)


@pytest.fixture(scope="module")
def L():
    from uav_bs_ctrl_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def operands():
    """per (K1, K2, H): the cell's weights (0.3 x normal), ReLU-like inputs and tanh-like hidden states for the largest N, and the
    float64 reference of every quantity; a case reads the leading N rows.  Never written."""
    out = {}
    for K1, K2, H in CONFIGS:
        rng = np.random.default_rng(9530 + K1 + K2 + H)
        K, N = K1 + K2, max(ROWS)
        o = dict(W_ih=0.3 * rng.standard_normal((3 * H, K)), W_hh=0.3 * rng.standard_normal((3 * H, H)), b_ih=0.3 * rng.standard_normal(3 * H),
                 b_hh=0.3 * rng.standard_normal(3 * H), inp=1.5 * np.maximum(rng.standard_normal((N, K)), 0), h=np.tanh(rng.standard_normal((N, H))))
        o = {k: v.astype(np.float32) for k, v in o.items()}
        d = {k: v.astype(np.float64) for k, v in o.items()}
        gi, gh = d["inp"] @ d["W_ih"].T, d["h"] @ d["W_hh"].T
        pr = gi[:, :H] + gh[:, :H] + d["b_ih"][:H] + d["b_hh"][:H]
        pz = gi[:, H:2 * H] + gh[:, H:2 * H] + d["b_ih"][H:2 * H] + d["b_hh"][H:2 * H]
        gin, ghn = gi[:, 2 * H:] + d["b_ih"][2 * H:], gh[:, 2 * H:] + d["b_hh"][2 * H:]
        r, z = 1 / (1 + np.exp(-pr)), 1 / (1 + np.exp(-pz))
        n = np.tanh(gin + r * ghn)
        o.update(pre=(pr, pz, gin, ghn), h_new=(1 - z) * n + z * d["h"])
        cell = th.nn.GRUCell(K, H).double()
        cell.load_state_dict({"weight_ih": th.from_numpy(d["W_ih"]), "weight_hh": th.from_numpy(d["W_hh"]), "bias_ih": th.from_numpy(d["b_ih"]),
                              "bias_hh": th.from_numpy(d["b_hh"])})
        with th.no_grad():
            assert th.allclose(cell(th.from_numpy(d["inp"]), th.from_numpy(d["h"])), th.from_numpy(o["h_new"]), rtol=0, atol=1e-12)
        out[(K1, K2, H)] = o
    return out


class _Guarded:
    """[rows, cols] fp32 output between GUARD rows of SENTINEL words"""

    def __init__(self, rows, cols):
        self.rows = rows
        self.buf = th.full((rows + 2 * GUARD, cols), SENTINEL, dtype=th.int32, device="cuda")
        self.ptr = self.buf[GUARD].data_ptr()

    def result(self, what):
        th.cuda.synchronize()
        guards = th.cat([self.buf[:GUARD], self.buf[GUARD + self.rows:]])
        assert bool((guards == SENTINEL).all()), f"{what}: a guard row was written"
        return self.buf[GUARD:GUARD + self.rows].cpu().numpy().view(np.float32)

    def untouched(self):
        th.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())


def _weights(L, o, K, H):
    dev = lambda a: th.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    w = {k: dev(o[k]) for k in ("W_ih", "W_hh", "b_ih", "b_hh")}
    w["planes"] = th.empty(L.lib().uavgnn_gru_cell_h2_workspace_bytes(K, H), dtype=th.uint8, device="cuda")
    L.check(L.lib().uavgnn_gru_split_weights_h2(w["W_ih"].data_ptr(), K, w["W_hh"].data_ptr(), H, w["planes"].data_ptr(), L.stream()), "gru split")
    return w


def _cell(L, w, pieces, h, rm, N, H, save, what):
    """one launch; pieces: [(host array [N, K_i])], one or two; -> h' [N, H], pre_save [N, 4 H] or None (host, fp32)"""
    views = [_view(p, 3, 4 + 4 * i) for i, p in enumerate(pieces)]
    hv = _view(h, 3, 0)
    rm_d = th.from_numpy(np.ascontiguousarray(rm)).cuda()
    h_out, pre = _Guarded(N, H), _Guarded(N, 4 * H) if save else None
    a, b = views[0], views[1] if len(views) > 1 else None
    code = L.lib().uavgnn_gru_cell_fwd_h2(a.data_ptr(), a.stride(0), a.shape[1], L.ptr(b), 0 if b is None else b.stride(0),
                                          0 if b is None else b.shape[1], hv.data_ptr(), N, H, rm_d.data_ptr(), w["planes"].data_ptr(),
                                          w["b_ih"].data_ptr(), w["b_hh"].data_ptr(), h_out.ptr, None if pre is None else pre.ptr, L.stream())
    L.check(code, what)
    return h_out.result(what + ": h_out"), None if pre is None else pre.result(what + ": pre_save")


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("K1,K2,H", CONFIGS)
def test_cell_against_float64(L, operands, N, K1, K2, H):
    """N in {1, 127, 128, 129, 257} x (K1, K2, H) in {(256, 64, 256), (32, 0, 64), (32, 32, 64), (64, 32, 128)}"""
    o = operands[(K1, K2, H)]
    K = K1 + K2
    inp, h = o["inp"][:N], o["h"][:N]
    pieces = [inp[:, :K1]] + ([inp[:, K1:]] if K2 else [])
    rm = np.maximum(row_absmax(inp), row_absmax(h))
    w = _weights(L, o, K, H)
    case = f"N {N} K1 {K1} K2 {K2} H {H}"
    h_train, pre = _cell(L, w, pieces, h, rm, N, H, True, case + " training")
    h_nograd, _ = _cell(L, w, pieces, h, rm, N, H, False, case + " no-grad")
    assert np.array_equal(h_train.view(np.int32), h_nograd.view(np.int32)), "the training and the no-grad call give different h'"
    if K2:
        h_cat, pre_cat = _cell(L, w, [inp], h, rm, N, H, True, case + " concatenated")
        assert np.array_equal(h_train.view(np.int32), h_cat.view(np.int32)), "the two-piece call's h' differs from the concatenated call's"
        assert np.array_equal(pre.view(np.int32), pre_cat.view(np.int32)), "the two-piece call's pre_save differs from the concatenated call's"
    assert_close(th.from_numpy(h_train), th.from_numpy(o["h_new"][:N]), 1e-5, f"h' ({case})")
    # the four saved sets: linear in the products
    W_ih, W_hh, b_ih, b_hh = o["W_ih"], o["W_hh"], o["b_ih"], o["b_hh"]
    bw = np.maximum(row_absmax(W_ih), row_absmax(W_hh))                  # one scale per unit's row of [W_ih | W_hh]
    xh = np.concatenate([inp, h], 1)
    for s, name in enumerate(("pr", "pz", "gin", "ghn")):
        g = slice(min(s, 2) * H, min(s, 2) * H + H)                      # the gate's rows of the weights: r, z, n, n
        if s < 2:
            x, wt, bias = xh, np.concatenate([W_ih[g], W_hh[g]], 1), np.abs(b_ih[g]) + np.abs(b_hh[g])
        else:
            x, wt, bias = (inp, W_ih[g], b_ih[g]) if s == 2 else (h, W_hh[g], b_hh[g])
        got, ref = pre[:, s * H:(s + 1) * H], o["pre"][s][:N]
        ratios = {r: worst_ratio(got, ref, nt_bound(x, wt, rm, bw[g], r, ref, bias)) for r in sorted({1, 4, R_ASSERT})}
        _record("gru_cell_fwd_h2", f"pre_save {name}", case, ratios[1], ratios[4])
        print(f"{case} {name}: worst error / bound {ratios[1]:.3f} (r = 1) {ratios[4]:.3f} (r = 4)")
        assert ratios[R_ASSERT] <= 1.0, f"{case}: pre_save {name} {ratios[R_ASSERT]:.3f} x the bound (r = {R_ASSERT})"


def test_argument_table(L, operands):
    """the return codes of include/uavgnn.h; a refused call and N == 0 write neither h_out nor pre_save."""
    K1, K2, H = 32, 32, 64
    o = operands[(K1, K2, H)]
    N = 8
    w = _weights(L, o, K1 + K2, H)
    a, b, hv = _view(o["inp"][:N, :K1], 3, 4), _view(o["inp"][:N, K1:], 3, 8), _view(o["h"][:N], 3, 0)
    rm = th.from_numpy(np.maximum(row_absmax(o["inp"][:N]), row_absmax(o["h"][:N]))).cuda()
    h_out, pre = _Guarded(N, H), _Guarded(N, 4 * H)
    st = L.stream()

    def cell(inp=a.data_ptr(), ld=a.stride(0), k1=K1, inp2=b.data_ptr(), ld2=b.stride(0), k2=K2, h=hv.data_ptr(), n=N, hh=H, r=rm.data_ptr(),
             out=h_out.ptr):
        return L.lib().uavgnn_gru_cell_fwd_h2(inp, ld, k1, inp2, ld2, k2, h, n, hh, r, w["planes"].data_ptr(), w["b_ih"].data_ptr(),
                                              w["b_hh"].data_ptr(), out, pre.ptr, st)
    unsupported = {"K1 % 32": cell(k1=16, k2=16), "K2 % 32": cell(k2=16), "K1 < 32": cell(k1=0, k2=64, ld2=b.stride(0) + 32), "H % 64": cell(hh=32),
                   "ld_inp % 4": cell(ld=a.stride(0) + 1), "ld_inp2 % 4": cell(ld2=b.stride(0) + 2), "inp misaligned": cell(inp=a.data_ptr() + 4),
                   "inp2 misaligned": cell(inp2=b.data_ptr() + 8), "h misaligned": cell(h=hv.data_ptr() + 4), "h_out misaligned": cell(out=h_out.ptr + 4)}
    invalid = {"row_absmax NULL": cell(r=None), "inp2 NULL with K2 > 0": cell(inp2=None), "ld_inp < K1": cell(ld=K1 - 4), "ld_inp2 < K2": cell(ld2=K2 - 4),
               "inp NULL": cell(inp=None), "h NULL": cell(h=None), "h_out NULL": cell(out=None), "N < 0": cell(n=-1), "K2 < 0": cell(k2=-32)}
    assert {k: v for k, v in unsupported.items() if v != EUNSUPPORTED} == {}
    assert {k: v for k, v in invalid.items() if v != EINVAL} == {}
    assert cell(n=0) == 0
    assert h_out.untouched() and pre.untouched()
    assert cell() == 0                                            # ... and the same pointers and sizes are a valid call
    h_out.result("the valid call: h_out")
    pre.result("the valid call: pre_save")

"""`-m gpu`: the 256 x 96 and 256 x 160 output tiles of csrc/gemm_tn_h2.hip (uavgnn_gemm_tn_h2_tj) against the 256 x 128 kernel, which the
golden fixtures of tests/test_f16x2_kernels_golden_gpu.py pin: the order in which an output element is accumulated does not depend on the
tile width, so every partial P[s] is the 128-wide kernel's bit for bit for the same chunk count - no tolerance.  Then each width against
float64 under the floor of INTEGRATION.md, the non-finite contract, the width rule with its chunk counts, and ops.GEMM_TN_TILES on / off on
a learner update.  Shapes are the smallest that take every path: one and several slices per chunk, a shorter and an empty last chunk,
clamped row tiles (Mo = 260, 36), one and two column tiles per width, row strides beyond the column count."""
import os
import sys

import numpy as np
import pytest
import torch as th

from tests.test_f16x2_emulation import A_GPU, B_FLOOR
from tests.util import grad_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_f16x2_golden as rec  # noqa: E402

SHAPES = [(260, 96), (260, 160), (768, 320), (256, 96), (36, 192)]
ROWS = (64, 256, 32 * 7)
CHUNKS = (1, 2, 3)
N_MAX, MO_MAX, KO_MAX, PAD = 256, 768, 320, 8


@pytest.fixture(scope="module")
def lib():
    from uav_bs_ctrl_amd import _lib as L
    return L.lib()


@pytest.fixture(scope="module")
def operands():
    """dY [256, 768 + 8], X [256, 320 + 8] of the `ladder` pattern (normal x 2^-(0 .. 30) per element, x 2^(-6 .. 6) per column), one
    dominant element per operand and an all-zero column each; every case reads a leading block of them (ld > columns).  Never written."""
    gen = th.Generator().manual_seed(9511)
    dy, x = rec.ladder(gen, N_MAX, MO_MAX + PAD, 0), rec.ladder(gen, N_MAX, KO_MAX + PAD, 0)
    dy[37, 5] = 2.0 ** 12
    x[41, 70] = -2.0 ** 12
    dy[:, 9] = 0.0
    x[:, 3] = 0.0
    return dy, x


def _chunk_rows(n, S):
    c = -(-n // S)
    c = -(-c // 32) * 32
    return [(min(s * c, n), min(s * c + c, n)) for s in range(S)]


def _launch(lib, dy, x, Mo, Ko, n, S, tj, acc, cy=None, cx=None, P=None):
    """[S + 1, Mo, Ko]: the S partials behind what P held (acc) or NaN, and one guard chunk no launch may touch."""
    from uav_bs_ctrl_amd import _lib as L
    dyv, xv = dy[:n, :Mo], x[:n, :Ko]
    cy = dyv.abs().amax(0) if cy is None else cy
    cx = xv.abs().amax(0) if cx is None else cx
    P = th.full((S + 1, Mo, Ko), float("nan"), device="cuda") if P is None else P.clone()
    L.check(lib.uavgnn_gemm_tn_h2_tj(dyv.data_ptr(), dyv.stride(0), Mo, xv.data_ptr(), xv.stride(0), Ko, n, cy.data_ptr(), cx.data_ptr(),
                                     P.data_ptr(), S, int(acc), tj, L.stream()), f"gemm_tn_h2_tj {tj}")
    return P


def _bits(t):
    return t.contiguous().view(th.int32)


@pytest.mark.parametrize("Mo,Ko", SHAPES)
def test_partials_bit_equal_across_widths(lib, operands, Mo, Ko):
    """uavgnn_gemm_tn_h2_tj at 96 and 160 columns == the same call at 128, every P[s] and the guard chunk, plain and accumulating, for
    n_rows in {64, 256, 224} x S in {1, 2, 3}; the rule's own width (tj = 0) is one of them."""
    dy, x = operands
    assert dy.stride(0) > Mo and x.stride(0) > Ko
    gen = th.Generator().manual_seed(Mo * 1000 + Ko)
    for n in ROWS:
        for S in CHUNKS:
            P0 = th.randn(S + 1, Mo, Ko, generator=gen).cuda()
            for acc in (0, 1):
                want = _launch(lib, dy, x, Mo, Ko, n, S, 128, acc, P=P0)
                assert th.equal(_bits(want[S]), _bits(P0[S])), "the 128-wide launch wrote behind its partials"
                if not acc:
                    assert not bool(th.isnan(want[:S]).any()), "the 128-wide launch left an output unwritten"
                for tj in (96, 160, 0):
                    got = _launch(lib, dy, x, Mo, Ko, n, S, tj, acc, P=P0)
                    if not th.equal(_bits(got), _bits(want)):
                        bad = (_bits(got) != _bits(want)).nonzero()
                        pytest.fail(f"[{Mo} x {Ko}] n {n} S {S} acc {acc} width {tj}: {len(bad)} of {got.numel()} words differ from the "
                                    f"128-wide kernel, first at (chunk, row, column) {tuple(int(v) for v in bad[0])}")


@pytest.mark.parametrize("Mo,Ko", SHAPES)
def test_each_width_against_float64(lib, operands, Mo, Ko):
    """per chunk: |P[s] - dy_s^T x_s (float64)| <= 2^-20 sum |dy||x| + 2^-38 (B_y sum |x| + B_x sum |dy|), B the column bounds passed
    (the floor with per-column bounds); an empty chunk is exactly zero."""
    dy, x = operands
    for tj in sorted({96, 160, lib.uavgnn_gemm_tn_h2_width(Ko)}):
        for n in ROWS:
            dyv, xv = dy[:n, :Mo], x[:n, :Ko]
            cy, cx = dyv.abs().amax(0).double(), xv.abs().amax(0).double()
            for S in CHUNKS:
                P = _launch(lib, dy, x, Mo, Ko, n, S, tj, 0)[:S].double()
                for s, (r0, r1) in enumerate(_chunk_rows(n, S)):
                    a, b = dyv[r0:r1].double(), xv[r0:r1].double()
                    ref = a.t() @ b
                    bound = A_GPU * (a.abs().t() @ b.abs()) + B_FLOOR * (cy[:, None] * b.abs().sum(0)[None, :] + cx[None, :] * a.abs().sum(0)[:, None])
                    err = (P[s] - ref).abs()
                    worst = float((err / bound.clamp_min(1e-300)).max())
                    print(f"[{Mo} x {Ko}] width {tj} n {n} S {S} chunk {s}: worst error / floor {worst:.3f}")
                    assert bool((err <= bound).all()), f"[{Mo} x {Ko}] width {tj} n {n} S {S} chunk {s}: {worst:.3f} x the floor"
                    if r0 == r1:
                        assert not bool(P[s].any())


@pytest.mark.parametrize("tj", [96, 160])
@pytest.mark.parametrize("Mo,Ko", [(260, 160), (36, 192)])
def test_non_finite_and_too_small_bounds_yield_nan(lib, operands, tj, Mo, Ko):
    """A column that holds Inf / NaN under an Inf / NaN bound (uavgnn_col_absmax leaves Inf) or whose bound is 2^8 too small (f16 overflow) gives NaN in
    every output of that column in the chunks whose rows hold such an element, and in no other output; every other row / column of P is
    the clean launch's bit for bit."""
    dy, x = operands
    n, S = 256, 3
    rows = _chunk_rows(n, S)
    clean = _launch(lib, dy, x, Mo, Ko, n, S, tj, 0)[:S]
    cy0, cx0 = dy[:n, :Mo].abs().amax(0), x[:n, :Ko].abs().amax(0)
    for which, col, C in (("dY", 17, Mo), ("X", Ko - 2, Ko)):
        src = dy if which == "dY" else x
        for kind in ("inf", "nan", "small"):
            d, xx, cy, cx = dy, x, cy0.clone(), cx0.clone()
            t = src.clone()
            if kind == "small":
                bound = (cy if which == "dY" else cx)
                bound[col] = bound[col] * 2.0 ** -8
                e = int(np.frexp(float(bound[col]))[1]) - 1                      # bound in [2^e, 2^(e + 1)): the scale is 2^(14 - e)
                over = t[:n, col].abs().double() * 2.0 ** (14 - e) >= 65520.0    # rounds to the f16 infinity
                hit = [bool(over[r0:r1].any()) for r0, r1 in rows]
                assert any(hit)
            else:
                t[100, col] = float(kind)
                (cy if which == "dY" else cx)[col] = float(kind)          # (a NaN bound scales like an infinite one)
                hit = [r0 <= 100 < r1 for r0, r1 in rows]
            d, xx = (t, x) if which == "dY" else (dy, t)
            P = _launch(lib, d, xx, Mo, Ko, n, S, tj, 0, cy=cy, cx=cx)[:S]
            line = P[:, col, :] if which == "dY" else P[:, :, col]              # [S, outputs that depend on the column]
            for s in range(S):
                if hit[s]:
                    assert bool(th.isnan(line[s]).all()), f"{which} column {col} ({kind}), width {tj}: a number in chunk {s}"
                else:
                    assert not bool(th.isnan(line[s]).any()), f"{which} column {col} ({kind}), width {tj}: NaN in chunk {s}"
            keep = th.ones(C, dtype=th.bool, device="cuda")
            keep[col] = False
            rest, rest0 = (P[:, keep, :], clean[:, keep, :]) if which == "dY" else (P[:, :, keep], clean[:, :, keep])
            assert th.equal(_bits(rest), _bits(rest0)), f"{which} column {col} ({kind}), width {tj}: another output changed"


def test_width_rule_and_chunk_counts(lib):
    """160 where 160 divides Ko and 128 does not, 96 where 96 does and neither of them, 128 otherwise (640 stays on 128); the chunk count
    is the largest multiple of 8 with tiles x S <= 512 at that width, in chunks of at least 512 rows."""
    want = {20: 128, 64: 128, 96: 96, 128: 128, 160: 160, 192: 96, 256: 128, 320: 160, 480: 160, 512: 128, 640: 128}
    n = 51 * 32768
    for Ko, tj in want.items():
        assert lib.uavgnn_gemm_tn_h2_width(Ko) == tj, Ko
        for Mo in (256, 768):
            tiles = -(-Mo // 256) * -(-Ko // tj)
            S = 512 // tiles
            S = S // 8 * 8 if S >= 8 else max(S, 1)
            assert lib.uavgnn_gemm_tn_h2_chunks(n, Mo, Ko) == S == lib.uavgnn_gemm_tn_h2_chunks_tj(n, Mo, Ko, tj), (Mo, Ko)
            assert lib.uavgnn_gemm_tn_h2_chunks_tj(n, Mo, Ko, 0) == S
            tiles128 = -(-Mo // 256) * -(-Ko // 128)
            S128 = 512 // tiles128
            assert lib.uavgnn_gemm_tn_h2_chunks_tj(n, Mo, Ko, 128) == (S128 // 8 * 8 if S128 >= 8 else max(S128, 1))
    # the four products of the benchmark's update: (Mo, Ko) -> chunks
    assert [lib.uavgnn_gemm_tn_h2_chunks(n, Mo, Ko) for Mo, Ko in ((768, 320), (768, 256), (256, 512), (256, 96))] == [80, 80, 128, 512]
    assert lib.uavgnn_gemm_tn_h2_chunks_tj(n, 768, 320, 128) == 56
    assert lib.uavgnn_gemm_tn_h2_chunks(2048, 768, 320) == 4 and lib.uavgnn_gemm_tn_h2_chunks(64, 260, 96) == 1      # >= 512 rows per chunk
    assert lib.uavgnn_gemm_tn_h2_chunks(100, 768, 320) == 0 and lib.uavgnn_gemm_tn_h2_chunks_tj(n, 768, 320, 64) == 0  # rows % 32, unknown width


def test_learner_update_with_and_without_the_tiles(monkeypatch):
    """learner.accumulate at N = 1024 agents, T = 3 (4096 time-batched rows), the thresholds lowered until the f16x2 weight gradients
    reduce the sequence: with ops.GEMM_TN_TILES off (every product on 128-wide tiles at their chunk count) and on, every slice of the flat
    gradient buffer is bit-equal except W_ih - whose row sum is cut into another number of chunks - and W_ih passes grad_close against
    the float64 oracle either way."""
    from tests.gpu_util import _exp3_learner_and_sequence, _LibSpy, _oracle_at_gpu_branch
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    B, n, M, T = 128, 8, 10, 3
    N = B * n
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    monkeypatch.setattr(ops, "GEMM_TN_MIN_ROWS", 4096)
    # the per-step f16x2 products that leave the column bounds of the recurrent weights' gradients take 4096 rows and 128 tiles in production
    monkeypatch.setattr(ops, "GEMM_X3_MIN_ROWS", 1024)
    monkeypatch.setattr(ops, "GEMM_X3_SMALL_GRID", 8)
    flats, outs = {}, {}
    for on in (False, True):
        monkeypatch.setattr(ops, "GEMM_TN_TILES", on)
        del spy.calls[:]
        learner, batch = _exp3_learner_and_sequence(B, n, M, T, "dense", seed=3)      # (seeded: the same learner and batch both times)
        outs[on] = learner.accumulate(dict(batch))
        flats[on] = learner.grads.flat.clone()
        entry = "uavgnn_gemm_tn_h2" if on else "uavgnn_gemm_tn_h2_tj"
        launched = {(a[2], a[5]): a[10] for nm, a in spy.calls if nm == entry}      # (Mo, Ko) -> S
        assert {(768, 320), (768, 256), (256, 96), (256, 512)} <= set(launched), (on, launched)
        rows = (T + 1) * N
        assert launched[(768, 320)] == min(rows // 512, 80 if on else 56)
    monkeypatch.undo()
    l64, _, g64, l32, g32 = _oracle_at_gpu_branch(learner, batch, outs[True]["QVals"].detach().cpu(), T, N, "tiles A/B")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        a, b = (flats[on][o:o + prm.numel()].view_as(prm) for on in (False, True))
        if prm.shape == (768, 320):
            for on, got in ((False, a), (True, b)):
                grad_close(got, g64[k], f"GEMM_TN_TILES={int(on)}: grad {k}", ref32=g32[k], floor=0.0)
        else:
            assert th.equal(_bits(a), _bits(b)), f"grad {k} depends on GEMM_TN_TILES"

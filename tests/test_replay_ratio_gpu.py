"""`-m gpu`: ``MultiAgentQLearner.accumulate`` over rho > 1 chunks - the replay ratio of ``learner.update`` (run.py:55-57,:97 of the
reference consumes 32 stored sequences per update; bench.py's ``value_rho32`` leg) - on the production dispatch.

A chunk after the first is the only caller that finds state left by another chunk of the same update: the slots of ops.WeightGradSink
(the accumulate modes of uavgnn_gemm_tn_h2 and uavgnn_colsum_acc add into them), the buffers of the sequence stage (row maxima, column
sums) and the bounds end_sequence() derives from them, the frozen_weights() plane and K1-image caches.  Chunks of one update may also
take different kernels: the K1 launch with row maxima (and the f16x2 f_aggr product behind it) depends on the edge count.  The one-chunk
test (tests/test_gpu_parity.py: test_learner_update_at_exp3_sizes_vs_oracle) covers none of this; the host logic of rho > 1 is pinned on
the CPU by tests/test_dp_gloo.py.

Three kinds of check: the float64 oracle on distinct chunks; bit-level invariants that follow from the code (a scale by 1/2 is exact and
every accumulating kernel adds its finished contribution once, ``*p = ACC ? *p + v : v``); and the replay of a captured update."""
import pytest
import torch as th

from tests.gpu_util import _exp3_learner_and_sequence, _LibSpy, _oracle_at_gpu_branch
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 0.0        # no blanket absolute floor (as tests/test_gpu_parity.py)
TN_ROWS = 4096          # GEMM_TN_MIN_ROWS of the 16384-row cases: the f16x2 weight gradients reduce their sequence (production: 2^18)


def _chunk(B, n, M, T, dist, seed):
    """One more sampled batch of bench.py's generator, with stored hidden states of its own."""
    import bench
    batch = bench.make_sequence(B, n, M, T, dist, th.device("cuda"), seed=seed, distinct=2)
    gen = th.Generator(device="cuda").manual_seed(5000 + seed)
    batch["h0"] = 0.1 * th.randn(B * n, 256, device="cuda", generator=gen)
    return batch


def _learner_and_chunks(B, n, T, specs):
    """The exp3 learner of the one-chunk test and one DISTINCT chunk per (dist, M) of `specs` (chunk 0 is the one-chunk test's batch)."""
    (dist0, M0), rest = specs[0], specs[1:]
    learner, c0 = _exp3_learner_and_sequence(B, n, M0, T, dist0, seed=3)
    return learner, [c0] + [_chunk(B, n, M, T, dist, seed=20 + i) for i, (dist, M) in enumerate(rest)]


def _k1_rowmax_expected(dist, M, T, N):
    """ops.py's choice of the K1 launch with row maxima for the time-batched encoder of one chunk (see the one-chunk test)."""
    return (T + 1) * N > (1 << 17) or (dist == "dense" and M >= 16 and (T + 1) * N >= 16384)


def _spied_accumulate(learner, chunks, mp):
    """learner.accumulate(chunks) under the library spy.  Returns (out, flat gradient buffer, per-chunk call lists): the list of calls is
    cut where each chunk's end_sequence() returned, so part i holds chunk i's forward, backward and time-batched reduction."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    real_lib, orig_end = L.lib, ops.WeightGradSink.end_sequence
    spy = _LibSpy(real_lib())
    cuts = []

    def end_spy(self):
        staged = self.seq is not None
        orig_end(self)
        if staged:
            cuts.append(len(spy.calls))
    mp.setattr(L, "lib", lambda: spy)
    mp.setattr(ops.WeightGradSink, "end_sequence", end_spy)
    out = learner.accumulate(chunks)
    flat = learner.grads.flat.clone()
    mp.setattr(L, "lib", real_lib)
    mp.setattr(ops.WeightGradSink, "end_sequence", orig_end)
    assert len(cuts) == len(chunks), f"time-batched staging not taken by every chunk: {len(cuts)} of {len(chunks)}"
    lo = [0] + cuts[:-1]
    parts = [list(zip(spy.calls[a:b], spy.results[a:b])) for a, b in zip(lo, cuts)]
    return out, flat, parts


def _faggr_on_h2(part):
    """(K1 launches that left row maxima, f_aggr products on the f16x2 kernel) among one chunk's calls.  The f_aggr forward is the only
    uavgnn_gemm_nt_h2 launch with the ReLU epilogue (flags bit 1, argument 14)."""
    k1 = sum(1 for (nm, _), rc in part if nm == "uavgnn_gatv2_hetero_fwd_rowmax" and rc == 0)
    h2 = sum(1 for (nm, a), _ in part if nm == "uavgnn_gemm_nt_h2" and a[14] & 2)
    return k1, h2


def _tn_h2_accumulate_flags(part):
    """The accumulate argument (11) of every uavgnn_gemm_tn_h2 launch of one chunk."""
    return [a[11] for (nm, a), _ in part if nm == "uavgnn_gemm_tn_h2"]


def _slices(learner, flat):
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    return {k: flat[off[id(p)]:off[id(p)] + p.numel()].view_as(p) for k, p in learner.policy_net.named_parameters()}


RHO_CASES = [
    # label, B, n, T, (dist, M) per chunk, GEMM_TN_MIN_ROWS
    ("1280 rows rho 3 D-dense", 160, 8, 3, [("dense", 20)] * 3, None),      # 1 / 3 is not exact
    ("1280 rows rho 3 D-env", 160, 8, 3, [("env", 20)] * 3, None),
    ("16384 rows rho 2 D-dense", 2048, 8, 1, [("dense", 20)] * 2, TN_ROWS),
    ("16384 rows rho 2 D-env", 2048, 8, 1, [("env", 20)] * 2, TN_ROWS),
    ("16384 rows rho 2 mixed", 2048, 8, 1, [("dense", 20), ("env", 20)], TN_ROWS),   # chunk 0 takes the K1 row maxima, chunk 1 does not
]


@pytest.mark.parametrize("label,B,n,T,specs,tn_rows", RHO_CASES, ids=[c[0] for c in RHO_CASES])
def test_replay_ratio_accumulate_vs_oracle(label, B, n, T, specs, tn_rows, monkeypatch):
    """Row L at rho > 1 where its production kernels dispatch: ``accumulate([chunk_0, ..., chunk_{rho-1}])`` on distinct sampled batches
    against the float64 oracle of every chunk - LossQ = the mean of the chunk losses, QVals = the last chunk's, EVERY slice of the flat
    gradient buffer = the mean of the chunk gradients (float32 oracle's mean for the error floor).  The kinks of the loss (double-Q
    argmax, encoder ReLUs) are taken per chunk at the branch the HIP path took, as in the one-chunk test."""
    from uav_bs_ctrl_amd import ops
    learner, chunks = _learner_and_chunks(B, n, T, specs)
    N, rho = B * n, len(chunks)
    with monkeypatch.context() as mp:
        if tn_rows is not None:
            mp.setattr(ops, "GEMM_TN_MIN_ROWS", tn_rows)
        out, flat, parts = _spied_accumulate(learner, chunks, mp)
        # the Q values of every chunk on its own (same dispatch): the branch the HIP path took on it
        q_gpu = [learner.accumulate(c)["QVals"].detach().cpu() for c in chunks]
    # --- the dispatch: per chunk, the kernels its own shapes select
    for i, ((dist, M), part) in enumerate(zip(specs, parts)):
        k1, h2 = _faggr_on_h2(part)
        if _k1_rowmax_expected(dist, M, T, N):
            assert k1 >= 1 and h2 >= 1, f"{label}: chunk {i} ({dist}) did not take the K1 row maxima + f16x2 f_aggr ({k1}, {h2})"
        else:
            assert k1 == 0 and h2 == 0, f"{label}: chunk {i} ({dist}) took the K1 row maxima + f16x2 f_aggr ({k1}, {h2})"
        assert any(nm == "uavgnn_colsum_acc" for (nm, _), _ in part), f"{label}: chunk {i} added no bias gradient into the sink"
    if tn_rows is not None:
        # the sink's f16x2 weight gradients: chunk 0 writes every slot (and f_aggr's own reduction never accumulates), every later
        # chunk adds into the slots chunk 0 wrote
        assert set(_tn_h2_accumulate_flags(parts[0])) == {0}, f"{label}: chunk 0 {_tn_h2_accumulate_flags(parts[0])}"
        for i in range(1, rho):
            assert 1 in _tn_h2_accumulate_flags(parts[i]), f"{label}: chunk {i} {_tn_h2_accumulate_flags(parts[i])}"
    # --- oracle, per chunk
    ref = [_oracle_at_gpu_branch(learner, c, q, T, N, f"{label}: chunk {i}") for i, (c, q) in enumerate(zip(chunks, q_gpu))]
    l64 = sum(r[0] for r in ref) / rho
    assert_close(out["LossQ"], l64, 1e-5, f"{label}: LossQ")
    assert_close(out["QVals"], ref[-1][1], 1e-5, f"{label}: QVals (last chunk)")
    got = _slices(learner, flat)
    for k in got:
        g64 = sum(r[2][k] for r in ref) / rho
        g32 = sum(r[4][k] for r in ref) / rho
        grad_close(got[k], g64, f"accumulate rho={rho} {label}: grad {k}", ref32=g32, floor=GRAD_FLOOR)


def _assert_bit_identical(learner, a, b, what):
    """Every slice of two flat gradient buffers bit for bit; the message names every parameter that differs."""
    sa, sb = _slices(learner, a), _slices(learner, b)
    bad = []
    for k in sa:
        if not th.equal(sa[k], sb[k]):
            d = (sa[k] - sb[k]).abs()
            bad.append(f"{k}: {int((sa[k] != sb[k]).sum())}/{d.numel()} differ, max |diff| {float(d.max()):.3e} "
                       f"(max |grad| {float(sa[k].abs().max()):.3e})")
    assert not bad, f"{what}:\n  " + "\n  ".join(bad)


BIT_CASES = [
    # label, B, n, M, T, (dist of chunk 0, dist of chunk 1), GEMM_TN_MIN_ROWS
    ("1280 rows D-dense", 160, 8, 20, 3, ("dense", "dense"), None),
    ("16384 rows mixed", 2048, 8, 20, 1, ("dense", "env"), TN_ROWS),
    ("C3 D-dense", 4096, 8, 80, 50, ("dense", "dense"), None),     # the benchmark's size: every f16x2 weight gradient at its production threshold
]


@pytest.mark.parametrize("label,B,n,M,T,dists,tn_rows", BIT_CASES, ids=[c[0] for c in BIT_CASES])
def test_replay_ratio_accumulate_is_scale_exact_and_order_free(label, B, n, M, T, dists, tn_rows, monkeypatch):
    """No oracle: what follows from the code.  Each chunk's loss is scaled by 1 / rho, exact for rho = 2, and every buffer a chunk adds
    into receives one finished contribution per chunk (autograd's AccumulateGrad into the flat buffer; the sink's kernels add at the end,
    ``*p = ACC ? *p + v : v``).  Hence ``accumulate([c, c])`` - the bench's form, the same dict twice - is ``accumulate(c)`` bit for bit,
    and ``accumulate([c0, c1])`` is ``accumulate([c1, c0])`` bit for bit: the flat gradient buffer and LossQ."""
    from uav_bs_ctrl_amd import ops
    learner, (c0, c1) = _learner_and_chunks(B, n, T, [(d, M) for d in dists])
    with monkeypatch.context() as mp:
        if tn_rows is not None:
            mp.setattr(ops, "GEMM_TN_MIN_ROWS", tn_rows)
        runs = {}
        for name, arg in (("c", c0), ("[c, c]", [c0, c0]), ("[c0, c1]", [c0, c1]), ("[c1, c0]", [c1, c0])):
            out = learner.accumulate(arg)
            runs[name] = (out["LossQ"].clone(), learner.grads.flat.clone())
    th.cuda.synchronize()
    for x, y in (("[c, c]", "c"), ("[c0, c1]", "[c1, c0]")):
        assert bool(th.isfinite(runs[x][1]).all()), f"{label}: accumulate({x}) left a non-finite gradient"
        assert th.equal(runs[x][0], runs[y][0]), f"{label}: LossQ of accumulate({x}) {float(runs[x][0])!r} != accumulate({y}) {float(runs[y][0])!r}"
        _assert_bit_identical(learner, runs[x][1], runs[y][1], f"{label}: accumulate({x}) vs accumulate({y})")


def test_replay_ratio_accumulate_graph_replay_is_the_eager_run(monkeypatch):
    """``GraphedCycle`` over ``accumulate([c0, c1])`` on chunks that take different kernels (chunk 0 D-dense with the K1 row maxima, chunk 1
    D-env without): the flat gradient buffer and LossQ of the replay are the eager run's bit for bit - the replay re-runs every cross-chunk
    handoff (sink slots, sequence-stage buffers, plane caches) from fixed addresses."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.graphs import GraphedCycle
    B, n, T = 2048, 8, 1
    learner, (c0, c1) = _learner_and_chunks(B, n, T, [("dense", 20), ("env", 20)])
    with monkeypatch.context() as mp:
        mp.setattr(ops, "GEMM_TN_MIN_ROWS", TN_ROWS)
        out, flat, parts = _spied_accumulate(learner, [c0, c1], mp)
        assert _faggr_on_h2(parts[0])[0] >= 1 and _faggr_on_h2(parts[1]) == (0, 0), "the chunks did not take different K1 launches"
        loss = out["LossQ"].clone()
        cyc = GraphedCycle(learner, lambda: learner.accumulate([c0, c1]))
        learner.grads.flat.fill_(float("nan"))
        out_g = cyc()
        th.cuda.synchronize()
    assert th.equal(out_g["LossQ"], loss), f"LossQ of the replay {float(out_g['LossQ'])!r} != eager {float(loss)!r}"
    _assert_bit_identical(learner, learner.grads.flat, flat, "graph replay of accumulate([c0, c1]) vs the eager run")

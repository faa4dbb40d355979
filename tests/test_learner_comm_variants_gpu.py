"""`-m gpu`: ``MultiAgentQLearner.accumulate`` for the two other communication variants of run_exp3.py's grid (``c`` = None and
``c`` = 'disc'; tests/test_gpu_parity.py covers 'tarmac') at exp3 sizes, on the kernels production dispatches there, against the float64
oracle (oracle/restatement.py:madrqn_loss; float32 for the error floor).  From 1 024 rows both variants leave the fused TarMAC step: the
GRU cell runs through ``ops.gru_cell`` without row maxima (the bf16x3 cell, csrc/gru_x3.hip), its backward is ``_GruCellFused.backward``
(gate kernel, then per-step products outside the time-batched staging), and 'disc' adds K5 (csrc/disc_comm.hip) with the Gumbel noise
drawn inside the kernel.  Helpers: tests/gpu_util.py."""
import json
import os

import pytest
import torch as th

from tests.gpu_util import EXP3, UPDATE_CASES, _exp3_learner_and_sequence, _LibSpy, _oracle_at_gpu_branch
from tests.util import _GRAD_LOG, GRAD_BASE, GRAD_FACTOR, assert_close, grad_close

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 0.0       # as tests/test_gpu_parity.py: no blanket absolute floor
MSG = EXP3["msg_size"]
_OUT = os.path.dirname(_GRAD_LOG)      # measurements go next to the gradient-error log of tests/util.py


def _record(name, row):
    try:
        os.makedirs(_OUT, exist_ok=True)
        with open(os.path.join(_OUT, name), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def _expected_dispatch(c, N, T, M, dist):
    """(C-ABI entries that must be called, entries that must NOT be) for one accumulate of variant c on N agents x (T + 1) steps - from
    uav_bs_ctrl_amd/ops.py."""
    T1N = (T + 1) * N
    # --- the time-batched observation encoder: the launches the tarmac test expects for the same size (the encoder does not depend on
    # the communication block; its input gradient arrives in the same _TimeSplit buffer)
    expect = {"uavgnn_gatv2_hetero_fwd_image", "uavgnn_gatv2_bwd", "uavgnn_relu_bwd_colsum"}
    k1_rowmax = T1N > (1 << 17) or (dist == "dense" and M >= 16 and T1N >= 16384)
    if k1_rowmax:       # K1 leaves the row maxima of its output; f_aggr's forward on the f16x2 kernel
        expect |= {"uavgnn_gatv2_hetero_fwd_rowmax", "uavgnn_gemm_nt_h2"}
        expect -= {"uavgnn_gatv2_hetero_fwd_image"}
    if N >= 4096:       # f_aggr on the bf16x3 kernel; its input gradient over the (T + 1) N rows on the f16x2 kernel
        expect |= {"uavgnn_gemm_nt_h2", "uavgnn_relu_bwd_colsum_rowmax"} | (set() if k1_rowmax else {"uavgnn_gemm_nt_x3"})
        expect -= {"uavgnn_relu_bwd_colsum"}
    # --- the recurrent step.  _gru -> ops.gru_cell(inp, h, cell) with rowmax=None: gru_cell_supported from GRU_FUSED_MIN_ROWS = 1024 rows,
    # then _gru_cell_launch takes the bf16x3 cell (K_in = 256 / 384 and H = 256 have an instantiation) with its weight planes.  Its
    # backward (_GruCellFused.backward) starts with the gate kernel on the saved pre-activations - no head, no column sums: those belong
    # to the fused TarMAC step
    assert N >= 1024
    expect |= {"uavgnn_gru_split_weights", "uavgnn_gru_cell_fwd_x3_opts", "uavgnn_gru_gates_bwd_fused"}
    if N >= 4096:
        # _mm_nn without row maxima: d inp = d_gi W_ih and d h += d_gh W_hh on the bf16x3 kernel (gemm_x3_supported from 4096 rows);
        # for 'disc' also the f_enc / f_dec products (ops.linear -> _mm_nt, 128 outputs)
        expect |= {"uavgnn_gemm_nt_x3"}
    if c == "disc":     # K5 with the noise drawn inside the kernel, and its backward through the transposed talk CSC
        expect |= {"uavgnn_disc_comm_fwd", "uavgnn_disc_comm_bwd"}
    # a silent re-route: the f16x2 cell (it needs a producer's row maxima), the fused TarMAC message kernels, the plain fp32 cell or the
    # vendor-GEMM + gate-kernel cell, the Q head kernel and the gate kernels of the fused TarMAC step, TarMAC's attention
    forbid = {"uavgnn_gru_cell_fwd_h2", "uavgnn_tarmac_msg_fwd", "uavgnn_tarmac_msg_fwd_rowmax", "uavgnn_tarmac_msg_prepare",
              "uavgnn_gru_cell_fwd", "uavgnn_gru_gates_fwd", "uavgnn_head_fwd", "uavgnn_gru_gates_bwd_fused_sums",
              "uavgnn_gru_gates_bwd_fused_sums_rowmax", "uavgnn_talk_attn_env_bwd"}
    if c is None:
        forbid |= {"uavgnn_disc_comm_fwd", "uavgnn_disc_comm_bwd"}
    return expect, forbid


def _kernel_bits(rec):
    """([E, msg] hard bits K5 chose for one recorded forward (True = class 0), [E, msg, 2] noise), by the kernel's fp32 rule
    (csrc/disc_comm.hip, disc_comm_fwd_kernel): t = (logit + noise) * inv_tau, the pair's softmax against its maximum, class 0 iff
    y0 >= y1.  The noise is the kernel's own stream for the recorded {seed, step} (test_disc_comm_in_kernel_gumbel_noise)."""
    from uav_bs_ctrl_amd import ops
    E = rec["E"]
    noise = ops.gumbel_noise(rec["rng"], E, MSG)
    le = rec["logits"].index_select(0, rec["src"].long()).view(E, MSG, 2)
    t = (le + noise) * rec["inv_tau"]
    t0, t1 = t[..., 0], t[..., 1]
    mx = th.maximum(t0, t1)
    x0, x1 = th.exp(t0 - mx), th.exp(t1 - mx)
    den = x0 + x1
    return (x0 / den) >= (x1 / den), noise


def _or_pattern(bits, off):
    """[N, 2 msg] 0/1 pattern of the OR, over every destination's in-edges (CSC), of the per-edge one-hot pairs."""
    N = off.numel() - 1
    dst = th.repeat_interleave(th.arange(N, device=bits.device), (off[1:] - off[:-1]).long())
    b = bits.to(th.int32)
    zero = th.zeros(N, MSG, dtype=th.int32, device=bits.device)
    o0 = zero.index_add(0, dst, b) > 0
    o1 = zero.index_add(0, dst, 1 - b) > 0
    return th.stack((o0, o1), 2).view(N, 2 * MSG)


def _grad_ratio(got, r64, r32):
    """max over the elements of |got - ref64| / grad_close's limit (<= 1 passes)."""
    a, r, r32 = got.detach().double().cpu(), r64.detach().double().cpu(), r32.detach().double().cpu()
    e32 = float((r32 - r).abs().max())
    lim = th.clamp(GRAD_BASE * (float(r.abs().max()) + r.abs()), min=max(GRAD_FLOOR, GRAD_FACTOR * e32))
    return float(((a - r).abs() / lim.clamp_min(1e-300)).max())


@pytest.mark.parametrize("c", [None, "disc"], ids=["none", "disc"])
@pytest.mark.parametrize("dist", ["env", "dense"])
@pytest.mark.parametrize("label,B,n,M,T", UPDATE_CASES)
def test_learner_update_comm_variant_vs_oracle(label, B, n, M, T, dist, c, monkeypatch):
    """``learner.accumulate`` for c = None / 'disc' on bench.py's sampled batches: the dispatched C-ABI set, LossQ and every Q value at
    1e-5 against float64, every slice of the flat gradient buffer under ``grad_close`` - at the branch the HIP path took for the double-Q
    argmax, the encoder's ReLUs and (disc) every hard Gumbel bit - and the captured ``GraphedCycle`` replay bit-identical to the eager run."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.graphs import GraphedCycle
    what = f"c={c} {label} {dist}"
    learner, batch = _exp3_learner_and_sequence(B, n, M, T, dist, seed=3, c=c)
    N = B * n
    nets = (learner.policy_net, learner.target_net)
    rng0 = None
    if c == "disc":
        # both networks' {seed, step} pairs set up front (the module would seed them from torch's generator on first use): the eager run
        # starts from a state the graph replay below can be put back to
        for i, net in enumerate(nets):
            net.f_comm.rng_state = th.tensor([0x5EED0000 + 7919 * i, 11 * i], dtype=th.int64, device="cuda")
        rng0 = [net.f_comm.rng_state.clone() for net in nets]
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    staged = []
    orig_end = ops.WeightGradSink.end_sequence

    def end_spy(self):
        staged.append(0 if self.seq is None else len(self.seq.bwd_steps))
        return orig_end(self)
    monkeypatch.setattr(ops.WeightGradSink, "end_sequence", end_spy)
    calls = []
    if c == "disc":
        orig_dca = ops.disc_comm_aggregate

        def dca_spy(logits, gumbel, g, tau=0.5, rng=None):
            assert gumbel is None and rng is not None, "DiscreteComm did not take the in-kernel noise"
            off, src = g.talk_csc()
            rec = dict(rng=rng.clone(), rng_ptr=rng.data_ptr(), E=int(src.numel()), logits=logits.detach().clone(), off=off, src=src,
                       inv_tau=1.0 / tau)
            res = orig_dca(logits, gumbel, g, tau=tau, rng=rng)
            rec["c"] = res.detach().clone()
            calls.append(rec)
            return res
        monkeypatch.setattr(ops, "disc_comm_aggregate", dca_spy)
    out = learner.accumulate(dict(batch))
    flat = learner.grads.flat.clone()
    monkeypatch.undo()
    called = set(spy.names)
    expect, forbid = _expected_dispatch(c, N, T, M, dist)
    _record("comm_variants_dispatch.jsonl", dict(case=what, called=sorted(called)))
    # --- the dispatch
    assert expect <= called, f"{what}: production kernels not dispatched: {sorted(expect - called)}"
    assert not (forbid & called), f"{what}: re-routed to {sorted(forbid & called)}"
    assert staged and max(staged) == 0, f"{what}: the time-batched staging serves only the TarMAC step: {staged}"
    # --- the kernel's own noise and hard bits (disc)
    disc = None
    if c == "disc":
        assert len(calls) == 2 * T + 1, f"{what}: {len(calls)} DiscreteComm forwards"
        ptrs = [nets[0].f_comm.rng_state.data_ptr(), nets[1].f_comm.rng_state.data_ptr()]
        assert [r["rng_ptr"] for r in calls] == [ptrs[k % 2] for k in range(2 * T + 1)], f"{what}: forwards do not alternate policy / target"
        gumbels, bits = [], []
        for k, r in enumerate(calls):
            # each network's step advances by one per forward, from the state set above
            assert th.equal(r["rng"].cpu(), rng0[k % 2].cpu() + th.tensor([0, k // 2])), f"{what}: rng_state of forward {k}"
            b, noise = _kernel_bits(r)
            # the reconstruction IS the kernel's: the OR over in-edges of these bits is the 0/1 pattern of K5's output, bit for bit
            assert th.equal(_or_pattern(b, r["off"]), r["c"] > 0.5), f"{what}: forward {k}: reconstructed hard bits disagree with K5's output"
            gumbels.append(noise.cpu())
            bits.append(b.cpu())
        disc = dict(gumbels=gumbels, bits=bits)
        calls.clear()
    # --- oracle, float64 (float32 for the error floor), at the branch the HIP path took
    cfg = dict(EXP3, c=c, exact_ties=True)      # exact_ties: K5's ownership rule (test_exp3_disc_comm_vs_oracle)
    stats = {}
    l64, _, g64, l32, g32 = _oracle_at_gpu_branch(learner, batch, out["QVals"].detach().cpu(), T, N, what, cfg=cfg, disc=disc, stats=stats)
    assert_close(out["LossQ"], l64, 1e-5, f"{what}: LossQ")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    worst = (0.0, "")
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        got = flat[o:o + prm.numel()].view_as(prm)
        worst = max(worst, (_grad_ratio(got, g64[k], g32[k]), k))
        grad_close(got, g64[k], f"learner.accumulate c={c} {label} {dist}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)
    _record("comm_variants_oracle.jsonl", dict(case=what, expect=sorted(expect), worst_grad_ratio=worst[0], worst_grad=worst[1], **stats))
    # --- the same accumulate as ONE replayed hipGraph leaves the eager flat gradient buffer, bit for bit
    cyc = GraphedCycle(learner, lambda: learner.accumulate(batch))
    if c == "disc":     # the replay draws the eager run's noise only from the eager run's {seed, step}
        for net, st in zip(nets, rng0):
            net.f_comm.rng_state.copy_(st)
    learner.grads.flat.fill_(float("nan"))
    out_g = cyc()
    th.cuda.synchronize()
    assert_close(out_g["LossQ"], l64, 1e-5, f"{what}: LossQ (graph replay)")
    assert th.equal(learner.grads.flat, flat), f"{what}: graph replay of accumulate differs from the eager run"

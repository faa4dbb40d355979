"""`-m gpu`: ``MultiAgentQLearner.accumulate`` with ``mixer=True`` (QMIX over TarMAC agents) at exp3 sizes, on the kernels production
dispatches there, against the float64 oracle (oracle/restatement.py:madrqn_loss with its ``mixer`` argument; float32 for the error floor).
With a mixer the loss reaches the agents only through ``d_qs`` of csrc/qmix.hip, and the mixer's own gradients leave ``d_proj`` through
``ops._LinearSplitK._grads`` (vendor GEMM, the split-K ``bmm`` from 4096 rows, ``_colsum``) - tests/test_gpu_parity.py compares that
update at the 12-row fixture only.  Helpers: tests/gpu_util.py."""
import time

import pytest
import torch as th

from oracle import restatement as R
from tests.gpu_util import UPDATE_CASES, _exp3_learner_and_sequence, _LibSpy, _oracle_at_gpu_branch
from tests.test_learner_comm_variants_gpu import _grad_ratio, _record
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 0.0       # as tests/test_gpu_parity.py: no blanket absolute floor

# the two smaller cases of UPDATE_CASES (480 and 1024 mixer rows), and T B = 4096 mixer rows at N = 4096 agents: the smallest row count at
# which WeightGradSink._chunks splits the hyper-network weight gradient into a batched product
CASES = [UPDATE_CASES[0] + ("env",), UPDATE_CASES[0] + ("dense",), UPDATE_CASES[1] + ("env",), ("mixer 4096 rows", 1024, 4, 6, 4, "env")]


def _expected_agent_dispatch(N, T, M, dist):
    """The C-ABI entries test_learner_update_at_exp3_sizes_vs_oracle (tests/test_gpu_parity.py) expects of one TarMAC accumulate on N <
    16 384 agents x (T + 1) steps: the mixer sits behind the agents and takes none of them away."""
    assert 1024 <= N < 16384
    expect = {"uavgnn_gatv2_hetero_fwd_image", "uavgnn_gru_cell_fwd_h2", "uavgnn_tarmac_msg_fwd_rowmax", "uavgnn_head_fwd",
              "uavgnn_gru_gates_bwd_fused_sums", "uavgnn_talk_attn_env_bwd", "uavgnn_gatv2_bwd", "uavgnn_colsum_acc",
              "uavgnn_relu_bwd_colsum"}
    k1_rowmax = (T + 1) * N > (1 << 17) or (dist == "dense" and M >= 16 and (T + 1) * N >= 16384)
    if k1_rowmax:
        expect |= {"uavgnn_gatv2_hetero_fwd_rowmax", "uavgnn_gemm_nt_h2"}
        expect -= {"uavgnn_gatv2_hetero_fwd_image"}
    if N >= 4096:
        expect |= {"uavgnn_gemm_nt_h2", "uavgnn_relu_bwd_colsum_rowmax"} | (set() if k1_rowmax else {"uavgnn_gemm_nt_x3"})
        expect -= {"uavgnn_relu_bwd_colsum"}
    return expect


@pytest.mark.parametrize("label,B,n,M,T,dist", CASES, ids=[f"{c[0]}-{c[5]}" for c in CASES])
def test_qmix_learner_update_vs_oracle(label, B, n, M, T, dist, monkeypatch):
    """``learner.accumulate`` with a mixer on bench.py's sampled batches: the dispatched C-ABI set, q_tot of the policy mixer, LossQ and
    every Q value at 1e-5 against float64, every slice of the flat gradient buffer (every parameter of the agent and of the mixer)
    under ``grad_close`` - at the branch the HIP path took for the double-Q argmax, the encoder's ReLUs and the
    mixer's two kinks (|w1|, |w_final|; the ReLU of V) - and the captured ``GraphedCycle`` replay bit-identical to the eager run."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.agents import qmix
    from uav_bs_ctrl_amd.graphs import GraphedCycle
    t_start = time.perf_counter()
    what = f"qmix {label} {dist}"
    learner, batch = _exp3_learner_and_sequence(B, n, M, T, dist, seed=3, mixer=True)
    N, e = B * n, learner.mixer.embed_dim
    assert batch["rews"].shape == batch["dones"].shape == (T, B, 1) and batch["states"].shape == (T + 1, B, learner.mixer.state_dim)
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    staged, mixes, torch_mixes = [], [], []
    orig_end, orig_mix, orig_torch = ops.WeightGradSink.end_sequence, ops.qmix_mix, qmix.mix_torch

    def end_spy(self):
        staged.append(0 if self.seq is None else len(self.seq.bwd_steps))
        return orig_end(self)

    def mix_spy(proj, qs, v2w, v2b):
        res = orig_mix(proj, qs, v2w, v2b)
        mixes.append(dict(proj=proj.detach().clone(), q_tot=res.detach().clone(), grad=proj.requires_grad))
        return res

    def torch_spy(*a, **k):
        torch_mixes.append(1)
        return orig_torch(*a, **k)
    monkeypatch.setattr(ops.WeightGradSink, "end_sequence", end_spy)
    monkeypatch.setattr(ops, "qmix_mix", mix_spy)
    monkeypatch.setattr(qmix, "mix_torch", torch_spy)
    out = learner.accumulate(dict(batch))
    flat = learner.grads.flat.clone()
    monkeypatch.undo()
    # --- the dispatch
    called = [c[0] for c in spy.calls]
    expect = _expected_agent_dispatch(N, T, M, dist)
    assert expect <= set(called), f"{what}: production kernels not dispatched: {sorted(expect - set(called))}"
    assert called.count("uavgnn_qmix_mix_fwd") == 2 and called.count("uavgnn_qmix_mix_bwd") == 1, f"{what}: mixing launches"
    assert not torch_mixes, f"{what}: the torch formulation of the mixing tail ran"
    assert max(staged) == T + 1, f"{what}: time-batched staging not taken: {staged}"
    assert len(mixes) == 2 and mixes[0]["grad"] and not mixes[1]["grad"], f"{what}: policy mixer first, target mixer second"
    assert mixes[0]["proj"].shape == (T * B, (n + 3) * e)
    # --- oracle, float64 (float32 for the error floor), at the branch the HIP path took
    stats = {}
    l64, q64, g64, l32, g32 = _oracle_at_gpu_branch(learner, batch, out["QVals"].detach().cpu(), T, N, what, stats=stats,
                                                    mixer_proj=mixes[0]["proj"].cpu())
    pm64 = {k: v.detach().cpu().double() for k, v in learner.mixer.state_dict().items()}
    chosen = q64[:-1].gather(2, batch["acts"].cpu()).view(T, B, n)
    q_tot64 = R.qmixer(chosen, batch["states"][:-1].cpu().double(), pm64)
    assert_close(mixes[0]["q_tot"].view(T, B, 1), q_tot64, 1e-5, f"{what}: q_tot of the policy mixer")
    assert_close(out["LossQ"], l64, 1e-5, f"{what}: LossQ")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    named = list(learner.policy_net.named_parameters()) + [("mixer." + k, p) for k, p in learner.mixer.named_parameters()]
    assert len(named) == len(learner.grads.params) and sum(p.numel() for _, p in named) == sum(p.numel() for p in learner.grads.params)
    worst, worst_mixer = (0.0, ""), (0.0, "")
    for k, prm in named:
        o = off[id(prm)]
        got = flat[o:o + prm.numel()].view_as(prm)
        ratio = (_grad_ratio(got, g64[k], g32[k]), k)
        worst, worst_mixer = max(worst, ratio), max(worst_mixer, ratio) if k.startswith("mixer.") else worst_mixer
        grad_close(got, g64[k], f"learner.accumulate {what}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)
    # --- the same accumulate as ONE replayed hipGraph leaves the eager flat gradient buffer, bit for bit
    cyc = GraphedCycle(learner, lambda: learner.accumulate(batch))
    learner.grads.flat.fill_(float("nan"))
    out_g = cyc()
    th.cuda.synchronize()
    assert_close(out_g["LossQ"], l64, 1e-5, f"{what}: LossQ (graph replay)")
    assert th.equal(learner.grads.flat, flat), f"{what}: graph replay of accumulate differs from the eager run"
    _record("qmix_oracle.jsonl", dict(case=what, mixer_rows=T * B, agents=N, called=sorted(set(called)), worst_grad_ratio=worst[0],
                                      worst_grad=worst[1], worst_mixer_grad_ratio=worst_mixer[0], worst_mixer_grad=worst_mixer[1],
                                      wall_s=round(time.perf_counter() - t_start, 2), **stats))

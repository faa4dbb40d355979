"""`-m gpu`: the learner's sequence-level route for agents without a communication block - time-batched encoder, ``unroll`` (one input
projection, one launch per step and direction of csrc/gru_rec.hip, one head) - at the reference's own operating point (32 sequences x
T = 10 x H = 256, algos/drqn/config.py), against the float64 oracle, with the dispatch it must take and the routes it must leave alone.
Parameters are the modules' own initialisers under a fixed seed (see tests/test_gru_rec_gpu.py)."""
import functools
import types

import pytest
import torch as th

from tests.gpu_util import EXP3, _exp3_learner_and_sequence, _LibSpy, _oracle_at_gpu_branch
from tests.test_exp1_pipeline_gpu import gnn_forward, oracle_loss, rnn_forward
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu
B_REF, T_REF, H_REF = 32, 10, 256


def _build(agent, B=B_REF, T=T_REF, H=H_REF, seed=17):
    """Seeded device rollout of T steps in B environments (4 x 5 GTs) -> a full replay of B sequences; target = policy + 0.01 randn."""
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    th.manual_seed(seed)
    p = SingleUbsParams(n_grps=4, gts_per_grp=5, episode_limit=4 * T)
    env = BatchedSingleUbsCoverageEnv(p, B, seed=3)
    args = types.SimpleNamespace(device="cuda", agent=agent, hidden_size=H, n_heads=4, n_layers=2, max_seq_len=T, gamma=0.99, polyak=0.995,
                                 batch_size=B, lr=5e-4, anneal_lr=False, seed=seed)
    learner = QLearner(env.get_env_info(agent), args)
    gen = th.Generator(device="cuda").manual_seed(seed)
    with th.no_grad():
        for prm in learner.target_net.parameters():
            prm.add_(0.01 * th.randn(prm.shape, device="cuda", generator=gen))
    buf = SingleUbsSequenceReplay(B, T, p.n_gts, H, n_envs=B, device="cuda")
    obs_in = lambda: env.graph() if agent == "gnn" else env.observations()["flat"]  # noqa: E731
    obs, h = env.reset(), learner.init_hidden(B)
    for _ in range(T):
        a, h2 = learner.act(obs_in(), h, 0.3)
        buf.stage_obs(dict(gt=obs["gt"], agent=obs["agent"], h=h))
        obs, rew, done, info = env.step(a)
        learner.cache(buf, None, None, a, rew, obs, h2, done, info["BadMask"], staged=True)
        h = h2
    assert len(buf) == B
    return learner, buf


@functools.lru_cache(maxsize=None)
def _case(agent):
    """The learner, its replay and the float64 / float32 oracle of the one gathered batch (shared by the routes; nothing here moves a
    parameter: the tests call ``accumulate`` only)."""
    learner, buf = _build(agent)
    batch = buf.gather(th.arange(B_REF, device="cuda"), agent)
    pol = {k: v.detach().clone() for k, v in learner.policy_net.state_dict().items()}
    tgt = {k: v.detach().clone() for k, v in learner.target_net.state_dict().items()}
    forward = gnn_forward if agent == "gnn" else rnn_forward
    o64 = oracle_loss(batch, pol, tgt, learner.gamma, forward, th.float64)
    o32 = oracle_loss(batch, pol, tgt, learner.gamma, forward, th.float32)
    return learner, buf, o64, o32


def _accumulate_spied(learner, batch, monkeypatch):
    from uav_bs_ctrl_amd import _lib as L
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    out = learner.accumulate(batch)
    monkeypatch.undo()
    grads = {k: prm.grad.detach().clone() for k, prm in learner.policy_net.named_parameters()}
    count = lambda name: sum(1 for n, _ in spy.calls if n == name)  # noqa: E731
    return out, grads, count


def _against_oracle(what, out, grads, batch, o64, o32):
    loss64, q64, g64 = o64
    print(f"{what}: LossQ {float(out['LossQ']):.8f} (float64 oracle {float(loss64):.8f})")
    assert_close(out["LossQ"], loss64, 1e-5, f"{what}: LossQ")
    assert_close(out["QVals"][:-1].gather(2, batch["acts"]), q64, 1e-5, f"{what}: Q(s, a)")
    for k, g_ref in g64.items():
        grad_close(grads[k], g_ref, f"{what}: grad {k}", ref32=o32[2][k])


@pytest.mark.parametrize("agent", ["gnn", "rnn"])
def test_exp1_update_at_the_reference_size_takes_the_sequence_route(agent, monkeypatch):
    learner, buf, o64, o32 = _case(agent)
    batch = buf.gather(th.arange(B_REF, device="cuda"), agent)
    assert float(batch["rews"].abs().max()) > 0
    out, grads, count = _accumulate_spied(learner, batch, monkeypatch)
    _against_oracle(f"exp1 {agent}", out, grads, batch, o64, o32)
    T = T_REF
    assert count("uavgnn_gru_rec_fwd") == 2 * T + 1 and count("uavgnn_gru_rec_bwd") == T + 1
    assert count("uavgnn_gru_gates_fwd") == 0
    if agent == "gnn":
        assert count("uavgnn_gatv2_fwd") == 2, "the encoder did not run time-batched (once per network)"


@pytest.mark.parametrize("route", ["GRU_SEQ off", "time_batched off"])
@pytest.mark.parametrize("agent", ["gnn", "rnn"])
def test_exp1_update_on_the_per_step_routes(agent, route, monkeypatch):
    from uav_bs_ctrl_amd import ops
    learner, buf, o64, o32 = _case(agent)
    if route == "GRU_SEQ off":
        monkeypatch.setattr(ops, "GRU_SEQ", False)
    batch = buf.gather(th.arange(B_REF, device="cuda"), agent, time_batched=route != "time_batched off")
    assert ("obs_all" in batch) == (route != "time_batched off")
    spy_patch = pytest.MonkeyPatch()
    try:
        out, grads, count = _accumulate_spied(learner, batch, spy_patch)
    finally:
        spy_patch.undo()
    _against_oracle(f"exp1 {agent}, {route}", out, grads, batch, o64, o32)
    assert count("uavgnn_gru_rec_fwd") == 0 and count("uavgnn_gru_rec_bwd") == 0
    assert count("uavgnn_gru_gates_fwd") == 2 * T_REF + 1


def test_exp1_update_above_the_row_threshold_keeps_the_fused_cells(monkeypatch):
    """1024 environments: per-step ``step`` on the fused cells, but the encoder time-batched through ``DrqnGnnAgent.encode``."""
    B, T = 1024, 2
    learner, buf = _build("gnn", B=B, T=T)
    batch = buf.gather(th.arange(B, device="cuda"), "gnn")
    pol = {k: v.detach().clone() for k, v in learner.policy_net.state_dict().items()}
    tgt = {k: v.detach().clone() for k, v in learner.target_net.state_dict().items()}
    out, grads, count = _accumulate_spied(learner, batch, monkeypatch)
    assert count("uavgnn_gru_rec_fwd") == 0 and count("uavgnn_gru_rec_bwd") == 0
    assert count("uavgnn_gatv2_fwd") == 2
    # the gradients too: the only route on which DrqnGnnAgent.step (which ignores dx_out) meets the fused cells and the time-split slots
    _against_oracle("exp1 gnn, 1024 environments", out, grads, batch, oracle_loss(batch, pol, tgt, learner.gamma, gnn_forward, th.float64),
                    oracle_loss(batch, pol, tgt, learner.gamma, gnn_forward, th.float32))


def _flat_grads(learner, flat):
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    return {k: flat[off[id(prm)]:off[id(prm)] + prm.numel()].view_as(prm) for k, prm in learner.policy_net.named_parameters()}


def test_rnn_agent_of_exp2_without_communication_takes_the_sequence_route(monkeypatch):
    """``MultiAgentQLearner`` with o='mlp', c=None (RnnAgent, double-Q) on 256 rows per step (64 environments of the 4-UBS map the flat
    batches of tests/test_exp2_device_pipeline_gpu.py are built from), T = 3, by that module's rules."""
    from tests import test_exp2_device_pipeline_gpu as X
    from uav_bs_ctrl_amd import RnnAgent
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    th.manual_seed(5)
    B, T = 64, 3
    N = 4 * B
    learner = MultiAgentQLearner(dict(obs_shape=X.F, n_actions=9, n_agents=4, episode_limit=T), X._args(None))
    assert isinstance(learner.policy_net, RnnAgent) and learner.double_q
    with th.no_grad():
        for p in learner.target_net.parameters():
            p.add_(th.randn_like(p) * 0.01)
    learner.invalidate_weight_cache()
    tm, extra = X._sequence(B, T, 7)
    batch = X._flat_batch(tm, extra)
    out, _, count = _accumulate_spied(learner, batch, monkeypatch)
    flat = learner.grads.flat.clone()
    assert count("uavgnn_gru_rec_fwd") == 2 * T + 1 and count("uavgnn_gru_rec_bwd") == T + 1 and count("uavgnn_gru_gates_fwd") == 0
    what = "exp2 c=None, 256 rows"
    l64, g64, g32, _ = X._oracle_at_mlp_branch(learner, batch, out["QVals"].detach(), T, N, what, dict(X._cfg(None), exact_ties=True), False)
    assert_close(out["LossQ"].reshape(()), l64.reshape(()), 1e-5, f"{what}: LossQ")
    for name, g in _flat_grads(learner, flat).items():
        grad_close(g, g64[name], f"{what}: grad {name}", ref32=g32[name])


def test_gnn_agent_without_communication_and_a_dueling_head_takes_the_sequence_route(monkeypatch):
    """The graph encoder, c=None, Dueling head, double-Q at 32 environments x 8 agents = 256 rows per step, T = 3, by the rules of
    tests/gpu_util.py (float64 evaluated at the branch the HIP path took)."""
    import bench
    from uav_bs_ctrl_amd.agents.heads import DuelingLayer
    real_args = bench.exp3_args

    def dueling_args(device, c="tarmac"):
        a = real_args(device, c=c)
        a.dueling = True
        return a
    monkeypatch.setattr(bench, "exp3_args", dueling_args)
    B, n, M, T = 32, 8, 10, 3
    learner, batch = _exp3_learner_and_sequence(B, n, M, T, "env", seed=3, c=None)
    monkeypatch.undo()
    assert isinstance(learner.policy_net.f_out, DuelingLayer) and learner.double_q
    out, _, count = _accumulate_spied(learner, dict(batch), monkeypatch)
    flat = learner.grads.flat.clone()
    assert count("uavgnn_gru_rec_fwd") == 2 * T + 1 and count("uavgnn_gru_rec_bwd") == T + 1 and count("uavgnn_gru_gates_fwd") == 0
    what = "exp3 c=None dueling, 256 rows"
    cfg = dict(EXP3, c=None, dueling=True, exact_ties=True)
    l64, _, g64, _, g32 = _oracle_at_gpu_branch(learner, batch, out["QVals"].detach().cpu(), T, B * n, what, cfg=cfg)
    assert_close(out["LossQ"], l64, 1e-5, f"{what}: LossQ")
    for name, g in _flat_grads(learner, flat).items():
        grad_close(g, g64[name], f"{what}: grad {name}", ref32=g32[name])


def test_the_same_seeds_give_the_same_bits():
    def run():
        learner, buf = _build("gnn")
        out = learner.accumulate(buf.gather(th.arange(B_REF, device="cuda"), "gnn"))
        flat = learner.grads.flat.clone()
        learner.apply()
        return out["LossQ"].clone(), out["QVals"].clone(), flat, learner.flat.flat.clone()
    for name, a, b in zip(("LossQ", "QVals", "flat gradient buffer", "parameters after apply"), run(), run()):
        assert th.equal(a, b), name

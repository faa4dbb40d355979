"""`-m gpu`: the learner with the quantile-regression head (``MultiAgentQLearner(quantiles=8)``) at the sizes of
tests/test_learner_prio_gpu.py (H = 32, six sequences, four agents, T = 3, K = 8).

TarMAC and no-comm, one-step and two-step targets, against the float64 oracle: oracle/restatement.py:madrqn_loss is shape-agnostic in its
plain head, so with ``f_out.weight [A K, H]`` its ``agent_out`` / ``target_out`` are the quantiles; the test forms the quantile loss
itself from them (``ops.qr_loss_torch`` in float64, which tests/test_quantile_host.py holds to tests/qr_ref.py at 1e-12, and qr_ref once
more on the value here) at the ReLU pattern and the double-Q choice the GPU took, and compares LossQ, ``last_td`` and every parameter
gradient.  The argmax over the quantile means is the one discontinuity of the tail: the GPU's choice must be float64's except on rows
whose top-two float64 means lie within 1e-5 max|q|, and at most one of the 72 rows may be such a row.  The seed of the shared case
(tests/test_learner_prio_gpu.py: 3) leaves float64 itself no such row - smallest top-two gap of the four cases, relative to max|q|:
MIN_GAP_MEASURED below, asserted to be above 1e-5 on every run.

exp1's ``QLearner`` (C = 1, max targets) against ``ops.qr_loss_torch`` on the learner's own quantiles; a captured update replays its
eager form bit for bit; ``act`` and an evaluation step give the quantile means of the same parameters."""
import functools

import numpy as np
import pytest
import torch as th

from oracle import restatement as R
from tests import qr_ref as QR
from tests.gpu_util import _exp3_learner_and_sequence, _gpu_relu_patterns, _oracle_obs, _ScriptedRelu
from tests.test_learner_prio_gpu import B, H, M, N_AGENTS, T, _cfg, _fresh
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu

K, A = 8, 9
N = B * N_AGENTS
# smallest (top-1 - top-2) / max|q| of the float64 means over the rows the double-Q choice is made on, over the four cases below
# (the two targets of a variant share its parameters): tarmac 1.034e-1, no-comm 3.538e-1 - four orders above the 1e-5 of the rule
MIN_GAP_MEASURED = 1.034e-1


@functools.lru_cache(maxsize=None)
def _case(c):
    """The learner of tests/test_learner_prio_gpu.py::_case with the quantile head (built once per variant; nothing moves a parameter)."""
    import bench
    real_args = bench.exp3_args

    def args(device, c="tarmac"):
        a = real_args(device, c=c)
        a.hidden_size, a.msg_size, a.key_size, a.quantiles = H, 8, 4, K       # the learner reads the option from its arguments too
        return a
    mp = pytest.MonkeyPatch()
    mp.setattr(bench, "exp3_args", args)
    try:
        learner, batch = _exp3_learner_and_sequence(B, N_AGENTS, M, T, "env", seed=3, c=c)
    finally:
        mp.undo()
    assert learner.quantiles == K and tuple(learner.policy_net.f_out.weight.shape) == (A * K, H)
    gen = th.Generator(device="cuda").manual_seed(5)
    batch["h0"] = 0.1 * th.randn(N, H, device="cuda", generator=gen)
    batch["h1"] = 0.1 * th.randn(N, H, device="cuda", generator=gen)
    d = th.zeros(T, B, 1, device="cuda")
    d[0, 1], d[1, 4], d[T - 1, 0] = 1.0, 1.0, 1.0          # episode ends at t = 0, mid-sequence and at t = T - 1
    batch["dones"] = d
    weights = th.tensor([1.0, 0.25, 0.7, 0.05, 0.5, 0.9], device="cuda")
    return learner, batch, weights


def _oracle_theta(learner, batch, dtype, relu_masks, cfg):
    """(policy parameters by name, theta_pol [T+1, N, A, K], theta_tgt [T, N, A, K], ReLU pre-activations) of the oracle."""
    pp = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in learner.policy_net.state_dict().items()}
    pt = {k: v.detach().cpu().to(dtype) for k, v in learner.target_net.state_dict().items()}
    obs = [_oracle_obs(g, dtype) for g in batch["obs"]]
    f = lambda t: t.detach().cpu().to(dtype)   # noqa: E731
    script, real = _ScriptedRelu(relu_masks), R.F
    R.F = script
    try:        # the oracle's own scalar tail is not used: any valid choice keeps it from taking an argmax over A K columns
        _, agent_out, target_out = R.madrqn_loss(obs, f(batch["h0"]), f(batch["h1"]), batch["acts"].cpu(), f(batch["rews"]), f(batch["dones"]),
                                                 pp, pt, cfg, learner.gamma, True, next_acts=th.zeros(T, N, 1, dtype=th.int64))
    finally:
        R.F = real
    assert tuple(agent_out.shape) == (T + 1, N, A * K) and tuple(target_out.shape) == (T, N, A * K)
    return pp, agent_out.view(T + 1, N, A, K), target_out.detach().view(T, N, A, K), script.pre


def _quantile_oracle(learner, batch, w, dtype, next_acts, relu_masks, cfg, n_step):
    """(loss, td [T, B, n], gradients by name) with the quantile loss formed HERE from the oracle's quantiles."""
    from uav_bs_ctrl_amd import ops
    pp, th_pol, th_tgt, _ = _oracle_theta(learner, batch, dtype, relu_masks, cfg)
    f = lambda t: t.detach().cpu().to(dtype)   # noqa: E731
    acts = batch["acts"].cpu().view(T, N, 1, 1).expand(T, N, 1, K)
    theta_a = th_pol[:-1].gather(2, acts).view(T, B, N_AGENTS, K)
    theta_next = th_tgt.gather(2, next_acts.view(T, N, 1, 1).expand(T, N, 1, K)).view(T, B, N_AGENTS, K)
    loss, td = ops.qr_loss_torch(theta_a, theta_next, f(batch["rews"]), f(batch["dones"]), f(w), learner.gamma, n_step, 1.0)
    if dtype == th.float64:
        rl, _, rtd, _, _ = QR.loss(theta_a.detach().numpy(), theta_next.numpy(), f(batch["rews"]).numpy(), f(batch["dones"]).numpy(),
                                   f(w).numpy(), learner.gamma, n_step, 1.0)
        assert abs(float(loss.detach()) - rl) <= 1e-12 * abs(rl) and np.abs(td.numpy() - rtd).max() <= 1e-12 * np.abs(rtd).max()
    names = [k for k, _ in learner.policy_net.named_parameters()]
    return loss.detach(), td.detach(), dict(zip(names, th.autograd.grad(loss, [pp[k] for k in names])))


@pytest.mark.parametrize("returns", [None, ("nstep", 2)], ids=["one-step", "nstep2"])
@pytest.mark.parametrize("c", ["tarmac", None], ids=["tarmac", "no-comm"])
def test_quantile_update_vs_oracle(c, returns):
    learner, batch, w = _case(c)
    cfg, what = _cfg(c), f"quantiles={K} returns={returns} c={c}"
    n_step = 1 if returns is None else returns[1]
    learner.returns = returns                  # the learner is shared between the cases: put back below
    try:
        out = learner.accumulate(_fresh(batch, weights=w))
        flat, td_gpu = learner.grads.flat.clone(), learner.last_td[0].clone()
        assert len(learner.last_td) == 1 and tuple(td_gpu.shape) == (T, B, N_AGENTS) and not learner.last_td[0].requires_grad
        td_out = th.full((T, B, N_AGENTS), float("nan"), device="cuda")
        learner.accumulate(_fresh(batch, weights=w, td_out=td_out))
        assert learner.last_td[0].data_ptr() == td_out.data_ptr() and th.equal(td_out, td_gpu), "td_out receives the same bits"
        assert th.equal(learner.grads.flat, flat), "the TD buffer changed the gradient"
        plain = learner.accumulate(_fresh(batch))
        assert not hasattr(learner, "last_td"), "a batch without weights left last_td"
        ones = learner.accumulate(_fresh(batch, weights=th.ones(B, device="cuda")))
        assert th.equal(ones["LossQ"], plain["LossQ"]) and th.equal(ones["QVals"], plain["QVals"])
    finally:
        learner.returns = None
    q_gpu = out["QVals"].detach().cpu()
    assert tuple(q_gpu.shape) == (T + 1, N, A), "QVals are the policy's per-action means"
    # float64 at its own branch: the means, the argmax rule, the ReLU rule of tests/gpu_util.py
    _, th_pol64, _, pre64 = _oracle_theta(learner, batch, th.float64, None, cfg)
    q64 = th_pol64.detach().mean(-1)
    assert_close(q_gpu, q64, 1e-5, f"{what}: QVals")
    scale = float(q64.abs().max())
    top2 = q64[1:].topk(2, dim=2).values
    gap = top2[..., 0] - top2[..., 1]
    print(f"{what}: smallest top-two gap of the float64 means {float(gap.min()) / scale:.3e} of max|q|")
    assert float(gap.min()) > 1e-5 * scale, "the float64 oracle itself has a tied row: pick another seed"
    na_gpu, na64 = q_gpu[1:].argmax(2, keepdim=True), q64[1:].argmax(2, keepdim=True)
    differs = (na_gpu != na64).squeeze(2)
    assert int(differs.sum()) <= 1 and (not bool(differs.any()) or float(gap[differs].max()) < 1e-5 * scale), \
        f"{what}: the GPU's double-Q choice differs from float64's on {int(differs.sum())} rows"
    patterns = _gpu_relu_patterns(learner, batch, T, N)
    flips = 0
    for i, m in patterns.items():
        pre = pre64[i].reshape(m.shape)
        flipped = (pre > 0) != m
        if bool(flipped.any()):
            flips += int(flipped.sum())
            assert float(pre[flipped].abs().max()) <= 1e-5 * float(pre.abs().max()), f"{what}: ReLU pattern of call {i} differs away from the kink"
    assert flips <= 1e-5 * sum(m.numel() for m in patterns.values()) + 2, f"{what}: {flips} ReLU elements flipped"
    # both oracles at the GPU's branch
    l64, td64, g64 = _quantile_oracle(learner, batch, w, th.float64, na_gpu, patterns, cfg, n_step)
    _, _, g32 = _quantile_oracle(learner, batch, w, th.float32, na_gpu, patterns, cfg, n_step)
    if n_step > 1:
        _, td1, _ = _quantile_oracle(learner, batch, w, th.float64, na_gpu, patterns, cfg, 1)
        assert float((td64 - td1).abs().max()) > 1e-2, "the n-step target equals the one-step target here: the case shows nothing"
    assert_close(out["LossQ"], l64, 1e-5, f"{what}: LossQ")
    assert_close(td_gpu, td64, 1e-5, f"{what}: last_td")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        grad_close(flat[o:o + prm.numel()].view_as(prm), g64[k], f"learner.accumulate {what}: grad {k}", ref32=g32[k])


def test_the_tarmac_agent_takes_the_generic_route(monkeypatch):
    """The fused TarMAC step keys on nn.Linear: with the quantile head the step is f_comm, then the head."""
    from uav_bs_ctrl_amd import ops
    learner, batch, w = _case("tarmac")
    monkeypatch.setattr(ops, "tarmac_step", lambda *a, **k: pytest.fail("the fused step took the quantile head"))
    out = learner.accumulate(_fresh(batch, weights=w))
    assert bool(th.isfinite(out["LossQ"]))


# ---- act and an evaluation step: the means ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ["tarmac", None], ids=["tarmac", "no-comm"])
def test_act_and_an_evaluation_step_use_the_quantile_means(c):
    from uav_bs_ctrl_amd.agents.heads import quantile_mode
    learner, batch, _ = _case(c)
    h = batch["h0"]
    net = learner.policy_net
    with th.no_grad():
        q, h2 = net(batch["obs"][0].fresh(), h)
        with quantile_mode(net, "quantiles"):
            theta, h2q = net(batch["obs"][0].fresh(), h)
    assert tuple(q.shape) == (N, A) and tuple(theta.shape) == (N, A * K) and th.equal(h2, h2q)
    want = theta.double().view(N, A, K).mean(-1)
    assert_close(q, want, 1e-5, "evaluation step: q against theta.view(N, A, K).mean(-1)")
    acts, h3 = learner.act(batch["obs"][0].fresh(), h, 0.0)       # greedy
    assert th.equal(h3, h2) and acts.dtype == th.int64 and tuple(acts.shape) == (N,)
    assert th.equal(acts, q.argmax(1)), "act is greedy on the means"
    top2 = want.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-5 * float(want.abs().max())
    assert int(clear.sum()) >= N - 1 and th.equal(acts[clear], want.argmax(1)[clear])


# ---- exp1 ------------------------------------------------------------------------------------------------------------------------------
def test_exp1_qlearner_vs_the_torch_arm():
    """C = 1, max targets (no double-Q): LossQ, last_td and the flat gradient with the kernels against the same update with both ops
    replaced by their torch arms on the learner's own quantiles."""
    import types

    from tests.test_exp1_graphed_gpu import _obs_in
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    Bq, Tq = 8, 3
    th.manual_seed(23)
    p = SingleUbsParams(n_grps=4, gts_per_grp=5, episode_limit=8 * Tq)
    env = BatchedSingleUbsCoverageEnv(p, Bq, seed=5)
    args = types.SimpleNamespace(device="cuda", agent="rnn", hidden_size=H, n_heads=4, n_layers=2, max_seq_len=Tq, gamma=0.99, polyak=0.995,
                                 batch_size=Bq, lr=5e-4, anneal_lr=False, seed=23)
    learner = QLearner(env.get_env_info("rnn"), args, quantiles=K, returns=("nstep", 2))
    assert learner.n_agents == 1 and not learner.double_q and learner.quantiles == K
    buf = SingleUbsSequenceReplay(2 * Bq, Tq, p.n_gts, H, n_envs=Bq, device="cuda")
    obs, h = env.reset(), learner.init_hidden(Bq)
    for _ in range(2 * Tq):
        a, h2 = learner.act(_obs_in(env, "rnn"), h, 0.3)
        buf.stage_obs(dict(gt=obs["gt"], agent=obs["agent"], h=h))
        obs, rew, done, info = env.step(a)
        learner.cache(buf, None, None, a, rew, obs, h2, done, info["BadMask"], staged=True)
        h = h2
    batch = buf.gather(th.arange(Bq, 2 * Bq, device="cuda"), "rnn")
    batch["dones"] = batch["dones"].clone()
    batch["dones"][1, 2] = 1.0
    w = th.linspace(0.2, 1.0, Bq, device="cuda")
    out = learner.accumulate(dict(batch, weights=w))
    flat, td = learner.grads.flat.clone(), learner.last_td[0].clone()
    assert tuple(td.shape) == (Tq, Bq, 1) and tuple(out["QVals"].shape) == (Tq + 1, Bq, learner.n_actions)
    seen = {}

    def select_arm(theta_pol, theta_tgt, acts, double_q):
        assert not double_q
        seen["theta"] = (theta_pol.detach().clone(), theta_tgt.clone())
        return ops.qr_select_torch(theta_pol, theta_tgt, acts, double_q)

    def loss_arm(theta_a, theta_next, rews, dones, weights, gamma, n_step=1, kappa=1.0, td_out=None, workspace=None):
        assert n_step == 2 and kappa == 1.0
        return ops.qr_loss_torch(theta_a, theta_next, rews, dones, weights, gamma, n_step, kappa)
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "qr_select", select_arm)
    mp.setattr(ops, "qr_loss", loss_arm)
    try:
        ref = learner.accumulate(dict(batch, weights=w))
    finally:
        mp.undo()
    assert tuple(seen["theta"][0].shape) == (Tq + 1, Bq, learner.n_actions, K)
    assert_close(out["QVals"], ref["QVals"], 1e-5, "exp1: QVals")
    assert_close(out["LossQ"], ref["LossQ"], 1e-5, "exp1: LossQ")
    assert_close(td, learner.last_td[0], 1e-5, "exp1: last_td")
    assert float(learner.grads.flat.abs().max()) > 0
    grad_close(flat, learner.grads.flat, "exp1 quantiles nstep 2: flat gradient", floor=0.0)
    # the max target: the target network's quantiles at the action of its own largest mean
    theta_tgt = seen["theta"][1]
    best = theta_tgt.double().mean(-1).argmax(2)
    _, theta_next, next_acts, _ = ops.qr_select(seen["theta"][0], theta_tgt, batch["acts"], False)
    assert th.equal(next_acts.long(), best) or int((next_acts.long() != best).sum()) <= 1


# ---- a captured update -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("returns", [None, ("nstep", 2)], ids=["one-step", "nstep2"])
def test_a_captured_update_replays_its_eager_form(returns):
    import types

    from uav_bs_ctrl_amd.graphs import Episode, GraphedUpdate
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(3)
    E = 4
    env = BatchedUbsCoverageEnv.from_map("debug", E, seed=11)
    args = types.SimpleNamespace(device="cuda", hidden_size=H, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                                 dueling=False, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9, max_seq_len=None, batch_size=4,
                                 seed=3)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    learner = MultiAgentQLearner(info, args, quantiles=K, returns=returns)
    rb = SequenceReplay(8, env.episode_limit, env.n_agents, env.n_gts, H, n_envs=E, state_dim=env.state_dim, r_comm=env.p.r_comm,
                        device_state=True, seed=21, prioritized=(0.6, 0.4, 0.9, 1e-3))
    kw = dict(batch_size=4, eps=(1.0, 0.05, 200.0), enc="gnn")
    Episode(learner, env, rb, train=False, **kw)()                 # four sequences into the ring
    Bs, Ts, n = 4, env.episode_limit, env.n_agents
    weights = rb.reserve_batch(Bs)
    gu = GraphedUpdate(learner, Bs, Ts, n, env.n_gts, env.p.r_comm, weights=weights)
    idx = rb.sample_indices(Bs)
    rb.gather_into(idx, gu)
    weights.copy_(th.tensor([1.0, 0.3, 0.6, 0.8], device="cuda"))
    opt = learner.optimizer
    state = (learner.flat.flat, learner.flat_target, opt.m, opt.v, opt.hyper)
    snap = [t.clone() for t in state]
    gu.td.fill_(float("nan"))
    out = gu()
    loss_g, q_g, td_g, after_g = out["LossQ"].clone(), out["QVals"].clone(), gu.td.clone(), [t.clone() for t in state]
    assert bool(th.isfinite(td_g).all()) and not th.equal(after_g[0], snap[0]), "the replay wrote no TD error or moved no parameter"
    assert tuple(q_g.shape) == (Ts + 1, Bs * n, env.n_actions)
    again = gu.td.data_ptr()
    for dst, src in zip(state, snap):
        dst.copy_(src)
    learner.invalidate_weight_cache()
    gu.td.fill_(float("nan"))
    out_e = learner.update(gu._batch())
    assert learner.last_td[0].data_ptr() == again, "the eager update did not write the graph's TD buffer"
    assert th.equal(out_e["LossQ"], loss_g) and th.equal(out_e["QVals"], q_g) and th.equal(gu.td, td_g), "replay and eager update differ"
    for name, a, b in zip(("parameters", "target parameters", "Adam m", "Adam v", "hyper"), state, after_g):
        assert th.equal(a, b), name
    # a second replay from the same state gives the same bits again (the mean fold and the loss's workspace hold no stale value)
    for dst, src in zip(state, snap):
        dst.copy_(src)
    gu.td.fill_(float("nan"))
    out2 = gu()
    assert th.equal(out2["LossQ"], loss_g) and th.equal(gu.td, td_g) and th.equal(state[0], after_g[0])
    rb.update_priorities(idx, td_g)
    rb.check()

"""`-m gpu`: the learner with multi-step TD targets (``MultiAgentQLearner(returns=...)``) at the sizes of tests/test_learner_prio_gpu.py
(H = 32, six sequences, four agents, T = 3).

TarMAC and no-comm against the float64 oracle: the test forms the multi-step weighted loss itself from
oracle/restatement.py:madrqn_loss's ``agent_out`` / ``target_out``, at the double-Q choice and the ReLU pattern the GPU took, and compares
LossQ, ``last_td`` and every parameter gradient.  QMIX (C = 1, share_reward) and exp1's ``QLearner`` against ``ops.td_targets_torch`` on
the learner's own (mixed) values.  A captured update with the option and a TD buffer replays its eager form bit for bit, and
``replay.update_priorities`` on its TD errors gives the priorities of tests/replay_prio_ref.py."""
import functools

import numpy as np
import pytest
import torch as th

from oracle import restatement as R
from tests import replay_prio_ref as P
from tests.gpu_util import _exp3_learner_and_sequence, _gpu_relu_patterns, _oracle_at_gpu_branch, _oracle_obs, _ScriptedRelu
from tests.test_learner_prio_gpu import B, H, M, N_AGENTS, T, _case, _cfg, _fresh
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu

RETURNS = [("nstep", 2), ("lambda", 0.7)]
IDS = ["nstep2", "lambda0.7"]


def _dones():
    """Episode ends inside the sequences: at t = 0, in the middle and at t = T - 1."""
    d = th.zeros(T, B, 1, device="cuda")
    d[0, 1], d[1, 4], d[T - 1, 0] = 1.0, 1.0, 1.0
    return d


def _targets64(V, r, done, gamma, returns):
    """The two targets from their definitions, in differentiable-free torch (V carries no gradient)."""
    kind, p = returns
    r, c = r.expand_as(V), (gamma * (1 - done)).expand_as(V)
    ys = []
    for t in range(T):
        if kind == "nstep":
            m = min(p, T - t)
            y, disc = th.zeros_like(V[0]), th.ones_like(V[0])
            for k in range(m):
                y = y + disc * r[t + k]
                disc = disc * c[t + k]
            ys.append(y + disc * V[t + m - 1])
    if kind == "lambda":
        G = r[T - 1] + c[T - 1] * V[T - 1]
        ys = [G]
        for t in range(T - 2, -1, -1):
            G = r[t] + c[t] * ((1 - p) * V[t] + p * G)
            ys.insert(0, G)
    return th.stack(ys)


def _returns_oracle(learner, batch, w, dtype, next_acts, relu_masks, cfg, returns):
    """(loss, td [T, B, n], gradients by name) with the multi-step weighted loss formed HERE from the oracle's Q values."""
    pp = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in learner.policy_net.state_dict().items()}
    pt = {k: v.detach().cpu().to(dtype) for k, v in learner.target_net.state_dict().items()}
    obs = [_oracle_obs(g, dtype) for g in batch["obs"]]
    f = lambda t: t.detach().cpu().to(dtype)   # noqa: E731
    acts, rews, dones = batch["acts"].cpu(), f(batch["rews"]), f(batch["dones"])
    script, real = _ScriptedRelu(relu_masks), R.F
    R.F = script
    try:
        _, agent_out, target_out = R.madrqn_loss(obs, f(batch["h0"]), f(batch["h1"]), acts, rews, dones, pp, pt, cfg, learner.gamma, True,
                                                 next_acts=next_acts)
    finally:
        R.F = real
    shp = (T, B, N_AGENTS)
    qvals = agent_out[:-1].gather(2, acts).view(shp)
    V = target_out.detach().gather(2, next_acts).view(shp)
    td = qvals - _targets64(V, rews, dones, learner.gamma, returns)
    loss = (f(w).view(1, B, 1) * td.square()).sum() / td.numel()
    names = [k for k, _ in learner.policy_net.named_parameters()]
    return loss.detach(), td.detach(), dict(zip(names, th.autograd.grad(loss, [pp[k] for k in names])))


@pytest.mark.parametrize("returns", RETURNS, ids=IDS)
@pytest.mark.parametrize("c", ["tarmac", None], ids=["tarmac", "no-comm"])
def test_multi_step_update_vs_oracle(c, returns):
    learner, batch, w = _case(c)
    batch = dict(batch, dones=_dones())
    cfg, what = _cfg(c), f"returns={returns} c={c}"
    assert learner.returns is None
    learner.returns = returns                 # the learner of tests/test_learner_prio_gpu.py is shared: put back below
    try:
        out = learner.accumulate(_fresh(batch, weights=w))
        flat = learner.grads.flat.clone()
        td_gpu = learner.last_td[0].clone()
        assert len(learner.last_td) == 1 and tuple(td_gpu.shape) == (T, B, N_AGENTS) and not learner.last_td[0].requires_grad
        # a fixed-address TD buffer receives the same bits, written by the kernel itself
        td_out = th.full((T, B, N_AGENTS), float("nan"), device="cuda")
        learner.accumulate(_fresh(batch, weights=w, td_out=td_out))
        assert learner.last_td[0].data_ptr() == td_out.data_ptr() and th.equal(td_out, td_gpu)
        assert th.equal(learner.grads.flat, flat), "the TD buffer changed the gradient"
        # without weights: no last_td, the loss of unit weights
        plain = learner.accumulate(_fresh(batch))
        assert not hasattr(learner, "last_td"), "a batch without weights left last_td"
        ones = learner.accumulate(_fresh(batch, weights=th.ones(B, device="cuda")))
        assert th.equal(ones["LossQ"], plain["LossQ"]) and th.equal(ones["QVals"], plain["QVals"])
    finally:
        learner.returns = None
    q_gpu = out["QVals"].detach().cpu()
    _oracle_at_gpu_branch(learner, batch, q_gpu, T, B * N_AGENTS, what, cfg=cfg)          # QVals, and that the branch is float64's up to ties
    na_gpu, patterns = q_gpu[1:].argmax(2, keepdim=True), _gpu_relu_patterns(learner, batch, T, B * N_AGENTS)
    l64, td64, g64 = _returns_oracle(learner, batch, w, th.float64, na_gpu, patterns, cfg, returns)
    _, _, g32 = _returns_oracle(learner, batch, w, th.float32, na_gpu, patterns, cfg, returns)
    l1, td1, _ = _returns_oracle(learner, batch, w, th.float64, na_gpu, patterns, cfg, ("nstep", 1))
    assert float((td64 - td1).abs().max()) > 1e-2, "the multi-step target equals the one-step target here: the case shows nothing"
    assert_close(out["LossQ"], l64, 1e-5, f"{what}: LossQ")
    assert_close(td_gpu, td64, 1e-5, f"{what}: last_td")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        grad_close(flat[o:o + prm.numel()].view_as(prm), g64[k], f"learner.accumulate {what}: grad {k}", ref32=g32[k])


# ---- against the torch arm on the learner's own values ------------------------------------------------------------------------------------
def _torch_arm(qvals, next_vals, rews, dones, weights, gamma, returns, td_out=None, workspace=None):
    from uav_bs_ctrl_amd import ops
    d = qvals - ops.td_targets_torch(next_vals.detach(), rews, dones, gamma, returns)
    w = th.ones(d.shape[1], device=d.device) if weights is None else weights
    return (d.square() * w.view(1, -1, 1)).sum() / d.numel(), d.detach()


def _kernel_vs_torch_arm(learner, make_batch, returns, what, C):
    """LossQ, last_td and the whole flat gradient of ``accumulate`` with the kernels against the same update with
    ``ops.td_return_loss`` replaced by the torch formulation (``ops.td_targets_torch``) - the select stays the kernel's."""
    from uav_bs_ctrl_amd import ops
    learner.returns = returns
    out = learner.accumulate(make_batch())
    flat, td = learner.grads.flat.clone(), learner.last_td[0].clone()
    assert tuple(td.shape)[2] == C
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "td_return_loss", _torch_arm)
    try:
        ref = learner.accumulate(make_batch())
    finally:
        mp.undo()
    assert th.equal(out["QVals"], ref["QVals"])
    assert_close(out["LossQ"], ref["LossQ"], 1e-5, f"{what}: LossQ")
    assert_close(td, learner.last_td[0], 1e-5, f"{what}: last_td")
    assert float(learner.grads.flat.abs().max()) > 0
    grad_close(flat, learner.grads.flat, f"{what}: flat gradient", floor=0.0)
    return out, td


@functools.lru_cache(maxsize=None)
def _qmix_case():
    import bench
    real_args = bench.exp3_args

    def args(device, c="tarmac"):
        a = real_args(device, c=c)
        a.hidden_size, a.msg_size, a.key_size = H, 8, 4
        return a
    mp = pytest.MonkeyPatch()
    mp.setattr(bench, "exp3_args", args)
    try:
        learner, batch = _exp3_learner_and_sequence(B, N_AGENTS, M, T, "env", seed=4, mixer=True)
    finally:
        mp.undo()
    gen = th.Generator(device="cuda").manual_seed(6)
    batch["h0"] = 0.1 * th.randn(B * N_AGENTS, H, device="cuda", generator=gen)
    batch["h1"] = 0.1 * th.randn(B * N_AGENTS, H, device="cuda", generator=gen)
    batch["dones"] = _dones()
    return learner, batch


@pytest.mark.parametrize("returns", RETURNS, ids=IDS)
def test_qmix_learner_vs_the_torch_arm(returns):
    learner, batch = _qmix_case()
    w = th.tensor([1.0, 0.25, 0.7, 0.05, 0.5, 0.9], device="cuda")
    assert learner.mixer is not None and tuple(batch["rews"].shape) == (T, B, 1)
    _kernel_vs_torch_arm(learner, lambda: _fresh(batch, weights=w), returns, f"qmix {returns}", 1)


def _exp1_case():
    from tests.test_exp1_graphed_gpu import _obs_in, _setup
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    Bq, Tq = 8, 3
    learner, env, p = _setup("rnn", Bq, Tq, H)
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
    return learner, batch, Bq


def test_exp1_qlearner_vs_the_torch_arm():
    from uav_bs_ctrl_amd.learner import QLearner
    learner, batch, Bq = _exp1_case()
    assert isinstance(learner, QLearner) and learner.n_agents == 1 and not learner.double_q
    w = th.linspace(0.2, 1.0, Bq, device="cuda")
    _kernel_vs_torch_arm(learner, lambda: dict(batch, weights=w), ("nstep", 2), "exp1 nstep 2", 1)
    _kernel_vs_torch_arm(learner, lambda: dict(batch, weights=w), ("lambda", 0.7), "exp1 lambda 0.7", 1)
    # the one-step settings are the default path's TD errors, bit for bit
    learner.returns = None
    learner.accumulate(dict(batch, weights=w))
    want = learner.last_td[0].clone()
    for returns in (("nstep", 1), ("lambda", 0.0)):
        learner.returns = returns
        learner.accumulate(dict(batch, weights=w))
        assert th.equal(learner.last_td[0], want), returns


# ---- a captured update ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("returns", RETURNS, ids=IDS)
def test_a_captured_update_replays_its_eager_form_and_feeds_the_priorities(returns):
    from tests.test_prio_episode_gpu import PRIO, _multi
    from tests.test_replay_prio_gpu import _host_u32
    from uav_bs_ctrl_amd.graphs import Episode, GraphedUpdate
    learner, env, rb, kw = _multi()
    learner.returns = returns
    Bs, Ts, n = 4, env.episode_limit, env.n_agents
    Episode(learner, env, rb, train=False, **kw)()                 # four sequences into the ring
    weights = rb.reserve_batch(Bs)
    gu = GraphedUpdate(learner, Bs, Ts, n, env.n_gts, env.p.r_comm, weights=weights)
    idx = rb.sample_indices(Bs)
    rb.gather_into(idx, gu)
    weights.copy_(th.tensor([1.0, 0.3, 0.6, 0.8], device="cuda"))   # equal priorities draw unit weights: make them count
    opt = learner.optimizer
    state = (learner.flat.flat, learner.flat_target, opt.m, opt.v, opt.hyper)
    snap = [t.clone() for t in state]
    gu.td.fill_(float("nan"))
    out = gu()
    loss_g, td_g, after_g = out["LossQ"].clone(), gu.td.clone(), [t.clone() for t in state]
    assert bool(th.isfinite(td_g).all()) and not th.equal(after_g[0], snap[0]), "the replay wrote no TD error or moved no parameter"
    again = gu.td.data_ptr()
    for dst, src in zip(state, snap):
        dst.copy_(src)
    learner.invalidate_weight_cache()
    gu.td.fill_(float("nan"))
    out_e = learner.update(gu._batch())
    assert learner.last_td[0].data_ptr() == again, "the eager update did not write the graph's TD buffer"
    assert th.equal(out_e["LossQ"], loss_g) and th.equal(gu.td, td_g), "replay and eager update differ"
    for name, a, b in zip(("parameters", "target parameters", "Adam m", "Adam v", "hyper"), state, after_g):
        assert th.equal(a, b), name
    # one-step TD errors differ: the option reached the captured update
    learner.returns = None
    learner.accumulate(gu._batch())
    assert not th.equal(gu.td, td_g)
    # the priority update reads these TD errors
    before, top = _host_u32(rb.prio), int(rb.prio_max)
    rb.update_priorities(idx, td_g)
    want, want_top, bit = P.update(td_g.cpu().numpy(), idx.tolist(), rb.capacity, PRIO[0], PRIO[2], PRIO[3], before, top)
    assert bit == 0 and np.abs(_host_u32(rb.prio).astype(np.int64) - want.astype(np.int64)).max() <= 1
    assert abs(int(rb.prio_max) - want_top) <= 1
    rb.check()

"""`-m gpu`: the learner with the noisy-net Q head (``MultiAgentQLearner(noisy=sigma0)`` / ``QLearner``).

The update is tied to the path the float64 tests already hold (tests/test_learner_dueling_gpu.py and its models) WITHOUT touching the
oracle: with both networks' noise pairs fixed, ``accumulate`` of the noisy learner must equal - bit for bit - ``accumulate`` of a PLAIN twin
learner with identical parameters whose two heads are set to the folds of those pairs; the sigmas' gradients are the twin's head gradients
times the fold's noise, formed in fp32.  Then the dispatch (through ``_LibSpy`` on both shared objects) and the three modes."""
import types

import pytest
import torch as th

from tests.gpu_util import UPDATE_CASES, _exp3_learner_and_sequence, _LibSpy

pytestmark = pytest.mark.gpu

SIGMA0 = 0.5
PAIRS = ((2 ** 40 + 11, 5), (2 ** 40 + 12, 9))          # (seed, step) of the policy's and of the target network's head
CASES = {label: (B, n, M, T) for label, B, n, M, T in UPDATE_CASES}


def _exp3_learner(B, n, M, T, noisy, c="tarmac"):
    """``_exp3_learner_and_sequence`` from a copy of bench.exp3_args with ``noisy`` set (the route of test_learner_dueling_gpu._learner)."""
    import bench
    real_args = bench.exp3_args

    def args(device, c="tarmac"):
        a = real_args(device, c=c)
        if noisy is not None:
            a.noisy = noisy
        return a
    mp = pytest.MonkeyPatch()
    mp.setattr(bench, "exp3_args", args)
    try:
        return _exp3_learner_and_sequence(B, n, M, T, "env", seed=3, c=c)
    finally:
        mp.undo()


def _fresh(batch):
    """fresh graph objects: the indices a batch builds lazily and keeps are built in this call, whoever ran first"""
    if not isinstance(batch.get("obs"), list) or not hasattr(batch["obs"][0], "fresh"):
        return dict(batch)
    fb = dict(batch, obs=[g.fresh() for g in batch["obs"]])
    for k in ("obs_all", "obs_all_next"):
        if k in batch:
            fb[k] = batch[k].fresh()
    return fb


def _set_pairs(learner, pairs=PAIRS):
    for net, (seed, step) in zip((learner.policy_net, learner.target_net), pairs):
        net.f_out.rng_state = th.tensor([seed, step], dtype=th.int64, device="cuda")


def _spied(fn):
    """fn() with both shared objects spied -> (result, main spy, ext spy)."""
    from uav_bs_ctrl_amd import _lib as L
    mp = pytest.MonkeyPatch()
    main, ext = _LibSpy(L.lib()), _LibSpy(L.ext())
    mp.setattr(L, "lib", lambda: main)
    mp.setattr(L, "ext", lambda: ext)
    try:
        return fn(), main, ext
    finally:
        mp.undo()


def _count(spy, name):
    return sum(1 for n, _ in spy.calls if n == name)


def _twin_check(what, noisy, plain, batch):
    """The bit-for-bit statement of the module docstring; returns the two spies of the noisy accumulate and the twin's main spy."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.agents.heads import NoisyLinear
    assert isinstance(noisy.policy_net.f_out, NoisyLinear) and type(plain.policy_net.f_out) is th.nn.Linear
    with th.no_grad():
        for net_n, net_p in ((noisy.policy_net, plain.policy_net), (noisy.target_net, plain.target_net)):
            sd = net_n.state_dict()
            for k, v in net_p.state_dict().items():
                v.copy_(sd[k])
    assert noisy.flat.intact() and plain.flat.intact()
    noisy.invalidate_weight_cache()
    _set_pairs(noisy)
    out_n, main_n, ext_n = _spied(lambda: noisy.accumulate(_fresh(batch)))
    g_n = {k: p.grad.detach().clone() for k, p in noisy.policy_net.named_parameters()}
    for net, (seed, step) in zip((noisy.policy_net, noisy.target_net), PAIRS):
        assert net.f_out.rng_state.tolist() == [seed, step + 1], f"{what}: one draw per network and loss consumes one step"
        assert net.f_out.noisy_mode == "off" and net.f_out._fold is None
    folds = []
    with th.no_grad():
        for net_n, net_p, (seed, step) in zip((noisy.policy_net, noisy.target_net), (plain.policy_net, plain.target_net), PAIRS):
            rng = th.tensor([seed, step], dtype=th.int64, device="cuda")
            W_eff, b_eff, f_in, f_out = ops.noisy_fold(*net_n.f_out.params(), rng=rng)
            net_p.f_out.weight.copy_(W_eff)
            net_p.f_out.bias.copy_(b_eff)
            folds.append((f_in, f_out))
    plain.invalidate_weight_cache()
    out_p, main_p, _ = _spied(lambda: plain.accumulate(_fresh(batch)))
    g_p = {k: p.grad.detach().clone() for k, p in plain.policy_net.named_parameters()}
    assert bool(th.isfinite(out_n["LossQ"])) and th.equal(out_n["LossQ"], out_p["LossQ"]), f"{what}: LossQ {out_n['LossQ']} vs {out_p['LossQ']}"
    assert th.equal(out_n["QVals"], out_p["QVals"]), f"{what}: Q values"
    other = [k for k in g_p if not k.startswith("f_out.")]
    assert len(other) == len(g_p) - 2 and set(g_n) == set(g_p) | {"f_out.weight_sigma", "f_out.bias_sigma"}
    bad = [k for k in other if not th.equal(g_n[k], g_p[k])]
    assert not bad, f"{what}: gradients of {bad} differ from the plain twin's"
    assert th.equal(g_n["f_out.weight"], g_p["f_out.weight"]) and th.equal(g_n["f_out.bias"], g_p["f_out.bias"]), f"{what}: the means' gradients"
    f_in, f_out = folds[0]
    assert th.equal(g_n["f_out.weight_sigma"], g_p["f_out.weight"] * (f_out[:, None] * f_in[None, :])), f"{what}: d weight_sigma"
    assert th.equal(g_n["f_out.bias_sigma"], g_p["f_out.bias"] * f_out), f"{what}: d bias_sigma"
    assert float(g_n["f_out.weight_sigma"].abs().max()) > 0 and float(g_n["f_out.bias_sigma"].abs().max()) > 0
    return main_n, ext_n, main_p


# ---- (a), (b): c = 'tarmac' at the smallest update case ----------------------------------------------------------------------------------
def test_tarmac_update_equals_the_plain_update_at_the_folds_and_keeps_the_device_path():
    label = "1280 rows"
    B, n, M, T = CASES[label]
    noisy, batch = _exp3_learner(B, n, M, T, SIGMA0)
    plain, _ = _exp3_learner(B, n, M, T, None)
    main_n, ext_n, main_p = _twin_check(f"tarmac {label}", noisy, plain, batch)
    called = lambda spy: {nm for nm, _ in spy.calls if not nm.endswith("_supported")}      # noqa: E731
    assert "uavgnn_head_fwd" in called(main_p) and "uavgnn_tarmac_msg_fwd_rowmax" in called(main_p), "the plain learner left the path this test follows"
    assert called(main_n) == called(main_p), f"only noisy {sorted(called(main_n) - called(main_p))}, only plain {sorted(called(main_p) - called(main_n))}"
    for name in ("uavgnn_head_fwd", "uavgnn_tarmac_msg_fwd_rowmax", "uavgnn_gemm_tn_h2"):
        assert _count(main_n, name) == _count(main_p, name), f"{name}: {_count(main_n, name)} calls, plain {_count(main_p, name)} (staging)"
    assert _count(ext_n, "uavgnn_noisy_fold") == 2, "one fold per network"
    assert _count(ext_n, "uavgnn_noisy_fold_bwd") == 1, "one transpose per loss"
    assert _count(ext_n, "uavgnn_noisy_head_fwd") == 0 and _count(ext_n, "uavgnn_noisy_noise") == 0

    # learner.act: the per-row launch, one step consumed; an evaluation-style forward: neither
    _set_pairs(noisy)
    obs, h = batch["obs"][0].fresh(), batch["h0"]
    (acts, h2), main_a, ext_a = _spied(lambda: noisy.act(obs, h, 0.0))
    assert acts.shape == (B * n,) and _count(ext_a, "uavgnn_noisy_head_fwd") == 1 and _count(main_a, "uavgnn_head_fwd") == 0
    assert _count(ext_a, "uavgnn_noisy_fold") == 0
    assert noisy.policy_net.f_out.rng_state.tolist() == [PAIRS[0][0], PAIRS[0][1] + 1]
    assert noisy.target_net.f_out.rng_state.tolist() == list(PAIRS[1])
    with th.no_grad():
        (q_eval, _), main_e, ext_e = _spied(lambda: noisy.policy_net(batch["obs"][0].fresh(), h))
    assert not ext_e.calls and _count(main_e, "uavgnn_head_fwd") == 1
    assert noisy.policy_net.f_out.rng_state.tolist() == [PAIRS[0][0], PAIRS[0][1] + 1], "an evaluation consumes nothing"
    pf = noisy.policy_net.f_out
    with th.no_grad():
        from uav_bs_ctrl_amd import ops
        assert th.equal(q_eval, ops.head_fwd(h2, pf.weight, pf.bias)), "an evaluation is the plain head on the means"
        # the rollout's rows are the stream's: the launch over h' at the pair the act consumed
        with noisy.rollout_noise():
            _set_pairs(noisy)
            q_roll, h_roll = noisy.policy_net(batch["obs"][0].fresh(), h)
        assert th.equal(h_roll, h2)
        rng = th.tensor(list(PAIRS[0]), dtype=th.int64, device="cuda")
        assert th.equal(q_roll, ops.head_fwd(h2, pf.weight, pf.bias, noisy=(pf.weight_sigma, pf.bias_sigma, rng)))
        assert th.equal(acts, q_roll.argmax(1)), "eps = 0: the actions are the noisy rows' maxima"


# ---- (c): c = None and exp1 on the unroll route --------------------------------------------------------------------------------------
def test_update_without_communication_equals_the_plain_update_at_the_folds():
    B, n, M, T = 32, 8, 10, 3                   # "256 rows": the unrolled case of tests/test_learner_dueling_gpu.py
    noisy, batch = _exp3_learner(B, n, M, T, SIGMA0, c=None)
    plain, _ = _exp3_learner(B, n, M, T, None, c=None)
    main_n, ext_n, main_p = _twin_check("c=None 256 rows", noisy, plain, batch)
    assert _count(main_n, "uavgnn_gru_rec_fwd") > 0 and _count(main_n, "uavgnn_gru_rec_fwd") == _count(main_p, "uavgnn_gru_rec_fwd"), "the unroll route"
    assert _count(ext_n, "uavgnn_noisy_fold") == 2 and _count(ext_n, "uavgnn_noisy_fold_bwd") == 1


def _exp1(noisy, agent="rnn", B=32, T=10, H=256, seed=17):
    """tests/test_exp1_unroll_gpu.py::_build's learner at the reference's operating point, with the option."""
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    th.manual_seed(seed)
    p = SingleUbsParams(n_grps=4, gts_per_grp=5, episode_limit=4 * T)
    env = BatchedSingleUbsCoverageEnv(p, B, seed=3)
    args = types.SimpleNamespace(device="cuda", agent=agent, hidden_size=H, n_heads=4, n_layers=2, max_seq_len=T, gamma=0.99, polyak=0.995,
                                 batch_size=B, lr=5e-4, anneal_lr=False, seed=seed)
    return QLearner(env.get_env_info(agent), args, noisy=noisy), env, p


def test_exp1_update_equals_the_plain_update_at_the_folds():
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    B, T, H = 32, 10, 256
    noisy, env, p = _exp1(SIGMA0)
    plain, _, _ = _exp1(None)
    assert not hasattr(noisy.args, "mixer") or noisy.args.mixer is False
    gen = th.Generator(device="cuda").manual_seed(17)
    with th.no_grad():
        for prm in noisy.target_net.parameters():
            prm.add_(0.01 * th.randn(prm.shape, device="cuda", generator=gen))
    buf = SingleUbsSequenceReplay(B, T, p.n_gts, H, n_envs=B, device="cuda")
    obs, h = env.reset(), noisy.init_hidden(B)
    for _ in range(T):                      # a training rollout of the noisy learner itself fills the ring
        a, h2 = noisy.act(env.observations()["flat"], h, 0.3)
        buf.stage_obs(dict(gt=obs["gt"], agent=obs["agent"], h=h))
        obs, rew, done, info = env.step(a)
        noisy.cache(buf, None, None, a, rew, obs, h2, done, info["BadMask"], staged=True)
        h = h2
    assert len(buf) == B and int(noisy.policy_net.f_out.rng_state[1]) == T, "one step per rollout launch"
    batch = buf.gather(th.arange(B, device="cuda"), "rnn")
    main_n, ext_n, main_p = _twin_check("exp1 rnn", noisy, plain, batch)
    assert _count(main_n, "uavgnn_gru_rec_fwd") > 0 and _count(main_n, "uavgnn_gru_rec_fwd") == _count(main_p, "uavgnn_gru_rec_fwd"), "the unroll route"
    assert _count(ext_n, "uavgnn_noisy_fold") == 2 and _count(ext_n, "uavgnn_noisy_fold_bwd") == 1


# ---- (d): rollout and evaluation modes ------------------------------------------------------------------------------------------------
def _multi(noisy=SIGMA0, seed=3, Hs=64):
    """tests/test_learner_dueling_gpu.py::_multi (debug map, H = 64: the narrowest width the head kernels cover) with the option."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(seed)
    E = 4
    env = BatchedUbsCoverageEnv.from_map("debug", E, seed=11)
    args = types.SimpleNamespace(device="cuda", hidden_size=Hs, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                                 dueling=False, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9, max_seq_len=None,
                                 batch_size=4, seed=seed)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    return MultiAgentQLearner(info, args, noisy=noisy), env


def test_rollout_steps_advance_the_pair_and_repeat_when_it_is_put_back():
    learner, env = _multi()
    env.reset()
    h = 0.1 * th.randn(env.B * env.n_agents, 64, device="cuda")
    _set_pairs(learner)

    @th.no_grad()
    def roll():
        with learner.rollout_noise():
            return learner.policy_net(env.graph(), h)
    (q1, h1), (q2, h2) = roll(), roll()
    assert th.equal(h1, h2) and not th.equal(q1, q2), "the same h', other noise: the step advanced"
    assert float((q1 == q2).float().mean()) < 0.01
    assert learner.policy_net.f_out.rng_state.tolist() == [PAIRS[0][0], PAIRS[0][1] + 2]
    _set_pairs(learner)
    (q3, _), (q4, _) = roll(), roll()
    assert th.equal(q3, q1) and th.equal(q4, q2), "the pair put back: the same rows"
    with th.no_grad():
        q_mean = learner.policy_net(env.graph(), h)[0]
    assert learner.policy_net.f_out.rng_state.tolist() == [PAIRS[0][0], PAIRS[0][1] + 2], "outside the scope nothing is consumed"
    assert not th.equal(q_mean, q1)
    # the same hidden state in every row: with a draw shared by a team or by the launch the rows would repeat
    same = h[:1].expand_as(h).contiguous()
    with th.no_grad(), learner.rollout_noise():
        q_same = learner.policy_net.f_out(same)
    assert len({tuple(r.tolist()) for r in q_same}) == q_same.shape[0], "every agent of every environment has its own draw"


def test_graphed_evaluation_does_not_depend_on_the_pair():
    from uav_bs_ctrl_amd.graphs import GraphedEvaluation
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    learner, _ = _multi()
    _set_pairs(learner)
    test_env = BatchedUbsCoverageEnv.from_map("debug", 4, seed=31)
    ev = GraphedEvaluation(learner, test_env, 8, eps=0.05, seed=5, enc="gnn")
    env_pair, ev_pair = test_env.reset_rng.clone(), ev.rng.clone()
    tables = []
    for pairs in (PAIRS, ((1, 0), (2, 0))):
        test_env.reset_rng.copy_(env_pair)
        ev.rng.copy_(ev_pair)
        for net, (seed, step) in zip((learner.policy_net, learner.target_net), pairs):
            net.f_out.rng_state.copy_(th.tensor([seed, step], dtype=th.int64))
        ev()
        th.cuda.synchronize()
        tables.append(ev.table.clone())
        assert learner.policy_net.f_out.rng_state.tolist() == list(pairs[0]), "an evaluation consumes nothing"
    assert bool(th.isfinite(tables[0]).all()) and th.equal(tables[0], tables[1])

"""`-m gpu`: the noisy-net Q head through ``Run`` at the smallest sizes of tests/run_args.py ('debug' map, 4 environments, batch 4; H = 64,
the narrowest width csrc/ext/noisy_head.hip covers): ``Run.create(..., noisy=0.5)`` trains the sigmas, ``config.json`` / checkpoints /
``state.pt`` carry what they must, a run killed and resumed ends bit for bit where the uninterrupted one ends, a ``GraphedEpisode`` equals
the eager ``Episode``, ``series`` evaluates the directory with the means, and a run without the option writes no key."""
import json
import math
import types

import pytest
import torch as th

from tests.gpu_util import _LibSpy
from tests.run_args import small_args
from tests.test_run_gpu import _differences, _run_state, _without_time

pytestmark = pytest.mark.gpu

E, E_TEST, SEED, SIGMA0 = 4, 2, 3, 0.5


def _create(out, exp="exp3", env="debug", epochs=2, **kw):
    from uav_bs_ctrl_amd.run import Run
    over = dict(epochs=epochs) if exp == "exp1" else dict(epochs=epochs, hidden_size=64)
    return Run.create(exp, env, small_args(exp, **over), str(out), exp_name="noisy", seed=SEED, n_envs=E, n_test_envs=E_TEST, **kw)


def _sigmas(learner):
    f = learner.policy_net.f_out
    return th.cat((f.weight_sigma.detach().flatten(), f.bias_sigma.detach().flatten())).clone()


def test_a_run_with_the_option_trains_the_sigmas_and_writes_what_it_must(tmp_path):
    from uav_bs_ctrl_amd.agents.heads import NoisyLinear
    run = _create(tmp_path / "on", noisy=SIGMA0)
    lr = run.learner
    assert run.noisy == SIGMA0 and isinstance(lr.policy_net.f_out, NoisyLinear) and isinstance(lr.target_net.f_out, NoisyLinear)
    assert not hasattr(run.args, "noisy"), "the learner works on a copy of args"
    s0 = _sigmas(lr)
    assert th.equal(s0, th.full_like(s0, SIGMA0 / math.sqrt(64)))
    pairs0 = [m.rng_state.clone() for m in (lr.policy_net.f_out, lr.target_net.f_out)]
    assert all(int(p[1]) == 0 for p in pairs0) and int(pairs0[0][0]) != int(pairs0[1][0]), "seeded before the captures, each network its own"
    run.train()
    run.logger.close()
    s1 = _sigmas(lr)
    assert bool(th.isfinite(s1).all()) and float((s1 != s0).float().mean()) > 0.5, "the TD loss trains the sigmas"
    steps = [int(m.rng_state[1]) for m in (lr.policy_net.f_out, lr.target_net.f_out)]
    assert steps[0] > steps[1] > 0, f"rollout launches and folds consumed the policy's steps, folds the target's: {steps}"
    out = tmp_path / "on"
    assert json.loads((out / "config.json").read_text())["uav_bs_ctrl_amd"]["noisy"] == SIGMA0
    ck = th.load(str(out / "checkpoint_epoch2.pt"), map_location="cpu")
    assert {"f_out.weight", "f_out.bias", "f_out.weight_sigma", "f_out.bias_sigma"} <= set(ck["model_state_dict"])
    assert th.equal(ck["comm_rng_state"]["f_out"], lr.policy_net.f_out.rng_state.cpu())
    st = th.load(str(out / "state.pt"), map_location="cpu")["tensors"]
    assert th.equal(st["comm.policy.f_out"], lr.policy_net.f_out.rng_state.cpu())
    assert th.equal(st["comm.target.f_out"], lr.target_net.f_out.rng_state.cpu())
    losses = [float(r[_without_time(out)[0].index("LossQ")]) for r in _without_time(out)[1]]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)


@pytest.mark.parametrize("exp", ["exp3", "exp1"])
def test_a_resumed_noisy_run_ends_where_the_uninterrupted_run_ends(tmp_path, exp):
    from uav_bs_ctrl_amd.run import Run
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    env = "debug" if exp == "exp3" else SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10)
    extra = dict(prioritized=(0.6, 0.4, 0.9, 1e-3), returns=("lambda", 0.8), compact_replay=True) if exp == "exp3" else {}
    whole = _create(tmp_path / "whole", exp, env, epochs=4, noisy=SIGMA0, **extra)      # (composition: the other opt-in options beside it)
    whole.train()
    want = _run_state(whole)
    whole.logger.close()
    del whole
    part = _create(tmp_path / "part", exp, env, epochs=4, noisy=SIGMA0, **extra)
    part.train(epochs=2)
    part.logger.close()
    del part
    th.cuda.synchronize()
    th.manual_seed(12345)                                  # nothing of the resumed run may depend on the process's generator
    run = Run.resume(str(tmp_path / "part"))
    assert run.noisy == SIGMA0 and run.epoch == 2
    run.train()
    run.logger.close()
    got = _run_state(run)
    assert {"comm.policy.f_out", "comm.target.f_out"} <= set(got)
    assert not _differences(want, got), _differences(want, got)
    assert _without_time(tmp_path / "part") == _without_time(tmp_path / "whole") and len(_without_time(tmp_path / "part")[1]) == 4


def _multi(seed=3):
    """tests/test_learner_dueling_gpu.py::_multi with the noisy head (H = 64), the pairs seeded as ``Run`` seeds them."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.run import seed_comm_modules
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(seed)
    E_, Hs = 4, 64
    env = BatchedUbsCoverageEnv.from_map("debug", E_, seed=11)
    args = types.SimpleNamespace(device="cuda", hidden_size=Hs, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                                 dueling=False, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9, max_seq_len=None,
                                 batch_size=4, seed=seed)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    learner = MultiAgentQLearner(info, args, noisy=SIGMA0)
    seed_comm_modules(learner, 77)
    rb = SequenceReplay(8, env.episode_limit, env.n_agents, env.n_gts, Hs, n_envs=E_, state_dim=env.state_dim, r_comm=env.p.r_comm,
                        device_state=True, seed=21)
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 200.0), enc="gnn")


def test_graphed_episode_with_the_noisy_head_replays_the_eager_episode(monkeypatch):
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    spy = _LibSpy(L.ext())
    monkeypatch.setattr(L, "ext", lambda: spy)
    l_e, env_e, rb_e, kw = _multi()
    l_g, env_g, rb_g, _ = _multi()
    assert th.equal(l_e.flat.flat, l_g.flat.flat), "the two learners were not built from the same seed"
    p0 = l_e.flat.flat.clone()
    eager, graphed = Episode(l_e, env_e, rb_e, **kw), GraphedEpisode(l_g, env_g, rb_g, **kw)
    names = {n for n, _ in spy.calls}
    assert {"uavgnn_noisy_head_fwd", "uavgnn_noisy_fold", "uavgnn_noisy_fold_bwd"} <= names, f"the capture took {sorted(names)}"
    assert th.equal(l_g.flat.flat, p0), "the warm-up left its traces"
    assert [m.rng_state.tolist() for m in (l_g.policy_net.f_out, l_g.target_net.f_out)] == [[77, 0], [78, 0]], "... in the pairs"
    out_e, out_g = eager(), graphed()
    th.cuda.synchronize()
    monkeypatch.undo()
    assert th.equal(out_e["LossQ"], out_g["LossQ"]) and bool(th.isfinite(out_g["LossQ"]))
    assert not th.equal(l_g.flat.flat, p0), "the episode did not train"
    size = int(rb_g.state[1])
    assert size > 0 and rb_g.state.tolist() == rb_e.state.tolist()
    assert th.equal(l_e.flat.flat, l_g.flat.flat), "parameters"
    assert th.equal(l_e.flat_target, l_g.flat_target), "target"
    bad = [k for k in rb_e.mem if not th.equal(rb_e.mem[k][:size], rb_g.mem[k][:size])]
    assert not bad, f"ring (actions among it): {bad}"
    for net in ("policy_net", "target_net"):
        a, b = getattr(l_e, net).f_out.rng_state, getattr(l_g, net).f_out.rng_state
        assert th.equal(a, b) and int(a[1]) > 0, f"{net}: pairs {a.tolist()} / {b.tolist()}"
    out_e2, out_g2 = eager(), graphed()            # a second replay continues the stream where an eager run continues it
    th.cuda.synchronize()
    assert th.equal(out_e2["LossQ"], out_g2["LossQ"]) and th.equal(l_e.flat.flat, l_g.flat.flat)


def test_series_evaluates_the_directory_with_the_means_and_a_plain_run_writes_no_key(tmp_path):
    from uav_bs_ctrl_amd import series as S
    from uav_bs_ctrl_amd.agents.heads import NoisyLinear
    from uav_bs_ctrl_amd.run import Run
    run = _create(tmp_path / "on", noisy=SIGMA0)
    run.train()
    run.logger.close()
    del run
    d = S.describe(str(tmp_path / "on"), "cuda")
    assert d.args.noisy == SIGMA0 and dict(d.key[2:])["noisy"] == SIGMA0
    runner = S.PolicyRunner(d, 4, n_envs=2)
    head = runner.learner.policy_net.f_out
    assert isinstance(head, NoisyLinear)
    path = str(tmp_path / "on" / "checkpoint_epoch2.pt")
    tables = [runner(path, 5)]
    ck = th.load(path, map_location="cuda")
    sd = ck["model_state_dict"]
    assert th.equal(head.weight_sigma, sd["f_out.weight_sigma"]) and th.equal(head.weight, sd["f_out.weight"]), "the checkpoint loads into it"
    assert float(sd["f_out.weight_sigma"].abs().min()) > 0
    # the same checkpoint with its sigmas zeroed: whatever noise an evaluation drew would vanish with them
    sd["f_out.weight_sigma"], sd["f_out.bias_sigma"] = th.zeros_like(sd["f_out.weight_sigma"]), th.zeros_like(sd["f_out.bias_sigma"])
    th.save(ck, str(tmp_path / "zeroed.pt"))
    tables.append(runner(str(tmp_path / "zeroed.pt"), 5))
    assert float(head.weight_sigma.abs().max()) == 0.0
    assert tables[0].keys() == tables[1].keys() and all((tables[0][k] == tables[1][k]).all() for k in tables[0]), "evaluated with the means"

    off = _create(tmp_path / "off")
    assert off.noisy is None and type(off.learner.policy_net.f_out) is th.nn.Linear and off.learner._noisy_policy == []
    off.train(epochs=1)
    off.logger.close()
    assert "noisy" not in json.loads((tmp_path / "off" / "config.json").read_text())["uav_bs_ctrl_amd"]
    st = th.load(str(tmp_path / "off" / "state.pt"), map_location="cpu")["tensors"]
    assert not any(k.startswith("comm.") for k in st), "no pair without the option"
    del off
    back = Run.resume(str(tmp_path / "off"))
    assert back.noisy is None and type(back.learner.policy_net.f_out) is th.nn.Linear
    back.logger.close()
    assert dict(S.describe(str(tmp_path / "off"), "cuda").key[2:])["noisy"] is None

"""`-m gpu`: ``uav_bs_ctrl_amd.run.Run`` - the ``train()`` driver over the device loop.

Sizes: map 'debug' (3 UBSs x 4 GTs, episode limit 10, T = 10) for the multi-UBS setups, ``SingleUbsParams(n_grps=2, gts_per_grp=3,
episode_limit=10)`` with T = 5 for exp1; H = 32, 4 training environments, batch 4, a ring of 8 (it wraps and is full when saved),
steps_per_epoch = 80 (two episode replays), update_after = 40 (the first replay collects, every later one trains), 4 evaluation episodes on
2 evaluation environments, save_freq = 2, lr annealing on.

1. the driver adds nothing: three epochs of ``Run.train()`` end bit for bit where the loop of INTEGRATION.md ends, written out here;
2. eager equals graphed;  3. a run interrupted after two of four epochs and resumed ends bit for bit where the uninterrupted one ends;
4. ``save_replay=False``;  5. the run directory;  6. ``explore_seed`` of ``Episode`` / ``GraphedEpisode``;  7. divergence."""
import json
import os
import shutil
import types

import numpy as np
import pytest
import torch as th

from tests.run_args import small_args

pytestmark = pytest.mark.gpu

E, E_TEST, SEED = 4, 2, 3


def _setup(name, **over):
    """(exp, env, args) of the three setups."""
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    if name == "exp1-rnn":
        return "exp1", SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10), small_args("exp1", **over)
    return "exp3", "debug", small_args("exp3", c={"multi-tarmac": "tarmac", "multi-disc": "disc"}[name], **over)


SETUPS = ("multi-tarmac", "multi-disc", "exp1-rnn")


def _create(name, out, **kw):
    from uav_bs_ctrl_amd.run import Run
    over = {k: kw.pop(k) for k in list(kw) if k in ("epochs",)}
    exp, env, args = _setup(name, **over)
    return Run.create(exp, env, args, str(out), exp_name=name, seed=SEED, n_envs=E, n_test_envs=E_TEST, **kw)


def _state(learner, replay, collect, train, evaluation, env, test_env, film):
    """Every tensor a run leaves behind: parameters, target, Adam moments, hyper, ring rows below `size`, all counters, the random pairs,
    the evaluation's table and film."""
    from uav_bs_ctrl_amd.run import comm_modules
    opt = learner.optimizer
    single = not hasattr(env, "map_rng")
    out = dict(params=learner.flat.flat, target=learner.flat_target, adam_m=opt.m, adam_v=opt.v, hyper=opt.hyper, state=replay.state,
               rng=replay.rng, status=replay.status, eval_rng=evaluation.rng, table=evaluation.table, film=film.buf,
               env_rng=env.rng if single else env.map_rng, test_env_rng=test_env.rng if single else test_env.map_rng)
    for n, ep in (("collect", collect), ("train", train)):
        out.update({f"{n}.t": ep.t, f"{n}.eps": ep.eps, f"{n}.explore": ep.explore})
    size = int(replay.state[1])
    out.update({"mem." + k: v[:size] for k, v in replay.mem.items()})
    out.update({"comm." + n: m.rng_state for n, m in comm_modules(learner)})
    return {k: v.detach().clone() for k, v in out.items()}


def _run_state(run):
    return _state(run.learner, run.replay, run.collect, run.train_episode, run.evaluation, run.env, run.test_env, run.film)


def _differences(a, b):
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    return [k for k in a if a[k].shape != b[k].shape or not th.equal(a[k], b[k])]


def _rows(out):
    """(header, [row cells]) of progress.txt."""
    lines = (out / "progress.txt").read_text().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [line.split("\t") for line in lines[1:-1]]


def _without_time(out):
    head, rows = _rows(out)
    i = head.index("Time")
    return head, [r[:i] + r[i + 1:] for r in rows]


_CACHE = {}


def _three_epochs(name, tmp_path_factory):
    """The graphed three-epoch run of a setup, once per session: (directory, final state, host counters)."""
    if name not in _CACHE:
        out = tmp_path_factory.mktemp(name.replace("-", "_")) / "run"
        run = _create(name, out)
        run.train()
        run.logger.close()
        _CACHE[name] = (out, _run_state(run), dict(epoch=run.epoch, replays=run.replays, interacts=run.interacts, active=run.active))
        del run
    return _CACHE[name]


# ---- 1. the driver adds nothing ---------------------------------------------------------------------------------------------------------
def _hand_loop(name, epochs):
    """INTEGRATION.md's three snippets put together by hand, from the run's seeds: returns (final state, [summary() per epoch])."""
    from uav_bs_ctrl_amd import run as R
    from uav_bs_ctrl_amd.film import Film
    from uav_bs_ctrl_amd.graphs import GraphedEpisode, GraphedEvaluation
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner, QLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay, SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
    from uav_bs_ctrl_amd.stats import EpochStats
    exp, spec, args = _setup(name)
    args = types.SimpleNamespace(**args)
    seeds = R.derive_seeds(SEED)
    th.manual_seed(seeds["torch"])
    if exp == "exp1":
        enc, T = args.agent, args.max_seq_len
        env, test_env = (BatchedSingleUbsCoverageEnv(spec, B, seed=seeds[k]) for B, k in ((E, "train_env"), (E_TEST, "test_env")))
        learner = QLearner(env.get_env_info(enc), args)
        rb = SingleUbsSequenceReplay(args.replay_size, T, env.n_gts, args.hidden_size, n_envs=E, device_state=True, seed=seeds["replay"])
        keys = ["EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx"]
    else:
        enc, T = "gnn", 10
        env, test_env = (BatchedUbsCoverageEnv.from_map(spec, B, seed=seeds[k]) for B, k in ((E, "train_env"), (E_TEST, "test_env")))
        learner = MultiAgentQLearner(env.get_env_info(enc), args)
        rb = SequenceReplay(args.replay_size, T, env.n_agents, env.n_gts, args.hidden_size, n_envs=E, r_comm=env.p.r_comm,
                            device_state=True, seed=seeds["replay"])
        keys = ["EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx", "ProbCollision"]
    R.seed_comm_modules(learner, seeds["comm"])
    st = EpochStats(keys + ["LossQ"] + ["Test" + k for k in keys], "cuda")
    film = Film(test_env, args.num_test_episodes)
    kw = dict(eps=(1.0, 0.05, args.decay_steps), enc=enc, stats=st, explore_seed=seeds["explore"])
    collect = GraphedEpisode(learner, env, rb, args.batch_size, train=False, **kw)
    train = GraphedEpisode(learner, env, rb, args.batch_size, train=True, **kw)
    test_agent = GraphedEvaluation(learner, test_env, args.num_test_episodes, eps=0.05, seed=seeds["evaluation"], enc=enc, stats=st, film=film)
    update_after = max(args.update_after, args.batch_size * T)
    rows, interacts = [], 0
    for _ in range(epochs):
        for _ in range(args.steps_per_epoch // (E * env.episode_limit)):
            collecting = interacts < update_after
            if not collecting and int(train.t) == 0:
                train.t.copy_(collect.t)
                train.explore.copy_(collect.explore)
            (collect if collecting else train)()
            interacts += E * env.episode_limit
        test_agent()
        learner.lr_scheduler.step()
        rows.append(st.summary())
        st.reset()
    rb.check()
    return _state(learner, rb, collect, train, test_agent, env, test_env, film), rows


@pytest.mark.parametrize("name", SETUPS)
def test_the_driver_ends_where_the_hand_written_loop_ends(name, tmp_path_factory):
    out, state, counters = _three_epochs(name, tmp_path_factory)
    hand, summaries = _hand_loop(name, 3)
    assert not _differences(state, hand), _differences(state, hand)
    assert counters == dict(epoch=3, replays=6, interacts=240, active="train")
    assert state["state"].tolist()[1] == 8 and int(state["train.t"]) == 240 and int(state["collect.t"]) == 40
    assert state["train.explore"].tolist()[1] == 60 and state["eval_rng"].tolist()[1] == 3 * 2 * 10, "one draw per step"
    assert not th.equal(state["params"], state["target"]) and float(state["hyper"][1]) == (5 if name != "exp1-rnn" else 10)
    head, rows = _rows(out)
    assert len(rows) == 3 and [r[0] for r in rows] == ["1", "2", "3"]
    assert [r[head.index("Episode")] for r in rows] == ["8", "16", "24"]
    assert [r[head.index("TotalEnvInteracts")] for r in rows] == ["80", "160", "240"]
    for cells, s in zip(rows, summaries):
        for col, cell in zip(head, cells):
            key = col if col in s else "Average" + col
            if key in s:                                   # a statistics column: the text of the hand loop's value
                assert cell == str(s[key]), (col, cell, s[key])
        assert s["NLossQ"] > 0 and s["NonFiniteLossQ"] == 0 and s["NTestEpRet"] == 4 and s["NEpRet"] == 8
    assert all(np.isfinite(float(c)) for r in rows for c in r)
    if name == "exp1-rnn":
        from uav_bs_ctrl_amd.run import eps_thres
        assert [r[head.index("ExploreEps")] for r in rows] == [str(eps_thres(t, 200.0)) for t in (79, 159, 239)]
        assert "ProbCollision" not in head and head.index("FairIdx") < head.index("TotalThroughput")


# ---- 2. eager equals graphed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETUPS)
def test_the_eager_run_ends_where_the_graphed_run_ends(name, tmp_path, tmp_path_factory):
    out, state, _ = _three_epochs(name, tmp_path_factory)
    run = _create(name, tmp_path / "eager", graphed=False)
    run.train()
    run.logger.close()
    assert not _differences(state, _run_state(run)), _differences(state, _run_state(run))
    assert _without_time(tmp_path / "eager") == _without_time(out)


# ---- 3. resume --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETUPS)
def test_a_resumed_run_ends_where_the_uninterrupted_run_ends(name, tmp_path):
    from uav_bs_ctrl_amd.run import Run, RunDirectoryError
    whole = _create(name, tmp_path / "whole", epochs=4)
    whole.train()
    want = _run_state(whole)
    whole.logger.close()
    del whole
    part = _create(name, tmp_path / "part", epochs=4)
    part.train(epochs=2)
    assert part.epoch == 2 and os.path.exists(tmp_path / "part" / "state.pt") and not os.path.exists(tmp_path / "part" / "state.pt.tmp")
    part.logger.close()
    del part
    th.cuda.synchronize()
    th.manual_seed(12345)                                  # nothing of the resumed run may depend on the process's generator
    run = Run.resume(str(tmp_path / "part"))
    assert (run.epoch, run.replays, run.interacts, run.active) == (2, 4, 160, "train") and len(run.replay) == 8
    run.train()
    run.logger.close()
    got = _run_state(run)
    assert not _differences(want, got), _differences(want, got)
    assert run.epoch == 4 and int(got["train.t"]) == 320
    head, rows = _without_time(tmp_path / "part")
    assert (head, rows) == _without_time(tmp_path / "whole") and len(rows) == 4
    assert (tmp_path / "part" / "progress.txt").read_text().count("Epoch\t") == 1, "one header"
    t_head, t_rows = _rows(tmp_path / "part")
    times = [float(r[t_head.index("Time")]) for r in t_rows]
    assert times == sorted(times), "Time accumulates across the resume"
    a, b = (th.load(str(tmp_path / d / "checkpoint_epoch4.pt"), map_location="cpu") for d in ("whole", "part"))
    assert a["model_state_dict"].keys() == b["model_state_dict"].keys() and a["epoch"] == b["epoch"] == 4 and a["t"] == b["t"] == 319
    assert all(th.equal(a["model_state_dict"][k], b["model_state_dict"][k]) for k in a["model_state_dict"])
    with pytest.raises(RunDirectoryError, match="already complete"):
        Run.resume(str(tmp_path / "part"))


# ---- 4. save_replay=False, and a config.json that no longer fits --------------------------------------------------------------------------
def test_a_run_resumed_without_its_ring_collects_again(tmp_path):
    from uav_bs_ctrl_amd.run import Run, RunDirectoryError
    part = _create("multi-tarmac", tmp_path / "part", save_replay=False)
    part.train(epochs=2)
    updates = part.replay.rng.tolist()[1]
    assert len(part.replay) == 8 and updates == 3 and part.active == "train"
    t_before = int(part.train_episode.t)
    part.logger.close()
    del part
    assert th.load(str(tmp_path / "part" / "state.pt"), map_location="cpu")["mem"] is None
    shutil.copytree(tmp_path / "part", tmp_path / "other")
    run = Run.resume(str(tmp_path / "part"))
    assert len(run.replay) == 0 and run.ring_base == 160 and run.replay.rng.tolist()[1] == updates
    run.train()
    # epoch 3: the first replay collects (0 < 40 interactions since the ring was emptied), the second one trains
    assert run.replay.rng.tolist()[1] == updates + 1 and run.active == "train" and len(run.replay) == 8
    assert int(run.train_episode.t) == t_before + 80 and int(run.collect.t) == t_before + 40, "the schedule went through both graphs"
    run.replay.check()
    run.logger.close()
    head, rows = _rows(tmp_path / "part")
    assert len(rows) == 3 and np.isfinite(float(rows[2][head.index("LossQ")]))
    # the same directory with another hidden size in config.json: the rebuilt tensors do not fit state.pt
    cfg = json.loads((tmp_path / "other" / "config.json").read_text())
    next(iter(cfg["args"].values()))["hidden_size"] = 64
    (tmp_path / "other" / "config.json").write_text(json.dumps(cfg))
    with pytest.raises(RunDirectoryError, match="does not rebuild the shapes"):
        Run.resume(str(tmp_path / "other"))


# ---- 5. the run directory -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multi-tarmac", "exp1-rnn"])
def test_the_run_directory(name, tmp_path, tmp_path_factory):
    from uav_bs_ctrl_amd.film import load_and_run_policy
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner, QLearner
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
    out, _, _ = _three_epochs(name, tmp_path_factory)
    names = sorted(os.listdir(out))
    assert names == sorted(["config.json", "progress.txt", "state.pt", "checkpoint_epoch2.pt", "checkpoint_epoch3.pt"]
                           + [f"epoch2_episode{n}" for n in range(4)]), names
    for n in range(4):
        d = out / f"epoch2_episode{n}"
        assert sorted(os.listdir(d)) == ["others.csv", "path_ubs.csv", "pos_gts.csv"]
        assert len((d / "path_ubs.csv").read_text().strip().split("\n")) == 3 + 10 + 1       # three header lines, episode_limit + 1 rows
    cfg = json.loads((out / "config.json").read_text())
    assert cfg["exp_name"] == name and cfg["seed"] == SEED and cfg["uav_bs_ctrl_amd"]["n_envs"] == E
    args = types.SimpleNamespace(**list(cfg["args"].values())[0])                            # as test_policies.py:47-60 reads it
    exp, spec, _ = _setup(name)
    if exp == "exp1":
        assert cfg["env_fn"] == "SingleUbsCoverageEnv" and cfg["env_kwargs"]["n_grps"] == 2
        env = BatchedSingleUbsCoverageEnv(spec, 2, seed=5)
        learner, enc = QLearner(env.get_env_info(args.agent), args), args.agent
    else:
        assert cfg["env_fn"] == "MultiUbsCoverageEnv" and cfg["env_kwargs"]["map_id"] == "debug"
        env = BatchedUbsCoverageEnv.from_map(cfg["env_kwargs"]["map_id"], 2, seed=5)
        learner, enc = MultiAgentQLearner(env.get_env_info("gnn"), args), "gnn"
    rsts = load_and_run_policy(str(out / "checkpoint_epoch3.pt"), learner, env, 2, str(tmp_path / "films"), seed=1, enc=enc)
    assert rsts["EpRet"].shape == (2,) and np.isfinite(rsts["EpRet"]).all() and os.path.exists(tmp_path / "films" / "episode1" / "path_ubs.csv")
    ck = th.load(str(out / "checkpoint_epoch3.pt"), map_location="cpu")
    assert ck["epoch"] == 3 and ck["t"] == 239 and "lr_scheduler_state_dict" in ck


def test_multi_ubs_env_info():
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    env = BatchedUbsCoverageEnv.from_map("r400", 2, seed=0)
    want = dict(state_shape=env.state_dim, n_actions=env.n_actions, n_agents=4, episode_limit=40)
    assert env.get_env_info("gnn") == dict(obs_shape=dict(agent=2, ubs=2, gt=4), **want)
    assert env.get_env_info("mlp") == dict(obs_shape=31, **want)            # the width INTEGRATION.md quotes for 'r400'
    o = env.reset_from_map()
    assert sum(int(np.prod(o[k].shape[2:])) for k in ("agent", "gt", "ubs")) == 31
    with pytest.raises(ValueError, match="enc"):
        env.get_env_info("rnn")


# ---- 6. explore_seed ------------------------------------------------------------------------------------------------------------------------
def test_explore_seed_selects_by_the_philox_rule_from_the_episodes_own_pair():
    from tests import eval_ref
    from tests.test_graphed_episode_gpu import SETUPS as EP_SETUPS
    from uav_bs_ctrl_amd.graph import from_padded_obs
    from uav_bs_ctrl_amd.graphs import Episode
    learner, env, rb, kw = EP_SETUPS["multi-tarmac"]()
    kw = dict(kw, eps=(0.5, 0.05, 200.0))                  # step 0 explores with probability 0.5: both branches of the rule
    gen = learner._gen.get_state()
    ep = Episode(learner, env, rb, train=False, explore_seed=21, **kw)
    assert ep.explore.tolist() == [21, 0]
    ep()
    assert ep.explore.tolist() == [21, env.episode_limit], "the pair advances by one per step"
    assert th.equal(learner._gen.get_state(), gen), "the learner's generator was used"
    m, n = rb.mem, env.n_agents                            # the E sequences just committed: step 0 of each
    with th.no_grad():
        obs = from_padded_obs(m["gt"][:env.B, 0], m["ubs"][:env.B, 0], m["agent"][:env.B, 0], m["d_u2u"][:env.B, 0], env.p.r_comm, static=True)
        q, _ = learner.policy_net(obs, learner.init_hidden(env.B))
    assert float(m["h"][:env.B, 0].abs().max()) == 0.0
    want = eval_ref.eps_greedy_philox(q.cpu().numpy(), learner.n_actions, n, 21, 0, np.float32(0.5))
    got = m["act"][:env.B, 0].reshape(-1).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    u_team, _ = eval_ref.draws(21, 0, env.B * n, n)
    assert 0 < int((u_team <= np.float32(0.5)).sum()) < env.B, "the seed leaves one branch untested"


@pytest.mark.parametrize("name", ["multi-tarmac", "exp1-rnn"])
def test_graphed_episode_with_explore_seed_replays_the_eager_one(name):
    from tests.test_graphed_episode_gpu import SETUPS as EP_SETUPS, _snapshot
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    l_e, env_e, rb_e, kw = EP_SETUPS[name]()
    l_g, env_g, rb_g, _ = EP_SETUPS[name]()
    eager, graphed = Episode(l_e, env_e, rb_e, explore_seed=9, **kw), GraphedEpisode(l_g, env_g, rb_g, explore_seed=9, **kw)
    assert graphed.explore.tolist() == [9, 0], "the warm-up left its draws"
    for ep in range(3):
        out_e, out_g = eager(), graphed()
        assert th.equal(out_e["LossQ"], out_g["LossQ"]) and th.equal(eager.explore, graphed.explore), f"episode {ep}"
        a, b = _snapshot(l_e, env_e, rb_e, eager), _snapshot(l_g, env_g, rb_g, graphed)
        size = int(rb_g.state[1])
        bad = [k for k in a if not (th.equal(a[k][:size], b[k][:size]) if k.startswith("mem.") else th.equal(a[k], b[k]))]
        assert not bad, f"episode {ep}: {bad}"
    assert size == rb_g.capacity, "the ring was not compared whole"
    assert 3 * env_g.episode_limit // rb_g.T * env_g.B > rb_g.capacity, "the configuration does not wrap the ring"
    assert graphed.explore.tolist() == [9, 3 * env_g.episode_limit]
    rb_g.check()


# ---- 7. divergence ----------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_loss_stops_the_run_after_its_row(tmp_path):
    from uav_bs_ctrl_amd.run import TrainingDiverged
    run = _create("multi-tarmac", tmp_path / "run")
    run.learner.flat.flat.fill_(float("inf"))
    run.learner.invalidate_weight_cache()
    with pytest.raises(TrainingDiverged, match="epoch 1"):
        run.train()
    run.logger.close()
    head, rows = _rows(tmp_path / "run")
    assert len(rows) == 1 and rows[0][0] == "1" and rows[0][head.index("LossQ")] == "nan"
    assert not os.path.exists(tmp_path / "run" / "state.pt") and run.epoch == 0

"""`-m gpu`: prioritised replay through the device loop at the sizes of tests/test_graphed_episode_gpu.py and tests/test_run_gpu.py
('debug' map, 4 environments, batch 4): ``GraphedEpisode`` = ``Episode`` bit for bit over three episodes with the option on (exp3 TarMAC,
the compact ring, exp1) - priorities and their maximum included; what a commit and an update leave in ``prio``; and ``Run``: a resumed
run ends where the uninterrupted one ends, ``state.pt`` holds the two tensors, a directory written without the key builds none."""
import json
import types

import pytest
import torch as th

from tests.run_args import small_args
from tests.test_run_compact_gpu import _final, _same, _without_time

pytestmark = pytest.mark.gpu

EPISODES = 3
PRIO = (0.6, 0.4, 0.9, 1e-3)
E, E_TEST, SEED, EPOCHS = 4, 2, 3, 2


def _multi(compact=False, seed=3):
    """tests/test_graphed_episode_gpu.py::_multi on a prioritised ring (``compact``: a CompactSequenceReplay)."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import CompactSequenceReplay, SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(seed)
    Hs = 32
    env = BatchedUbsCoverageEnv.from_map("debug", E, seed=11)
    args = types.SimpleNamespace(device="cuda", hidden_size=Hs, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                                 dueling=False, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9, max_seq_len=None,
                                 batch_size=4, seed=seed)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    learner = MultiAgentQLearner(info, args)
    if compact:
        rb = CompactSequenceReplay.for_env(env, 8, env.episode_limit, Hs, seed=21, prioritized=PRIO)
    else:
        rb = SequenceReplay(8, env.episode_limit, env.n_agents, env.n_gts, Hs, n_envs=E, state_dim=env.state_dim, r_comm=env.p.r_comm,
                            device_state=True, seed=21, prioritized=PRIO)
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 200.0), enc="gnn")


def _exp1(seed=4):
    """tests/test_graphed_episode_gpu.py::_exp1('rnn') on a prioritised ring: two segments, two updates per episode, the ring wraps."""
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    th.manual_seed(seed)
    Hs, T = 32, 5
    p = SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10)
    env = BatchedSingleUbsCoverageEnv(p, E, seed=12)
    args = types.SimpleNamespace(device="cuda", agent="rnn", hidden_size=Hs, n_heads=4, n_layers=2, max_seq_len=T, gamma=0.99,
                                 polyak=0.9, batch_size=4, lr=1e-3, anneal_lr=False, seed=seed)
    learner = QLearner(env.get_env_info("rnn"), args)
    rb = SingleUbsSequenceReplay(20, T, p.n_gts, Hs, n_envs=E, device_state=True, seed=22, prioritized=PRIO)
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 300.0), enc="rnn")


def _snapshot(learner, rb, ep):
    opt = learner.optimizer
    out = dict(params=learner.flat.flat, target=learner.flat_target, adam_m=opt.m, adam_v=opt.v, hyper=opt.hyper, state=rb.state,
               rng=rb.rng, status=rb.status, prio=rb.prio, prio_max=rb.prio_max, is_weights=rb.is_weights, t=ep.t, eps=ep.eps)
    out.update({"mem." + k: v for k, v in rb.mem.items()})
    return {k: v.clone() for k, v in out.items()}


SETUPS = {"multi-tarmac": _multi, "compact": lambda: _multi(compact=True), "exp1-rnn": _exp1}


@pytest.mark.parametrize("name", list(SETUPS))
def test_graphed_episode_replays_the_eager_episode_with_priorities(name):
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    from uav_bs_ctrl_amd.replay import PRIO_ONE
    l_e, env_e, rb_e, kw = SETUPS[name]()
    l_g, env_g, rb_g, _ = SETUPS[name]()
    p0 = l_e.flat.flat.clone()
    eager, graphed = Episode(l_e, env_e, rb_e, **kw), GraphedEpisode(l_g, env_g, rb_g, **kw)
    assert eager.upd.weights is rb_e.is_weights and graphed.upd.weights is rb_g.is_weights, "the update reads the sampler's weights in place"
    assert th.equal(l_g.flat.flat, p0) and rb_g.state.tolist() == [0, 0], "the warm-up left its traces"
    assert rb_g.prio.tolist() == [PRIO_ONE] * rb_g.capacity and rb_g.prio_max.tolist() == [PRIO_ONE], "the warm-up left its priorities"
    for ep in range(EPISODES):
        out_e, out_g = eager(), graphed()
        assert th.equal(out_e["LossQ"], out_g["LossQ"]) and th.equal(eager.idx, graphed.idx), f"episode {ep}"
        assert bool(th.isfinite(out_g["LossQ"])) and bool((graphed.idx[1:] >= graphed.idx[:-1]).all())
        a, b = _snapshot(l_e, rb_e, eager), _snapshot(l_g, rb_g, graphed)
        size = int(rb_g.state[1])
        bad = [k for k in a if not (th.equal(a[k][:size], b[k][:size]) if k.startswith("mem.") else th.equal(a[k], b[k]))]
        assert not bad, f"episode {ep}: {bad}"
    assert size == rb_g.capacity, "the ring was not compared whole"
    assert not th.equal(l_g.flat.flat, p0) and (rb_g.prio != PRIO_ONE).any(), "the episodes did not train or wrote no priority"
    assert int(rb_g.prio_max) >= PRIO_ONE and int(rb_g.prio.min()) >= 1
    rb_g.check()
    rb_e.check()


def test_what_a_commit_and_an_update_leave_in_prio():
    from uav_bs_ctrl_amd.graphs import Episode
    from uav_bs_ctrl_amd.replay import PRIO_ONE
    learner, env, rb, kw = _multi()
    train = Episode(learner, env, rb, **kw)
    collect = Episode(learner, env, rb, train=False, **kw)
    train()                                                  # 4 sequences committed at PRIO_ONE, one update on a batch of them
    sampled = train.idx.unique()
    assert rb.state.tolist() == [4, 4] and int(sampled.max()) < 4
    assert (rb.prio[sampled] != PRIO_ONE).all(), "the sampled slots kept the initial priority"
    rest = th.ones(8, dtype=th.bool, device="cuda")
    rest[sampled] = False
    assert (rb.prio[rest] == PRIO_ONE).all(), "a slot outside the batch was rewritten"
    top = int(rb.prio_max)
    assert top >= max(PRIO_ONE, int(rb.prio[sampled].max())), "prio_max is the running maximum (every valid row enters it)"
    assert (rb.is_weights == 1.0).all(), "a draw over equal priorities carries unit weights"
    rb.prio_max.fill_(top + 12345)
    before = rb.prio.clone()
    collect()                                                # commits slots 4..7 and updates nothing
    assert rb.state.tolist() == [0, 8] and (rb.prio[4:] == top + 12345).all(), "freshly committed slots hold prio_max"
    assert th.equal(rb.prio[:4], before[:4]) and int(rb.prio_max) == top + 12345
    rb.check()


# ---- through Run -------------------------------------------------------------------------------------------------------------------------
def _create(out, **kw):
    from uav_bs_ctrl_amd.run import Run
    return Run.create("exp3", "debug", small_args("exp3", epochs=EPOCHS), str(out), exp_name="prio", seed=SEED, n_envs=E,
                      n_test_envs=E_TEST, **kw)


def test_a_resumed_prioritised_run_ends_where_the_uninterrupted_one_ends(tmp_path):
    from uav_bs_ctrl_amd.replay import PRIO_ONE
    from uav_bs_ctrl_amd.run import Run
    whole = _create(tmp_path / "whole", prioritized=PRIO, compact_replay=True)
    assert whole.replay.prioritized == PRIO and type(whole.replay).__name__ == "CompactSequenceReplay"
    whole.train()
    whole.logger.close()
    cfg = json.loads((tmp_path / "whole" / "config.json").read_text())["uav_bs_ctrl_amd"]
    assert cfg["prioritized"] == list(PRIO) and cfg["compact_replay"] is True
    assert (whole.replay.prio != PRIO_ONE).any(), "no update wrote a priority: the comparison is vacuous"
    part = _create(tmp_path / "part", prioritized=PRIO, compact_replay=True)
    part.train(epochs=1)
    part.logger.close()
    state = th.load(tmp_path / "part" / "state.pt", map_location="cpu", weights_only=False)
    assert tuple(state["tensors"]["replay.prio"].shape) == (8,) and tuple(state["tensors"]["replay.prio_max"].shape) == (1,)
    assert th.equal(state["tensors"]["replay.prio"], part.replay.prio.cpu())
    del part
    run = Run.resume(str(tmp_path / "part"))
    assert run.prioritized == PRIO and run.epoch == 1 and th.equal(run.replay.prio.cpu(), state["tensors"]["replay.prio"])
    run.train()
    run.logger.close()
    assert _without_time(tmp_path / "part") == _without_time(tmp_path / "whole")
    assert not _same(_final(tmp_path / "part"), _final(tmp_path / "whole"))
    assert th.equal(run.learner.flat.flat, whole.learner.flat.flat)
    for name in ("prio", "prio_max", "state", "rng", "status"):
        assert th.equal(getattr(run.replay, name), getattr(whole.replay, name)), name
    run.replay.check()


def test_a_directory_written_without_the_key_resumes_without_priorities(tmp_path):
    from uav_bs_ctrl_amd.run import Run
    off = _create(tmp_path / "off")
    assert off.prioritized is None and off.replay.prioritized is None and not hasattr(off.replay, "prio")
    off.train(epochs=1)
    off.logger.close()
    assert "prioritized" not in json.loads((tmp_path / "off" / "config.json").read_text())["uav_bs_ctrl_amd"]
    state = th.load(tmp_path / "off" / "state.pt", map_location="cpu", weights_only=False)
    assert not [k for k in state["tensors"] if "prio" in k]
    del off
    run = Run.resume(str(tmp_path / "off"))
    assert run.prioritized is None and not hasattr(run.replay, "prio") and run.train_episode.upd.weights is None
    run.train()
    run.logger.close()
    assert run.epoch == EPOCHS

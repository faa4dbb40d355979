"""`-m gpu`: QMIX on the device loop - ``graphs.GraphedUpdate`` carries a state batch, and ``graphs.Episode`` / ``GraphedEpisode`` train
a learner with ``mixer=True``: the setup of tests/test_graphed_episode_gpu.py (`_multi`: 'debug' map, TarMAC, H = 32, E = 4, batch 4,
a ring of 8) with a mixer of embed_dim 8, the team reward stored once and the simulator's global state in the ring."""
import types

import pytest
import torch as th

pytestmark = pytest.mark.gpu

EPISODES = 3


def _multi(seed=3, state_dim=None, rew_dim=1):
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(seed)
    E, Hs = 4, 32
    env = BatchedUbsCoverageEnv.from_map("debug", E, seed=11)
    args = types.SimpleNamespace(device="cuda", hidden_size=Hs, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                                 dueling=False, mixer=True, embed_dim=8, share_reward=True, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9,
                                 max_seq_len=None, batch_size=4, seed=seed)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit,
                state_shape=env.state_dim)
    learner = MultiAgentQLearner(info, args)
    rb = SequenceReplay(8, env.episode_limit, env.n_agents, env.n_gts, Hs, n_envs=E, state_dim=env.state_dim if state_dim is None else state_dim,
                        r_comm=env.p.r_comm, rew_dim=rew_dim, device_state=True, seed=21)
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 200.0), enc="gnn")


def _learner_state(learner):
    opt = learner.optimizer
    return dict(params=learner.flat.flat, target=learner.flat_target, adam_m=opt.m, adam_v=opt.v, hyper=opt.hyper)


def _snapshot(learner, env, rb, ep):
    out = dict(_learner_state(learner), state=rb.state, rng=rb.rng, status=rb.status, t=ep.t, eps=ep.eps, pos_ubs=env.pos_ubs,
               pos_gts=env.pos_gts, prior=env.prior, avg_rate=env.avg_rate, env_t=env.t, ep_ret=env.ep_ret, env_rng=env.map_rng)
    out.update({"mem." + k: v for k, v in rb.mem.items()})
    out.update({"out." + k: v for k, v in env.out.items()})
    return {k: v.clone() for k, v in out.items()}


def _buffers(gu):
    o = gu.obs
    return dict(gt=o.gt, ubs=o.ubs, agent=o.agent, d_u2u=o.d_u2u, h0=gu.h0, h1=gu.h1, acts=gu.acts, rews=gu.rews, dones=gu.dones,
                states=gu.states)


def test_graphed_update_with_a_mixer_loads_the_states_and_replays_the_eager_update():
    from uav_bs_ctrl_amd.graphs import Episode, GraphedUpdate
    l_g, env, rb, kw = _multi()
    l_e, _, _, _ = _multi()
    Episode(l_g, env, rb, train=False, **kw)()            # one collected episode: four committed sequences with their states
    assert len(rb) == 4 and float(rb.mem["state"][:4].abs().sum()) > 0
    T, n, M, B = rb.T, env.n_agents, env.n_gts, 4
    gu = GraphedUpdate(l_g, B, T, n, M, env.p.r_comm, rew_dim=1)
    ge = GraphedUpdate(l_e, B, T, n, M, env.p.r_comm, rew_dim=1, capture=False)
    assert gu.states.shape == (T + 1, B, env.state_dim) and "states" in gu._batch()
    idx = th.tensor([2, 0, 3, 1], device="cuda")
    gu.load({k: v.index_select(0, idx) for k, v in rb.mem.items()})
    ge.load_from(rb, idx)
    a, b = _buffers(gu), _buffers(ge)
    bad = [k for k in a if not th.equal(a[k], b[k])]
    assert not bad, f"load and load_from differ in {bad}"
    assert th.equal(gu.states, rb.mem["state"].index_select(0, idx).transpose(0, 1)) and float(gu.states.abs().sum()) > 0
    p0 = l_g.flat.flat.clone()
    assert th.equal(l_e.flat.flat, p0), "the capture's warm-up updates left their traces"
    for i in range(3):
        out_g = gu()
        out_e = l_e.update(ge._batch())
        assert th.equal(out_g["LossQ"], out_e["LossQ"]) and bool(th.isfinite(out_g["LossQ"])), f"update {i}"
        sa, sb = _learner_state(l_g), _learner_state(l_e)
        bad = [k for k in sa if not th.equal(sa[k], sb[k])]
        assert not bad, f"update {i}: {bad}"
    assert not th.equal(l_g.flat.flat[l_g.n_policy:], p0[l_g.n_policy:]), "the mixer did not move"


def test_graphed_episode_with_a_mixer_replays_the_eager_episode():
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    l_e, env_e, rb_e, kw = _multi()
    l_g, env_g, rb_g, _ = _multi()
    assert th.equal(l_e.flat.flat, l_g.flat.flat), "the two learners were not built from the same seed"
    p0, t0 = l_e.flat.flat.clone(), l_e.flat_target.clone()
    assert l_e.n_policy < p0.numel(), "the flat buffer holds no mixer"
    eager, graphed = Episode(l_e, env_e, rb_e, **kw), GraphedEpisode(l_g, env_g, rb_g, **kw)
    assert eager.with_state and eager.upd.states is not None
    assert th.equal(l_g.flat.flat, p0) and rb_g.state.tolist() == [0, 0] and int(graphed.t) == 0, "the warm-up left its traces"
    losses = []
    for ep in range(EPISODES):
        out_e, out_g = eager(), graphed()
        losses.append(out_g["LossQ"].clone())
        assert th.equal(out_e["LossQ"], out_g["LossQ"]) and th.equal(eager.idx, graphed.idx), f"episode {ep}"
        a, b = _snapshot(l_e, env_e, rb_e, eager), _snapshot(l_g, env_g, rb_g, graphed)
        size = int(rb_g.state[1])
        bad = [k for k in a if not (th.equal(a[k][:size], b[k][:size]) if k.startswith("mem.") else th.equal(a[k], b[k]))]
        assert not bad, f"episode {ep}: {bad}"
    assert size == rb_g.capacity, "the ring was not compared whole"
    assert all(bool(th.isfinite(x)) for x in losses), f"losses {losses}"
    k = l_g.n_policy
    assert not th.equal(l_g.flat.flat[k:], p0[k:]), "the mixer's parameters did not move"
    assert not th.equal(l_g.flat_target[k:], t0[k:]), "the target mixer did not move"
    assert not th.equal(l_g.flat.flat[:k], p0[:k])
    assert float(rb_g.mem["state"].abs().sum()) > 0
    rb_g.check()


def test_episode_refuses_a_replay_that_does_not_fit_the_mixer():
    from uav_bs_ctrl_amd.graphs import Episode
    learner, env, rb, kw = _multi(state_dim=0)
    with pytest.raises(ValueError, match="state"):
        Episode(learner, env, rb, **kw)
    learner, env, rb, kw = _multi(state_dim=3)
    with pytest.raises(ValueError, match="state"):
        Episode(learner, env, rb, **kw)
    learner, env, rb, kw = _multi(rew_dim=3)
    with pytest.raises(ValueError, match="rew_dim"):
        Episode(learner, env, rb, **kw)

"""`-m gpu`: ``graphs.GraphedEpisode`` - a whole training episode (reset, rollout, caching, commits, sampling, gathers, updates) as one
graph replay - against ``graphs.Episode``, the same launches issued eagerly on a device-state replay: after three episodes the
parameters, the target, the Adam moments, the ring, its counters, the simulator's state and the exploration counter are identical
bit for bit.  What a graph with baked-in host state would get wrong is asserted by name: the sampled batch moves between replays,
the ring wraps, epsilon decays."""
import types

import pytest
import torch as th

pytestmark = pytest.mark.gpu

EPISODES = 3


def _multi(seed=3, c="tarmac"):
    """'debug' map (3 UBSs x 4 GTs, episode limit 10), TarMAC (or ``c``), H = 32, E = 4, batch 4, a ring of 8: episode 3 wraps."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(seed)
    E, Hs = 4, 32
    env = BatchedUbsCoverageEnv.from_map("debug", E, seed=11)
    args = types.SimpleNamespace(device="cuda", hidden_size=Hs, c=c, n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                                 dueling=False, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9, max_seq_len=None,
                                 batch_size=4, seed=seed)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    learner = MultiAgentQLearner(info, args)
    rb = SequenceReplay(8, env.episode_limit, env.n_agents, env.n_gts, Hs, n_envs=E, state_dim=env.state_dim, r_comm=env.p.r_comm,
                        device_state=True, seed=21)
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 200.0), enc="gnn")


def _exp1(agent, seed=4):
    """exp1: n_grps = 2, gts_per_grp = 3, T = 5 with the episode limit overridden to 10 - two segments, two updates per episode."""
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    th.manual_seed(seed)
    E, Hs, T = 4, 32, 5
    p = SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10)
    env = BatchedSingleUbsCoverageEnv(p, E, seed=12)
    args = types.SimpleNamespace(device="cuda", agent=agent, hidden_size=Hs, n_heads=4, n_layers=2, max_seq_len=T, gamma=0.99,
                                 polyak=0.9, batch_size=4, lr=1e-3, anneal_lr=False, seed=seed)
    learner = QLearner(env.get_env_info(agent), args)
    rb = SingleUbsSequenceReplay(20, T, p.n_gts, Hs, n_envs=E, device_state=True, seed=22)     # 24 sequences committed: the ring wraps
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 300.0), enc=agent)


def _snapshot(learner, env, rb, ep):
    opt = learner.optimizer
    out = dict(params=learner.flat.flat, target=learner.flat_target, adam_m=opt.m, adam_v=opt.v, hyper=opt.hyper, state=rb.state,
               rng=rb.rng, status=rb.status, t=ep.t, eps=ep.eps, pos_ubs=env.pos_ubs, pos_gts=env.pos_gts, prior=env.prior,
               avg_rate=env.avg_rate, env_t=env.t, ep_ret=env.ep_ret, env_rng=env.map_rng if hasattr(env, "map_rng") else env.rng)
    out.update({"mem." + k: v for k, v in rb.mem.items()})
    out.update({"out." + k: v for k, v in env.out.items()})
    return {k: v.clone() for k, v in out.items()}


SETUPS = {"multi-tarmac": _multi, "exp1-gnn": lambda: _exp1("gnn"), "exp1-rnn": lambda: _exp1("rnn")}


@pytest.mark.parametrize("name", list(SETUPS))
def test_graphed_episode_replays_the_eager_episode(name):
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    l_e, env_e, rb_e, kw = SETUPS[name]()
    l_g, env_g, rb_g, _ = SETUPS[name]()
    assert th.equal(l_e.flat.flat, l_g.flat.flat), "the two learners were not built from the same seed"
    p0 = l_e.flat.flat.clone()
    eager, graphed = Episode(l_e, env_e, rb_e, **kw), GraphedEpisode(l_g, env_g, rb_g, **kw)
    assert th.equal(l_g.flat.flat, p0) and rb_g.state.tolist() == [0, 0] and int(graphed.t) == 0, "the warm-up left its traces"
    assert rb_g.rng.tolist() == rb_e.rng.tolist() and int(rb_g.status) == 0
    idxs, epss, losses = [], [], []
    for ep in range(EPISODES):
        out_e, out_g = eager(), graphed()
        idxs.append(graphed.idx.clone()), epss.append(float(graphed.eps)), losses.append(out_g["LossQ"].clone())
        assert th.equal(out_e["LossQ"], out_g["LossQ"]) and th.equal(eager.idx, graphed.idx), f"episode {ep}"
        a, b = _snapshot(l_e, env_e, rb_e, eager), _snapshot(l_g, env_g, rb_g, graphed)
        # ring rows beyond `size` still hold what the capture's warm-up episodes wrote: the whole ring is compared once it is full
        size = int(rb_g.state[1])
        bad = [k for k in a if not (th.equal(a[k][:size], b[k][:size]) if k.startswith("mem.") else th.equal(a[k], b[k]))]
        assert not bad, f"episode {ep}: {bad}"
    assert size == rb_g.capacity, "the ring was not compared whole"
    E, limit = env_g.B, env_g.episode_limit
    commits = EPISODES * limit // rb_g.T * E
    assert commits > rb_g.capacity, "the configuration does not wrap the ring"
    assert rb_g.state.tolist() == [commits % rb_g.capacity, rb_g.capacity]
    updates = EPISODES * limit // rb_g.T
    assert rb_g.rng.tolist()[1] == updates and int(graphed.t) == EPISODES * limit * E
    assert not th.equal(l_g.flat.flat, p0) and all(bool(th.isfinite(x)) for x in losses)
    # what a graph with baked-in host state would get wrong
    assert not th.equal(idxs[1], idxs[2]) or not th.equal(idxs[0], idxs[1]), "every replay sampled the same batch"
    assert epss[0] > epss[1] > epss[2] and epss[2] < kw["eps"][0], f"epsilon does not decay across replays: {epss}"
    rb_g.check()


def test_collect_only_graph_fills_the_ring_and_leaves_the_parameters():
    from uav_bs_ctrl_amd.graphs import GraphedEpisode
    learner, env, rb, kw = _exp1("rnn")
    opt = learner.optimizer
    state = (learner.flat.flat, learner.flat_target, opt.m, opt.v, opt.hyper)
    snap = [t.clone() for t in state]
    collect = GraphedEpisode(learner, env, rb, train=False, **kw)
    assert collect() is None and len(rb) == 8
    first = rb.mem["gt"][:8].clone()
    collect(), collect()
    assert rb.state.tolist() == [4, 20] and int(collect.t) == 3 * 10 * 4 and rb.rng.tolist()[1] == 0
    assert not th.equal(rb.mem["gt"][:4], first[:4]), "the wrapped commit wrote elsewhere"
    assert th.equal(rb.mem["gt"][4:8], first[4:8])
    assert float(rb.mem["gt"].abs().sum(dim=(1, 2, 3)).min()) > 0, "a ring slot was never written"
    for t, s in zip(state, snap):
        assert th.equal(t, s), "the collect-only graph moved the learner"
    rb.check()


def _trace_state(learner):
    """What constructing a graph must leave as it found it: the learner's five state tensors, its generator, every comm ``rng_state``."""
    opt = learner.optimizer
    out = dict(params=learner.flat.flat, target=learner.flat_target, adam_m=opt.m, adam_v=opt.v, hyper=opt.hyper, gen=learner._gen.get_state())
    for name, net in (("policy", learner.policy_net), ("target", learner.target_net)):
        out.update({f"comm.{name}.{mn}": m.rng_state for mn, m in net.named_modules() if hasattr(m, "rng_state")})
    return {k: v.clone() for k, v in out.items()}


def test_constructing_graphed_update_and_cycle_leaves_no_trace():
    """``GraphedUpdate`` and ``GraphedCycle`` run their body for real before the capture - updates that move parameters, moments and the
    step count, DiscreteComm forwards that advance the in-kernel noise counters, ``act`` calls that draw from the generator - and put all of
    it back: bit-identical before and after construction.  One replay of the cycle then moves every one of them (the test has teeth)."""
    from uav_bs_ctrl_amd.graphs import GraphedCycle, GraphedUpdate
    from uav_bs_ctrl_amd.run import seed_comm_modules
    learner, env, _, _ = _multi(c="disc")
    B, T, n, M = 4, 3, env.n_agents, env.n_gts
    seed_comm_modules(learner, 77)           # the noise counters exist before the captures: there is something to restore
    # fixed-address inputs of the cycle: a batch of T + 1 simulator steps and the observation graph of the last one
    hold = GraphedUpdate(learner, B, T, n, M, env.p.r_comm, capture=False)
    gen = th.Generator(device="cuda").manual_seed(5)
    env.reset_from_map()
    for t in range(T + 1):
        o = env.observations()
        hold.obs.gt[t].copy_(o["gt"]), hold.obs.ubs[t].copy_(o["ubs"]), hold.obs.agent[t].copy_(o["agent"]), hold.obs.d_u2u[t].copy_(o["d_u2u"])
        acts = th.randint(env.n_actions, (B * n,), device="cuda", generator=gen)
        if t < T:
            hold.acts[t].copy_(acts.view(-1, 1))
            hold.rews[t].copy_(env.step(acts)[1])
    hold.h0.normal_(0.0, 0.1, generator=gen), hold.h1.normal_(0.0, 0.1, generator=gen)
    g, h = env.graph(with_comm=True, static=True), learner.init_hidden(B)
    keys = {"params", "target", "adam_m", "adam_v", "hyper", "gen", "comm.policy.f_comm", "comm.target.f_comm"}
    before = _trace_state(learner)
    assert set(before) == keys, sorted(before)
    GraphedUpdate(learner, B, T, n, M, env.p.r_comm)
    after = _trace_state(learner)
    assert not [k for k in before if not th.equal(before[k], after[k])], "GraphedUpdate's warm-up left its traces"

    def body():
        _, h1 = learner.act(g, h, 0.3)
        learner.act(g, h1, 0.3)
        return learner.update(hold._batch())
    cycle = GraphedCycle(learner, body)
    after = _trace_state(learner)
    assert not [k for k in before if not th.equal(before[k], after[k])], "GraphedCycle's warm-up left its traces"
    out = cycle()
    moved = _trace_state(learner)
    assert bool(th.isfinite(out["LossQ"])) and not [k for k in before if k != "gen" and th.equal(before[k], moved[k])], \
        "a replay of the cycle left part of the state where it was: the check above proves nothing for it"


def test_arguments():
    from uav_bs_ctrl_amd.graphs import Episode
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    learner, env, rb, kw = _exp1("rnn")
    with pytest.raises(ValueError, match="multiple"):
        Episode(learner, env, SingleUbsSequenceReplay(20, 3, env.n_gts, 32, n_envs=4, device_state=True, seed=1), **kw)
    with pytest.raises(ValueError, match="device-state"):
        Episode(learner, env, SingleUbsSequenceReplay(20, 5, env.n_gts, 32, n_envs=4), **kw)
    with pytest.raises(ValueError, match="n_envs"):
        Episode(learner, env, SingleUbsSequenceReplay(20, 5, env.n_gts, 32, n_envs=2, device_state=True, seed=1), **kw)

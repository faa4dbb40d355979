"""`-m gpu`: ``replay.CompactSequenceReplay`` - the ring that stores simulator state and rebuilds observations - against
``replay.SequenceReplay(device_state=True)`` fed from the same simulator and policy: the same sampled indices, the same update buffers, the
same training run.  Every comparison is bit for bit.

1. ring parity ('debug': episode limit 10, T = 5, E = 4, capacity 6 - the ring wraps): ``gather_into`` and ``gather`` of both rings;
2. training parity: ``Episode`` on either ring, ``GraphedEpisode`` on the compact one; one case on the many-workgroup sampler;
3. ``bytes_per_sequence``."""
import types

import pytest
import torch as th

pytestmark = pytest.mark.gpu


def _args(c="tarmac", o="gnn", mixer=False, Hs=32, seed=3):
    a = types.SimpleNamespace(device="cuda", hidden_size=Hs, c=c, o=o, n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                              dueling=False, mixer=mixer, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9, max_seq_len=None, batch_size=4,
                              seed=seed)
    if mixer:
        a.embed_dim, a.share_reward = 8, True
    return a


def _learner_env(map_id="debug", E=4, **kw):
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    args = _args(**kw)
    th.manual_seed(args.seed)
    env = BatchedUbsCoverageEnv.from_map(map_id, E, seed=11)
    return MultiAgentQLearner(env.get_env_info(args.o), args), env


def _rings(env, cap, T, Hs, mixer, seed=21):
    from uav_bs_ctrl_amd.replay import CompactSequenceReplay, SequenceReplay
    rd = 1 if mixer else None
    full = SequenceReplay(cap, T, env.n_agents, env.n_gts, Hs, n_envs=env.B, state_dim=env.state_dim if mixer else 0,
                          r_comm=env.p.r_comm, rew_dim=rd, device_state=True, seed=seed)
    comp = CompactSequenceReplay.for_env(env, cap, T, Hs, rew_dim=rd, seed=seed)
    return full, comp


def _graph_tensors(g):
    """Every tensor of an observation batch, by name."""
    from uav_bs_ctrl_amd.graph import FlatObsBatch
    out = {} if isinstance(g, FlatObsBatch) else {f"feat.{nt}": x for nt, x in g.ndata["feat"].items()}
    out["agent_feat"] = g.agent_feat()
    if g.graph_off is not None:
        out["graph_off"] = g.graph_off
    for et, r in g._rels.items():
        out.update({f"{et}.{a}": getattr(r, a) for a in ("off", "src", "eid") if getattr(r, a) is not None})
    return out


def _buffers(gu):
    o = gu.obs
    out = {"obs.gt": o.gt, "obs.ubs": o.ubs, "obs.agent": o.agent, "obs.d_u2u": o.d_u2u, "h0": gu.h0, "h1": gu.h1, "acts": gu.acts,
           "rews": gu.rews, "dones": gu.dones, "states": gu.states}
    return {k: v for k, v in out.items() if v is not None}


# ---- 1. ring parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc,c,mixer", [("gnn", "tarmac", False), ("mlp", None, False), ("gnn", "tarmac", True)],
                         ids=["gnn-tarmac", "mlp-rnn", "gnn-qmix"])
def test_both_rings_fed_from_one_simulator_hand_the_update_the_same_bits(enc, c, mixer):
    from uav_bs_ctrl_amd.graphs import GraphedUpdate, _builder
    T, cap, B, Hs = 5, 6, 4, 32
    learner, env = _learner_env(c=c, o=enc, mixer=mixer, Hs=Hs)
    E, n, M = env.B, env.n_agents, env.n_gts
    full, comp = _rings(env, cap, T, Hs, mixer)
    build, gen = _builder(enc), th.Generator(device="cuda").manual_seed(7)
    with_comm = c is not None
    for _ in range(3):
        env.reset_from_map()
        h = learner.init_hidden(E)
        for _ in range(env.episode_limit):
            o = env.observations()
            staged = dict(gt=o["gt"], ubs=o["ubs"], agent=o["agent"], d_u2u=o["d_u2u"], h=h.view(E, n, -1))
            if mixer:
                staged["state"] = o["state"]
            full.stage_obs(staged)
            comp.stage_obs(dict(env.replay_state(), h=h.view(E, n, -1)))
            with th.no_grad():
                _, h2 = learner.policy_net(build(o["gt"], o["ubs"], o["agent"], o["d_u2u"] if with_comm else None, env.p.r_comm,
                                                 static=True), h)
            acts = th.randint(env.n_actions, (E * n,), device="cuda", generator=gen)
            o2, rew, done, info = env.step(acts)
            st = o2["state"] if mixer else None
            learner.cache(full, None, None, st, acts, rew, o2, h2, st, done, info["BadMask"], staged=True)
            learner.cache(comp, None, None, None, acts, rew, env.replay_state(), h2, None, done, info["BadMask"], staged=True)
            h = h2
    commits = 3 * env.episode_limit // T * E
    assert commits > cap and full.state.tolist() == comp.state.tolist() == [commits % cap, cap], "the ring did not wrap"
    assert "state" not in comp.mem and comp.mem["h"].shape[1] == 2
    for k in ("act", "rew", "done"):
        assert th.equal(full.mem[k], comp.mem[k]), k
    assert th.equal(full.mem["h"][:, :2], comp.mem["h"])
    idx_f, idx_c = full.sample_indices(B), comp.sample_indices(B)
    assert th.equal(idx_f, idx_c) and full.rng.tolist() == comp.rng.tolist()
    idx = th.tensor([5, 0, 3, 3], device="cuda")                 # the last slot, a repeat, out of order
    for ix in (idx_f, idx):
        a, b = (GraphedUpdate(learner, B, T, n, M, env.p.r_comm, rew_dim=1 if mixer else None, enc=enc, capture=False) for _ in range(2))
        for v in _buffers(b).values():
            v.fill_(-1 if v.dtype == th.int64 else float("nan"))
        full.gather_into(ix, a), comp.gather_into(ix, b)
        fa, fb = _buffers(a), _buffers(b)
        assert fa.keys() == fb.keys() and ("states" in fa) == mixer and ("obs.d_u2u" in fa) == (enc == "gnn" or with_comm)
        bad = [k for k in fa if not th.equal(fa[k], fb[k])]
        assert not bad, f"gather_into differs in {bad}"
        assert float(fa["obs.gt"][..., 0].sum()) > 0, "no GT was ever seen: the comparison is vacuous"
    ga, gb = full.gather(idx, enc), comp.gather(idx, enc)
    assert set(ga) == set(gb)
    for k in ("h0", "h1", "acts", "rews", "dones") + (("states",) if mixer else ()):
        assert th.equal(ga[k], gb[k]), k
    assert gb["states"].shape == (T + 1, B, env.state_dim)
    lists = [("obs", ga["obs"], gb["obs"])] + [(k, [ga[k]], [gb[k]]) for k in ("obs_all", "obs_all_next") if k in ga]
    for name, xs, ys in lists:
        assert len(xs) == len(ys)
        for t, (x, y) in enumerate(zip(xs, ys)):
            tx, ty = _graph_tensors(x), _graph_tensors(y)
            assert tx.keys() == ty.keys(), (name, t)
            bad = [k for k in tx if tx[k].shape != ty[k].shape or not th.equal(tx[k], ty[k])]
            assert not bad, f"gather: {name}[{t}] differs in {bad}"
    full.check(), comp.check()


# ---- 2. training parity ---------------------------------------------------------------------------------------------------------------------
def _train(kind, ring, map_id="debug", cap=12, T=5, Hs=32, **kw):
    """2 collect + 2 training episodes of ``Episode`` ('eager') or ``GraphedEpisode`` ('graphed') on a full or a compact ring, from fixed
    seeds: ([LossQ of every update], the flat parameter buffer, the ring counters)."""
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    learner, env = _learner_env(map_id, Hs=Hs, **kw)
    mixer = bool(kw.get("mixer"))
    full, comp = _rings(env, cap, T or env.episode_limit, Hs, mixer)
    rb = comp if ring == "compact" else full
    cls = GraphedEpisode if kind == "graphed" else Episode
    ekw = dict(batch_size=4, eps=(1.0, 0.05, 200.0), enc=kw.get("o", "gnn"), explore_seed=5)
    collect, train = cls(learner, env, rb, train=False, **ekw), cls(learner, env, rb, train=True, **ekw)
    losses = []

    class _Spy:                       # LossQ of EVERY update, not only the episode's last
        @staticmethod
        def push(**vals):
            if "LossQ" in vals:
                losses.append(vals["LossQ"].clone())
    if kind == "eager":
        train.stats = _Spy
    for _ in range(2):
        collect()
    train.t.copy_(collect.t), train.explore.copy_(collect.explore)
    for _ in range(2):
        out = train()
        if kind == "graphed":
            losses.append(out["LossQ"].clone())
    rb.check()
    assert all(bool(th.isfinite(x)) for x in losses) and losses
    return losses, learner.flat.flat.clone(), rb.state.tolist() + rb.rng.tolist()


@pytest.mark.parametrize("kw", [dict(), dict(mixer=True), dict(o="mlp", c=None)], ids=["gnn-tarmac", "gnn-qmix", "mlp-rnn"])
def test_training_on_the_compact_ring_equals_training_on_the_full_ring(kw):
    lf, pf, cf = _train("eager", "full", **kw)
    lc, pc, cc = _train("eager", "compact", **kw)
    assert len(lf) == len(lc) == 4 and cf == cc                   # two segments per episode, one update each
    assert all(th.equal(a, b) for a, b in zip(lf, lc)), f"LossQ: {[float(x) for x in lf]} against {[float(x) for x in lc]}"
    assert th.equal(pf, pc), "the parameters differ after training on the two rings"
    lg, pg, cg = _train("graphed", "compact", **kw)
    assert cg == cc and th.equal(pg, pc), "GraphedEpisode on the compact ring does not replay its eager form"
    assert th.equal(lg[-1], lc[-1]) and th.equal(lg[0], lc[1])     # the graphed run reports the last update of each episode


def test_the_many_workgroup_sampler_over_a_compact_ring():
    from uav_bs_ctrl_amd.replay import NARROW_SAMPLER_CAPACITY
    # n = 1, M = 1, T = episode limit = 20; the flattened-observation agent: the graph encoder has no instantiation of 4 heads at H = 8
    kw = dict(map_id="test", cap=NARROW_SAMPLER_CAPACITY + 1, T=None, Hs=8, o="mlp", c=None)
    lf, pf, cf = _train("eager", "full", **kw)
    lc, pc, cc = _train("eager", "compact", **kw)
    assert cf == cc and len(lf) == len(lc) == 2
    assert all(th.equal(a, b) for a, b in zip(lf, lc)) and th.equal(pf, pc)


# ---- 3. bytes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_id,T,Hs,rd", [("debug", 5, 32, None), ("debug", 10, 8, 1), ("test", 1, 8, None)])
def test_bytes_per_sequence_is_the_formula_and_what_the_ring_holds(map_id, T, Hs, rd):
    from uav_bs_ctrl_amd.replay import CompactSequenceReplay, SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    env = BatchedUbsCoverageEnv.from_map(map_id, 2, seed=1)
    rb = CompactSequenceReplay.for_env(env, 4, T, Hs, rew_dim=rd, seed=1)
    n, M, r = env.n_agents, env.n_gts, env.n_agents if rd is None else rd
    want = (T + 1) * (16 * n + 8 * M) + 8 * M + 8 * n * Hs + 8 * T * n + 4 * T * r + 4 * T
    assert rb.bytes_per_sequence == want == sum(v[0].numel() * v.element_size() for v in rb.mem.values())
    full = SequenceReplay(4, T, n, M, Hs, n_envs=2, state_dim=env.state_dim, rew_dim=rd, device_state=True, seed=1)
    assert want < sum(v[0].numel() * v.element_size() for v in full.mem.values())

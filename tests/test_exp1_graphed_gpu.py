"""`-m gpu`: the captured experiment-1 steps - ``graphs.GraphedSingleUbsAct`` on the simulator's own observation buffers and
``graphs.GraphedSingleUbsUpdate`` on a gather in ``SingleUbsSequenceReplay.mem`` layout - replay the eager calls bit for bit."""
import types

import pytest
import torch as th

pytestmark = pytest.mark.gpu


def _setup(agent, B, T, H, seed=23):
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    th.manual_seed(seed)
    p = SingleUbsParams(n_grps=4, gts_per_grp=5, episode_limit=8 * T)
    env = BatchedSingleUbsCoverageEnv(p, B, seed=5)
    args = types.SimpleNamespace(device="cuda", agent=agent, hidden_size=H, n_heads=4, n_layers=2, max_seq_len=T, gamma=0.99, polyak=0.995,
                                 batch_size=B, lr=5e-4, anneal_lr=False, seed=seed)
    return QLearner(env.get_env_info(agent), args), env, p


def _obs_in(env, agent):
    return env.graph() if agent == "gnn" else env.observations()["flat"]


@pytest.mark.parametrize("agent", ["gnn", "rnn"])
def test_graphed_act_on_the_simulators_buffers_replays_the_eager_act(agent):
    from uav_bs_ctrl_amd.graphs import GraphedSingleUbsAct
    B = 32
    learner, env, p = _setup(agent, B, 10, 256)
    env.reset()
    ga = GraphedSingleUbsAct(learner, B, p.n_gts, agent, obs=(env.out["obs_gt"], env.out["obs_agent"]))
    ptrs = (env.out["obs_gt"].data_ptr(), env.out["obs_agent"].data_ptr())
    env.reset()
    h = 0.3 * th.randn(B, 256, device="cuda")
    for visit in range(2):
        assert (env.out["obs_gt"].data_ptr(), env.out["obs_agent"].data_ptr()) == ptrs, "the simulator moved its observation buffers"
        acts_g, h_g = ga(None, None, h, 0.0)
        acts_g, h_g = acts_g.clone(), h_g.clone()
        acts_e, h_e = learner.act(_obs_in(env, agent), h, 0.0)
        assert acts_g.shape == (B,) and acts_g.dtype == th.int64
        assert th.equal(h_g, h_e) and th.equal(acts_g, acts_e), f"visit {visit}"
        if visit == 0:
            for _ in range(2):
                env.step(acts_e)
            h = h_e.clone()
    acts_r, _ = ga(None, None, h, 1.0)
    assert int(acts_r.min()) >= 0 and int(acts_r.max()) < env.n_actions
    # buffers of the graph's own, filled by the call
    gb = GraphedSingleUbsAct(learner, B, p.n_gts, agent)
    o = env.observations()
    acts_b, h_b = gb(o["gt"], o["agent"], h, 0.0)
    acts_e, h_e = learner.act(_obs_in(env, agent), h, 0.0)
    assert th.equal(h_b, h_e) and th.equal(acts_b, acts_e)


@pytest.mark.parametrize("B,T,H", [(8, 3, 32), (32, 10, 256)])
@pytest.mark.parametrize("agent", ["gnn", "rnn"])
def test_graphed_update_replays_the_eager_update(agent, B, T, H):
    from uav_bs_ctrl_amd.graphs import GraphedSingleUbsUpdate
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    learner, env, p = _setup(agent, B, T, H)
    buf = SingleUbsSequenceReplay(2 * B, T, p.n_gts, H, n_envs=B, device="cuda")
    obs, h = env.reset(), learner.init_hidden(B)
    for _ in range(2 * T):
        a, h2 = learner.act(_obs_in(env, agent), h, 0.3)
        buf.stage_obs(dict(gt=obs["gt"], agent=obs["agent"], h=h))
        obs, rew, done, info = env.step(a)
        learner.cache(buf, None, None, a, rew, obs, h2, done, info["BadMask"], staged=True)
        h = h2
    assert len(buf) == 2 * B
    gather = lambda idx: {k: v.index_select(0, idx) for k, v in buf.mem.items()}  # noqa: E731
    m1, m2 = gather(th.arange(0, B, device="cuda")), gather(th.arange(B, 2 * B, device="cuda"))
    gu = GraphedSingleUbsUpdate(learner, B, T, p.n_gts, agent)
    opt = learner.optimizer
    state = (learner.flat.flat, learner.flat_target, opt.m, opt.v, opt.hyper)
    snap = [t.clone() for t in state]
    out_g = gu(m1)
    loss_g, q_g = out_g["LossQ"].clone(), out_g["QVals"].clone()
    after_g = [t.clone() for t in state]
    assert not th.equal(after_g[0], snap[0]), "the update did not move the parameters"
    for dst, src in zip(state, snap):
        dst.copy_(src)
    learner.invalidate_weight_cache()
    # the graph's batch is the replay's own gather of the same sequences
    ref = buf.gather(th.arange(0, B, device="cuda"), agent)
    got = gu._batch()
    for k in ("h0", "h1", "acts", "rews", "dones"):
        assert th.equal(got[k], ref[k]), k
    out_e = learner.update(got)
    assert th.equal(out_e["LossQ"], loss_g) and th.equal(out_e["QVals"], q_g)
    for name, a, b in zip(("parameters", "target parameters", "Adam m", "Adam v", "hyper"), state, after_g):
        assert th.equal(a, b), name
    loss_2 = gu(m2)["LossQ"].clone()
    assert bool(th.isfinite(loss_2)) and not th.equal(loss_2, loss_g), "the graph replayed captured values, not its buffers"

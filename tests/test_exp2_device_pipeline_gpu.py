"""`-m gpu`: exp2 (o='mlp') on the device path - simulator -> flattened-observation batch (graph.from_padded_obs_flat) -> agent
-> learner, against NumPy / the float64 oracle (oracle/restatement.py, enc='mlp').  Map: the reference's 'r400' (HotSpot, 4 UBSs,
4 GTs, r_comm = 400 m; envs/mubs_cov/maps.py) with uniform initial placements."""
import types

import numpy as np
import pytest
import torch as th

from oracle import restatement as R
from tests.gpu_util import _LibSpy, _ScriptedRelu
from tests.test_learner_comm_variants_gpu import _kernel_bits, _or_pattern
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu

R400 = dict(n_ubs=4, n_gts=4, n_rbs=1, range_pos=2000.0, episode_limit=40, dt=20.0, r_cov=100.0, r_sns=200.0, r_comm=400.0,
            vels=(5.0, 10.0), n_dirs=4, reward_scale_rate=10.0)
F = 2 + 4 * 5 + 3 * 3      # = 31


def _env(B, seed):
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv, MapParams
    env = BatchedUbsCoverageEnv(MapParams(**R400), B)
    gen = th.Generator(device="cuda").manual_seed(seed)
    env.reset(generator=gen)
    for _ in range(3):
        env.step(th.randint(env.n_actions, (B, 4), device="cuda", generator=gen))
    return env


def _args(c, H=256):
    return types.SimpleNamespace(device="cuda", hidden_size=H, c=c, o="mlp", n_heads=4, n_layers=2, msg_size=64, key_size=16,
                                 n_rounds=1, dueling=False, mixer=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999,
                                 max_seq_len=None, batch_size=None, seed=0)


def _oracle_graph(g):
    off, src = g.talk_csc()
    return dict(x_flat=g.agent_feat().double(), talk_off=off.long(), talk_src=src.long())


def _oracle_params(net):
    """state_dict in float64 with RnnAgent's enc.N mapped to GnnAgent's enc.enc.N (the oracle reads the dense encoder under enc.enc)."""
    from uav_bs_ctrl_amd import RnnAgent
    out = {}
    for k, v in net.state_dict().items():
        if isinstance(net, RnnAgent) and k.startswith("enc."):
            k = "enc." + k
        out[k] = v.detach().double()
    return out


def _cfg(c):
    return dict(enc="mlp", c=c, n_layers=2, n_heads=4, key_size=16, msg_size=64, n_rounds=1, dueling=False)


def test_flat_batch_from_the_simulator_follows_the_contract():
    from uav_bs_ctrl_amd.graph import FLAT_OBS_ORDER, from_padded_obs, from_padded_obs_flat
    assert FLAT_OBS_ORDER == ("agent", "gt", "ubs")       # gym 0.21's Dict sorts the keys of a plain dict
    env = _env(1024, 1)
    o = env.observations()
    g = from_padded_obs_flat(o["gt"], o["ubs"], o["agent"], o["d_u2u"], R400["r_comm"])
    B, n = 1024, 4
    want = np.concatenate([o["agent"].cpu().numpy().reshape(B * n, -1), o["gt"].cpu().numpy().reshape(B * n, -1),
                           o["ubs"].cpu().numpy().reshape(B * n, -1)], 1)
    got = g.agent_feat().cpu().numpy()
    assert got.shape == (B * n, F) and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert g.ndata["feat"]["agent"] is g.agent_feat()
    ref = from_padded_obs(o["gt"], o["ubs"], o["agent"], o["d_u2u"], R400["r_comm"])
    for a, b in zip(g.talk_csc() + (g.talk_eid(),), ref.talk_csc() + (ref.talk_eid(),)):
        assert th.equal(a, b)
    assert 0 < g.number_of_edges("talk") < B * n * n          # finite r_comm: some pairs out of range
    sl = g.slice_agents(8, 16)
    assert sl.num_nodes("agent") == 8 and th.equal(sl.agent_feat(), g.agent_feat()[8:16])


def _disc_spy(monkeypatch, calls):
    """Records every DiscreteComm forward (as tests/test_learner_comm_variants_gpu.py does): the device {seed, step}, the per-node logits
    and the talk CSC, so that the kernel's own noise and hard bits can be reconstructed (_kernel_bits) and handed to the oracle."""
    from uav_bs_ctrl_amd import ops
    orig = ops.disc_comm_aggregate

    def spy(logits, gumbel, g, tau=0.5, rng=None):
        assert gumbel is None and rng is not None, "DiscreteComm did not take the in-kernel noise"
        off, src = g.talk_csc()
        rec = dict(rng=rng.clone(), E=int(src.numel()), logits=logits.detach().clone(), off=off, src=src, inv_tau=1.0 / tau)
        res = orig(logits, gumbel, g, tau=tau, rng=rng)
        rec["c"] = res.detach().clone()
        calls.append(rec)
        return res
    monkeypatch.setattr(ops, "disc_comm_aggregate", spy)


def _disc_branch(calls, what):
    """{gumbels, bits} per recorded forward: the kernel's noise stream and the hard bits it chose, checked against K5's own output."""
    gumbels, bits = [], []
    for k, r in enumerate(calls):
        b, noise = _kernel_bits(r)
        assert th.equal(_or_pattern(b, r["off"]), r["c"] > 0.5), f"{what}: forward {k}: reconstructed hard bits disagree with K5's output"
        gumbels.append(noise)
        bits.append(b)
    return dict(gumbels=gumbels, bits=bits)


@pytest.mark.parametrize("c", [None, "tarmac", "disc"])
def test_agent_forwards_on_the_flat_batch_match_the_oracle(c, monkeypatch):
    from uav_bs_ctrl_amd import GnnAgent, RnnAgent
    from uav_bs_ctrl_amd.graph import from_padded_obs_flat
    th.manual_seed(3)
    env = _env(1024, 2)
    o = env.observations()
    g = from_padded_obs_flat(o["gt"], o["ubs"], o["agent"], o["d_u2u"], R400["r_comm"])
    net = (RnnAgent if c is None else GnnAgent)(F, 9, _args(c)).cuda()
    h = th.randn(g.num_nodes("agent"), 256, device="cuda") * 0.5
    calls, kw = [], {}
    if c == "disc":
        net.f_comm.rng_state = th.tensor([0x5EED0000, 3], dtype=th.int64, device="cuda")
        _disc_spy(monkeypatch, calls)
    with th.no_grad():
        q, h2 = net(g, h)
    if c == "disc":
        assert len(calls) == 1
        d = _disc_branch(calls, "forward")
        kw = dict(gumbel=d["gumbels"][0].double(), hard=d["bits"][0])
    q_ref, h_ref = R.gnn_agent_forward(_oracle_graph(g), h.double(), _oracle_params(net), _cfg(c), **kw)
    assert_close(q, q_ref, 1e-5, f"q c={c}")
    assert_close(h2, h_ref, 1e-5, f"h' c={c}")
    # the reference contract of RnnAgent: an [N, F] tensor through the existing kernels
    if c is None:
        with th.no_grad():
            q_t, h_t = net(g.agent_feat().clone(), h)
        assert_close(q_t, q_ref, 1e-5, "q [N, F] input")


def _sequence(B, T, seed):
    """T + 1 steps of simulator observations (time-major) + stored hidden states / actions / rewards / dones."""
    env = _env(B, seed)
    gen = th.Generator(device="cuda").manual_seed(seed)
    steps = []
    for _ in range(T + 1):
        o = env.observations()
        steps.append({k: o[k].clone() for k in ("gt", "ubs", "agent", "d_u2u")})
        env.step(th.randint(env.n_actions, (B, 4), device="cuda", generator=gen))
    tm = {k: th.stack([s[k] for s in steps]) for k in steps[0]}          # [T+1, B, ...]
    N = B * 4
    return tm, dict(h0=th.randn(N, 256, device="cuda", generator=gen) * 0.3, h1=th.randn(N, 256, device="cuda", generator=gen) * 0.3,
                    acts=th.randint(9, (T, N, 1), device="cuda", generator=gen),
                    rews=th.rand(T, B, 4, device="cuda", generator=gen), dones=(th.rand(T, B, 1, device="cuda", generator=gen) < 0.1).float())


def _flat_batch(tm, extra, static=False):
    from uav_bs_ctrl_amd.graph import from_padded_obs_flat
    T = tm["gt"].shape[0] - 1
    rows = lambda x, lo: x[lo:].reshape((-1,) + x.shape[2:])  # noqa: E731
    obs = [from_padded_obs_flat(tm["gt"][t], tm["ubs"][t], tm["agent"][t], tm["d_u2u"][t], R400["r_comm"], static) for t in range(T + 1)]
    return dict(obs=obs, obs_all=from_padded_obs_flat(rows(tm["gt"], 0), rows(tm["ubs"], 0), rows(tm["agent"], 0), static=static),
                obs_all_next=from_padded_obs_flat(rows(tm["gt"], 1), rows(tm["ubs"], 1), rows(tm["agent"], 1), static=static), **extra)


def _enc_linears(net):
    from uav_bs_ctrl_amd import RnnAgent
    seq = net.enc if isinstance(net, RnnAgent) else net.enc.enc
    return [m for m in seq if isinstance(m, th.nn.Linear)]


def _oracle_update_mlp(learner, batch, dtype, next_acts=None, relu_masks=None, cfg=None, gumbels=None, hard_bits=None, disc_logits=None):
    """tests/gpu_util.py:_oracle_update for the flattened-observation agents (oracle enc='mlp', evaluated on the GPU): loss, policy outputs,
    the gradient of every policy parameter and the ReLU pre-activations in call order (n_layers per agent forward)."""
    from uav_bs_ctrl_amd import RnnAgent
    key = lambda k: "enc." + k if isinstance(learner.policy_net, RnnAgent) and k.startswith("enc.") else k  # noqa: E731
    pp = {key(k): v.detach().to(dtype).clone().requires_grad_(True) for k, v in learner.policy_net.state_dict().items()}
    pt = {key(k): v.detach().to(dtype).clone() for k, v in learner.target_net.state_dict().items()}
    f = lambda t: t.detach().to(dtype)   # noqa: E731
    obs = []
    for g in batch["obs"]:
        d = dict(x_flat=f(g.agent_feat()))
        if g.has_relation("talk"):
            d["talk_off"], d["talk_src"] = g.talk_csc()
        obs.append(d)
    script, real, real_dc = _ScriptedRelu(relu_masks), R.F, R.disc_comm

    def disc_spy(g, x, h, p, *a, **k):
        disc_logits.append(R.disc_logits(x, h, p).detach().index_select(0, R.talk_edges(g)[0]))
        return real_dc(g, x, h, p, *a, **k)
    R.F = script
    if disc_logits is not None:
        R.disc_comm = disc_spy
    try:
        loss, agent_out, _ = R.madrqn_loss(obs, f(batch["h0"]), f(batch["h1"]), batch["acts"], f(batch["rews"]), f(batch["dones"]), pp, pt,
                                           cfg, learner.gamma, True, next_acts=next_acts, gumbels=gumbels, hard_bits=hard_bits)
    finally:
        R.F, R.disc_comm = real, real_dc
    names = [k for k, _ in learner.policy_net.named_parameters()]
    return loss.detach(), agent_out.detach(), dict(zip(names, th.autograd.grad(loss, [pp[key(k)] for k in names]))), script.pre


def _gpu_relu_patterns_mlp(learner, batch, T, N, fused):
    """{call index of _ScriptedRelu: activation pattern} of the POLICY forwards as the HIP path evaluated them: the encoder's layers on the
    time-batched flat batch (the learner's own launches - the fused kernel or th.cat + linear_relu -, same inputs: same bits)."""
    from uav_bs_ctrl_amd import ops
    lins = _enc_linears(learner.policy_net)
    parts = batch["obs_all"].parts
    with th.no_grad():
        xs = [ops._FlatLinearReLU.apply(lins[0].weight, lins[0].bias, *parts) if fused else
              ops.linear_relu(th.cat(parts, 1), lins[0].weight, lins[0].bias)]
        for lin in lins[1:]:
            xs.append(ops.linear_relu(xs[-1], lin.weight, lin.bias))
    nl, masks = len(lins), {}
    for t in range(T + 1):
        fwd = 2 * t                    # policy forward of step t is forward number 2 t (target forwards in between)
        for l in range(nl):
            masks[nl * fwd + l] = xs[l][t * N:(t + 1) * N] > 0
    return masks


def _oracle_at_mlp_branch(learner, batch, q_gpu, T, N, what, cfg, fused, disc=None):
    """tests/gpu_util.py:_oracle_at_gpu_branch for enc='mlp': float64 (and float32, for the error floor) evaluated at the double-Q argmax,
    the encoder ReLU patterns and (disc) the hard bits the HIP path chose, after checking that each of those choices differs from float64's
    own only where float64 sits on the discontinuity (2e-5 of the Q scale / 1e-5 of the pre-activation scale / 2e-5 of the logit scale)."""
    hb = None if disc is None else disc["bits"]
    gum = lambda dt: None if disc is None else [g.to(dt) for g in disc["gumbels"]]   # noqa: E731
    trace = None if disc is None else []
    l64, q64, g64, pre64 = _oracle_update_mlp(learner, batch, th.float64, cfg=cfg, gumbels=gum(th.float64), hard_bits=hb, disc_logits=trace)
    assert_close(q_gpu, q64, 1e-5, f"{what}: QVals")
    na_gpu, na64 = q_gpu[1:].argmax(2, keepdim=True), q64[1:].argmax(2, keepdim=True)
    diff = (na_gpu != na64).squeeze(2)
    if bool(diff.any()):
        top2 = q64[1:].topk(2, dim=2).values
        assert float((top2[..., 0] - top2[..., 1])[diff].max()) <= 2e-5 * float(q64.abs().max()), f"{what}: argmax differs off a tie"
    patterns = _gpu_relu_patterns_mlp(learner, batch, T, N, fused)
    flips = 0
    for i, m in patterns.items():
        pre = pre64[i].reshape(m.shape)
        flipped = (pre > 0) != m
        if bool(flipped.any()):
            flips += int(flipped.sum())
            assert float(pre[flipped].abs().max()) <= 1e-5 * float(pre.abs().max()), f"{what}: ReLU call {i} differs off the kink"
    assert flips <= 1e-5 * sum(m.numel() for m in patterns.values()) + 2, f"{what}: {flips} ReLU elements flipped"
    if disc is not None:
        assert len(trace) == len(hb) == 2 * T + 1
        n_other = n_bits = 0
        for k, (lg, g, bits) in enumerate(zip(trace, disc["gumbels"], hb)):
            lg = lg.view(bits.shape[0], -1, 2)
            margin = (lg[..., 0] + g[..., 0].double()) - (lg[..., 1] + g[..., 1].double())
            other = (margin >= 0) != bits
            n_bits += bits.numel()
            if bool(other.any()):
                n_other += int(other.sum())
                assert float(margin[other].abs().max()) <= 2e-5 * float(lg.abs().max()), f"{what}: hard bit of forward {k} off the tie"
        assert n_other <= 1e-5 * n_bits + 2, f"{what}: {n_other} hard bits differ from float64's"
    if flips or bool(diff.any()):
        l64, q64, g64, _ = _oracle_update_mlp(learner, batch, th.float64, next_acts=na_gpu, relu_masks=patterns, cfg=cfg,
                                              gumbels=gum(th.float64), hard_bits=hb)
    l32, _, g32, _ = _oracle_update_mlp(learner, batch, th.float32, next_acts=na_gpu, relu_masks=patterns, cfg=cfg, gumbels=gum(th.float32),
                                        hard_bits=hb)
    return l64, g64, g32, flips


@pytest.mark.parametrize("mode", ["1", "auto"])      # the fused kernels / the measured default (th.cat + linear_relu when training)
@pytest.mark.parametrize("B", [1024, 4096])          # 4 096 and 16 384 rows per step
@pytest.mark.parametrize("c", [None, "tarmac", "disc"])
def test_learner_accumulate_matches_the_oracle(c, B, mode, monkeypatch):
    from uav_bs_ctrl_amd import RnnAgent, ops
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    what = f"c={c} B={B} mode={mode}"
    monkeypatch.setattr(ops, "FLAT_OBS_FUSED", mode)
    th.manual_seed(5)
    T, N = 3, 4 * B
    learner = MultiAgentQLearner(dict(obs_shape=F, n_actions=9, n_agents=4, episode_limit=T), _args(c))
    assert isinstance(learner.policy_net, RnnAgent) == (c is None)
    with th.no_grad():       # a target that differs from the policy, as after the first polyak step
        for p in learner.target_net.parameters():
            p.add_(th.randn_like(p) * 0.01)
    learner.invalidate_weight_cache()
    tm, extra = _sequence(B, T, 7)
    batch = _flat_batch(tm, extra)
    calls = []
    if c == "disc":
        for i, net in enumerate((learner.policy_net, learner.target_net)):
            net.f_comm.rng_state = th.tensor([0x5EED0000 + 7919 * i, 11 * i], dtype=th.int64, device="cuda")
        _disc_spy(monkeypatch, calls)
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    out = learner.accumulate(batch)
    flat = learner.grads.flat.clone()
    monkeypatch.undo()
    names = set(spy.names)
    if mode == "1":
        assert {"uavgnn_flat_obs_fwd", "uavgnn_flat_obs_wgrad"} <= names, f"{what}: dispatch"
    else:   # the measured default: the policy's (differentiated) layer on th.cat + linear_relu; the target's no-grad encode of the
        #     T N rows on the fused forward while that is at most FLAT_OBS_AUTO_MAX_ROWS rows
        assert "uavgnn_flat_obs_wgrad" not in names, f"{what}: dispatch"
        assert ("uavgnn_flat_obs_fwd" in names) == (T * N <= ops.FLAT_OBS_AUTO_MAX_ROWS), f"{what}: dispatch"
    disc = None
    if c == "disc":
        assert len(calls) == 2 * T + 1, f"{what}: {len(calls)} DiscreteComm forwards"
        disc = _disc_branch(calls, what)
    cfg = dict(_cfg(c), exact_ties=True)       # exact_ties: K5's ownership rule
    l64, g64, g32, flips = _oracle_at_mlp_branch(learner, batch, out["QVals"].detach(), T, N, what, cfg, mode == "1", disc)
    assert_close(out["LossQ"].reshape(()), l64.reshape(()), 1e-5, f"{what}: LossQ")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    for name, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        grad_close(flat[o:o + prm.numel()].view_as(prm), g64[name], f"{what}: grad {name}", ref32=g32[name])


@pytest.mark.parametrize("c", [None, "tarmac"])
def test_graphed_act_and_update_replay_the_eager_calls(c):
    from uav_bs_ctrl_amd.graph import from_padded_obs_flat
    from uav_bs_ctrl_amd.graphs import GraphedAct, GraphedUpdate
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    th.manual_seed(9)
    B, T = 256, 3
    learner = MultiAgentQLearner(dict(obs_shape=F, n_actions=9, n_agents=4, episode_limit=T), _args(c))
    tm, extra = _sequence(B, T, 11)
    # act
    ga = GraphedAct(learner, B, 4, 4, R400["r_comm"], enc="mlp")
    h = extra["h0"]
    acts_g, h_g = ga(tm["gt"][0], tm["ubs"][0], tm["agent"][0], tm["d_u2u"][0], h, 0.0)
    acts_g, h_g = acts_g.clone(), h_g.clone()
    g = from_padded_obs_flat(tm["gt"][0], tm["ubs"][0], tm["agent"][0], tm["d_u2u"][0] if c is not None else None, R400["r_comm"],
                             static=True)
    acts_e, h_e = learner.act(g, h, 0.0)
    assert th.equal(h_g, h_e) and th.equal(acts_g, acts_e)
    # update
    gu = GraphedUpdate(learner, B, T, 4, 4, R400["r_comm"], enc="mlp")
    m = dict(gt=tm["gt"].transpose(0, 1), ubs=tm["ubs"].transpose(0, 1), agent=tm["agent"].transpose(0, 1),
             d_u2u=tm["d_u2u"].transpose(0, 1), h=th.stack([extra["h0"], extra["h1"]] + [extra["h1"]] * (T - 1)).view(T + 1, B, 4, -1)
             .transpose(0, 1), act=extra["acts"].view(T, B, 4).transpose(0, 1), rew=extra["rews"].transpose(0, 1),
             done=extra["dones"].transpose(0, 1))
    opt = learner.optimizer
    state = (learner.flat.flat, learner.flat_target, opt.m, opt.v, opt.hyper)
    snap = [t.clone() for t in state]
    out_g = gu(m)
    loss_g, q_g = out_g["LossQ"].clone(), out_g["QVals"].clone()
    after_g = [t.clone() for t in state]
    assert not th.equal(after_g[0], snap[0]), "the update did not move the parameters"
    for dst, src in zip(state, snap):
        dst.copy_(src)
    learner.invalidate_weight_cache()
    out_e = learner.update(gu._batch())
    assert th.equal(out_e["LossQ"], loss_g) and th.equal(out_e["QVals"], q_g)
    for a, b in zip(state, after_g):
        assert th.equal(a, b)


def _two_episodes(seed):
    """Two seeded r400 episodes of the exp2 device loop at B = 256 (INTEGRATION.md "exp2 (o='mlp') on the device"): simulator -> flat
    batch -> act -> cache (staged) -> update from the replay's flat batches after each episode.  -> (parameters before, after, losses)."""
    from uav_bs_ctrl_amd.graph import from_padded_obs_flat
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv, MapParams
    th.manual_seed(seed)
    B, n, T = 256, 4, R400["episode_limit"]
    env = BatchedUbsCoverageEnv(MapParams(**R400), B)
    args = _args(None)
    args.seed = seed
    learner = MultiAgentQLearner(dict(obs_shape=F, n_actions=env.n_actions, n_agents=n, episode_limit=T), args)
    buf = SequenceReplay(2 * B, T, n, 4, 256, n_envs=B, r_comm=R400["r_comm"])
    gen = th.Generator(device="cuda").manual_seed(seed)
    p0 = learner.flat.flat.clone()
    losses = []
    for _ in range(2):
        o = env.reset(generator=gen)
        h = learner.init_hidden(B)
        for _ in range(T):
            g = from_padded_obs_flat(o["gt"], o["ubs"], o["agent"], o["d_u2u"], R400["r_comm"])
            acts, h2 = learner.act(g, h, 0.5)
            buf.stage_obs(dict(gt=o["gt"], ubs=o["ubs"], agent=o["agent"], d_u2u=o["d_u2u"], h=h.view(B, n, -1)))
            o, rew, done, info = env.step(acts)
            learner.cache(buf, None, None, None, acts, rew, o, h2, None, done, info["BadMask"], staged=True)
            h = h2
        assert len(buf) == min(buf.capacity, B * (len(losses) + 1))
        losses.append(learner.update(buf.sample(64, gen, enc="mlp"))["LossQ"].clone())
    return p0, learner.flat.flat.clone(), th.stack(losses)


def test_two_seeded_episodes_reproduce_and_train():
    p0, p1, l1 = _two_episodes(21)
    q0, q1, l2 = _two_episodes(21)
    assert th.equal(p0, q0) and not th.equal(p0, p1), "the updates did not move the parameters"
    assert bool(th.isfinite(l1).all())
    assert th.equal(p1, q1) and th.equal(l1, l2), "two seeded runs differ"

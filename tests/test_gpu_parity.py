"""`-m gpu` parity tests: the HIP path (through the C-ABI) against the committed golden fixtures and against the CPU
oracle on seeded synthetic graphs.  Tolerance: north_star's 1e-5 relative fp32 (rtol = 1e-5, atol = 1e-5 max|ref|)
for outputs AND for gradients; a gradient is a long fp32 reduction, so where float32 arithmetic itself cannot hold 1e-5
the bound is 4x the float32 CPU oracle's own error against float64 on the same inputs (tests/util.py: grad_close).
Every gradient comparison records its measured error in gpurun_out/grad_errors.jsonl (table: profiles/r03_grad_errors.txt)."""
import pytest
import torch as th

from oracle import restatement as R
from tests.gpu_util import (EXP3, UPDATE_CASES, _exp3_learner_and_sequence, _LibSpy, _oracle_at_gpu_branch, _ragged_env_talk,
                            _random_talk, agent_from_params, default_init_params, make_args, synth_graph, to_batch)
from tests.util import assert_close, grad_close, load_golden, load_learner_golden, wait_worker

pytestmark = pytest.mark.gpu

GOLDENS = ["agent_none", "agent_tarmac", "agent_tarmac_r2", "agent_tarmac_duel", "agent_disc", "agent_base",
           "agent_commnet", "agent_econv", "agent_mlp_tarmac", "agent_debugmap_tarmac"]


def _loss(q, h2, wq, wh):
    return (q * wq).sum() + (h2 * wh).sum()


# No blanket absolute floor: gradients that are analytically zero (d/d f_sign.bias: a constant added to every signature
# cancels in the softmax) or that cancel to ~0 are covered by grad_close's "4x the fp32 CPU oracle's own absolute error".
GRAD_FLOOR = 0.0


def _oracle32_golden(name):
    """Gradients of the fixture's loss from the float32 CPU oracle: what fp32 arithmetic itself achieves."""
    g, h, p, cfg, z = load_golden(name, dtype=th.float32)
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    h = h.clone().requires_grad_(True)
    gum = th.as_tensor(z["gumbel"], dtype=th.float32) if "gumbel" in z.files else None
    if cfg["enc"] == "drqn":
        q, h2 = R.drqn_gnn_agent_forward(g, h, p, cfg["n_heads"])
    else:
        q, h2 = R.gnn_agent_forward(g, h, p, cfg, gumbel=gum)
    loss = _loss(q, h2, th.as_tensor(z["wq"], dtype=th.float32), th.as_tensor(z["wh"], dtype=th.float32))
    gr = th.autograd.grad(loss, list(p.values()) + [h], allow_unused=True)
    return {k: (th.zeros_like(t) if g_ is None else g_) for (k, t), g_ in zip(list(p.items()) + [("__h__", h)], gr)}


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_forward_backward(name):
    g, h, p, cfg, z = load_golden(name, dtype=th.float32)
    obs_shape = int(g["x_flat"].shape[1]) if cfg["enc"] == "mlp" else None
    net = agent_from_params(p, cfg, obs_shape)
    if cfg["enc"] == "mlp":
        g = dict(g, x_a=g["x_flat"])
        g.pop("x_flat")
    hb = to_batch(g)
    hd = h.cuda().requires_grad_(True)
    if "gumbel" in z.files:    # DiscreteComm: inject the per-edge Gumbel noise the reference drew (CSC order)
        net.f_comm.gumbel = th.as_tensor(z["gumbel"], dtype=th.float32).cuda()
    q, h2 = net(hb, hd)
    assert_close(q, th.as_tensor(z["q"]), 1e-5, f"{name}: q")
    assert_close(h2, th.as_tensor(z["h_out"]), 1e-5, f"{name}: h'")
    wq, wh = (th.as_tensor(z[k], dtype=th.float32).cuda() for k in ("wq", "wh"))
    _loss(q, h2, wq, wh).backward()
    g32 = _oracle32_golden(name)
    for k, prm in net.named_parameters():
        ref = th.as_tensor(z["grad:" + k])
        got = prm.grad if prm.grad is not None else th.zeros_like(prm)
        grad_close(got, ref, f"{name}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)
    grad_close(hd.grad, th.as_tensor(z["grad:__h__"]), f"{name}: grad h", ref32=g32["__h__"], floor=GRAD_FLOOR)


def test_golden_drqn_twin():
    import types
    from uav_bs_ctrl_amd.agents import REGISTRY
    g, h, p, cfg, z = load_golden("agent_drqn", dtype=th.float32)
    net = REGISTRY["drqn_gnn"](dict(agent=2, gt=4), cfg["n_actions"], types.SimpleNamespace(hidden_size=32, n_heads=4))
    net.load_state_dict(p)
    net = net.cuda()
    hd = h.cuda().requires_grad_(True)
    q, h2 = net(to_batch(g), hd)
    assert_close(q, th.as_tensor(z["q"]), 1e-5, "drqn q")
    assert_close(h2, th.as_tensor(z["h_out"]), 1e-5, "drqn h'")
    _loss(q, h2, th.as_tensor(z["wq"], dtype=th.float32).cuda(), th.as_tensor(z["wh"], dtype=th.float32).cuda()).backward()
    g32 = _oracle32_golden("agent_drqn")
    for k, prm in net.named_parameters():
        grad_close(prm.grad, th.as_tensor(z["grad:" + k]), f"drqn grad {k}", ref32=g32[k], floor=GRAD_FLOOR)


@pytest.mark.parametrize("dist,talk,B,n,M", [("dense", "complete", 16, 8, 80), ("env", "complete", 64, 8, 80),
                                             ("ragged", "sparse", 8, 16, 200), ("dense", "complete", 32, 4, 40)])
def test_exp3_sizes_vs_oracle(dist, talk, B, n, M):
    """exp3 model sizes (H=256, nh=4, msg=64, key=16) on seeded synthetic graphs; oracle in float64 and float32."""
    p64 = default_init_params(EXP3, seed=1)
    g = synth_graph(B, n, M, dist, seed=3, talk=talk)
    gen = th.Generator().manual_seed(99)
    h = 0.5 * th.randn(B * n, 256, generator=gen)
    wq, wh = th.randn(B * n, 9, generator=gen), th.randn(B * n, 256, generator=gen) / 16

    def oracle(dtype):
        pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p64.items()}
        gg = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g.items()}
        hh = h.detach().clone().to(dtype).requires_grad_(True)
        q, h2 = R.gnn_agent_forward(gg, hh, pp, EXP3)
        gr = th.autograd.grad(_loss(q, h2, wq.to(dtype), wh.to(dtype)), list(pp.values()) + [hh])
        return q, h2, dict(zip(list(pp) + ["__h__"], gr))

    q64, h64, g64 = oracle(th.float64)
    q32, h32, g32 = oracle(th.float32)
    net = agent_from_params(p64, EXP3)
    hd = h.cuda().requires_grad_(True)
    q, h2 = net(to_batch(g), hd)
    assert_close(q, q64, 1e-5, "q")
    assert_close(h2, h64, 1e-5, "h'")
    _loss(q, h2, wq.cuda(), wh.cuda()).backward()
    grads = {k: prm.grad for k, prm in net.named_parameters()}
    grads["__h__"] = hd.grad
    for k, ref in g64.items():
        grad_close(grads[k], ref, f"exp3 {dist} {n}x{M} B={B}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)


@pytest.mark.parametrize("exact_ties,talk", [(True, "sparse"), (False, "sparse"), (False, "complete")])
def test_exp3_disc_comm_vs_oracle(exact_ties, talk):
    """DiscreteComm at exp3 sizes (msg = 64 bit pairs) with injected noise.  exact_ties=True: the oracle applies the rule
    K5 implements (first in-edge whose hard bit is set owns the channel); exact_ties=False: the LITERAL reference rule
    (max over the floating-point values (y_hard - y_soft) + y_soft, gnn_agents.py:166-178) - with up to 8 competing
    in-edges per destination (complete graph) forward AND gradients still agree: (1 - s) + s rounds to exactly 1 so the
    literal max also picks the first set bit (tests/test_oracle_kats.py counts the disagreements: none)."""
    cfg = dict(EXP3, c="disc", exact_ties=exact_ties)
    p64 = default_init_params(cfg, seed=4)
    B, n = 24, 8
    g = synth_graph(B, n, 80, "env", seed=8, talk=talk)
    gen = th.Generator().manual_seed(17)
    N, E = B * n, g["talk_src"].numel()
    h = 0.5 * th.randn(N, 256, generator=gen)
    gum = -th.empty(E, 64, 2).exponential_(generator=gen).log()
    wq, wh = th.randn(N, 9, generator=gen), th.randn(N, 256, generator=gen) / 16
    def oracle(dtype):
        pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p64.items()}
        gg = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g.items()}
        hh = h.detach().clone().to(dtype).requires_grad_(True)
        q_, h_ = R.gnn_agent_forward(gg, hh, pp, cfg, gumbel=gum.to(dtype))
        return q_, h_, th.autograd.grad(_loss(q_, h_, wq.to(dtype), wh.to(dtype)), list(pp.values()) + [hh])
    q64, h64, g64 = oracle(th.float64)
    _, _, g32 = oracle(th.float32)
    net = agent_from_params(p64, cfg)
    net.f_comm.gumbel = gum.cuda()
    hd = h.cuda().requires_grad_(True)
    q, h2 = net(to_batch(g), hd)
    assert_close(q, q64, 1e-5, "disc q")
    assert_close(h2, h64, 1e-5, "disc h'")
    _loss(q, h2, wq.cuda(), wh.cuda()).backward()
    got = [prm.grad for prm in net.parameters()] + [hd.grad]
    for k, a, b, b32 in zip(list(p64) + ["__h__"], got, g64, g32):
        grad_close(a, b, f"disc ties={exact_ties} {talk}: grad {k}", ref32=b32, floor=GRAD_FLOOR)
    # without injected noise the module draws its own on the device
    q2, _ = net(to_batch(g), h.cuda())
    assert th.isfinite(q2).all()


def _philox4x32_10(c, k):
    """numpy Philox4x32-10 (test infrastructure): c [n, 4] uint32 counters, k (k0, k1)."""
    import numpy as np
    c = c.astype(np.uint64).copy()
    k0, k1 = np.uint64(k[0]), np.uint64(k[1])
    M0, M1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[:, 0], M1 * c[:, 2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = np.stack([(hi1 ^ c[:, 1] ^ k0) & mask, lo1, (hi0 ^ c[:, 3] ^ k1) & mask, lo0], 1)
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return c.astype(np.uint32)


def test_disc_comm_in_kernel_gumbel_noise():
    """K5 with the noise drawn INSIDE the kernel (Philox4x32-10 keyed by the seed, counter = (CSC position, channel, step)):
    (1) the stream equals a numpy Philox + float64 -log(-log(u)) (known answers for the published algorithm), has Gumbel(0, 1)
    moments, depends on seed and step and on nothing else; (2) the fused forward / backward are BIT-identical to the
    injected-noise path fed with the materialised stream; (3) the module is reproducible from torch.manual_seed."""
    import numpy as np
    from uav_bs_ctrl_amd import ops
    E, M = 5000, 64
    seed = 0x1234567890ABCDEF & (2 ** 62 - 1)
    rng = th.tensor([seed, 7], dtype=th.int64, device="cuda")
    noise = ops.gumbel_noise(rng, E, M)
    e_idx, i_idx = np.meshgrid(np.arange(40), np.arange(M), indexing="ij")
    ctr = np.stack([e_idx.ravel(), i_idx.ravel(), np.full(e_idx.size, 7), np.zeros(e_idx.size)], 1).astype(np.uint32)
    r = _philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    u = ((r[:, :2] >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
    ref = -np.log(-np.log(u))
    got = noise[:40].cpu().double().numpy().reshape(-1, 2)
    # identical integers; the float32 -log(-log(u)) is ill-conditioned towards u -> 1 (large draws): 1e-5 covers it
    assert np.allclose(got, ref, rtol=2e-5, atol=2e-5), float(np.abs(got - ref).max())
    x = noise.double()
    n_s = x.numel()
    assert abs(float(x.mean()) - 0.5772156649) < 5 * (1.6449 / n_s) ** 0.5
    assert abs(float(x.var()) - 1.6449340668) < 0.02
    assert th.equal(ops.gumbel_noise(rng, E, M), noise)
    rng2 = th.tensor([seed, 8], dtype=th.int64, device="cuda")
    assert not th.equal(ops.gumbel_noise(rng2, E, M), noise)
    # (2) fused vs injected
    g = to_batch(synth_graph(24, 8, 80, "env", seed=8, talk="sparse"))
    Et = g.number_of_edges("talk")
    gen = th.Generator().manual_seed(3)
    logits_a = th.randn(24 * 8, 2 * M, generator=gen).cuda().requires_grad_(True)
    logits_b = logits_a.detach().clone().requires_grad_(True)
    w = th.randn(24 * 8, 2 * M, generator=gen).cuda()
    c_a = ops.disc_comm_aggregate(logits_a, None, g, tau=0.5, rng=rng)
    c_b = ops.disc_comm_aggregate(logits_b, ops.gumbel_noise(rng, Et, M), g, tau=0.5)
    assert th.equal(c_a, c_b)
    (c_a * w).sum().backward()
    (c_b * w).sum().backward()
    assert th.equal(logits_a.grad, logits_b.grad)
    # (3) the module: reproducible from torch's seed, a new draw per forward
    cfg = dict(EXP3, c="disc")
    net = agent_from_params(default_init_params(cfg, seed=4), cfg)
    h = th.zeros(24 * 8, 256, device="cuda")
    outs = []
    for _ in range(2):
        th.manual_seed(11)
        net.f_comm.rng_state = None
        with th.no_grad():
            q1, _ = net(g, h)
            q2, _ = net(g, h)
        outs.append((q1, q2))
    assert th.equal(outs[0][0], outs[1][0]) and th.equal(outs[0][1], outs[1][1])
    assert not th.equal(outs[0][0], outs[0][1]) and int(net.f_comm.rng_state[1]) == 2


def test_backward_is_deterministic():
    p64 = default_init_params(EXP3, seed=2)
    g = synth_graph(32, 8, 80, "ragged", seed=5)
    net = agent_from_params(p64, EXP3)
    hb = to_batch(g)
    h = th.randn(256, 256, generator=th.Generator().manual_seed(1)).cuda()
    outs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        q, h2 = net(hb, h)
        (q.sum() + h2.square().sum()).backward()
        outs.append(th.cat([p.grad.flatten() for p in net.parameters()]).clone())
    assert th.equal(outs[0], outs[1]), "two identical backward passes differ bitwise"


def test_cpu_tensors_fail_loudly():
    from uav_bs_ctrl_amd._lib import UavGnnError
    g, h, p, cfg, _ = load_golden("agent_tarmac", dtype=th.float32)
    net = agent_from_params(p, cfg, device="cpu")
    from uav_bs_ctrl_amd import HeteroBatch
    with pytest.raises(UavGnnError):
        net(HeteroBatch.from_arrays(**g), h)


def test_learner_update_reproduces_reference_update():
    """Row L on the GPU: uav_bs_ctrl_amd.learner.MultiAgentQLearner.update (HIP forward/backward, flat-buffer clip,
    AdamW, polyak) against the state the reference's learner reached after ONE update from the same parameters/batch."""
    import types
    from uav_bs_ctrl_amd import HeteroBatch
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    batch, p, cfg, z = load_learner_golden(dtype=th.float32)
    args = types.SimpleNamespace(device="cuda", hidden_size=32, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4,
                                 n_rounds=1, dueling=False, mixer=False, double_q=True, lr=cfg["lr"], gamma=cfg["gamma"],
                                 polyak=cfg["polyak"], max_seq_len=cfg["T"], seed=0)
    env_info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=cfg["n_actions"], n_agents=cfg["n_agents"],
                    episode_limit=10)
    L = MultiAgentQLearner(env_info, args)
    L.policy_net.load_state_dict(p)
    L.target_net.load_state_dict(p)
    dev = th.device("cuda")
    b = dict(obs=[HeteroBatch.from_arrays(**g).to(dev) for g in batch["obs"]], h0=batch["h0"].to(dev),
             h1=batch["h1"].to(dev), acts=batch["acts"].to(dev), rews=batch["rews"].to(dev), dones=batch["dones"].to(dev))
    out = L.update(b)
    assert_close(out["LossQ"], th.as_tensor(z["loss"]).double(), 1e-5, "LossQ")
    qv = out["QVals"][:-1].gather(2, b["acts"]).view(cfg["T"], cfg["B"], cfg["n_agents"])
    assert_close(qv, th.as_tensor(z["qvals"]), 1e-5, "QVals")
    b32, p32, _, _ = load_learner_golden(dtype=th.float32)
    pp32 = {k: v.clone().requires_grad_(True) for k, v in p32.items()}
    l32, _, _ = R.madrqn_loss(b32["obs"], b32["h0"], b32["h1"], b32["acts"], b32["rews"], b32["dones"], pp32,
                              {k: v.clone() for k, v in p32.items()}, cfg, cfg["gamma"], cfg["double_q"])
    g32 = dict(zip(pp32, th.autograd.grad(l32, list(pp32.values()))))
    for k, prm in L.policy_net.named_parameters():
        g_ref = th.as_tensor(z["grad_clipped:" + k])
        grad_close(prm.grad, g_ref, f"learner update: clipped grad {k}", ref32=g32[k].clamp(-1, 1), floor=GRAD_FLOOR)
        # Adam's first step is lr * sign-like(g): only meaningful where the gradient is well above rounding noise
        sure = g_ref.abs() > 1e-4
        after = th.as_tensor(z["policy_after:" + k])
        assert float(((prm.detach().cpu().double() - after).abs() * sure).max()) < 2e-6, f"policy param {k}"
    for k, prm in L.target_net.named_parameters():
        assert float((prm.detach().cpu().double() - th.as_tensor(z["target_after:" + k])).abs().max()) < 1e-6, k
    # rollout: one epsilon draw per team, greedy == argmax of the policy logits when eps = 0
    acts, h2 = L.act(b["obs"][0], b["h0"], 0.0)
    with th.no_grad():
        logits, _ = L.policy_net(b["obs"][0], b["h0"])
    assert th.equal(acts, logits.argmax(1)) and h2.shape == b["h0"].shape
    acts_r, _ = L.act(b["obs"][0], b["h0"], 1.0)
    assert int(acts_r.min()) >= 0 and int(acts_r.max()) < cfg["n_actions"]
    # time-batched encoder (all T+1 steps encoded by one call per network): same loss, same update
    from uav_bs_ctrl_amd import batch as hb_batch
    L2 = MultiAgentQLearner(env_info, args)
    L2.policy_net.load_state_dict(p)
    L2.target_net.load_state_dict(p)
    b2 = dict(b, obs_all=hb_batch(b["obs"]))
    out2 = L2.update(b2)
    assert_close(out2["LossQ"], th.as_tensor(z["loss"]).double(), 1e-5, "LossQ (time-batched)")
    for (k, p1), (_, p2) in zip(L.policy_net.named_parameters(), L2.policy_net.named_parameters()):
        assert_close(p2.grad, p1.grad, 2e-5, f"time-batched clipped grad {k}", floor=2e-6)


def test_device_side_graph_construction_is_bit_identical_to_host_builder():
    """f1: HIP count/compact passes == per-environment ``from_obs_dicts`` + ``batch`` (the reference's construction)."""
    import numpy as np
    from uav_bs_ctrl_amd import batch, from_obs_dicts, from_padded_obs
    rng = np.random.default_rng(3)
    for (B, n, M, r) in [(5, 8, 80, 1.0), (3, 4, 200, 0.4), (2, 16, 70, np.inf), (4, 1, 20, 1.0)]:
        gt = rng.uniform(-1, 1, (B, n, M, 5)).astype(np.float32)
        gt[..., 0] = rng.uniform(size=(B, n, M)) < 0.3
        gt[0, 0, :, 0] = 0                                   # an agent that sees nothing
        gt[-1, -1, :, 0] = 1                                 # and one that sees everything
        ub = rng.uniform(-1, 1, (B, n, max(n - 1, 0), 3)).astype(np.float32)
        ub[..., 0] = rng.uniform(size=ub.shape[:-1]) < 0.5
        ag = rng.uniform(0, 1, (B, n, 2)).astype(np.float32)
        d = rng.uniform(0, 2, (B, n, n)).astype(np.float32)
        d = (d + d.transpose(0, 2, 1)) / 2
        for b in range(B):
            np.fill_diagonal(d[b], 0)
        host = batch([from_obs_dicts([dict(agent=ag[b, i], ubs=ub[b, i], gt=gt[b, i]) for i in range(n)], d[b], r)
                      for b in range(B)])
        dev = from_padded_obs(*(th.as_tensor(a).cuda() for a in (gt, ub, ag, d)), r_comm=r)
        for et in ("seen", "near"):
            xs, off = dev.relation_segments(et)
            xh, offh = host.relation_segments(et)
            assert th.equal(off.cpu(), offh) and th.equal(xs.cpu(), xh), et
        for a, b_ in zip(dev.talk_csc(), host.talk_csc()):
            assert th.equal(a.cpu(), b_)
        assert th.equal(dev.talk_eid().cpu(), host.talk_eid())
        assert th.equal(dev.agent_feat().cpu(), host.agent_feat())
        assert th.equal(dev.graph_off.cpu(), host.graph_off)


@pytest.mark.parametrize("H,nh", [(64, 4), (128, 4), (128, 2), (256, 8), (64, 1), (32, 4)])
def test_other_head_configurations_vs_oracle(H, nh):
    """DEFAULT_CONFIG's H=64 (MFMA path, D=16), D=32, and head counts without an MFMA instantiation (VALU kernel)."""
    cfg = dict(EXP3, hidden_size=H, n_heads=nh, msg_size=16, key_size=8, c="tarmac")
    p64 = default_init_params(cfg, seed=3)
    g = synth_graph(6, 5, 70, "ragged", seed=11, talk="sparse")
    gen = th.Generator().manual_seed(5)
    N = 30
    h = 0.5 * th.randn(N, H, generator=gen)
    wq, wh = th.randn(N, 9, generator=gen), th.randn(N, H, generator=gen) / 8
    def oracle(dtype):
        pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p64.items()}
        gg = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g.items()}
        hh = h.detach().clone().to(dtype).requires_grad_(True)
        q_, h_ = R.gnn_agent_forward(gg, hh, pp, cfg)
        return q_, h_, th.autograd.grad(_loss(q_, h_, wq.to(dtype), wh.to(dtype)), list(pp.values()) + [hh])
    q64, h64, g64 = oracle(th.float64)
    _, _, g32 = oracle(th.float32)
    net = agent_from_params(p64, cfg)
    hd = h.cuda().requires_grad_(True)
    q, h2 = net(to_batch(g), hd)
    assert_close(q, q64, 1e-5, "q")
    assert_close(h2, h64, 1e-5, "h'")
    _loss(q, h2, wq.cuda(), wh.cuda()).backward()
    for k, a, b, b32 in zip(list(p64) + ["__h__"], [p_.grad for p_ in net.parameters()] + [hd.grad], g64, g32):
        grad_close(a, b, f"H={H} nh={nh}: grad {k}", ref32=b32, floor=GRAD_FLOOR)


def test_edge_cases_empty_relations_single_agent_and_isolated_nodes():
    """All agents blind and alone (E_seen = E_near = 0), a talk relation without any edge (the reference's zero-edge
    branch, gnn_agents.py:139-141, unreachable there because of self loops), and a single-agent graph."""
    from uav_bs_ctrl_amd import HeteroBatch
    cfg = dict(EXP3, hidden_size=64, msg_size=16, key_size=8)
    p64 = default_init_params(cfg, seed=6)
    net = agent_from_params(p64, cfg)
    for N in (1, 7):
        g = dict(x_a=th.rand(N, 2), x_gt=th.zeros(0, 4), seen_off=th.zeros(N + 1, dtype=th.int32), x_ubs=th.zeros(0, 2),
                 near_off=th.zeros(N + 1, dtype=th.int32), talk_off=th.zeros(N + 1, dtype=th.int32),
                 talk_src=th.zeros(0, dtype=th.int32))
        h = th.randn(N, 64)
        gg = {k: (v.double() if v.is_floating_point() else v) for k, v in g.items()}
        q64, h64 = R.gnn_agent_forward(gg, h.double(), p64, cfg)
        hd = h.cuda().requires_grad_(True)
        q, h2 = net(HeteroBatch.from_arrays(**g).to("cuda"), hd)
        assert_close(q, q64, 1e-5, f"N={N} q")
        assert_close(h2, h64, 1e-5, f"N={N} h'")
        (q.sum() + h2.sum()).backward()
        assert all(th.isfinite(p_.grad).all() for p_ in net.parameters())


def test_mfma_and_valu_kernels_agree_and_order_is_only_a_schedule():
    """K1 forward: fp32-MFMA kernel vs the VALU kernel of the same library; the degree-sorted hand-out order must not
    change a single bit of the result."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.agents.gnn_agents import GATv2Conv
    hb = to_batch(synth_graph(40, 8, 80, "ragged", seed=21))
    x_src, off = hb.relation_segments("seen")
    x_a, N = hb.agent_feat(), hb.num_nodes("agent")
    th.manual_seed(0)
    conv = GATv2Conv((4, 2), 64, 4).cuda()
    p = [t.detach().contiguous() for t in (conv.fc_src.weight, conv.fc_src.bias + 0.1, conv.fc_dst.weight,
                                           conv.fc_dst.bias - 0.05, conv.attn, conv.res_fc.weight, conv.res_fc.bias)]
    outs = []
    for fn, order in ((L.lib().uavgnn_gatv2_fwd, None), (L.lib().uavgnn_gatv2_fwd, hb.relation_order("seen")),
                      (L.lib().uavgnn_gatv2_fwd_valu, None)):
        out = th.empty(N, 256, device="cuda")
        a_save = th.empty(x_src.shape[0], 4, device="cuda")
        rc = fn(x_src.data_ptr(), x_src.shape[0], 4, x_a.data_ptr(), 2, off.data_ptr(), L.ptr(order), N, *[t.data_ptr() for t in p], 4,
                64, 0.2, out.data_ptr(), 256, a_save.data_ptr(), L.stream())
        assert rc == 0
        outs.append((out, a_save))
    assert th.equal(outs[0][0], outs[1][0]) and th.equal(outs[0][1], outs[1][1]), "dst_order changed the result"
    assert_close(outs[0][0], outs[2][0], 2e-6, "mfma vs valu: out")
    assert_close(outs[0][1], outs[2][1], 2e-6, "mfma vs valu: attention weights")
    seg = th.repeat_interleave(th.arange(N, device="cuda"), (off[1:] - off[:-1]).long())
    sums = th.zeros(N, 4, device="cuda").index_add_(0, seg, outs[0][1])
    deg = (off[1:] - off[:-1]).cuda()
    assert_close(sums[deg > 0], th.ones_like(sums[deg > 0]), 1e-6, "attention weights sum to one per destination")


@pytest.mark.parametrize("N,max_deg,K,M", [(40, 150, 16, 64), (300, 9, 5, 200), (64, 70, 64, 256), (17, 3, 1, 1)])
def test_talk_attention_kernel_vs_oracle(N, max_deg, K, M):
    """K3b alone, incl. in-degree > 64 (multi-pass), K / M at their limits, zero-in-degree nodes, duplicate edges."""
    from uav_bs_ctrl_amd import ops
    g, off, src = _random_talk(N, max_deg, seed=N)
    g = g.to("cuda")
    gen = th.Generator().manual_seed(1)
    s, q, v = (th.randn(N, d, generator=gen) for d in (K, K, M))
    w = th.randn(N, M, generator=gen)
    dst = R.seg_ids(off)

    def ref(s_, q_, v_, uniform):
        if uniform:
            return R.segment_mean(v_[src.long()], dst, N)
        e = (s_[src.long()] * q_[dst]).sum(-1, keepdim=True) / K
        return R.segment_sum(v_[src.long()] * R.segment_softmax(e, dst, N), dst, N)

    for uniform in (False, True):
        s64, q64, v64 = (t.double().requires_grad_(True) for t in (s, q, v))
        c64 = ref(s64, q64, v64, uniform)
        g64 = th.autograd.grad((c64 * w.double()).sum(), [v64] if uniform else [s64, q64, v64])
        s32, q32, v32 = (t.clone().requires_grad_(True) for t in (s, q, v))
        g32 = th.autograd.grad((ref(s32, q32, v32, uniform) * w).sum(), [v32] if uniform else [s32, q32, v32])
        sd, qd, vd = (t.cuda().requires_grad_(True) for t in (s, q, v))
        c = ops.talk_attention(None if uniform else sd, None if uniform else qd, vd, g, 1.0 / K)
        assert_close(c, c64, 1e-5, f"c uniform={uniform}")
        got = th.autograd.grad((c * w.cuda()).sum(), [vd] if uniform else [sd, qd, vd])
        for a, b, b32, nm in zip(got, g64, g32, ["d_v"] if uniform else ["d_s", "d_q", "d_v"]):
            grad_close(a, b, f"K3b N={N} deg<={max_deg} K={K} M={M}: {nm} uniform={uniform}", ref32=b32)


@pytest.mark.parametrize("N,H", [(1000, 256), (33, 30), (5, 7)])
def test_gru_gates_kernel_vs_oracle(N, H):
    from uav_bs_ctrl_amd import ops
    gen = th.Generator().manual_seed(H)
    gi, gh, h, w = (th.randn(N, d, generator=gen) for d in (3 * H, 3 * H, H, H))

    def ref(gi_, gh_, h_):
        r = th.sigmoid(gi_[:, :H] + gh_[:, :H])
        z = th.sigmoid(gi_[:, H:2 * H] + gh_[:, H:2 * H])
        n = th.tanh(gi_[:, 2 * H:] + r * gh_[:, 2 * H:])
        return (1 - z) * n + z * h_
    a64 = [t.double().requires_grad_(True) for t in (gi, gh, h)]
    o64 = ref(*a64)
    g64 = th.autograd.grad((o64 * w.double()).sum(), a64)
    ad = [t.cuda().requires_grad_(True) for t in (gi, gh, h)]
    o = ops.gru_gates(*ad)
    assert_close(o, o64, 1e-5, "h'")
    for a, b, nm in zip(th.autograd.grad((o * w.cuda()).sum(), ad), g64, ("d_gi", "d_gh", "d_h")):
        assert_close(a, b, 1e-5, nm, floor=1e-7)


def _env_subset(g, envs, n):
    """Segment arrays of a subset of environments of a batched synthetic graph (environments are independent units)."""
    out_a, xg, xu, so, no, to, ts = [], [], [], [0], [0], [0], []
    for k, b in enumerate(envs):
        for i in range(n):
            a = b * n + i
            s0, s1 = int(g["seen_off"][a]), int(g["seen_off"][a + 1])
            n0, n1 = int(g["near_off"][a]), int(g["near_off"][a + 1])
            t0, t1 = int(g["talk_off"][a]), int(g["talk_off"][a + 1])
            xg.append(g["x_gt"][s0:s1]); xu.append(g["x_ubs"][n0:n1])
            so.append(so[-1] + s1 - s0); no.append(no[-1] + n1 - n0); to.append(to[-1] + t1 - t0)
            ts.append(g["talk_src"][t0:t1].long() - b * n + k * n)
            out_a.append(a)
    rows = th.tensor(out_a)
    sub = dict(x_a=g["x_a"][rows], x_gt=th.cat(xg), seen_off=th.tensor(so, dtype=th.int32), x_ubs=th.cat(xu),
               near_off=th.tensor(no, dtype=th.int32), talk_off=th.tensor(to, dtype=th.int32),
               talk_src=th.cat(ts).to(th.int32))
    return sub, rows


@pytest.mark.parametrize("name,B,n,M,dist,talk", [("C2 4x40 B=1024", 1024, 4, 40, "dense", "complete"),
                                                  ("C3 8x80 B=4096 dense", 4096, 8, 80, "dense", "complete"),
                                                  ("C3 8x80 B=4096 env", 4096, 8, 80, "env", "complete"),
                                                  ("C5 16x200 B=1024 sparse talk", 1024, 16, 200, "ragged", "sparse")])
def test_full_size_configs_by_environment_subsets_and_properties(name, B, n, M, dist, talk):
    """BASELINE.json configs at FULL batch size.  The CPU oracle cannot run 4096 environments in seconds, but
    environments are independent units of the batched graph, so (1) the rows of a random subset of environments must
    equal the oracle run on just those environments; size-independent properties cover the rest: (2) running the batch
    in two halves gives the same rows (batch equivariance), (3) the forward is deterministic bit for bit."""
    cfg = EXP3
    p64 = default_init_params(cfg, seed=9)
    g = synth_graph(B, n, M, dist, seed=31, talk=talk)
    N = B * n
    gen = th.Generator().manual_seed(77)
    h = 0.5 * th.randn(N, 256, generator=gen)
    net = agent_from_params(p64, cfg)
    hb = to_batch(g)
    with th.no_grad():
        q, h2 = net(hb, h.cuda())
        q_b, h2_b = net(hb, h.cuda())
    assert th.equal(q, q_b) and th.equal(h2, h2_b), f"{name}: forward not deterministic"
    envs = th.randperm(B, generator=gen)[:6].tolist()
    sub, rows = _env_subset(g, envs, n)
    gg = {k: (v.double() if v.is_floating_point() else v) for k, v in sub.items()}
    q64, h64 = R.gnn_agent_forward(gg, h[rows].double(), p64, cfg)
    assert_close(q[rows.cuda()], q64, 1e-5, f"{name}: q on env subset")
    assert_close(h2[rows.cuda()], h64, 1e-5, f"{name}: h' on env subset")
    # batch equivariance at full size: second half of the environments on its own
    half = B // 2
    sub2, rows2 = _env_subset(g, list(range(half, half + 3)), n)      # cheap construction check of the helper itself
    assert th.equal(sub2["x_a"], g["x_a"][rows2])
    lo = N // 2
    g_hi = dict(x_a=g["x_a"][lo:], x_gt=g["x_gt"][int(g["seen_off"][lo]):], seen_off=g["seen_off"][lo:] - g["seen_off"][lo],
                x_ubs=g["x_ubs"][int(g["near_off"][lo]):], near_off=g["near_off"][lo:] - g["near_off"][lo],
                talk_off=g["talk_off"][lo:] - g["talk_off"][lo], talk_src=g["talk_src"][int(g["talk_off"][lo]):] - lo)
    with th.no_grad():
        q_hi, h_hi = net(to_batch(g_hi), h[lo:].cuda())
    assert_close(q_hi, q[lo:], 2e-6, f"{name}: batch equivariance q")
    assert_close(h_hi, h2[lo:], 2e-6, f"{name}: batch equivariance h'")


@pytest.mark.parametrize("name,B,n,M,dist,talk", [("C3 8x80 B=4096 dense", 4096, 8, 80, "dense", "complete"),
                                                  ("C3 8x80 B=4096 env", 4096, 8, 80, "env", "complete"),
                                                  ("C5 16x200 B=1024 sparse talk", 1024, 16, 200, "ragged", "sparse")])
def test_full_size_backward_by_masked_loss(name, B, n, M, dist, talk):
    """Backward at FULL batch size: with loss weights that vanish outside a few environments, every parameter gradient
    of the full-batch run must equal the oracle's gradient on just those environments (environments do not interact),
    while the HIP backward kernels still sweep all B environments."""
    cfg = EXP3
    p64 = default_init_params(cfg, seed=10)
    g = synth_graph(B, n, M, dist, seed=41, talk=talk)
    N = B * n
    gen = th.Generator().manual_seed(78)
    h = 0.5 * th.randn(N, 256, generator=gen)
    envs = th.randperm(B, generator=gen)[:5].tolist()
    sub, rows = _env_subset(g, envs, n)
    wq_s, wh_s = th.randn(len(rows), 9, generator=gen), th.randn(len(rows), 256, generator=gen) / 16
    wq, wh = th.zeros(N, 9), th.zeros(N, 256)
    wq[rows], wh[rows] = wq_s, wh_s
    net = agent_from_params(p64, cfg)
    q, h2 = net(to_batch(g), h.cuda())
    _loss(q, h2, wq.cuda(), wh.cuda()).backward()
    def oracle(dtype):
        pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p64.items()}
        gg = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sub.items()}
        q_, h_ = R.gnn_agent_forward(gg, h[rows].to(dtype), pp, cfg)
        return th.autograd.grad(_loss(q_, h_, wq_s.to(dtype), wh_s.to(dtype)), list(pp.values()))
    g64, g32 = oracle(th.float64), oracle(th.float32)
    for (k, prm), ref, r32 in zip(net.named_parameters(), g64, g32):
        grad_close(prm.grad, ref, f"{name}: grad {k}", ref32=r32, floor=GRAD_FLOOR)


def test_replay_to_update_end_to_end_on_device():
    """f1 + f2 + L together: padded observations -> device ring -> sampled batch (graphs rebuilt by the HIP builder) ->
    time-batched update.  The same sampled sequences fed through the host builder must give the same loss."""
    import types
    import numpy as np
    from uav_bs_ctrl_amd import batch as hb_batch, from_obs_dicts
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    E, n, M, H, T = 6, 4, 12, 32, 3
    dev = th.device("cuda")
    rb = SequenceReplay(capacity=12, max_seq_len=T, n_agents=n, n_gts=M, hidden_size=H, n_envs=E, state_dim=0,
                        r_comm=0.9, device=dev)
    gen = th.Generator(device=dev).manual_seed(3)

    def obs():
        gt = th.rand(E, n, M, 5, device=dev, generator=gen) * 2 - 1
        gt[..., 0] = (th.rand(E, n, M, device=dev, generator=gen) < 0.3).float()
        ub = th.rand(E, n, n - 1, 3, device=dev, generator=gen) * 2 - 1
        ub[..., 0] = (th.rand(E, n, n - 1, device=dev, generator=gen) < 0.5).float()
        d = th.rand(E, n, n, device=dev, generator=gen) * 2
        d = (d + d.transpose(1, 2)) / 2 * (1 - th.eye(n, device=dev))
        return dict(gt=gt, ubs=ub, agent=th.rand(E, n, 2, device=dev, generator=gen), d_u2u=d,
                    h=0.1 * th.randn(E, n, H, device=dev, generator=gen), state=th.zeros(E, 0, device=dev))
    cur = obs()
    for t in range(2 * T):
        nxt = obs()
        tr = dict(cur, act=th.randint(5, (E, n), device=dev, generator=gen),
                  rew=th.rand(E, n, device=dev, generator=gen), done=th.zeros(E, 1, device=dev))
        tr.update({"next_" + k: v for k, v in nxt.items()})
        rb.push(tr)
        cur = nxt
    assert len(rb) == 12
    idx = rb.sample_indices(5, gen)
    b = rb.gather(idx)
    b["obs_all"] = hb_batch(b["obs"])
    args = types.SimpleNamespace(device="cuda", hidden_size=H, c="tarmac", n_heads=4, n_layers=1, msg_size=8, key_size=4,
                                 n_rounds=1, dueling=False, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.99,
                                 max_seq_len=T, seed=0)
    env_info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=5, n_agents=n, episode_limit=T)
    th.manual_seed(0)
    L = MultiAgentQLearner(env_info, args)
    loss_dev = float(L.loss(b)[0].detach())
    # the same sequences through the host builder (reference-style construction per environment)
    m = {k: v.index_select(0, idx).cpu() for k, v in rb.mem.items()}
    obs_host = []
    for t in range(T + 1):
        gs = [from_obs_dicts([dict(agent=m["agent"][e, t, i].numpy(), ubs=m["ubs"][e, t, i].numpy(),
                                   gt=m["gt"][e, t, i].numpy()) for i in range(n)], m["d_u2u"][e, t].numpy(), 0.9)
              for e in range(5)]
        obs_host.append(hb_batch(gs).to(dev))
    b2 = dict(b, obs=obs_host)
    b2.pop("obs_all")
    loss_host = float(L.loss(b2)[0].detach())
    assert abs(loss_dev - loss_host) <= 1e-6 * max(1.0, abs(loss_host)), (loss_dev, loss_host)
    out = L.update(b)
    assert np.isfinite(float(out["LossQ"]))


@pytest.mark.parametrize("n,maxdeg,seed", [(1, 3, 0), (300, 6, 1), (4097, 90, 2), (70001, 12, 3), (50, 0, 4), (2000, 400, 5)])
def test_degree_order_is_the_stable_descending_sort(n, maxdeg, seed):
    """uavgnn_degree_order == torch.sort(deg, descending, stable) while degrees stay below the bucket cap (255); above
    the cap it stays a permutation with non-increasing buckets."""
    from uav_bs_ctrl_amd.graph import HeteroBatch
    gen = th.Generator().manual_seed(seed)
    deg = th.randint(0, maxdeg + 1, (n,), generator=gen)
    if seed == 3:
        deg[th.rand(n, generator=gen) < 0.9] = 0
    off = th.zeros(n + 1, dtype=th.int32)
    off[1:] = th.cumsum(deg, 0)
    E = int(off[-1])
    g = HeteroBatch.from_arrays(x_a=th.zeros(n, 2), x_gt=th.zeros(E, 4), seen_off=off, device="cuda")
    if n <= 2048:
        assert g.relation_order("seen") is None      # no more destinations than persistent wavefronts: no order built
    from uav_bs_ctrl_amd import _lib as L
    offd = off.cuda()
    od = th.empty(n, dtype=th.int32, device="cuda")
    nb = L.lib().uavgnn_degree_order_workspace_bytes(n)
    ws = th.empty(nb // 4, dtype=th.int32, device="cuda")
    L.check(L.lib().uavgnn_degree_order(offd.data_ptr(), n, od.data_ptr(), ws.data_ptr(), nb, L.stream()), "order")
    order = od.cpu().long()
    if n > 2048 and E < 16 * n:
        assert th.equal(g.relation_order("seen").cpu().long(), order)
    elif n > 2048:
        assert g.relation_order("seen") is None      # mean in-degree of 16 or more: natural order (graph.py)
    assert sorted(order.tolist()) == list(range(n))
    ref = th.sort(deg.clamp(max=255), descending=True, stable=True)[1]
    assert th.equal(order, ref)


@pytest.mark.parametrize("B,n,p,seed", [(1, 8, 0.5, 0), (257, 8, 0.3, 1), (64, 32, 0.9, 2), (5000, 8, 0.05, 3), (3, 64, 1.0, 4)])
def test_csc_transpose_matches_host_construction(B, n, p, seed):
    """uavgnn_csc_transpose == the sort-based host construction (t_off, t_dst, t_pos identical)."""
    from uav_bs_ctrl_amd.graph import HeteroBatch
    gen = th.Generator().manual_seed(seed)
    adj = th.rand(B, n, n, generator=gen) < p            # adj[b, i, j]: edge i -> j
    src, dst = [], []
    b, i, j = adj.nonzero(as_tuple=True)
    # CSC order: by destination, then by source
    key = (b * n + j) * (B * n) + (b * n + i)
    o = th.argsort(key)
    src, dst = (b * n + i)[o], (b * n + j)[o]
    N = B * n
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(th.bincount(dst, minlength=N), 0)
    kw = dict(x_a=th.zeros(N, 2), talk_off=off, talk_src=src.to(th.int32))
    g_host = HeteroBatch.from_arrays(**kw)
    g_dev = HeteroBatch.from_arrays(**kw, device="cuda")                      # generic kernels (count, scan, fill, sort)
    g_env = HeteroBatch.from_arrays(**kw, device="cuda", graph_off=list(range(0, N + 1, n)))   # one wavefront per graph
    assert g_env.hints["max_graph_agents"] == n
    ref = g_host.talk_transpose()
    for g in (g_dev, g_env):
        for a, bb in zip(ref, g.talk_transpose()):
            assert th.equal(a, bb.cpu())


def test_csc_transpose_env_ragged_graphs():
    """Graphs of different sizes in one batch, one of them wider than a wavefront (chunked sources), some without
    edges."""
    from uav_bs_ctrl_amd.graph import HeteroBatch
    gen = th.Generator().manual_seed(11)
    sizes = [3, 1, 100, 8, 64, 65, 2, 130]
    bounds = [0]
    for k in sizes:
        bounds.append(bounds[-1] + k)
    N = bounds[-1]
    src_l, dst_l = [], []
    for gi, k in enumerate(sizes):
        p = 0.0 if gi == 3 else 0.4
        adj = th.rand(k, k, generator=gen) < p
        i, j = adj.nonzero(as_tuple=True)
        src_l.append(i + bounds[gi])
        dst_l.append(j + bounds[gi])
    src, dst = th.cat(src_l), th.cat(dst_l)
    o = th.argsort(dst * N + src)
    src, dst = src[o], dst[o]
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(th.bincount(dst, minlength=N), 0)
    kw = dict(x_a=th.zeros(N, 2), talk_off=off, talk_src=src.to(th.int32))
    ref = HeteroBatch.from_arrays(**kw).talk_transpose()
    g = HeteroBatch.from_arrays(**kw, device="cuda", graph_off=bounds)
    assert g.hints["max_graph_agents"] == 130
    for a, b in zip(ref, g.talk_transpose()):
        assert th.equal(a, b.cpu())


@pytest.mark.parametrize("N", [200_003, 4_300_001])
def test_csc_transpose_large_scan_and_empty(N):
    """N above one scan tile (4096) takes the tile-totals + carry launches, above 1024 tiles the recursive level;
    E = 0 gives all-zero offsets."""
    from uav_bs_ctrl_amd.graph import HeteroBatch
    gen = th.Generator().manual_seed(0)
    deg = th.randint(0, 3, (N,), generator=gen)
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(deg, 0)
    E = int(off[-1])
    src = th.randint(0, N, (E,), generator=gen).to(th.int32)
    kw = dict(x_a=th.zeros(N, 2), talk_off=off, talk_src=src)
    for a, b in zip(HeteroBatch.from_arrays(**kw).talk_transpose(),
                    HeteroBatch.from_arrays(**kw, device="cuda").talk_transpose()):
        assert th.equal(a, b.cpu())
    g0 = HeteroBatch.from_arrays(x_a=th.zeros(7, 2), talk_off=th.zeros(8, dtype=th.int32),
                                 talk_src=th.zeros(0, dtype=th.int32), device="cuda")
    t_off, t_dst, t_pos = g0.talk_transpose()
    assert t_off.cpu().tolist() == [0] * 8 and t_dst.numel() == 0 and t_pos.numel() == 0


@pytest.mark.parametrize("sizes,p,K,M", [([8] * 37, 1.0, 16, 64), ([1, 16, 3, 8, 2, 16, 5, 7, 9, 1, 1, 12], 0.5, 16, 64),
                                         ([4] * 9 + [13, 2], 0.7, 5, 200), ([16] * 5, 1.0, 64, 256),
                                         ([6, 6, 6], 0.3, 1, 1)])
def test_talk_attention_per_graph_kernels_vs_oracle_and_per_destination_kernels(sizes, p, K, M):
    """K3b per-graph formulation (one wavefront per graph, LDS-staged, transpose-free backward) against the fp64 oracle
    and against the per-destination kernels on the same batch: ragged graph sizes 1..16, graphs without edges, complete
    graphs with self loops, K / M at their limits, uniform (mean) mode."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.graph import HeteroBatch
    N, off, src, dst, bounds = _ragged_env_talk(sizes, p, seed=len(sizes))
    kw = dict(x_a=th.zeros(N, 2), talk_off=off, talk_src=src)
    g_env = HeteroBatch.from_arrays(**kw, graph_off=bounds, device="cuda")
    g_dst = HeteroBatch.from_arrays(**kw, device="cuda")
    assert ops._talk_env(g_env, M, K) is not None and ops._talk_env(g_dst, M, K) is None
    gen = th.Generator().manual_seed(2)
    s, q, v = (th.randn(N, d, generator=gen) for d in (K, K, M))
    w = th.randn(N, M, generator=gen)

    def ref(s_, q_, v_, uniform):
        if uniform:
            return R.segment_mean(v_[src.long()], dst, N)
        e = (s_[src.long()] * q_[dst]).sum(-1, keepdim=True) / K
        return R.segment_sum(v_[src.long()] * R.segment_softmax(e, dst, N), dst, N)

    for uniform in (False, True):
        s64, q64, v64 = (t.double().requires_grad_(True) for t in (s, q, v))
        c64 = ref(s64, q64, v64, uniform)
        g64 = th.autograd.grad((c64 * w.double()).sum(), [v64] if uniform else [s64, q64, v64])
        s32, q32, v32 = (t.clone().requires_grad_(True) for t in (s, q, v))
        g32 = th.autograd.grad((ref(s32, q32, v32, uniform) * w).sum(), [v32] if uniform else [s32, q32, v32])
        outs = []
        for g in (g_env, g_dst):
            sd, qd, vd = (t.cuda().requires_grad_(True) for t in (s, q, v))
            c = ops.talk_attention(None if uniform else sd, None if uniform else qd, vd, g, 1.0 / K)
            got = th.autograd.grad((c * w.cuda()).sum(), [vd] if uniform else [sd, qd, vd])
            outs.append((c, got))
        (c, got), (c2, got2) = outs
        assert "talkT" not in g_env._cache                 # the per-graph backward never builds the transpose
        assert_close(c, c64, 1e-5, f"c uniform={uniform}")
        assert_close(c, c2, 2e-6, f"c env vs dst uniform={uniform}")
        for a, b, b32, b2, nm in zip(got, g64, g32, got2, ["d_v"] if uniform else ["d_s", "d_q", "d_v"]):
            grad_close(a, b, f"K3b per graph K={K} M={M}: {nm} uniform={uniform}", ref32=b32)
            assert_close(a, b2, 1e-5, f"{nm} env vs dst uniform={uniform}", floor=1e-6)


def test_talk_attention_per_graph_kernels_with_parallel_edges():
    """Parallel (duplicate) talk edges: the dense per-graph attention matrix accumulates them, like the edge-wise sum."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.graph import HeteroBatch
    N, off, src, dst, bounds = _ragged_env_talk([5, 8, 3], 0.6, seed=4)
    # duplicate every third edge (stays inside its graph and its destination segment)
    keep = th.arange(src.numel())
    dup = keep[::3]
    idx = th.sort(th.cat([keep, dup]))[0]
    src, dst = src[idx], dst[idx]
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(th.bincount(dst, minlength=N), 0)
    K, M = 16, 64
    g = HeteroBatch.from_arrays(x_a=th.zeros(N, 2), talk_off=off, talk_src=src, graph_off=bounds, device="cuda")
    assert ops._talk_env(g, M, K) is not None
    gen = th.Generator().manual_seed(5)
    s, q, v = (th.randn(N, d, generator=gen).double().requires_grad_(True) for d in (K, K, M))
    w = th.randn(N, M, generator=gen).double()
    e = (s[src.long()] * q[dst]).sum(-1, keepdim=True) / K
    c64 = R.segment_sum(v[src.long()] * R.segment_softmax(e, dst, N), dst, N)
    g64 = th.autograd.grad((c64 * w).sum(), [s, q, v])
    sd, qd, vd = (t.detach().float().cuda().requires_grad_(True) for t in (s, q, v))
    c = ops.talk_attention(sd, qd, vd, g, 1.0 / K)
    assert_close(c, c64, 1e-5, "c")
    got = th.autograd.grad((c * w.float().cuda()).sum(), [sd, qd, vd], retain_graph=True)
    s32, q32, v32 = (t.detach().float().requires_grad_(True) for t in (s, q, v))
    e32 = (s32[src.long()] * q32[dst]).sum(-1, keepdim=True) / K
    c32 = R.segment_sum(v32[src.long()] * R.segment_softmax(e32, dst, N), dst, N)
    g32 = th.autograd.grad((c32 * w.float()).sum(), [s32, q32, v32])
    for a, b, b32, nm in zip(got, g64, g32, ["d_s", "d_q", "d_v"]):
        grad_close(a, b, f"K3b parallel edges: {nm}", ref32=b32)
    # duplicates are summed in CSC order by the lane of the first one (no float atomics): bit-exact run to run
    for _ in range(5):
        c2 = ops.talk_attention(sd, qd, vd, g, 1.0 / K)
        assert th.equal(c2, c)
        for a, b in zip(th.autograd.grad((c2 * w.float().cuda()).sum(), [sd, qd, vd]), got):
            assert th.equal(a, b)


def test_talk_attention_per_graph_kernel_fails_loudly_on_a_wrong_hint():
    """A graph larger than the hinted bound must not be silently mis-computed: its rows come back NaN."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.graph import HeteroBatch
    N, off, src, dst, bounds = _ragged_env_talk([4, 9, 4], 1.0, seed=0)
    g = HeteroBatch.from_arrays(x_a=th.zeros(N, 2), talk_off=off, talk_src=src, graph_off=bounds, device="cuda",
                                hints={"max_graph_agents": 4})
    v = th.randn(N, 8, device="cuda")
    c = ops.talk_attention(None, None, v, g, 1.0)
    assert th.isnan(c[4:13]).all() and th.isfinite(c[:4]).all() and th.isfinite(c[13:]).all()


def test_agent_paths_per_graph_and_per_destination_agree():
    """The whole TarMAC agent (fused step) through both K3b formulations: hints present -> per-graph kernels, hints
    stripped -> per-destination kernels + device-built transpose.  Same loss and gradients."""
    from gpu_util import synth_graph, to_batch, default_init_params, agent_from_params
    cfg = dict(enc="gnn", c="tarmac", n_heads=4, key_size=16, msg_size=64, n_rounds=1, dueling=False, hidden_size=64,
               n_actions=7)
    B, n, M = 48, 8, 20
    g1 = to_batch(synth_graph(B, n, M, dist="env", seed=3, talk="sparse"))
    g2 = g1.fresh()
    g2.hints = {}
    p = default_init_params(cfg, seed=1)
    res = []
    for g in (g1, g2):
        net = agent_from_params(p, cfg)
        h = 0.1 * th.randn(B * n, 64, device="cuda", generator=th.Generator(device="cuda").manual_seed(0))
        h.requires_grad_(True)
        q, h2 = net(g, h)
        loss = (q ** 2).mean() + (h2 ** 2).mean()
        loss.backward()
        res.append((loss.detach(), {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None},
                    h.grad.clone()))
    assert ("talkT" in g2._cache) and ("talkT" not in g1._cache)
    assert_close(res[0][0], res[1][0], 1e-6, "loss")
    assert_close(res[0][2], res[1][2], 1e-5, "d_h", floor=1e-7)
    for k in res[0][1]:
        assert_close(res[0][1][k], res[1][1][k], 1e-5, k, floor=1e-7)


@pytest.mark.parametrize("N,C,S,view", [(32768, 768, 256, None), (32768, 768, 256, (512, 768)), (32768, 96, 256, None),
                                        (32768, 9, 256, None), (1000, 7, 8, None), (77, 300, 4, None),
                                        (4096, 66, 16, (1, 64)), (130, 9, 64, None), (5, 1, 8, None)])
def test_colsum_accumulate_kernel(N, C, S, view):
    """uavgnn_colsum_acc: acc[S, C] += row-blocked column sums; wide (float4 and scalar), narrow and strided layouts,
    ragged last block, repeated accumulation, bit-reproducible."""
    from uav_bs_ctrl_amd import _lib as L
    gen = th.Generator(device="cuda").manual_seed(N + C)
    x = th.randn(N, C, device="cuda", generator=gen)
    xv = x if view is None else x[:, view[0]:view[1]]
    Cv = xv.shape[1]
    outs = []
    for rep in range(2):
        acc = th.zeros(S, Cv, device="cuda")
        for _ in range(3):
            L.check(L.lib().uavgnn_colsum_acc(xv.data_ptr(), xv.stride(0), N, Cv, acc.data_ptr(), S, L.stream()), "colsum")
        outs.append(acc)
    assert th.equal(outs[0], outs[1])
    R = (N + S - 1) // S
    ref = th.zeros(S, Cv, dtype=th.float64)
    xd = xv.double().cpu()
    for s_ in range(S):
        ref[s_] = 3 * xd[s_ * R:(s_ + 1) * R].sum(0)
    assert_close(outs[0], ref, 1e-5, "partials", floor=1e-5)
    assert_close(outs[0].sum(0), 3 * xd.sum(0), 1e-5, "column sums", floor=1e-4)


@pytest.mark.parametrize("D,maxdeg,N", [(64, 7, 4000), (64, 3, 257), (32, 8, 1000), (16, 7, 300), (64, 20, 3000)])
def test_low_degree_k1_kernel_agrees_with_mfma_and_valu(D, maxdeg, N):
    """K1 forward on a two-feature relation: the low-degree kernel (what uavgnn_gatv2_fwd dispatches to when the mean
    in-degree is <= 8) against the MFMA and the VALU kernels of the same library - outputs and saved attention weights;
    in-degrees above 8 exercise its multi-pass online softmax; zero-degree destinations included."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.agents.gnn_agents import GATv2Conv
    gen = th.Generator().manual_seed(D + maxdeg)
    deg = th.randint(0, maxdeg + 1, (N,), generator=gen)
    if maxdeg > 8:                      # keep the mean at or below 8 so that the dispatcher picks the low-degree kernel
        deg[th.rand(N, generator=gen) < 0.5] = 1
    deg[0], deg[1] = maxdeg, 0
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(deg, 0)
    E = int(off[-1])
    assert E <= 8 * N
    x_src = (th.rand(E, 2, generator=gen) * 2 - 1).cuda()
    x_a = th.rand(N, 2, generator=gen).cuda()
    off = off.cuda()
    th.manual_seed(1)
    conv = GATv2Conv((2, 2), D, 4).cuda()
    p = [t.detach().contiguous() for t in (conv.fc_src.weight, conv.fc_src.bias + 0.1, conv.fc_dst.weight,
                                           conv.fc_dst.bias - 0.05, conv.attn, conv.res_fc.weight, conv.res_fc.bias)]
    H = 4 * D
    outs = []
    for fn in (L.lib().uavgnn_gatv2_fwd, L.lib().uavgnn_gatv2_fwd_mfma, L.lib().uavgnn_gatv2_fwd_valu):
        out = th.full((N, H), float("nan"), device="cuda")
        a_save = th.full((max(E, 1), 4), float("nan"), device="cuda")
        rc = fn(x_src.data_ptr(), E, 2, x_a.data_ptr(), 2, off.data_ptr(), None, N, *[t.data_ptr() for t in p], 4, D, 0.2,
                out.data_ptr(), H, a_save.data_ptr(), L.stream())
        assert rc == 0
        outs.append((out, a_save))
    for i, nm in ((1, "mfma"), (2, "valu")):
        assert_close(outs[0][0], outs[i][0], 2e-6, f"low-degree vs {nm}: out")
        assert_close(outs[0][1], outs[i][1], 2e-6, f"low-degree vs {nm}: attention weights", floor=1e-7)
    # inference mode (no attention weights saved) gives the same rows
    out2 = th.empty(N, H, device="cuda")
    rc = L.lib().uavgnn_gatv2_fwd(x_src.data_ptr(), E, 2, x_a.data_ptr(), 2, off.data_ptr(), None, N,
                                  *[t.data_ptr() for t in p], 4, D, 0.2, out2.data_ptr(), H, None, L.stream())
    assert rc == 0 and th.equal(out2, outs[0][0])


@pytest.mark.parametrize("B,n,A,eps", [(4096, 8, 9, 0.05), (3, 5, 4, 1.0), (7, 1, 2, 0.0), (1000, 4, 13, 0.5)])
def test_eps_greedy_selection_kernel(B, n, A, eps):
    """uavgnn_eps_greedy == argmax / one draw per team / uniform random action, on the same uniforms."""
    from uav_bs_ctrl_amd import _lib as L
    gen = th.Generator(device="cuda").manual_seed(B + A)
    N = B * n
    q = th.randn(N, A + 3, device="cuda", generator=gen)[:, :A]           # row stride A + 3
    u = th.rand(B + N, device="cuda", generator=gen)
    acts = th.empty(N, dtype=th.int64, device="cuda")
    L.check(L.lib().uavgnn_eps_greedy(q.data_ptr(), q.stride(0), N, A, n, u.data_ptr(), u.data_ptr() + 4 * B, float(eps),
                                      acts.data_ptr(), L.stream()), "eps_greedy")
    explore = (u[:B] <= eps).repeat_interleave(n)
    rand = (u[B:] * A).long().clamp(max=A - 1)
    ref = th.where(explore, rand, q.argmax(1))
    assert th.equal(acts, ref)
    if eps == 0.0:
        assert th.equal(acts, q.argmax(1))


def test_reference_style_merge_graph_runs_the_same_as_the_vectorised_builder():
    """the graph a reference-style caller assembles - dgl.merge([dgl.batch(per-agent graphs), comm])
    then common.cat - must give the agent the same outputs as ``from_obs_dicts`` (it used to inherit the per-agent
    boundaries of the observation operand and silently turned every message into a self loop)."""
    import numpy as np
    from tests.test_host_logic import _obs, _reference_style_env_graph
    from uav_bs_ctrl_amd import batch, from_obs_dicts
    rng = np.random.default_rng(9)
    n, M = 5, 12
    slow_l, fast_l = [], []
    for _ in range(3):
        obs = _obs(rng, n, M)
        d = rng.uniform(0, 2, (n, n))
        d = (d + d.T) / 2
        np.fill_diagonal(d, 0)
        slow_l.append(_reference_style_env_graph(obs, d, 1.2))
        fast_l.append(from_obs_dicts(obs, d, 1.2))
    slow, fast = batch(slow_l).to("cuda"), batch(fast_l).to("cuda")
    assert th.equal(slow.graph_off, fast.graph_off) and slow.hints["max_graph_agents"] == n
    for c in ("tarmac", "base", "commnet", "econv"):
        cfg = dict(EXP3, c=c, hidden_size=32, msg_size=8, key_size=4)
        net = agent_from_params(default_init_params(cfg, seed=1), cfg)
        h = th.randn(3 * n, 32, generator=th.Generator().manual_seed(0)).cuda()
        with th.no_grad():
            (q1, h1), (q2, h2) = net(slow, h), net(fast, h)
        assert th.equal(q1, q2) and th.equal(h1, h2), c
        # and it is not the degenerate c_v = v_v: the oracle on the same arrays agrees
        g = {k: v for k, v in zip(("talk_off", "talk_src"), (t.cpu() for t in fast.talk_csc()))}
        for et, kx, ko in (("seen", "x_gt", "seen_off"), ("near", "x_ubs", "near_off")):
            x, off = fast.relation_segments(et)
            g[kx], g[ko] = x.cpu().double(), off.cpu()
        g["x_a"] = fast.agent_feat().cpu().double()
        q_ref, _ = R.gnn_agent_forward(g, h.cpu().double(),
                                        {k: v.detach().cpu().double() for k, v in net.state_dict().items()}, cfg)
        assert_close(q1, q_ref, 1e-5, f"merge-built graph, c={c}")


def test_talk_attention_per_graph_kernel_fails_loudly_on_foreign_sources():
    """A graph_off that does not delimit the talk relation (sources outside the destination's graph) gives NaN rows,
    forward and backward - never a silent self loop."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.graph import HeteroBatch
    n = 4
    off = th.arange(0, n * n + 1, n, dtype=th.int32)
    src = th.arange(n, dtype=th.int32).repeat(n)                       # complete graph over 4 agents
    g = HeteroBatch.from_arrays(x_a=th.zeros(n, 2), talk_off=off, talk_src=src,
                                graph_off=th.arange(0, n + 1, dtype=th.int32), device="cuda",
                                hints={"max_graph_agents": 1})       # WRONG: claims 4 one-agent graphs
    s, q, v = (th.randn(n, d).cuda().requires_grad_(True) for d in (16, 16, 64))
    c = ops.talk_attention(s, q, v, g, 1.0 / 16)
    assert bool(th.isnan(c).all())
    (dv,) = th.autograd.grad(c.sum(), [v])
    assert bool(th.isnan(dv).all())


def test_reference_style_data_polyak_reaches_the_fused_target_step():
    """``p_targ.data.mul_/add_`` (learner.py:165-166) on the target net must change what its fused
    no-grad step computes (the stacked projection weight used to be cached on version counters that .data ops skip)."""
    cfg = dict(EXP3, hidden_size=32, msg_size=8, key_size=4)
    p64 = default_init_params(cfg, seed=3)
    pol, tgt = agent_from_params(p64, cfg), agent_from_params(p64, cfg)
    g = to_batch(synth_graph(4, 8, 20, "ragged", seed=1))
    h = th.randn(32, 32, generator=th.Generator().manual_seed(0)).cuda()
    with th.no_grad():
        q0, _ = tgt(g, h)                                               # builds the stacked weight
        for p in pol.parameters():
            p.mul_(1.5)
    for p, p_targ in zip(pol.parameters(), tgt.parameters()):
        p_targ.data.mul_(0.5)
        p_targ.data.add_((1 - 0.5) * p.data)
    with th.no_grad():
        q1, _ = tgt(g, h)
    p_new = {k: v.detach().cpu().double() for k, v in tgt.state_dict().items()}
    gd = synth_graph(4, 8, 20, "ragged", seed=1)
    q_ref, _ = R.gnn_agent_forward({k: (v.double() if v.is_floating_point() else v) for k, v in gd.items()
                                    if k != "graph_off"}, h.cpu().double(), p_new, cfg)
    assert_close(q1, q_ref, 1e-5, "target net after .data polyak")
    assert float((q1 - q0).abs().max()) > 1e-3


def test_qmix_learner_update_reproduces_reference_update():
    """Row f4 on the GPU: learner.update with mixer=True (HIP agent + QMixer + target mixer; clip on the agent only,
    learner.py:145-148,:159) against the state the REFERENCE learner reached from the same parameters / batch
    (tests/golden/learner_update_qmix.npz, captured from algos/madrqn/learner.py + mixers.py)."""
    from tests.test_replay_mixer import _qmix_learner
    L, batch, cfg, z = _qmix_learner("cuda", th.float32)
    out = L.update(batch)
    assert_close(out["LossQ"], th.as_tensor(z["loss"]).double(), 1e-5, "QMIX LossQ")
    # what float32 arithmetic itself achieves: the same learner on the CPU with the oracle as its agent
    import uav_bs_ctrl_amd.learner as LM
    from tests.test_dp_gloo import OracleAgent
    saved = LM.agent_REGISTRY
    LM.agent_REGISTRY = {"gnn": OracleAgent}
    try:
        Lc, bc, _, _ = _qmix_learner("cpu", th.float32)
        Lc.grads.zero_()
        Lc.loss(bc)[0].backward()
        g32 = {("policy", k.removeprefix("inner.")): p_.grad.clone().clamp(-1, 1) for k, p_ in Lc.policy_net.named_parameters()}
        g32.update({("mixer", k): p_.grad.clone() for k, p_ in Lc.mixer.named_parameters()})
    finally:
        LM.agent_REGISTRY = saved
    for tag, mod, tmod in (("policy", L.policy_net, L.target_net), ("mixer", L.mixer, L.target_mixer)):
        for k, prm in mod.named_parameters():
            g_ref = th.as_tensor(z[f"grad:{tag}:{k}"])
            grad_close(prm.grad, g_ref, f"QMIX update: {tag} grad {k}", ref32=g32[(tag, k)], floor=GRAD_FLOOR)
            sure = g_ref.abs() > 1e-4          # Adam's first step is lr * sign-like(g): only where g is above noise
            after = th.as_tensor(z[f"after:{tag}:{k}"])
            assert float(((prm.detach().cpu().double() - after).abs() * sure).max()) < 2e-6, f"{tag} param {k}"
        for k, prm in tmod.named_parameters():
            # where the gradient is rounding noise (e.g. f_sign.bias: analytically zero) Adam moves the policy parameter
            # by +-lr whatever the sign of the noise, and polyak carries (1 - polyak) of that into the target
            sure = th.as_tensor(z[f"grad:{tag}:{k}"]).abs() > 1e-4
            diff = (prm.detach().cpu().double() - th.as_tensor(z[f"target_after:{tag}:{k}"])).abs()
            assert float((diff * sure).max()) < 1e-6 and float(diff.max()) < 2.1 * cfg["lr"] * (1 - cfg["polyak"]) + 1e-6, k
    # the mixer's gradients are NOT clipped (learner.py:159 clips policy_net only), the agent's are
    assert float(max(p.grad.abs().max() for p in L.policy_net.parameters())) <= 1.0


def _nccl_ws1_worker(port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from uav_bs_ctrl_amd import HeteroBatch
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    th.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=th.device("cuda", 0))
    try:
        import types
        batch, p, cfg, z = load_learner_golden(dtype=th.float32)
        args = types.SimpleNamespace(device="cuda", hidden_size=32, c="tarmac", n_heads=4, n_layers=2, msg_size=8,
                                     key_size=4, n_rounds=1, dueling=False, mixer=False, double_q=True, lr=cfg["lr"],
                                     gamma=cfg["gamma"], polyak=cfg["polyak"], max_seq_len=cfg["T"], seed=0)
        env_info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=cfg["n_actions"], n_agents=cfg["n_agents"],
                        episode_limit=10)
        dev = th.device("cuda")
        b = dict(obs=[HeteroBatch.from_arrays(**g).to(dev) for g in batch["obs"]], h0=batch["h0"].to(dev),
                 h1=batch["h1"].to(dev), acts=batch["acts"].to(dev), rews=batch["rews"].to(dev),
                 dones=batch["dones"].to(dev))
        res = []
        for group in ("none", "world"):
            L = MultiAgentQLearner(env_info, args, process_group=None)
            L.policy_net.load_state_dict(p)
            L.target_net.load_state_dict(p)
            if group == "none":     # reference arm: the collective path switched off entirely
                L.grads.all_reduce_mean_ = lambda g=None: None
            else:                   # the real thing: broadcast + RCCL all-reduce on the flat buffer, forced at world size 1
                from uav_bs_ctrl_amd import learner as LM
                LM.broadcast_parameters(L.policy_net, 0, None, force=True)
                L.grads.force_collective = True
            out = L.update(b)
            th.cuda.synchronize()
            res.append((float(out["LossQ"]), th.cat([p_.detach().reshape(-1) for p_ in L.policy_net.parameters()]).cpu(),
                        L.grads.flat.detach().cpu().clone()))
        q.put(("ok", res[0][0] == res[1][0], bool(th.equal(res[0][1], res[1][1])), bool(th.equal(res[0][2], res[1][2])),
               float(z["loss"]), res[1][0]))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put(("err", traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_rccl_path_at_world_size_one_equals_the_non_distributed_step():
    """the nccl (= RCCL) branch has never run on hardware.  One process, world size 1: start-up
    broadcast of the flat parameter copy + all-reduce of the flat gradient buffer through RCCL around a real HIP-agent
    update must leave loss, gradients and parameters BIT-identical to the update with the collective switched off."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=_nccl_ws1_worker, args=(port, q))
    pr.start()
    try:
        res = wait_worker(pr, q, timeout=480)
    finally:
        pr.join(timeout=60)
        if pr.is_alive():
            pr.kill()
    assert res[0] == "ok", res[1]
    _, same_loss, same_params, same_grads, loss_ref, loss = res
    assert same_loss and same_params and same_grads
    assert abs(loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))


def _nccl_graphed_worker(port, q):
    """world size 1 over RCCL: GraphedUpdate must cut the capture at the collective (two graphs + an eager all-reduce of the
    flat gradient buffer between their replays) and leave the same parameters as eager non-distributed updates."""
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    th.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=th.device("cuda", 0))
    try:
        from uav_bs_ctrl_amd import batch as hb_batch
        from uav_bs_ctrl_amd.graphs import GraphedUpdate
        from uav_bs_ctrl_amd.replay import SequenceReplay
        dev, (E, n, M, T, Bs) = th.device("cuda"), (12, 4, 30, 4, 6)
        L1, L2 = _graph_learner(n, T, seed=1), _graph_learner(n, T, seed=1)
        L2.grads.force_collective = True
        assert L2.needs_collective() and not L1.needs_collective()
        rb = SequenceReplay(capacity=E, max_seq_len=T, n_agents=n, n_gts=M, hidden_size=256, n_envs=E, state_dim=0,
                            r_comm=0.9, device=dev)
        gen = th.Generator(device=dev).manual_seed(7)

        def obs():
            gt, ub, ag, d = _padded_obs(gen, (E,), n, M, dev)
            return dict(gt=gt, ubs=ub, agent=ag, d_u2u=d, h=0.1 * th.randn(E, n, 256, device=dev, generator=gen),
                        state=th.zeros(E, 0, device=dev))
        cur = obs()
        for t in range(T):
            nxt = obs()
            tr = dict(cur, act=th.randint(9, (E, n), device=dev, generator=gen), rew=th.rand(E, n, device=dev, generator=gen),
                      done=(th.rand(E, 1, device=dev, generator=gen) < 0.2).float())
            tr.update({"next_" + k: v for k, v in nxt.items()})
            rb.push(tr)
            cur = nxt
        gu = GraphedUpdate(L2, Bs, T, n, M, r_comm=0.9)
        split = bool(gu.split)
        losses = []
        for it in range(2):
            idx = rb.sample_indices(Bs, gen)
            b = rb.gather(idx)
            b["obs_all"] = hb_batch(b["obs"])
            out_e = L1.update(b)
            out_g = gu({k: v.index_select(0, idx) for k, v in rb.mem.items()})
            losses.append((float(out_e["LossQ"]), float(out_g["LossQ"])))
        th.cuda.synchronize()
        scale = float(L1.flat.flat.abs().max())
        q.put(("ok", split, losses, float((L1.flat.flat - L2.flat.flat).abs().max()) / scale,
               float((L1.flat_target - L2.flat_target).abs().max()) / scale, float(L2.optimizer.hyper[1])))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put(("err", traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_graphed_update_is_cut_at_the_rccl_collective_and_equals_eager_updates():
    """the hipGraph-captured update with the gradient all-reduce in the loop.  The all-reduce is NOT
    captured: the update is two graphs (accumulate / apply) around an eager RCCL all-reduce of the flat buffer."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=_nccl_graphed_worker, args=(port, q))
    pr.start()
    try:
        res = wait_worker(pr, q, timeout=480)
    finally:
        pr.join(timeout=60)
        if pr.is_alive():
            pr.kill()
    assert res[0] == "ok", res[1]
    _, split, losses, d_pol, d_tgt, steps = res
    assert split, "the capture was not cut at the collective"
    for le, lg in losses:
        assert abs(le - lg) <= 1e-5 * max(1.0, abs(le)), (le, lg)
    assert d_pol <= 1e-5 and d_tgt <= 1e-5 and steps == 2.0, (d_pol, d_tgt, steps)


def test_bench_step_under_force_dist_equals_the_plain_run():
    """bench.py's own step() (rollout forwards + update on the HIP agent) launched the way the driver launches a rank -
    torch.distributed.run, RCCL initialised, the flat gradient buffer pushed through the all-reduce at world size 1 - must
    leave the SAME parameter checksum and loss as the plain single-process run."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    small = ["--gpus", "1", "--steps", "2", "--warmup", "0", "--B", "32", "--T", "4", "--no-cpu-baseline", "--no-end-to-end",
             "--no-fp32-leg", "--no-rho-leg"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    plain = subprocess.run([sys.executable, "bench.py", *small], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-2000:]
    distd = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                            "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", *small, "--force-dist"],
                           cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert distd.returncode == 0, distd.stderr[-2000:]
    a = json.loads(plain.stdout.strip().splitlines()[-1])
    b = json.loads(distd.stdout.strip().splitlines()[-1])
    assert a["params_checksum"] == b["params_checksum"], (a["params_checksum"], b["params_checksum"])
    assert a["loss"] == b["loss"] and b["n_gpus"] == 1


@pytest.mark.parametrize("B,n,M,dist,seed", [(16, 8, 80, "dense", 0), (64, 8, 80, "env", 1), (9, 5, 40, "ragged", 2),
                                             (7, 16, 30, "ragged", 3), (1, 1, 12, "ragged", 4), (33, 3, 100, "env", 5),
                                             (5, 20, 10, "ragged", 6), (4400, 8, 12, "env", 7), (2, 3, 600, "dense", 8)])
def test_fused_hetero_k1_equals_per_relation_kernels(B, n, M, dist, seed):
    """gatv2_hetero.hip (both relations, one launch; `near` on blocks of 16 destinations, one score tile per edge slot with
    [x_u ; x_v] in the contraction) against the per-relation kernels on the same inputs: outputs, saved attention weights and
    - through them - the parameter gradients.  Covers N that is not a multiple of 16 (masked rows of the last block), near
    degrees above 8 and above 16 (n = 16 / 20: two / three passes through the online softmax, raw scores re-normalised in
    place), isolated `near` destinations, destinations isolated in `seen` with / without a hand-out order, and - 35 200
    destinations = 2 200 blocks for 2 048 wavefronts - the several-blocks-per-wavefront path of the time-batched launches
    (next block's inputs prefetched, opposite part order on the two wavefronts of a SIMD); 600 `seen` in-edges per destination =
    38 row tiles: more raw scores than the wavefront's LDS row buffer parks (33 tiles), the rest go through a_save itself."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.agents.gnn_agents import GraphObservationEncoder
    import types
    g = synth_graph(B, n, M, dist, seed=seed)
    N = B * n
    if n > 2:      # make some `near` destinations isolated / low-degree: drop a random subset of near edges
        gen = th.Generator().manual_seed(seed)
        keep = th.rand(g["x_ubs"].shape[0], generator=gen) < 0.8
        keep[: n - 1] = False                                 # destination 0 keeps nothing
        deg = th.zeros(N, dtype=th.int64).index_add_(0, th.repeat_interleave(th.arange(N), n - 1), keep.long())
        g["x_ubs"] = g["x_ubs"][keep]
        g["near_off"] = th.cat([th.zeros(1, dtype=th.int64), th.cumsum(deg, 0)]).to(th.int32)
    th.manual_seed(seed)
    enc = GraphObservationEncoder(dict(agent=2, ubs=2, gt=4), types.SimpleNamespace(n_heads=4, hidden_size=256)).cuda()
    with th.no_grad():
        for p in enc.parameters():
            if p.dim() == 1:
                p.add_(0.05 * th.randn_like(p))
    w = th.randn(N, 256, generator=th.Generator().manual_seed(7)).cuda()
    res = {}
    for fused in (True, False):
        ops.HETERO_FUSED = fused
        try:
            hb = to_batch(g)
            enc.zero_grad(set_to_none=True)
            ops.KERNEL_TIMER.reset(enabled=True)
            x = enc(hb)
            names = set(ops.KERNEL_TIMER.summary())
            ops.KERNEL_TIMER.enabled = False
            assert ("gatv2_hetero_fwd" in names) == fused, names
            (x * w).sum().backward()
            with th.no_grad():
                xi = enc(to_batch(g))                          # inference launch (no attention saving)
            res[fused] = (x.detach(), xi, {k: p.grad.clone() for k, p in enc.named_parameters()})
        finally:
            ops.HETERO_FUSED = True
    (xf, xif, gf), (xp, xip, gp) = res[True], res[False]
    assert th.equal(xf, xif) and th.equal(xp, xip)
    assert_close(xf, xp, 2e-6, "fused vs per-relation encoder output")
    for k in gf:
        assert_close(gf[k], gp[k], 2e-5, f"grad {k} through fused-forward attention weights", floor=1e-6)


def test_fused_hetero_k1_bf16_score_gemm_equals_the_fp32_mfma_build(monkeypatch):
    """The score GEMM of the fused K1 forward on the bf16 matrix cores (exact three-way operand splits, six products per fp32
    product; phase N with the channel bias in the free K slots) against the fp32-MFMA build of the same kernel
    (csrc/gatv2_hetero_f32.hip, phases bit 8): output rows and saved attention weights to fp32 rounding, on dense, env and
    ragged degree distributions - and the fp32 build really is a different kernel."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.agents.gnn_agents import GraphObservationEncoder
    import types
    th.manual_seed(3)
    enc = GraphObservationEncoder(dict(agent=2, ubs=2, gt=4), types.SimpleNamespace(n_heads=4, hidden_size=256)).cuda()
    with th.no_grad():
        for c in enc.f_conv.values():
            for b in (c.fc_src.bias, c.fc_dst.bias, c.res_fc.bias):
                b.normal_(0, 0.1)
    for dist_name, B, n, M in (("dense", 64, 8, 80), ("env", 256, 8, 80), ("ragged", 33, 5, 200)):
        hb = to_batch(synth_graph(B, n, M, dist_name, seed=B))
        rels = [(*hb.relation_segments(et), hb.relation_order(et), enc.f_conv[et]) for et in ("seen", "near")]
        outs = []
        for flag in (True, False):
            monkeypatch.setattr(ops, "K1_BF16Z", flag)
            with th.no_grad():
                outs.append(ops.hetero_gatv2(hb.agent_feat(), 4, rels))
        assert not th.equal(outs[0], outs[1]), "both arms ran the same kernel"
        assert_close(outs[0], outs[1], 2e-6, f"{dist_name}: bf16x3 score GEMM vs fp32 MFMA")
        xa = hb.agent_feat().clone().requires_grad_(False)
        monkeypatch.setattr(ops, "K1_BF16Z", True)
        o1 = ops.hetero_gatv2(xa, 4, rels)
        g1 = th.autograd.grad(o1.square().sum(), [enc.f_conv["seen"].fc_src.weight, enc.f_conv["near"].attn])
        monkeypatch.setattr(ops, "K1_BF16Z", False)
        o2 = ops.hetero_gatv2(xa, 4, rels)
        g2 = th.autograd.grad(o2.square().sum(), [enc.f_conv["seen"].fc_src.weight, enc.f_conv["near"].attn])
        for a, b in zip(g1, g2):
            assert_close(a, b, 1e-5, f"{dist_name}: gradients through the saved attention weights")


def test_fused_hetero_k1_raw_rows_vs_oracle(monkeypatch):
    """The [N, 2H] row block of the fused launch against the float64 oracle, relation by relation (before f_aggr)."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.agents.gnn_agents import GATv2Conv
    g = synth_graph(40, 8, 80, "ragged", seed=11)
    hb = to_batch(g)
    th.manual_seed(3)
    convs = [GATv2Conv((4, 2), 64, 4).cuda(), GATv2Conv((2, 2), 64, 4).cuda()]
    with th.no_grad():
        for c in convs:
            for p in c.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * th.randn_like(p))
    rels = []
    for et, c in zip(("seen", "near"), convs):
        xs, off = hb.relation_segments(et)
        rels.append((xs, off, hb.relation_order(et), c))
    with th.no_grad():
        out = ops.hetero_gatv2(hb.agent_feat(), 4, rels)
        monkeypatch.setattr(ops, "K1_BF16Z", False)
        out_f32 = ops.hetero_gatv2(hb.agent_feat(), 4, rels)       # the fp32-MFMA build of the same kernel
    errs = {}
    for i, (et, kx, ko, c) in enumerate((("seen", "x_gt", "seen_off", convs[0]), ("near", "x_ubs", "near_off", convs[1]))):
        p64 = {k: v.detach().cpu().double() for k, v in c.state_dict().items()}
        ref = R.gatv2_conv_seg(g[kx].double(), g["x_a"].double(), g[ko], p64, 4).reshape(320, -1)
        assert_close(out[:, 256 * i:256 * (i + 1)], ref, 1e-5, f"fused rows, relation {et}")
        assert_close(out_f32[:, 256 * i:256 * (i + 1)], ref, 1e-5, f"fused rows (fp32-MFMA build), relation {et}")
        scale = float(ref.abs().max())
        errs[et] = (float((out[:, 256 * i:256 * (i + 1)].cpu().double() - ref).abs().max()) / scale,
                    float((out_f32[:, 256 * i:256 * (i + 1)].cpu().double() - ref).abs().max()) / scale)
    # "fp32 accuracy" of the bf16-matrix-core score GEMM, measured: its error against float64 is of the size of the fp32-MFMA
    # build's on the same data (both ~1e-7 of max|row|)
    for et, (e_bf16, e_f32) in errs.items():
        assert e_bf16 <= 2.0 * e_f32 + 2e-7, (et, e_bf16, e_f32)


def test_fused_adamw_clip_polyak_kernel_matches_torch_and_checkpoints_interchange():
    """uavgnn_adamw_polyak over flat buffers == clip_grad_value_ + torch.optim.AdamW.step + the polyak loop of
    learner.py:157-166, over several steps with a changing learning rate (LambdaLR), odd parameter sizes (each padded to four floats
    by FlatParams, so the kernel's scalar tail is NOT reached from here: tests/test_grid_caps_gpu.py runs it through the C ABI) and a
    clip boundary inside the buffer; FusedAdamW's state_dict loads into torch.optim.AdamW and vice versa."""
    import torch.nn as nn
    from uav_bs_ctrl_amd.learner import FlatGradBuffer
    from uav_bs_ctrl_amd.optim import FlatParams, FusedAdamW

    def make():
        th.manual_seed(5)
        a = nn.Sequential(nn.Linear(7, 13), nn.Linear(13, 3)).cuda()       # odd sizes: 91+13+39+3
        b = nn.Linear(5, 9).cuda()                                          # "mixer": not clipped
        return a, b
    (pa, pb), (ta, tb), (ra, rb), (rta, rtb) = make(), make(), make(), make()
    fp = FlatParams([pa, pb])
    tflat = fp.mirror([ta, tb])
    grads = FlatGradBuffer(fp.params, fp.index_of, fp.numel)
    opt = FusedAdamW(fp, grads.flat, lr=3e-3, clip=0.05, n_clip=fp.span(1), target_flat=tflat, polyak=0.9)
    sched = th.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: max(0.4, 1 - e / 4))
    rparams = list(ra.parameters()) + list(rb.parameters())
    ropt = th.optim.AdamW(rparams, lr=3e-3)
    rsched = th.optim.lr_scheduler.LambdaLR(ropt, lr_lambda=lambda e: max(0.4, 1 - e / 4))
    gen = th.Generator(device="cuda").manual_seed(1)
    for it in range(6):
        gs = [0.2 * th.randn(p.shape, device="cuda", generator=gen) for p in rparams]
        grads.zero_()
        for p, g_ in zip(fp.params, gs):
            p.grad.copy_(g_)
        for p, g_ in zip(rparams, gs):
            p.grad = g_.clone()
        opt.step()
        nn.utils.clip_grad_value_(ra.parameters(), 0.05)
        ropt.step()
        with th.no_grad():
            for p, pt in zip(rparams, list(rta.parameters()) + list(rtb.parameters())):
                pt.data.mul_(0.9)
                pt.data.add_((1 - 0.9) * p.data)
        sched.step(), rsched.step()
        for p, q in zip(fp.params, rparams):
            assert_close(p, q, 2e-6, f"param after step {it}", floor=1e-7)
            assert_close(p.grad, q.grad, 1e-7, "clipped gradient written back")
        for p, q in zip(list(ta.parameters()) + list(tb.parameters()), list(rta.parameters()) + list(rtb.parameters())):
            assert_close(p, q, 2e-6, f"target after step {it}", floor=1e-7)
    assert fp.intact() and abs(opt.param_groups[0]["lr"] - ropt.param_groups[0]["lr"]) < 1e-12
    # checkpoints: fused -> torch and torch -> fused continue identically
    import copy
    sd_f, sd_r = copy.deepcopy(opt.state_dict()), copy.deepcopy(ropt.state_dict())   # what torch.save / load would hand over
    assert set(sd_f["state"][0]) == set(sd_r["state"][0]) and float(sd_f["state"][0]["step"]) == 6.0
    ropt2 = th.optim.AdamW(rparams, lr=1.0)
    ropt2.load_state_dict(sd_f)
    opt.load_state_dict(sd_r)
    gs = [0.2 * th.randn(p.shape, device="cuda", generator=gen) for p in rparams]
    grads.zero_()
    for p, g_ in zip(fp.params, gs):
        p.grad.copy_(g_)
    for p, g_ in zip(rparams, gs):
        p.grad = g_.clone()
    opt.step()
    nn.utils.clip_grad_value_(ra.parameters(), 0.05)
    ropt2.step()
    for p, q in zip(fp.params, rparams):
        assert_close(p, q, 2e-6, "param after checkpoint interchange", floor=1e-7)


def _padded_obs(gen, lead, n, M, dev):
    gt = th.rand(*lead, n, M, 5, device=dev, generator=gen) * 2 - 1
    gt[..., 0] = (th.rand(*lead, n, M, device=dev, generator=gen) < 0.3).float()
    ub = th.rand(*lead, n, n - 1, 3, device=dev, generator=gen) * 2 - 1
    ub[..., 0] = (th.rand(*lead, n, n - 1, device=dev, generator=gen) < 0.6).float()
    d = th.rand(*lead, n, n, device=dev, generator=gen) * 2
    d = (d + d.transpose(-1, -2)) / 2 * (1 - th.eye(n, device=dev))
    return gt, ub, th.rand(*lead, n, 2, device=dev, generator=gen), d


def _graph_learner(n, T, seed=0):
    import types
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    args = types.SimpleNamespace(device="cuda", hidden_size=256, c="tarmac", n_heads=4, n_layers=1, msg_size=64, key_size=16,
                                 n_rounds=1, dueling=False, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.99,
                                 max_seq_len=T, seed=0)
    th.manual_seed(seed)
    return MultiAgentQLearner(dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=9, n_agents=n, episode_limit=T), args)


def test_graphed_act_replays_the_eager_rollout_step():
    """hipGraph capture of learner.act (device graph builder in static mode + no-grad policy forward + selection with the
    exploration rate in device memory): replays on NEW observations equal the eager step on the same observations."""
    from uav_bs_ctrl_amd import from_padded_obs
    from uav_bs_ctrl_amd.graphs import GraphedAct
    dev, (B, n, M) = th.device("cuda"), (3, 8, 50)
    L = _graph_learner(n, 5)
    ga = GraphedAct(L, B, n, M, r_comm=1.2)
    gen = th.Generator(device=dev).manual_seed(4)
    h = 0.1 * th.randn(B * n, 256, device=dev, generator=gen)
    for it in range(3):
        gt, ub, ag, d = _padded_obs(gen, (B,), n, M, dev)
        acts, h2 = ga(gt, ub, ag, d, h, 0.0)
        g = from_padded_obs(gt, ub, ag, d, 1.2)
        acts_e, h2_e = L.act(g, h, 0.0)
        assert th.equal(acts, acts_e), it
        assert_close(h2, h2_e, 1e-6, f"h' replay {it}")
        h = h2.clone()
    acts_r, _ = ga(gt, ub, ag, d, h, 1.0)                       # everyone explores: uniform random actions
    a1 = acts_r.clone()
    acts_r, _ = ga(gt, ub, ag, d, h, 1.0)
    assert int(a1.min()) >= 0 and int(a1.max()) < 9 and not th.equal(a1, acts_r)   # fresh randomness every replay


def test_graphed_act_at_4096_agents_captures_the_matrix_core_kernels():
    """The same capture at a batch where the bf16x3 GRU cell and GEMM are in use (512 envs x 8 agents: weight-split launches,
    512-thread workgroups with 120-148 KB of LDS, per-call plane buffers from the graph's pool): the replay equals the eager
    step and repeats bit for bit."""
    from uav_bs_ctrl_amd import from_padded_obs, ops
    from uav_bs_ctrl_amd.graphs import GraphedAct
    dev, (B, n, M) = th.device("cuda"), (512, 8, 50)
    L = _graph_learner(n, 6)
    ga = GraphedAct(L, B, n, M, r_comm=1.2)
    gen = th.Generator(device=dev).manual_seed(5)
    h = 0.1 * th.randn(B * n, 256, device=dev, generator=gen)
    gt, ub, ag, d = _padded_obs(gen, (B,), n, M, dev)
    assert ops.gru_cell_supported(th.empty(B * n, 320, device=dev), h) and ops.gemm_x3_supported(th.empty(B * n, 512, device=dev), 256, 512)
    acts, h2 = ga(gt, ub, ag, d, h, 0.0)
    acts, h2 = acts.clone(), h2.clone()
    acts_e, h2_e = L.act(from_padded_obs(gt, ub, ag, d, 1.2), h, 0.0)
    assert_close(h2, h2_e, 1e-6, "h' replay vs eager")
    assert float((acts != acts_e).float().mean()) < 1e-3          # argmax ties at the 1e-7 level aside
    acts_r, h2_r = ga(gt, ub, ag, d, h, 0.0)
    assert th.equal(acts_r, acts) and th.equal(h2_r, h2)


def test_graphed_update_replays_the_eager_update():
    """hipGraph capture of the WHOLE update (device graph builder for all T+1 steps, time-batched encoder, 2T+1
    forwards, BPTT backward, clip + AdamW + polyak in one launch): two replays on two sampled batches leave the same
    loss, policy and target parameters as two eager updates of an identical learner on the same batches."""
    from uav_bs_ctrl_amd import batch as hb_batch
    from uav_bs_ctrl_amd.graphs import GraphedUpdate
    from uav_bs_ctrl_amd.replay import SequenceReplay
    dev, (E, n, M, T, Bs) = th.device("cuda"), (12, 4, 30, 4, 6)
    L1, L2 = _graph_learner(n, T, seed=1), _graph_learner(n, T, seed=1)
    assert th.equal(L1.flat.flat, L2.flat.flat)
    rb = SequenceReplay(capacity=E, max_seq_len=T, n_agents=n, n_gts=M, hidden_size=256, n_envs=E, state_dim=0,
                        r_comm=0.9, device=dev)
    gen = th.Generator(device=dev).manual_seed(7)

    def obs():
        gt, ub, ag, d = _padded_obs(gen, (E,), n, M, dev)
        return dict(gt=gt, ubs=ub, agent=ag, d_u2u=d, h=0.1 * th.randn(E, n, 256, device=dev, generator=gen),
                    state=th.zeros(E, 0, device=dev))
    cur = obs()
    for t in range(T):
        nxt = obs()
        tr = dict(cur, act=th.randint(9, (E, n), device=dev, generator=gen), rew=th.rand(E, n, device=dev, generator=gen),
                  done=(th.rand(E, 1, device=dev, generator=gen) < 0.2).float())
        tr.update({"next_" + k: v for k, v in nxt.items()})
        rb.push(tr)
        cur = nxt
    gu = GraphedUpdate(L2, Bs, T, n, M, r_comm=0.9)
    assert th.equal(L1.flat.flat, L2.flat.flat) and float(L2.optimizer.hyper[1]) == 0.0   # capture left no trace
    for it in range(2):
        idx = rb.sample_indices(Bs, gen)
        b = rb.gather(idx)
        b["obs_all"] = hb_batch(b["obs"])
        out_e = L1.update(b)
        out_g = gu({k: v.index_select(0, idx) for k, v in rb.mem.items()})
        assert_close(out_g["LossQ"], out_e["LossQ"], 1e-5, f"loss, replay {it}")
    assert_close(L2.flat.flat, L1.flat.flat, 1e-5, "policy parameters after two replays", floor=1e-7)
    assert_close(L2.flat_target, L1.flat_target, 1e-5, "target parameters after two replays", floor=1e-7)
    assert float(L2.optimizer.hyper[1]) == 2.0


@pytest.mark.parametrize("N,maxdeg,seed", [(4096, 7, 0), (257, 8, 1), (33, 3, 2), (1000, 20, 3), (2, 0, 4), (501, 1, 5)])
def test_low_degree_k1_backward_pair_kernel_agrees_with_generic(N, maxdeg, seed):
    """gatv2_bwd_pair_kernel (two destinations per wavefront, lane = (head, destination half, edge slot) / lane <-> four
    channels) against the generic one-destination-per-wavefront backward on the same inputs: every parameter gradient.
    Odd N, isolated destinations, degrees above 8 (several passes), all-isolated input; and bit-exact repeatability."""
    from uav_bs_ctrl_amd import _lib as L
    gen = th.Generator().manual_seed(seed)
    deg = th.randint(0, maxdeg + 1, (N,), generator=gen)
    if N > 8:
        deg[3] = 0
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(deg, 0)
    E = int(off[-1])
    dev = "cuda"
    x_src = (th.rand(max(E, 1), 2, generator=gen) * 2 - 1).to(dev)
    x_dst = th.rand(N, 2, generator=gen).to(dev)
    H = 256
    prm = [(0.5 * th.randn(s, generator=gen)).to(dev) for s in ((H, 2), (H,), (H, 2), (H,), (H,), (H, 2), (H,))]
    W_s, b_s, W_d, b_d, attn, W_r, b_r = prm
    out = th.empty(N, 512, device=dev)
    a_save = th.empty(max(E, 1), 4, device=dev)
    lib, st, offd = L.lib(), L.stream(), off.to(dev)
    rc = lib.uavgnn_gatv2_fwd(x_src.data_ptr(), E, 2, x_dst.data_ptr(), 2, offd.data_ptr(), None, N, *[t.data_ptr() for t in prm],
                              4, 64, 0.2, out.data_ptr() + 1024, 512, a_save.data_ptr(), st)
    assert rc == 0
    d_out = th.randn(N, 512, generator=gen).to(dev)
    wsb = lib.uavgnn_gatv2_bwd_workspace_bytes(2, H)
    ws = th.empty(wsb // 4, device=dev)

    def run(fn):
        g = [th.full_like(t, float("nan")) for t in prm]
        rc = fn(x_src.data_ptr(), E, 2, x_dst.data_ptr(), 2, offd.data_ptr(), None, N, *[t.data_ptr() for t in prm[:5]], 4, 64, 0.2,
                out.data_ptr() + 1024, d_out.data_ptr() + 1024, 512, a_save.data_ptr(), *[t.data_ptr() for t in g],
                ws.data_ptr(), wsb, st)
        assert rc == 0, rc
        th.cuda.synchronize()
        return g
    g_pair, g_gen, g_pair2 = run(lib.uavgnn_gatv2_bwd), run(lib.uavgnn_gatv2_bwd_generic), run(lib.uavgnn_gatv2_bwd)
    for a, b, c, nm in zip(g_pair, g_gen, g_pair2, ["dW_s", "db_s", "dW_d", "db_d", "dattn", "dW_r", "db_r"]):
        assert th.equal(a, c), f"{nm}: pair kernel not bit-reproducible"
        assert_close(a, b, 2e-5, f"{nm}: pair vs generic", floor=1e-5 * max(1.0, float(N) ** 0.5 * 1e-2))


@pytest.mark.parametrize("N,lo,hi,seed,order", [(4096, 64, 64, 0, False), (8192, 100, 128, 1, False), (6001, 0, 140, 2, True),
                                                (32768, 20, 60, 3, False), (300, 16, 16, 4, True)])
def test_dense_k1_backward_on_the_matrix_cores_agrees_with_generic_and_is_bit_reproducible(N, lo, hi, seed, order):
    """The matrix-core K1 backward (csrc/gatv2_bwd_mfma.hip: destinations with 16 .. 128 in-edges take the per-(edge, channel)
    sums through bf16x3 MFMAs, the others a second launch of the packed-FMA kernel) against the generic backward on the same
    inputs, every parameter gradient, and bit-exact repeatability over ten launches.  Sizes put several destinations on
    every wavefront and two workgroups on every CU - the regime in which the first build of this kernel was irreproducible
    (a compiler-packed v_pk_fma_f32 with an operand select next to bf16 MFMAs: tools/ubench/mfma_pk_hazard.hip).
    The two kernels evaluate z = W_s x + c in different arithmetic (fp32 FMA chain / exact bf16 triple products), so the sign
    of a z within rounding of zero can differ: about one (edge, channel) pair in 3e7, each moving one gradient element by
    2 |de|.  Hence the rule: everything within 2e-5 of max|ref|, except at most 8 elements per tensor within 1e-3."""
    from uav_bs_ctrl_amd import _lib as L
    gen = th.Generator().manual_seed(seed)
    deg = th.randint(lo, hi + 1, (N,), generator=gen)
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(deg, 0)
    E = int(off[-1])
    assert E >= 16 * N, "the matrix-core path is chosen for a mean in-degree of 16 or more"
    dev = "cuda"
    x_src = (th.rand(E, 4, generator=gen) * 2 - 1).to(dev)
    x_dst = th.rand(N, 2, generator=gen).to(dev)
    H = 256
    prm = [(0.5 * th.randn(s, generator=gen)).to(dev) for s in ((H, 4), (H,), (H, 2), (H,), (H,), (H, 2), (H,))]
    out = th.empty(N, 512, device=dev)
    a_save = th.empty(E, 4, device=dev)
    lib, st, offd = L.lib(), L.stream(), off.to(dev)
    perm = th.argsort(deg, descending=True, stable=True).to(th.int32).to(dev) if order else None
    pp = perm.data_ptr() if order else None
    rc = lib.uavgnn_gatv2_fwd(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), pp, N, *[t.data_ptr() for t in prm],
                              4, 64, 0.2, out.data_ptr(), 512, a_save.data_ptr(), st)
    assert rc == 0
    d_out = th.randn(N, 512, generator=gen).to(dev)
    wsb = lib.uavgnn_gatv2_bwd_workspace_bytes(4, H)
    ws = th.empty(wsb // 4, device=dev)

    def run(fn):
        g = [th.full_like(t, float("nan")) for t in prm]
        rc = fn(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), pp, N, *[t.data_ptr() for t in prm[:5]], 4, 64, 0.2,
                out.data_ptr(), d_out.data_ptr(), 512, a_save.data_ptr(), *[t.data_ptr() for t in g], ws.data_ptr(), wsb, st)
        assert rc == 0, rc
        th.cuda.synchronize()
        return g
    g_mf, g_gen = run(lib.uavgnn_gatv2_bwd), run(lib.uavgnn_gatv2_bwd_generic)
    names = ["dW_s", "db_s", "dW_d", "db_d", "dattn", "dW_r", "db_r"]
    for rep in range(10):
        again = run(lib.uavgnn_gatv2_bwd)
        for a, c, nm in zip(g_mf, again, names):
            assert th.equal(a, c), f"{nm}: matrix-core backward not bit-reproducible (launch {rep + 2})"
    for a, b, nm in zip(g_mf, g_gen, names):
        assert bool(th.isfinite(a).all()), nm
        scale = float(b.abs().max())
        err = (a - b).abs()
        loose = int((err > 2e-5 * scale).sum())
        assert loose <= 8 and float(err.max()) <= 1e-3 * scale, (
            f"{nm}: {loose} elements beyond 2e-5 of max|ref|, worst {float(err.max()) / scale:.3e} of max|ref|")


@pytest.mark.parametrize("N,K_in,H", [(1000, 320, 256), (128, 256, 256), (77, 384, 256), (3, 32, 32), (4099, 96, 64)])
def test_fused_gru_cell_kernel_vs_oracle(N, K_in, H):
    """K4 as one kernel (csrc/gru_fused.hip: both GEMMs on fp32 MFMA into shared r / z and separate n accumulators, gates
    in the epilogue) against nn.GRUCell's math in float64, forward and every gradient (backward = gate kernel on the saved
    pre-activation sets + vendor GEMMs); N not a multiple of the 128-row tile, all supported K / H granularities; and
    against the unfused path (vendor GEMMs + gate kernel)."""
    from uav_bs_ctrl_amd import ops
    gen = th.Generator().manual_seed(N + H)
    cell = th.nn.GRUCell(K_in, H)
    with th.no_grad():
        for p in cell.parameters():
            p.copy_(0.3 * th.randn(p.shape, generator=gen))
    inp, h = th.randn(N, K_in, generator=gen), th.randn(N, H, generator=gen)
    w = th.randn(N, H, generator=gen)
    c64 = th.nn.GRUCell(K_in, H).double()
    c64.load_state_dict({k: v.double() for k, v in cell.state_dict().items()})
    i64, h64 = inp.double().requires_grad_(True), h.double().requires_grad_(True)
    ref = c64(i64, h64)
    gref = th.autograd.grad((ref * w.double()).sum(), [i64, h64] + list(c64.parameters()))
    i32, h32 = inp.clone().requires_grad_(True), h.clone().requires_grad_(True)
    g32 = th.autograd.grad((cell(i32, h32) * w).sum(), [i32, h32] + list(cell.parameters()))   # ATen's fp32 GRUCell on the CPU
    cell = cell.cuda()
    res = {}
    # (fused cell, bf16x3 arithmetic): the bf16-matrix-core cell (csrc/gru_x3.hip), the fp32-MFMA cell, vendor GEMMs + gates
    min_rows = ops.GRU_FUSED_MIN_ROWS
    for fused, x3 in ((True, True), (True, False), (False, False)):
        ops.GRU_FUSED, ops.GRU_X3, ops.GRU_FUSED_MIN_ROWS = fused, x3, 0   # the fused cells at every size, ragged tiles included
        try:
            i_d, h_d = inp.cuda().requires_grad_(True), h.cuda().requires_grad_(True)
            assert ops.gru_cell_supported(i_d, h_d) == fused
            out = ops.gru_cell(i_d, h_d, cell)
            got = th.autograd.grad((out * w.cuda()).sum(), [i_d, h_d] + list(cell.parameters()))
            with th.no_grad():
                out_ng = ops.gru_cell(inp.cuda(), h.cuda(), cell)
            assert th.equal(out_ng, out.detach())
            res[(fused, x3)] = (out.detach(), got)
        finally:
            ops.GRU_FUSED, ops.GRU_X3, ops.GRU_FUSED_MIN_ROWS = True, True, min_rows
    from uav_bs_ctrl_amd import _lib as L
    if L.lib().uavgnn_gru_cell_x3_supported(K_in, H):
        assert not th.equal(res[(True, True)][0], res[(True, False)][0]), "the bf16x3 cell did not run"
    for key, (out, got) in res.items():
        assert_close(out, ref, 1e-5, f"h' (fused, x3)={key}")
        for a, b, b32, nm in zip(got, gref, g32, ["d_inp", "d_h", "dW_ih", "dW_hh", "db_ih", "db_hh"]):
            grad_close(a, b, f"K4 N={N} K={K_in} H={H} (fused, x3)={key}: {nm}", ref32=b32)


@pytest.mark.parametrize("M,N,K,transpose", [(4096, 256, 512, False), (5000, 512, 256, True), (4097, 128, 96, False),
                                             (8192, 384, 768, True), (4200, 256, 32, False)])
def test_gemm_bf16x3_vs_float64(M, N, K, transpose):
    """csrc/gemm_x3.hip (fp32 GEMM as six exact bf16 x bf16 MFMA products per fp32 product) against the float64 product of the
    same operands: forward layout (B = W [N, K]) and input-gradient layout (B = W^T from W [K, N]), strided operands, rows /
    columns that do not fill the 128 x 128 tile, bias, accumulate and ReLU epilogues.  The error bound is the one an fp32
    GEMM is held to (relative to sum_k |a_k b_k|), and the vendor GEMM on the same data is measured next to it."""
    from uav_bs_ctrl_amd import ops
    gen = th.Generator().manual_seed(M + N + K)
    a_full = th.randn(M, K + 8, generator=gen).cuda()
    a = a_full[:, :K]                                             # row stride K + 8
    W_full = th.randn((K, N + 4) if transpose else (N, K + 4), generator=gen).cuda() * 0.1
    W = W_full[:, :N] if transpose else W_full[:, :K]             # strided weight view (as Wp[:, :H] in the TarMAC step)
    bias = th.randn(N, generator=gen).cuda()
    assert ops.gemm_x3_supported(a, N, K)
    B64 = W.double() if transpose else W.double().t()
    ref = a.double() @ B64
    scale = a.double().abs() @ B64.abs()
    out = ops.gemm_x3(a, W, transpose)
    err = ((out.double() - ref).abs() / scale).max().item()
    err_vendor = (((a @ (W if transpose else W.t())).double() - ref).abs() / scale).max().item()
    assert err < 6e-7, (err, err_vendor)                          # 10 x 2^-24: an fp32 accumulation of K <= 768 terms
    assert err < 2.0 * err_vendor + 1e-7, (err, err_vendor)
    out_b = ops.gemm_x3(a, W, transpose, bias=bias, relu=True)
    assert_close(out_b, th.relu(ref + bias.double()), 1e-5, "bias + relu epilogue", floor=1e-6)
    acc0 = th.randn(M, N + 8, generator=gen).cuda()
    acc = acc0.clone()
    ops.gemm_x3(a, W, transpose, out=acc[:, :N], accumulate=True)
    assert_close(acc[:, :N], ref + acc0[:, :N].double(), 1e-5, "accumulate epilogue", floor=1e-6)
    assert th.equal(acc[:, N:], acc0[:, N:]), "columns past N were written"
    assert th.equal(ops.gemm_x3(a, W, transpose), out), "not bit-reproducible"


@pytest.mark.parametrize("ea,eb", [(60, 60), (-60, -60), (-100, 40), (-120, 100), (-135, 120)])
def test_gemm_bf16x3_operand_range(ea, eb):
    """The three-way bf16 split at the ends of the fp32 exponent range.  bf16 has fp32's exponent range, so there is no
    overflow case and no scaling: operands of magnitude 2^60 x 2^60 (products near the top of fp32), 2^-60 x 2^-60 (products
    near the bottom of the normal range) and 2^-100 x 2^40 are held to the SAME bound as ordinary operands.  Below ~2^-110
    the low split terms of an operand (a2 ~ 2^-8 a, a3 ~ 2^-16 a) leave the normal bf16 range (< 2^-126) and may be lost,
    so for such operands the contract is the absolute bound  |err| <= 6e-7 sum|a b| + 2^-125 sum_k(|a_k| + |b_k|)
    (a lost term is at most 2^-126 times the other factor); fp32 denormal operands (2^-135) are inside it too."""
    from uav_bs_ctrl_amd import ops
    M, N, K = 4096, 256, 320
    gen = th.Generator().manual_seed(abs(ea) * 1000 + abs(eb))
    a = (th.randn(M, K, generator=gen) * 2.0 ** ea).cuda()
    W = (th.randn(N, K, generator=gen) * 2.0 ** eb).cuda()
    assert ops.gemm_x3_supported(a, N, K)
    out = ops.gemm_x3(a, W, False)
    assert th.isfinite(out).all()
    ref = a.double() @ W.double().t()
    scale = a.double().abs() @ W.double().abs().t()
    tiny = 2.0 ** -125 * (a.double().abs().sum(1, keepdim=True) + W.double().abs().sum(1).unsqueeze(0))
    err = (out.double() - ref).abs()
    # results below the fp32 normal range are outside any fp32 contract (the vendor GEMM flushes them as well)
    sure = ref.abs() > 2.0 ** -120
    if min(ea, eb) >= -100:
        assert float((err / scale)[sure].max()) < 6e-7, float((err / scale)[sure].max())
    assert bool((err <= 6e-7 * scale + tiny)[sure].all()), float((err / (6e-7 * scale + tiny))[sure].max())


@pytest.mark.gpu
def test_bf16x3_non_finite_and_near_overflow_operands_follow_the_documented_contract():
    """VERDICT r3 item 7.  The three-way split forms x - bf16(x): an Inf operand gives Inf - Inf = NaN where an fp32 GEMM gives
    Inf, and a FINITE |x| >= 0x7F7F8000 (within half a bf16 ulp of FLT_MAX: 3.3895e38) rounds its first term to Inf.  The
    contract (behavioural differences): a non-finite or near-overflow operand makes the outputs that depend
    on it NON-FINITE (NaN where fp32 may say Inf) and touches nothing else - every other output row / column carries the bits
    of the clean run; the largest operand that is still exact is 0x7F7F7FFF."""
    import struct
    from uav_bs_ctrl_amd import ops
    f = lambda bits: struct.unpack("f", struct.pack("I", bits))[0]   # noqa: E731
    M, N, K = 4096, 256, 320
    gen = th.Generator().manual_seed(5)
    a = th.randn(M, K, generator=gen).cuda()
    W = (0.05 * th.randn(N, K, generator=gen)).cuda()
    clean = ops.gemm_x3(a, W, False)
    bad = a.clone()
    bad[7, 3], bad[100, 0], bad[2000, 319] = float("inf"), float("nan"), f(0x7F7F8000)
    bad[3000, 5] = f(0x7F7F7FFF) * 2.0 ** -120           # ordinary value: a control row that stays clean
    out = ops.gemm_x3(bad, W, False)
    rows = th.tensor([7, 100, 2000], device="cuda")
    for r in (7, 100, 2000):
        assert not bool(th.isfinite(out[r]).all()), r
    keep = th.ones(M, dtype=th.bool, device="cuda")
    keep[rows] = False
    keep[3000] = False
    assert th.equal(out[keep], clean[keep])               # nothing leaks into other rows
    assert bool(th.isfinite(out[3000]).all())
    # the largest exactly representable operand: 0x7F7F7FFF splits into finite terms (products kept small by the weights)
    big = th.zeros(M, K, device="cuda")
    big[:, 0] = f(0x7F7F7FFF)
    Wt = th.zeros(N, K, device="cuda")
    Wt[:, 0] = 2.0 ** -10
    ob = ops.gemm_x3(big, Wt, False)
    assert bool(th.isfinite(ob).all())
    assert float((ob.double() - float(f(0x7F7F7FFF)) * 2.0 ** -10).abs().max()) <= 1e-6 * f(0x7F7F7FFF) * 2.0 ** -10
    # GRU cell: a non-finite input row gives a non-finite h' row and leaves the other agents alone
    cell = th.nn.GRUCell(K, 256).cuda()
    inp, h = th.randn(M, K, device="cuda"), th.randn(M, 256, device="cuda")
    with th.no_grad():
        y0 = ops.gru_cell(inp, h, cell)
        inp2 = inp.clone()
        inp2[11, 17] = float("inf")
        y1 = ops.gru_cell(inp2, h, cell)
    assert not bool(th.isfinite(y1[11]).all())
    m = th.ones(M, dtype=th.bool, device="cuda")
    m[11] = False
    assert th.equal(y1[m], y0[m])


def test_fused_gru_cell_operand_range():
    """K4 on the bf16 matrix cores with activations at the ends of the range: hidden state / input of magnitude 2^-115
    (their low split terms underflow bf16: they contribute < 2^-126 to a pre-activation of O(0.1)) and of magnitude 2^12
    (saturated gates: sigmoid -> 0 / 1, tanh -> +-1 exactly as ATen's), against float64."""
    from uav_bs_ctrl_amd import ops
    N, K_in, H = 2048, 320, 256
    gen = th.Generator().manual_seed(11)
    cell = th.nn.GRUCell(K_in, H)
    c64 = th.nn.GRUCell(K_in, H).double()
    c64.load_state_dict({k: v.double() for k, v in cell.state_dict().items()})
    cell = cell.cuda()
    for e in (-115, 12):
        inp, h = th.randn(N, K_in, generator=gen) * 2.0 ** e, th.randn(N, H, generator=gen) * 2.0 ** e
        with th.no_grad():
            ref = c64(inp.double(), h.double())
            ref32 = cell.cpu()(inp, h)            # ATen's fp32 cell on the host: what fp32 arithmetic delivers here
            cell = cell.cuda()
            out = ops.gru_cell(inp.cuda(), h.cuda(), cell)
        assert ops.gru_cell_supported(inp.cuda(), h.cuda())
        # at 2^12 the pre-activations are O(10^3) with an fp32 error of O(10^-3): wherever a gate is NOT saturated that
        # error is multiplied by |h| ~ 10^3 - any fp32 cell shows it, so the bound is grad_close's (1e-5 or 4x fp32's own)
        grad_close(out, ref, f"K4 operand range: h' at 2^{e}", ref32=ref32)


@pytest.mark.parametrize("n,Mo,Ko,views", [(32768, 768, 320, False), (5000, 96, 256, True), (4097, 9, 256, False),
                                           (70001, 256, 512, False), (4096, 130, 70, True)])
def test_gemm_tn_bf16x3_weight_gradient_vs_float64(n, Mo, Ko, views, monkeypatch):
    """csrc/gemm_tn_x3.hip (dW = dy^T x: contraction over the agent axis, operands transposed on their way into LDS, row
    chunks summed in a fixed order) against the float64 product: the layer shapes of the path (W_ih, stacked projections, Q
    head, f_aggr), row counts that do not fill the last 32-row slice / chunk, output sizes that do not fill the 128 x 128
    tile, column-sliced operand views, accumulate mode; error measured like an fp32 GEMM's (relative to sum |a b|) next to the
    vendor GEMM's on the same data; bit-reproducible."""
    from uav_bs_ctrl_amd import ops
    monkeypatch.setattr(ops, "GEMM_TN_MIN_ROWS", 4096)      # the dispatcher takes the kernel from 2^18 rows; test it from 4096
    gen = th.Generator().manual_seed(n + Mo + Ko)
    dy_full = (th.randn(n, Mo + (8 if views else 0), generator=gen) * 0.3).cuda()
    x_full = th.randn(n, Ko + (4 if views else 0), generator=gen).cuda()
    dy, x = dy_full[:, (8 if views else 0):], x_full[:, :Ko]
    assert ops.gemm_tn_x3_supported(dy, x)
    ref = dy.double().t() @ x.double()
    scale = dy.double().abs().t() @ x.double().abs()
    part = ops.gemm_tn_x3(dy, x)
    out = part.sum(0)
    assert out.shape == (Mo, Ko)
    err = float(((out.double() - ref).abs() / scale).max())
    err_vendor = float((((dy.t() @ x).double() - ref).abs() / scale).max())
    assert err <= max(2.0 * err_vendor, 1e-6), (err, err_vendor)
    assert_close(out, ref, 1e-5, "dW", floor=1e-5 * float(scale.max()) * 1e-2)
    assert th.equal(ops.gemm_tn_x3(dy, x), part), "not bit-reproducible"
    acc = part.clone()
    ops.gemm_tn_x3(dy, x, acc, accumulate=True)
    assert_close(acc.sum(0), 2 * ref, 1e-5, "accumulate mode", floor=1e-5 * float(scale.max()) * 1e-2)
    # the autograd paths that use it: ops.linear's weight gradient and the plain (sink-less) _wgrad
    W = th.randn(Mo, Ko, generator=gen).cuda().requires_grad_(True)
    xg = x.contiguous()
    (ops.linear(xg, W) * dy).sum().backward()
    assert_close(W.grad, ref, 1e-5, "ops.linear dW", floor=1e-5 * float(scale.max()) * 1e-2)


def test_linear_layers_take_the_bf16x3_kernel_and_match_vendor_path():
    """ops.linear / linear_relu forward and input gradient at an encoder-layer shape go through csrc/gemm_x3.hip (the span
    counter moves) and agree with the vendor-GEMM path within the fp32 tolerance, weight / bias gradients included."""
    from uav_bs_ctrl_amd import ops
    gen = th.Generator().manual_seed(5)
    x = th.randn(8192, 512, generator=gen).cuda().requires_grad_(True)
    W = (th.randn(256, 512, generator=gen) * 0.05).cuda().requires_grad_(True)
    b = th.randn(256, generator=gen).cuda().requires_grad_(True)
    w = th.randn(8192, 256, generator=gen).cuda()
    res = {}
    for x3 in (True, False):
        ops.GEMM_X3 = x3
        try:
            assert ops.gemm_x3_supported(x, 256, 512) == x3
            y = ops.linear(x, W, b)          # (the ReLU variant's backward masks with y > 0: a 1e-7 difference in y flips
            res[x3] = (y.detach(),) + th.autograd.grad((y * w).sum(), [x, W, b]) + (ops.linear_relu(x, W, b).detach(),)
        finally:                             #  the mask of entries at the kink, so gradients are compared on the plain layer)
            ops.GEMM_X3 = True
    assert not th.equal(res[True][0], res[False][0]), "the bf16x3 GEMM did not run"
    for a, c, nm in zip(res[True], res[False], ["y", "dx", "dW", "db", "relu(y)"]):
        assert_close(a, c, 2e-5, nm, floor=1e-5)


@pytest.mark.parametrize("transpose", [False, True])
def test_bf16x3_split_is_exact(transpose):
    """uavgnn_split_bf16x3: the three bf16 planes of a weight matrix sum back to the fp32 input EXACTLY (bit for bit) over
    46 binades of magnitude, both layouts, strided input - the property the "six exact products" argument of
    csrc/bf16x3.h rests on - and the terms shrink by >= 2^-8 per plane."""
    from uav_bs_ctrl_amd import _lib as L
    gen = th.Generator().manual_seed(11)
    R, C = 96, 130
    mag = th.exp2(th.randint(-23, 23, (R, C + 6), generator=gen).float())
    W_full = (th.randn(R, C + 6, generator=gen) * mag).cuda()
    W_full[0, :4] = th.tensor([0.0, -0.0, 1.0, -3.0e38])
    W = W_full[:, :C]                                              # row stride C + 6
    planes = th.empty(6 * R * C, dtype=th.uint8, device="cuda")
    L.check(L.lib().uavgnn_split_bf16x3(W.data_ptr(), W.stride(0), R, C, int(transpose), planes.data_ptr(), L.stream()), "split")
    th.cuda.synchronize()
    p = planes.view(th.bfloat16).view(3, C, R) if transpose else planes.view(th.bfloat16).view(3, R, C)
    ref = W.t() if transpose else W
    total = p[0].double() + p[1].double() + p[2].double()
    assert th.equal(total, ref.double()), "a1 + a2 + a3 != a"
    assert th.equal(total.float(), ref)
    a = ref.abs().double()
    assert bool((p[1].double().abs() <= a * 2.0 ** -8).all()) and bool((p[2].double().abs() <= a * 2.0 ** -16).all())


def test_frozen_weights_scope_reuses_planes_and_changes_nothing():
    """ops.frozen_weights() (the learner's loss forward + backward): weight planes of the bf16x3 kernels are split once per
    scope instead of once per call - same bits out; outside the scope a `.data` write to a weight is seen by the very next call."""
    from uav_bs_ctrl_amd import ops
    th.manual_seed(3)
    N, K, H = 4096, 320, 256
    cell = th.nn.GRUCell(K, H).cuda()
    inp, h = th.randn(N, K, device="cuda"), th.randn(N, H, device="cuda")
    x, W = th.randn(N, 512, device="cuda"), th.randn(256, 512, device="cuda") * 0.05
    with th.no_grad():
        y0, g0 = ops.gru_cell(inp, h, cell), ops.gemm_x3(x, W)
        with ops.frozen_weights():
            y1, g1 = ops.gru_cell(inp, h, cell), ops.gemm_x3(x, W)
            y2, g2 = ops.gru_cell(inp, h, cell), ops.gemm_x3(x, W)
            assert len(ops._PLANES) == 2                       # one entry per weight set, not per call
            with ops.frozen_weights():                         # nested scopes share the outer cache
                ops.gru_cell(inp, h, cell)
                assert len(ops._PLANES) == 2
        assert ops._PLANES is None
        assert th.equal(y0, y1) and th.equal(y1, y2) and th.equal(g0, g1) and th.equal(g1, g2)
        cell.weight_ih.data.mul_(0.5)
        W.data.mul_(2.0)
        y3, g3 = ops.gru_cell(inp, h, cell), ops.gemm_x3(x, W)
        ref = cell.double()(inp.double(), h.double())
        assert float((y3.double() - ref).abs().max()) <= 1e-5
        assert float((g3 - 2.0 * g0).abs().max()) == 0.0        # a power-of-two scale commutes with every rounding


def test_two_piece_gru_input_equals_the_concatenated_input():
    """uavgnn_gru_cell_fwd_x3_cat: the cell's input given as [x || c] from two buffers (no-grad TarMAC steps skip the
    concatenating copy) must produce the bits of the one-buffer call - same kernel, same slices, different base pointers."""
    from uav_bs_ctrl_amd import ops
    th.manual_seed(11)
    N, H, M = 5000, 256, 64          # not a multiple of the 128-row tile: the clamped tail rows are covered
    cell = th.nn.GRUCell(H + M, H).cuda()
    x, c, h = th.randn(N, H, device="cuda"), th.randn(N, M, device="cuda"), th.randn(N, H, device="cuda")
    with th.no_grad():
        assert ops.gru_cell_two_piece_supported(x, c, h)
        cat = th.cat((x, c), 1)
        y_cat, _ = ops._gru_cell_launch(cat, h, cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, save=False)
        y_two, _ = ops._gru_cell_launch(x, h, cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, save=False, inp2=c)
        assert th.equal(y_cat, y_two)
        ref = cell.double()(cat.double(), h.double())
        assert float((y_two.double() - ref).abs().max()) <= 1e-5
        # strided pieces (views into wider buffers) take the same path
        wide_x, wide_c = th.randn(N, H + 64, device="cuda"), th.randn(N, M + 32, device="cuda")
        xv, cv = wide_x[:, :H], wide_c[:, :M]
        assert ops.gru_cell_two_piece_supported(xv, cv, h)
        y_v, _ = ops._gru_cell_launch(xv, h, cell.float().weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, save=False, inp2=cv)
        y_r, _ = ops._gru_cell_launch(th.cat((xv, cv), 1), h, cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, save=False)
        assert th.equal(y_v, y_r)


def test_no_grad_tarmac_step_without_the_concatenated_copy_equals_the_training_forward():
    """agent forward under no_grad (two-piece cell input, K3b writes c alone) vs the same forward with grad enabled (the
    [x || c] buffer is built and kept for the backward): same logits and hidden state, bit for bit."""
    cfg = dict(enc="gnn", c="tarmac", n_heads=4, key_size=16, msg_size=64, n_rounds=1, dueling=False, hidden_size=256)
    B, n, M = 160, 8, 20
    from uav_bs_ctrl_amd import GnnAgent
    th.manual_seed(5)
    agent = GnnAgent(dict(agent=2, ubs=2, gt=4), 9, make_args(cfg)).cuda()
    g = to_batch(synth_graph(B, n, M, "ragged", seed=3))
    h = 0.3 * th.randn(B * n, 256, device="cuda")
    with th.no_grad():
        q0, h0 = agent(g, h)
    q1, h1 = agent(g.fresh(), h.clone().requires_grad_(True))
    assert th.equal(q0, q1.detach()) and th.equal(h0, h1.detach())


def _small_learner_and_batch(B=160, n=8, M=20, T=3, seed=0, **over):
    """exp3 learner + a synthetic sampled batch of B sequences (bench.py's generator): N = B n >= 1024 rows, so the recurrent
    step takes the fused matrix-core kernels the benchmark runs."""
    import bench
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    th.manual_seed(seed)
    args = bench.exp3_args("cuda")
    for k, v in over.items():
        setattr(args, k, v)
    learner = MultiAgentQLearner(dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=9, n_agents=n, episode_limit=T), args)
    batch = bench.make_sequence(B, n, M, T, "env", th.device("cuda"), seed=7, distinct=2)
    return learner, batch


@pytest.mark.gpu
def test_time_batched_weight_gradient_staging_equals_the_per_step_reductions(monkeypatch):
    """ops.WeightGradSink.begin_sequence / end_sequence (learner.accumulate): the weight and bias gradients of the T + 1
    recurrent steps reduced ONCE from time-batched buffers equal the per-step reductions of round 3 (same products, another
    summation order: 1e-5 relative), the staging is actually taken, and two staged runs agree bit for bit."""
    from uav_bs_ctrl_amd import ops
    learner, batch = _small_learner_and_batch()
    taken = []
    orig = ops.WeightGradSink.end_sequence

    def spy(self):
        taken.append(0 if self.seq is None else len(self.seq.bwd_steps))
        return orig(self)
    monkeypatch.setattr(ops.WeightGradSink, "end_sequence", spy)

    def grads(staged):
        monkeypatch.setattr(ops, "SEQ_STAGING", staged)
        fb = dict(batch, obs=[g.fresh() for g in batch["obs"]], obs_all=batch["obs_all"].fresh(),
                  obs_all_next=batch["obs_all_next"].fresh())
        learner.accumulate(fb)
        return learner.grads.flat.clone()
    g_step = grads(False)
    assert max(taken) == 0
    g_seq, g_seq2 = grads(True), grads(True)
    assert max(taken) == len(batch["obs"])                      # every recurrent step of the sequence was staged
    assert th.equal(g_seq, g_seq2)
    assert float(g_step.abs().max()) > 0
    assert_close(g_seq, g_step, 1e-5, "flat gradient, staged vs per-step")


@pytest.mark.gpu
def test_plane_cache_never_serves_a_recycled_weight_address():
    """TarMAC with a dueling head builds its stacked projection weight with th.cat on every call; with msg + 2 key =
    128 columns and N >= 4096 rows it takes the bf16x3 GEMM whose weight planes are cached per frozen_weights() scope under
    the weight's ADDRESS.  The target network's temporary is freed after its no-grad step, the policy network's next
    temporary may land on the same address: the cache entry keeps its weight alive, so the address cannot be recycled and
    the gradients with the scope equal the gradients without it."""
    from uav_bs_ctrl_amd import ops
    learner, batch = _small_learner_and_batch(B=512, n=8, M=10, T=2, dueling=True, msg_size=64, key_size=32)

    def grads(scope):
        fb = dict(batch, obs=[g.fresh() for g in batch["obs"]], obs_all=batch["obs_all"].fresh(),
                  obs_all_next=batch["obs_all_next"].fresh())
        if scope:
            learner.accumulate(fb)
        else:
            class _NoScope:
                def __enter__(self): return self
                def __exit__(self, *e): return False
            orig, ops.frozen_weights = ops.frozen_weights, _NoScope
            try:
                learner.accumulate(fb)
            finally:
                ops.frozen_weights = orig
        return learner.grads.flat.clone()
    g0, g1 = grads(False), grads(True)
    assert float(g0.abs().max()) > 0
    assert th.equal(g0, g1)


@pytest.mark.parametrize("N,H,n_out,with_dh", [(1000, 256, 9, True), (333, 64, 5, False), (4099, 256, 16, True), (7, 32, 1, True)])
def test_gate_gradient_kernel_with_the_head_gradient_folded_in(N, H, n_out, with_dh):
    """uavgnn_gru_gates_bwd_fused_head(pre, h, d_hout, dq, W_out) == uavgnn_gru_gates_bwd_fused(pre, h, d_hout + dq W_out):
    the gradient of h' formed inside the kernel (float64 reference for the sum), with and without an incoming d_hout."""
    from uav_bs_ctrl_amd import _lib as L
    gen = th.Generator().manual_seed(N + n_out)
    dev = "cuda"
    pre, h = th.randn(N, 4 * H, generator=gen).to(dev), th.randn(N, H, generator=gen).to(dev)
    dq, W = th.randn(N, n_out, generator=gen).to(dev), (0.3 * th.randn(n_out, H, generator=gen)).to(dev)
    d_hout = th.randn(N, H, generator=gen).to(dev) if with_dh else None
    tot = (dq.double() @ W.double() + (d_hout.double() if with_dh else 0.0)).float().contiguous()
    lib, st = L.lib(), L.stream()
    ref = [th.empty(N, 3 * H, device=dev), th.empty(N, 3 * H, device=dev), th.empty(N, H, device=dev)]
    got = [th.full_like(t, float("nan")) for t in ref]
    assert lib.uavgnn_gru_gates_bwd_fused(pre.data_ptr(), h.data_ptr(), tot.data_ptr(), N, H, *[t.data_ptr() for t in ref], st) == 0
    assert lib.uavgnn_gru_gates_bwd_fused_head(pre.data_ptr(), h.data_ptr(), L.ptr(d_hout), dq.data_ptr(), n_out, W.data_ptr(), N, H,
                                               *[t.data_ptr() for t in got], st) == 0
    th.cuda.synchronize()
    for a, b, nm in zip(got, ref, ("d_gi", "d_gh", "d_h")):
        assert_close(a, b, 2e-6, nm)
    # argument errors: a head without dq, too many outputs
    assert lib.uavgnn_gru_gates_bwd_fused_head(pre.data_ptr(), h.data_ptr(), None, None, n_out, W.data_ptr(), N, H,
                                               *[t.data_ptr() for t in got], st) == L.UAVGNN_EINVAL
    assert lib.uavgnn_gru_gates_bwd_fused_head(pre.data_ptr(), h.data_ptr(), None, dq.data_ptr(), 65, W.data_ptr(), N, H,
                                               *[t.data_ptr() for t in got], st) != 0


@pytest.mark.gpu
def test_gru_cell_backward_as_one_c_abi_call_equals_the_host_sequence():
    """uavgnn_gru_cell_bwd ("uavgnn_gru_cell_{fwd,bwd}"): gate gradients + d_inp = d_gi W_ih + d_h += d_gh W_hh in
    ONE C-ABI call equal what ops issues as three calls, and the gradients of nn.GRUCell in float64 (1e-5); the single
    workspace query agrees with the per-kernel queries."""
    from uav_bs_ctrl_amd import _lib as L, ops
    th.manual_seed(21)
    N, K, H = 4096 + 40, 320, 256          # not a multiple of the tiles
    cell = th.nn.GRUCell(K, H).cuda()
    inp, h = th.randn(N, K, device="cuda"), 0.5 * th.randn(N, H, device="cuda")
    d_hout = th.randn(N, H, device="cuda")
    lib = L.lib()
    with th.no_grad():
        h2, pre = ops._gru_cell_launch(inp, h, cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, save=True)
    nbytes = lib.uavgnn_gru_cell_bwd_workspace_bytes(K, H)
    assert nbytes == lib.uavgnn_workspace_bytes(5, K, H, 0) == 6 * 3 * H * (K + H)
    assert lib.uavgnn_workspace_bytes(4, K, H, 0) == lib.uavgnn_gru_cell_x3_workspace_bytes(K, H)
    assert lib.uavgnn_workspace_bytes(1, 4, 256, 0) == lib.uavgnn_gatv2_bwd_workspace_bytes(4, 256)
    assert lib.uavgnn_workspace_bytes(99, 1, 1, 1) == 0
    planes = th.empty(nbytes, dtype=th.uint8, device="cuda")
    L.check(lib.uavgnn_gru_split_weights_bwd(cell.weight_ih.data_ptr(), K, cell.weight_hh.data_ptr(), H, planes.data_ptr(),
                                             L.stream()), "split_bwd")
    d_gi, d_gh = th.empty(N, 3 * H, device="cuda"), th.empty(N, 3 * H, device="cuda")
    d_inp, d_h = th.empty(N, K, device="cuda"), th.empty(N, H, device="cuda")
    L.check(lib.uavgnn_gru_cell_bwd(pre.data_ptr(), h.data_ptr(), d_hout.data_ptr(), N, K, H, planes.data_ptr(), d_gi.data_ptr(),
                                    d_gh.data_ptr(), d_inp.data_ptr(), K, d_h.data_ptr(), L.stream()), "uavgnn_gru_cell_bwd")
    g_gi, g_gh, g_dh = ops._gru_gates_bwd_from_pre(pre, h, d_hout)
    assert th.equal(d_gi, g_gi) and th.equal(d_gh, g_gh)
    c64 = th.nn.GRUCell(K, H).cuda().double()
    c64.load_state_dict({k: v.double() for k, v in cell.state_dict().items()})
    i64, h64 = inp.double().requires_grad_(True), h.double().requires_grad_(True)
    (c64(i64, h64) * d_hout.double()).sum().backward()
    assert_close(d_inp, i64.grad, 1e-5, "d_inp")
    assert_close(d_h, h64.grad, 1e-5, "d_h")
    assert_close(d_gi.t() @ inp, c64.weight_ih.grad, 1e-5, "dW_ih from the kept operands")


@pytest.mark.gpu
@pytest.mark.parametrize("dist,save", [("env", False), ("dense", False), ("env", True)])
def test_fused_hetero_k1_writes_every_row_and_repeats_bit_for_bit(dist, save):
    """The fused K1 forward at C3 size, six launches into NaN-POISONED outputs: every element is written (a row store lost
    under a mask, an out-of-range buffer offset that wraps - both happened while the round-4 row-store path was built) and
    every launch returns the same bits (the raw-buffer-store variant returned another store's address operand in ~0.003 % of
    the rows under store back-pressure: tools/k1_check.py); the saved attention weights likewise."""
    import bench
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.agents.gnn_agents import GATv2Conv
    dev = th.device("cuda")
    gen = th.Generator(device=dev)
    gen.manual_seed(3)
    th.manual_seed(3)
    hb = bench.synth_batch_gpu(4096, 8, 80, dist, dev, gen)
    xs, so = hb.relation_segments("seen")
    xn, no = hb.relation_segments("near")
    order, x_a = hb.relation_order("seen"), hb.agent_feat()
    N = x_a.shape[0]
    ps = []
    for FS in (4, 2):
        c = GATv2Conv((FS, 2), 64, 4).to(dev)
        ps.append([t.detach().contiguous() for t in (c.fc_src.weight, c.fc_src.bias, c.fc_dst.weight, c.fc_dst.bias, c.attn,
                                                     c.res_fc.weight, c.res_fc.bias)])
    lib, st = L.lib(), L.stream()

    def run():
        out = th.full((N, 512), float("nan"), device=dev)
        a_s = th.full((max(xs.shape[0], 1), 4), float("nan"), device=dev)
        a_n = th.full((max(xn.shape[0], 1), 4), float("nan"), device=dev)
        rc = lib.uavgnn_gatv2_hetero_fwd(xs.data_ptr(), xs.shape[0], so.data_ptr(), L.ptr(order), xn.data_ptr(), xn.shape[0],
                                         no.data_ptr(), x_a.data_ptr(), N, L.ptr_array(ps[0]), L.ptr_array(ps[1]), 4, 64, 0.2,
                                         out.data_ptr(), 512, a_s.data_ptr() if save else None,
                                         a_n.data_ptr() if save else None, st)
        assert rc == 0
        th.cuda.synchronize()
        return out, a_s, a_n
    o1, s1, n1 = run()
    assert not bool(th.isnan(o1).any())
    if save:
        assert not bool(th.isnan(n1).any()) and (xs.shape[0] == 0 or not bool(th.isnan(s1).any()))
    for _ in range(5):
        o2, s2, n2 = run()
        assert th.equal(o1, o2)
        if save:
            assert th.equal(n1, n2) and th.equal(s1, s2)


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,M,dist,save,bias", [(4096, 8, 80, "env", False, True), (64, 8, 80, "dense", True, True),
                                                 (9, 5, 40, "ragged", True, False), (3, 2, 5, "env", False, True)])
def test_fused_hetero_k1_prepared_image_is_bit_identical_and_follows_the_parameters(B, n, M, dist, save, bias):
    """uavgnn_gatv2_hetero_prepare + uavgnn_gatv2_hetero_fwd_image: the parameter image built once by one workgroup and copied by
    the forward's workgroups gives the SAME BITS as the in-kernel prologue (outputs and saved attention weights), also without a
    res_fc bias and on a ragged N; a rebuilt image follows a parameter change; bad arguments are refused."""
    import bench
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.agents.gnn_agents import GATv2Conv
    dev = th.device("cuda")
    gen = th.Generator(device=dev)
    gen.manual_seed(11)
    th.manual_seed(11)
    hb = bench.synth_batch_gpu(B, n, M, dist, dev, gen)
    xs, so = hb.relation_segments("seen")
    xn, no = hb.relation_segments("near")
    order, x_a = hb.relation_order("seen"), hb.agent_feat()
    N = x_a.shape[0]
    ps = []
    for FS in (4, 2):
        c = GATv2Conv((FS, 2), 64, 4).to(dev)
        ps.append([t.detach().contiguous() for t in (c.fc_src.weight, c.fc_src.bias, c.fc_dst.weight, c.fc_dst.bias, c.attn,
                                                     c.res_fc.weight)] + [c.res_fc.bias.detach().contiguous() if bias else None])
    lib, st = L.lib(), L.stream()
    nbytes = lib.uavgnn_gatv2_hetero_image_bytes()
    assert nbytes > 0 and nbytes % 16 == 0 and lib.uavgnn_workspace_bytes(8, 0, 0, 0) == nbytes
    image = th.empty(nbytes, dtype=th.uint8, device=dev)

    def prepare():
        assert lib.uavgnn_gatv2_hetero_prepare(L.ptr_array(ps[0]), L.ptr_array(ps[1]), 4, 64, 0.2, image.data_ptr(), st) == 0

    def run(img):
        out = th.full((N, 512), float("nan"), device=dev)
        a_s = th.full((max(xs.shape[0], 1), 4), float("nan"), device=dev)
        a_n = th.full((max(xn.shape[0], 1), 4), float("nan"), device=dev)
        head = (xs.data_ptr(), xs.shape[0], so.data_ptr(), L.ptr(order), xn.data_ptr(), xn.shape[0], no.data_ptr(), x_a.data_ptr(), N,
                L.ptr_array(ps[0]), L.ptr_array(ps[1]), 4, 64, 0.2)
        tail = (out.data_ptr(), 512, a_s.data_ptr() if save else None, a_n.data_ptr() if save else None, 3, st)
        rc = lib.uavgnn_gatv2_hetero_fwd_image(*head, img.data_ptr(), *tail) if img is not None else \
            lib.uavgnn_gatv2_hetero_fwd_phases(*head, *tail)
        assert rc == 0
        th.cuda.synchronize()
        return out, a_s, a_n

    prepare()
    for a, b in zip(run(None), run(image)):
        assert th.equal(th.nan_to_num(a, nan=-7.0), th.nan_to_num(b, nan=-7.0))
    assert not bool(th.isnan(run(image)[0]).any())
    # the image is a function of the parameter values: stale until rebuilt
    ps[1][0].mul_(1.5)
    ps[0][4].add_(0.25)
    fresh = run(None)[0]
    assert not th.equal(run(image)[0], fresh)
    prepare()
    assert th.equal(run(image)[0], fresh)
    # refused: no image, misaligned image, missing parameter
    head = (xs.data_ptr(), xs.shape[0], so.data_ptr(), L.ptr(order), xn.data_ptr(), xn.shape[0], no.data_ptr(), x_a.data_ptr(), N,
            L.ptr_array(ps[0]), L.ptr_array(ps[1]), 4, 64, 0.2)
    out = th.empty((N, 512), device=dev)
    assert lib.uavgnn_gatv2_hetero_fwd_image(*head, None, out.data_ptr(), 512, None, None, 3, st) == L.UAVGNN_EINVAL
    assert lib.uavgnn_gatv2_hetero_fwd_image(*head, image.data_ptr() + 4, out.data_ptr(), 512, None, None, 3, st) == L.UAVGNN_EUNSUPPORTED
    assert lib.uavgnn_gatv2_hetero_prepare(L.ptr_array(ps[0]), L.ptr_array(ps[1]), 4, 64, 0.2, None, st) == L.UAVGNN_EINVAL
    assert lib.uavgnn_gatv2_hetero_prepare(L.ptr_array(ps[0]), L.ptr_array(ps[1]), 2, 64, 0.2, image.data_ptr(), st) == L.UAVGNN_EUNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("key_size", [16, 32])
def test_rollout_weight_cache_of_the_learner_is_invalidated_by_every_parameter_change(monkeypatch, key_size):
    """MultiAgentQLearner.act keeps weight planes and the K1 parameter image between optimiser steps (ops.frozen_weights store
    owned by the learner).  Rollout -> update -> rollout with the cache gives the same actions / hidden states as the same
    sequence with the cache switched off; load_state_dict (version counters) and load_checkpoint are seen as well.
    key_size 32: msg + 2 key = 128 projection columns at 4096 rows - the one shape where TarMAC's STACKED projection weight (a
    `.data` view with its own version counter) goes through the bf16x3 GEMM and its plane cache (a stale hit there)."""
    import copy
    from uav_bs_ctrl_amd import ops
    import bench

    def episode(cache_on):
        monkeypatch.setattr(ops, "K1_IMAGE", cache_on)
        learner, batch = _small_learner_and_batch(B=512, n=8, M=20, T=2, seed=5, key_size=key_size)
        if not cache_on:       # no persistent store at all: every call rebuilds its planes
            monkeypatch.setattr(learner, "_rollout_planes", None)
        gen = th.Generator(device="cuda")
        gen.manual_seed(1)
        obs = bench.synth_batch_gpu(512, 8, 20, "env", th.device("cuda"), gen)
        h = learner.init_hidden(512)
        outs = []
        for _ in range(2):
            acts, h = learner.act(obs, h, 0.0)
            outs += [acts.clone(), h.clone()]
        if cache_on:
            assert any(k[0] == "k1img" for k in learner._rollout_planes) and len(learner._rollout_planes) < 16
        learner.update(batch)
        assert not cache_on or len(learner._rollout_planes) == 0
        acts, h = learner.act(obs, h, 0.0)
        outs += [acts.clone(), h.clone()]
        sd = copy.deepcopy(learner.policy_net.state_dict())
        for k in sd:
            sd[k] = sd[k] * 0.5
        learner.policy_net.load_state_dict(sd)        # behind the learner's back, but through torch: version counters
        acts, h = learner.act(obs, h, 0.0)
        outs += [acts.clone(), h.clone()]
        with th.no_grad():                            # an in-place edit of ONE member of the stacked projection weight
            dict(learner.policy_net.named_parameters())[[k for k in sd if k.endswith("f_que.weight")][0]].mul_(-3.0)
        acts, h = learner.act(obs, h, 0.0)
        outs += [acts.clone(), h.clone()]
        return outs
    a, b = episode(True), episode(False)
    for x, y in zip(a, b):
        assert th.equal(x, y)


@pytest.mark.gpu
def test_graphed_cycle_replay_equals_the_eager_cycle():
    """graphs.GraphedCycle: T act calls on stored graphs + one update, captured once; a replay moves the parameters exactly as the
    eager cycle does from the same state (the rollout's draws do not feed the update: it trains on the stored batch)."""
    import bench
    from uav_bs_ctrl_amd.graphs import GraphedCycle
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    dev = th.device("cuda")
    n, M, T, B = 4, 10, 4, 8
    th.manual_seed(3)
    env_info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=9, n_agents=n, episode_limit=T)
    lr = MultiAgentQLearner(env_info, bench.exp3_args("cuda"))
    batch = bench.make_sequence(B, n, M, T, "dense", dev, seed=5, distinct=2)
    h_row = lr.init_hidden(1)[:1].clone()
    hs = []

    def body():
        obs = [g.fresh() for g in batch["obs"]]
        fb = dict(batch, obs=obs, obs_all=batch["obs_all"].fresh(), obs_all_next=batch["obs_all_next"].fresh())
        h = h_row.expand(n * B, -1).contiguous()
        for t in range(T):
            _, h = lr.act(obs[t].fresh(), h, 0.0)
        hs.append(h)
        return lr.update(fb)

    cyc = GraphedCycle(lr, body)
    state = [t.clone() for t in (lr.flat.flat, lr.flat_target, lr.optimizer.m, lr.optimizer.v, lr.optimizer.hyper)]
    out = cyc()
    th.cuda.synchronize()
    got = [lr.flat.flat.clone(), lr.flat_target.clone(), float(out["LossQ"]), hs[-1].clone()]
    out2 = cyc()                                   # a second replay starts from the moved parameters
    th.cuda.synchronize()
    got2 = [lr.flat.flat.clone(), float(out2["LossQ"])]
    for dst, src in zip((lr.flat.flat, lr.flat_target, lr.optimizer.m, lr.optimizer.v, lr.optimizer.hyper), state):
        dst.copy_(src)
    lr.invalidate_weight_cache()
    ref = body()
    th.cuda.synchronize()
    assert float(ref["LossQ"]) == got[2]
    assert th.equal(lr.flat.flat, got[0]) and th.equal(lr.flat_target, got[1])
    assert th.equal(hs[-1], got[3])
    ref2 = body()
    th.cuda.synchronize()
    assert float(ref2["LossQ"]) == got2[1] and th.equal(lr.flat.flat, got2[0])
    assert got2[1] != got[2]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(4096, 256, 768), (4100, 320, 256), (70, 128, 64)])
def test_gemm_bf16x3_tile_variants_are_bit_identical(M, N, K):
    """include/uavgnn.h: the tile variants of uavgnn_gemm_nt_x3 (256 x 128 eight waves, + interleaved staging, 128 x 128 and 64 x 128
    four waves - the one `ops.gemm_x3` picks for batches of a few thousand rows): bit-identical within the eight-wave pair and
    within the four-wave pair, every one of them inside the fp32 error bound."""
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    gen = th.Generator().manual_seed(M + K)
    a = th.randn(M, K, generator=gen).cuda()
    W = (0.1 * th.randn(N, K, generator=gen)).cuda()
    bias = th.randn(N, generator=gen).cuda()
    planes = th.empty(6 * N * K, dtype=th.uint8, device="cuda")
    L.check(lib.uavgnn_split_bf16x3(W.data_ptr(), K, N, K, 0, planes.data_ptr(), L.stream()), "split")
    y0 = th.randn(M, N, generator=gen).cuda()
    outs = []
    for flags in (0, 4, 8, 16):
        for epi in (0, 1, 2, 3):
            y = y0.clone()
            L.check(lib.uavgnn_gemm_nt_x3(a.data_ptr(), K, M, K, planes.data_ptr(), N, bias.data_ptr(), y.data_ptr(), N, epi | flags,
                                          L.stream()), f"gemm flags {flags} epilogue {epi}")
            outs.append((flags, epi, y))
    th.cuda.synchronize()
    ref = a.double() @ W.double().t() + bias.double()
    scale = a.double().abs() @ W.double().abs().t() + bias.double().abs()
    # the eight-wave kernels walk a slice half by half, the four-wave kernels term by term: two accumulation orders, each shared by
    # its two variants, both inside the fp32 bound
    for group in ((0, 4), (8, 16)):
        base = {epi: y for f, epi, y in outs if f == group[0]}
        assert float(((base[0].double() - ref).abs() / scale).max()) < 6e-7
        for f, epi, y in outs:
            if f in group:
                assert th.equal(y, base[epi]), f"variant {f}, epilogue {epi}: differs from variant {group[0]}"


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,A", [(1, 64, 1), (17, 128, 9), (4099, 256, 9), (32768, 256, 16), (100, 256, 5)])
def test_head_kernel_vs_float64(N, H, A):
    """csrc/head.hip (the Q head, gnn_agents.py:56: nn.Linear(H, n_actions)) against the float64 product: ragged row tiles, every
    supported width, padded row strides of h and W, the fp32 error bound of a K = H accumulation, untouched neighbours."""
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    gen = th.Generator().manual_seed(N + H + A)
    h_full = th.randn(N, H + 4, generator=gen).cuda()
    W_full = (0.2 * th.randn(A, H + 8, generator=gen)).cuda()
    h, W = h_full[:, :H], W_full[:, :H]
    b = th.randn(A, generator=gen).cuda()
    assert lib.uavgnn_head_supported(H, A) == 1
    q = th.full((N, A + 3), 7.0, device="cuda")
    L.check(lib.uavgnn_head_fwd(h.data_ptr(), h.stride(0), N, H, W.data_ptr(), W.stride(0), b.data_ptr(), A, q.data_ptr(), A + 3,
                                L.stream()), "uavgnn_head_fwd")
    th.cuda.synchronize()
    ref = h.double() @ W.double().t() + b.double()
    scale = h.double().abs() @ W.double().abs().t() + b.double().abs()
    err = float(((q[:, :A].double() - ref).abs() / scale).max())
    err_vendor = float(((th.addmm(b, h, W.t()).double() - ref).abs() / scale).max())
    assert err < 4e-7, (err, err_vendor)
    assert bool((q[:, A:] == 7.0).all()), "columns past n_actions were written"
    q2 = th.empty(N, A, device="cuda")
    L.check(lib.uavgnn_head_fwd(h.data_ptr(), h.stride(0), N, H, W.data_ptr(), W.stride(0), b.data_ptr(), A, q2.data_ptr(), A, L.stream()), "again")
    assert th.equal(q2, q[:, :A].contiguous()), "not bit-reproducible"
    assert lib.uavgnn_head_supported(512, 9) == 0 and lib.uavgnn_head_supported(256, 17) == 0
    assert lib.uavgnn_head_fwd(h.data_ptr() + 4, h.stride(0), N, H, W.data_ptr(), W.stride(0), b.data_ptr(), A, q2.data_ptr(), A,
                               L.stream()) == L.UAVGNN_EUNSUPPORTED       # a misaligned operand is refused, not mis-read


@pytest.mark.gpu
@pytest.mark.parametrize("M,K1,K2,N", [(16384, 768, 96, 256), (33001, 64, 32, 128), (16384, 32, 768, 384)])
def test_gemm_bf16x3_two_sources(M, K1, K2, N):
    """uavgnn_gemm_nt_x3_cat: the contraction over [X || X2] from two buffers (the GRU backward's d x = d_gi W_ih[:, :H] + d_proj
    Wp[:, :H] as one product) equals the float64 sum of the two products within the fp32 bound, and - bit for bit - the
    single-source kernel on the concatenated copy; strided operands, ragged rows; refused with the small-tile variants."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    lib = L.lib()
    gen = th.Generator().manual_seed(M + K1 + K2)
    a1 = th.randn(M, K1 + 4, generator=gen).cuda()[:, :K1]
    a2 = th.randn(M, K2 + 8, generator=gen).cuda()[:, :K2]
    W1 = (0.1 * th.randn(K1, N + 4, generator=gen)).cuda()[:, :N]
    W2 = (0.1 * th.randn(K2, N, generator=gen)).cuda()
    assert ops.gemm_x3_cat_supported(a1, a2, N)
    out = th.full((M, N + 4), 3.0, device="cuda")
    with ops.frozen_weights():
        ops.gemm_x3_cat(a1, a2, W1, W2, out[:, :N])
        again = ops.gemm_x3_cat(a1, a2, W1, W2, th.empty(M, N, device="cuda"))
    th.cuda.synchronize()
    ref = a1.double() @ W1.double() + a2.double() @ W2.double()
    scale = a1.double().abs() @ W1.double().abs() + a2.double().abs() @ W2.double().abs()
    assert float(((out[:, :N].double() - ref).abs() / scale).max()) < 6e-7
    assert bool((out[:, N:] == 3.0).all()) and th.equal(again, out[:, :N])
    one = ops.gemm_x3(th.cat((a1, a2), 1), th.cat((W1, W2), 0), True)
    assert th.equal(one, again), "two sources and the concatenated copy differ"
    planes = th.empty(6 * (K1 + K2) * N, dtype=th.uint8, device="cuda")
    Wc = th.cat((W1, W2), 0)
    L.check(lib.uavgnn_split_bf16x3(Wc.data_ptr(), N, K1 + K2, N, 1, planes.data_ptr(), L.stream()), "split")
    y = th.empty(M, N, device="cuda")
    for flag in (8, 16):
        assert lib.uavgnn_gemm_nt_x3_cat(a1.data_ptr(), a1.stride(0), K1, a2.data_ptr(), a2.stride(0), M, K1 + K2, planes.data_ptr(), N,
                                         None, y.data_ptr(), N, flag, L.stream()) == L.UAVGNN_EUNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("n,C", [(4096, 256), (5003, 64), (300000, 256), (7, 4)])
def test_relu_backward_fused_with_the_bias_gradient(n, C):
    """csrc/colsum.hip uavgnn_relu_bwd_colsum: out = dy where y > 0 else 0 and its row-blocked column sums in one pass, against
    torch's threshold_backward + float64 column sums; strided operands, ragged row blocks, in place; and ops._LinearReLU's backward
    with the fused pass equals the unfused one."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    lib = L.lib()
    gen = th.Generator().manual_seed(n + C)
    dy = th.randn(n, C + 4, generator=gen).cuda()[:, :C]
    y = th.relu(th.randn(n, C + 8, generator=gen)).cuda()[:, :C]
    S = ops._row_blocks(n)
    out = th.full((n, C + 4), 9.0, device="cuda")
    acc = th.ones(S, C, device="cuda")
    L.check(lib.uavgnn_relu_bwd_colsum(dy.data_ptr(), dy.stride(0), y.data_ptr(), y.stride(0), out.data_ptr(), C + 4, n, C, acc.data_ptr(), S,
                                       L.stream()), "uavgnn_relu_bwd_colsum")
    ref = th.ops.aten.threshold_backward(dy.contiguous(), y.contiguous(), 0.0)
    assert th.equal(out[:, :C], ref) and bool((out[:, C:] == 9.0).all())
    want = ref.double().sum(0) + S
    got = acc.double().sum(0)
    assert float((got - want).abs().max()) <= 1e-5 * float(ref.double().abs().sum(0).max() + 1.0)
    inplace = dy.contiguous().clone()
    acc2 = th.zeros(S, C, device="cuda")
    L.check(lib.uavgnn_relu_bwd_colsum(inplace.data_ptr(), C, y.data_ptr(), y.stride(0), inplace.data_ptr(), C, n, C, acc2.data_ptr(), S,
                                       L.stream()), "in place")
    assert th.equal(inplace, ref)
    if C >= 64 and n >= 4096:
        x = th.randn(n, 32, generator=gen).cuda().requires_grad_()
        W = (0.2 * th.randn(C, 32, generator=gen)).cuda().requires_grad_()
        b = th.randn(C, generator=gen).cuda().requires_grad_()
        g = th.randn(n, C, generator=gen).cuda()
        grads = {}
        for fused in (True, False):
            ops.RELU_BWD_FUSED = fused
            try:
                grads[fused] = th.autograd.grad(ops.linear_relu(x, W, b), (x, W, b), g)
            finally:
                ops.RELU_BWD_FUSED = True
        assert th.equal(grads[True][0], grads[False][0]) and th.equal(grads[True][1], grads[False][1])
        assert_close(grads[True][2], grads[False][2], 1e-5, "db", floor=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,head", [(4096, 256, True), (1000, 256, False), (33, 64, True), (32768, 256, True), (513, 128, False)])
def test_gate_gradient_kernel_column_sums(N, H, head):
    """uavgnn_gru_gates_bwd_fused_sums: the same d_gi / d_gh / d_h bits as uavgnn_gru_gates_bwd_fused[_head], and per-workgroup column
    sums whose total is the bias gradient of the cell - d_r | d_z | d_n (input side) | d_n (hidden side) - to fp32 accuracy against
    float64 sums of the gate gradients; bit-reproducible; H whose quarter does not divide 256 is refused through _sum_rows."""
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    gen = th.Generator().manual_seed(N + H)
    pre = th.randn(N, 4 * H, generator=gen).cuda()
    h = th.randn(N, H, generator=gen).cuda()
    dho = th.randn(N, H, generator=gen).cuda()
    A = 9
    dq = th.randn(N, A, generator=gen).cuda() if head else None
    W_out = (0.3 * th.randn(A, H, generator=gen)).cuda() if head else None
    G = lib.uavgnn_gru_gates_bwd_sum_rows(N, H)
    assert G > 0 and lib.uavgnn_gru_gates_bwd_sum_rows(N, 24) == 0       # 24 / 4 = 6 does not divide 256

    def run(with_sums):
        d_gi, d_gh, d_h = (th.full((N, 3 * H), float("nan"), device="cuda"), th.full((N, 3 * H), float("nan"), device="cuda"),
                           th.full((N, H), float("nan"), device="cuda"))
        sums = th.full((G, 4 * H), float("nan"), device="cuda") if with_sums else None
        if with_sums:
            rc = lib.uavgnn_gru_gates_bwd_fused_sums(pre.data_ptr(), h.data_ptr(), dho.data_ptr(), L.ptr(dq), A if head else 0, L.ptr(W_out),
                                                     N, H, d_gi.data_ptr(), d_gh.data_ptr(), d_h.data_ptr(), sums.data_ptr(), L.stream())
        elif head:
            rc = lib.uavgnn_gru_gates_bwd_fused_head(pre.data_ptr(), h.data_ptr(), dho.data_ptr(), dq.data_ptr(), A, W_out.data_ptr(), N, H,
                                                     d_gi.data_ptr(), d_gh.data_ptr(), d_h.data_ptr(), L.stream())
        else:
            rc = lib.uavgnn_gru_gates_bwd_fused(pre.data_ptr(), h.data_ptr(), dho.data_ptr(), N, H, d_gi.data_ptr(), d_gh.data_ptr(),
                                                d_h.data_ptr(), L.stream())
        L.check(rc, "gate gradients")
        th.cuda.synchronize()
        return d_gi, d_gh, d_h, sums

    a = run(False)
    b = run(True)
    for x, y in zip(a[:3], b[:3]):
        assert th.equal(x, y)
    sums = b[3]
    assert not bool(th.isnan(sums).any())
    tot = sums.double().sum(0)
    want = th.cat((a[0].double().sum(0), a[1][:, 2 * H:].double().sum(0)))
    scale = th.cat((a[0].double().abs().sum(0), a[1][:, 2 * H:].double().abs().sum(0))) + 1e-30
    assert float(((tot - want).abs() / scale).max()) < 2e-6
    assert th.equal(run(True)[3], sums), "not bit-reproducible"


@pytest.mark.gpu
def test_graphed_cycle_reports_the_loss_of_every_replay_across_device_synchronisation():
    """The LossQ a replayed whole-cycle graph hands back is the eager loss of the same update - also for replays behind a device
    synchronise, at a size (T B n = 204 800 terms) where torch's one-kernel full reduction to a scalar meets at a semaphore: with
    F.mse_loss the replays behind the first torch.cuda.synchronize() read back stale / partial values while the training step itself
    stayed right (learner._mse is a two-stage sum for that reason; tools/gc_loss_probe.py)."""
    import bench
    from uav_bs_ctrl_amd.graphs import GraphedCycle
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    dev = th.device("cuda")
    n, M, T, B = 4, 10, 50, 1024
    batch = bench.make_sequence(B, n, M, T, "dense", dev, seed=11, distinct=2)
    env_info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=9, n_agents=n, episode_limit=T)

    def make():
        th.manual_seed(5)
        lr = MultiAgentQLearner(env_info, bench.exp3_args("cuda"))
        h_row = lr.init_hidden(1)[:1].clone()

        def body():
            obs = [g.fresh() for g in batch["obs"]]
            fb = dict(batch, obs=obs, obs_all=batch["obs_all"].fresh(), obs_all_next=batch["obs_all_next"].fresh())
            h = h_row.expand(n * B, -1).contiguous()
            for t in range(3):                       # a short rollout in front of the update: the graph is a cycle, not just an update
                _, h = lr.act(obs[t].fresh(), h, 0.05)
            return lr.update(fb)
        return lr, body

    lr_g, body_g = make()
    lr_e, body_e = make()
    cyc = GraphedCycle(lr_g, body_g)
    want = []
    for _ in range(6):
        want.append(float(body_e()["LossQ"]))
    got = []
    for k in range(6):
        got.append(float(cyc()["LossQ"]))            # nothing but the read between two replays
        if k == 2:
            th.cuda.synchronize()
    assert got == want, (got, want)
    assert th.equal(lr_g.flat.flat, lr_e.flat.flat)


# ---------------------------------------------------------------------------------------------------------------------
# Round 6: the oracle on the path the benchmark times (learner.update at exp3 sizes with production kernel dispatch)
# (helpers: tests/gpu_util.py)

@pytest.mark.parametrize("dist", ["env", "dense"])
@pytest.mark.parametrize("label,B,n,M,T", UPDATE_CASES)
def test_learner_update_at_exp3_sizes_vs_oracle(label, B, n, M, T, dist, monkeypatch):
    """Row L where its production kernels dispatch (learner.py:110-157 of the reference): ``MultiAgentQLearner.accumulate`` on
    bench.py's sampled batches - time-batched encoder through ``_TimeSplit``, ``WeightGradSink`` staging, the f16x2 cell
    (>= 1024 rows) behind the fused message kernel that hands it the row maxima, the head kernel, the gate-gradient kernel with the folded head gradient and column
    sums, and at >= 4096 rows ``gemm_x3`` / ``gemm_nt_x3_cat`` / ``relu_bwd_colsum`` - against ``R.madrqn_loss`` in float64
    (float32 for the error floor): LossQ, every Q value, and EVERY slice of the flat gradient buffer under ``grad_close``.
    Then once more through the captured ``GraphedUpdate``."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    learner, batch = _exp3_learner_and_sequence(B, n, M, T, dist, seed=3)
    N = B * n
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    staged = []
    orig_end = ops.WeightGradSink.end_sequence

    def end_spy(self):
        staged.append(0 if self.seq is None else len(self.seq.bwd_steps))
        return orig_end(self)
    monkeypatch.setattr(ops.WeightGradSink, "end_sequence", end_spy)
    if N >= 16384:
        # the benchmark's sequence has 1.67 M time-batched rows: its weight gradients run on csrc/gemm_tn_h2.hip (taken from 2^18 rows).  This
        # case has (T + 1) N = 114 688: the threshold is lowered so that the SAME kernels reduce the sequence here (dW_ih, dW_hh, dW_aggr,
        # and dWp with swapped operands, column bounds from the per-step row maxima)
        monkeypatch.setattr(ops, "GEMM_TN_MIN_ROWS", 4096)
    out = learner.accumulate(dict(batch))
    flat = learner.grads.flat.clone()
    monkeypatch.undo()
    # --- the dispatch is the benchmark's
    called = set(spy.names)
    if N >= 16384:
        tn_shapes = {(a[2], a[5]) for nm, a in spy.calls if nm == "uavgnn_gemm_tn_h2"}      # (Mo, Ko) of every weight-gradient launch
        assert {(768, 320), (768, 256), (256, 96), (256, 512)} <= tn_shapes, tn_shapes
    assert max(staged) == T + 1, f"time-batched staging not taken: {staged}"
    expect = {"uavgnn_gatv2_hetero_fwd_image", "uavgnn_gru_cell_fwd_h2", "uavgnn_tarmac_msg_fwd_rowmax", "uavgnn_head_fwd",
              "uavgnn_gru_gates_bwd_fused_sums", "uavgnn_talk_attn_env_bwd", "uavgnn_gatv2_bwd", "uavgnn_colsum_acc",
              "uavgnn_relu_bwd_colsum"}
    # K1 leaves the row maxima of its output - and f_aggr's forward runs on the f16x2 kernel instead of bf16x3 - on time-batched launches of
    # more than 2^17 destinations and on any launch from 16 384 destinations whose `seen` relation is dense (ops.K1_ROWMAX_DENSE_DEG)
    k1_rowmax = (T + 1) * N > (1 << 17) or (dist == "dense" and M >= 16 and (T + 1) * N >= 16384)    # (D-dense: every agent sees ~M GTs)
    if k1_rowmax:
        expect |= {"uavgnn_gatv2_hetero_fwd_rowmax", "uavgnn_gemm_nt_h2"}
        expect -= {"uavgnn_gatv2_hetero_fwd_image"}
    if N >= 4096:       # f_aggr on the bf16x3 kernel (f16x2 behind a K1 launch with row maxima); its input gradient over the (T + 1) N time-batched rows on the f16x2 kernel
        expect |= {"uavgnn_gemm_nt_h2", "uavgnn_relu_bwd_colsum_rowmax"} | (set() if k1_rowmax else {"uavgnn_gemm_nt_x3"})
        expect -= {"uavgnn_relu_bwd_colsum"}
    if N >= 16384:      # d x of the recurrent step as ONE f16x2 product over [d_gi || d_proj] and d h += d_gh W_hh: from 128 tiles of 256 x 128
        expect |= {"uavgnn_gru_gates_bwd_fused_sums_rowmax", "uavgnn_gemm_nt_h2_rm2"}      # (d_proj's row maxima inside the d x launch)
        expect -= {"uavgnn_gru_gates_bwd_fused_sums"}
    assert expect <= called, f"{label}: production kernels not dispatched: {sorted(expect - called)}"
    # --- oracle, float64 (float32 for the error floor), at the branch the HIP path took (tests/gpu_util.py: _oracle_at_gpu_branch)
    l64, _, g64, l32, g32 = _oracle_at_gpu_branch(learner, batch, out["QVals"].detach().cpu(), T, N, f"{label} {dist}")
    assert_close(out["LossQ"], l64, 1e-5, f"{label} {dist}: LossQ")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        got = flat[o:o + prm.numel()].view_as(prm)
        grad_close(got, g64[k], f"learner.accumulate exp3 {label} {dist}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)
    # --- the same accumulate as ONE replayed hipGraph (what `bench.py --graphed-cycle` and a production loop replay): the flat
    # gradient buffer the replay leaves is the eager one, i.e. the oracle comparison above covers the graphed path too
    from uav_bs_ctrl_amd.graphs import GraphedCycle
    if N >= 16384:
        monkeypatch.setattr(ops, "GEMM_TN_MIN_ROWS", 4096)      # (the dispatch of the eager run above)
    cyc = GraphedCycle(learner, lambda: learner.accumulate(batch))
    learner.grads.flat.fill_(float("nan"))
    out_g = cyc()
    th.cuda.synchronize()
    assert_close(out_g["LossQ"], l64, 1e-5, f"{label} {dist}: LossQ (graph replay)")
    assert th.equal(learner.grads.flat, flat), f"{label} {dist}: graph replay of accumulate differs from the eager run"


def test_drqn_twin_at_exp1_hidden_size_vs_oracle():
    """BASELINE config 1's model (algos/drqn/agents/gnn_agents.py:9-30) at its production width: H = 256, 4 heads, 1 agent x 20
    GTs, B = 32 - forward and every gradient against the float64 / float32 oracle (the golden fixture runs it at H = 32)."""
    import types
    from uav_bs_ctrl_amd.agents import REGISTRY
    B, M, H = 32, 20, 256
    th.manual_seed(5)
    net = REGISTRY["drqn_gnn"](dict(agent=2, gt=4), 9, types.SimpleNamespace(hidden_size=H, n_heads=4))
    with th.no_grad():
        for prm in net.parameters():
            if prm.dim() == 1:
                prm.add_(0.05 * th.randn_like(prm))
    p64 = {k: v.detach().double().clone() for k, v in net.state_dict().items()}
    g = synth_graph(B, 1, M, "dense", seed=11)
    g = {k: g[k] for k in ("x_a", "x_gt", "seen_off")}
    gen = th.Generator().manual_seed(12)
    h = 0.5 * th.randn(B, H, generator=gen)
    wq, wh = th.randn(B, 9, generator=gen), th.randn(B, H, generator=gen) / 16

    def oracle(dtype):
        pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p64.items()}
        gg = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g.items()}
        hh = h.detach().clone().to(dtype).requires_grad_(True)
        q, h2 = R.drqn_gnn_agent_forward(gg, hh, pp, 4)
        gr = th.autograd.grad(_loss(q, h2, wq.to(dtype), wh.to(dtype)), list(pp.values()) + [hh])
        return q, h2, dict(zip(list(pp) + ["__h__"], gr))
    q64, h64, g64 = oracle(th.float64)
    _, _, g32 = oracle(th.float32)
    net = net.cuda()
    hd = h.cuda().requires_grad_(True)
    q, h2 = net(to_batch(g), hd)
    assert_close(q, q64, 1e-5, "drqn H=256: q")
    assert_close(h2, h64, 1e-5, "drqn H=256: h'")
    _loss(q, h2, wq.cuda(), wh.cuda()).backward()
    grads = {k: prm.grad for k, prm in net.named_parameters()}
    grads["__h__"] = hd.grad
    for k, ref in g64.items():
        grad_close(grads[k], ref, f"drqn twin H=256 1x{M} B={B}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# Round 6: the GRU cell on the f16 matrix cores ("f16x2": exactly scaled two-term splits, three products per fp32 product)

def _cell_error_row(tag, out, ref):
    """max / mean |out - ref| / (|ref| + max|ref|): the measure of profiles/r06_h2_error_tables.txt"""
    e = (out.double().cpu() - ref).abs() / (ref.abs() + ref.abs().max())
    return dict(what=tag, max=float(e.max()), mean=float(e.mean()))


@pytest.mark.parametrize("N,K_in,H", [(4096, 320, 256), (1000, 320, 256), (130, 64, 64), (2049, 96, 128)])
def test_gru_cell_f16x2_vs_float64_and_the_other_cells(N, K_in, H):
    """csrc/gru_h2.hip (nn.GRUCell at gnn_agents.py:246) against float64: h' inside the 1e-5 parity rule, every gradient under
    grad_close (the backward reads the pre-activations this forward saved), and an error that is not above the bf16x3 cell's or the
    vendor fp32 GEMM path's on the same data (the condition under which `dtype f32` stands) - model-like operands."""
    import json
    import os
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    assert L.lib().uavgnn_gru_cell_h2_supported(K_in, H)
    gen = th.Generator().manual_seed(N + H + 1)
    cell = th.nn.GRUCell(K_in, H)
    with th.no_grad():
        for p in cell.parameters():
            p.copy_(0.3 * th.randn(p.shape, generator=gen))
    inp, h = th.relu(th.randn(N, K_in, generator=gen)) * 1.5, th.tanh(th.randn(N, H, generator=gen))
    w = th.randn(N, H, generator=gen)
    c64 = th.nn.GRUCell(K_in, H).double()
    c64.load_state_dict({k: v.double() for k, v in cell.state_dict().items()})
    i64, h64 = inp.double().requires_grad_(True), h.double().requires_grad_(True)
    ref = c64(i64, h64)
    gref = th.autograd.grad((ref * w.double()).sum(), [i64, h64] + list(c64.parameters()))
    i32, h32 = inp.clone().requires_grad_(True), h.clone().requires_grad_(True)
    g32 = th.autograd.grad((cell(i32, h32) * w).sum(), [i32, h32] + list(cell.parameters()))
    cell = cell.cuda()
    min_rows = ops.GRU_FUSED_MIN_ROWS
    ops.GRU_FUSED_MIN_ROWS = 0
    try:
        i_d, h_d = inp.cuda().requires_grad_(True), h.cuda().requires_grad_(True)
        rm = ops.row_absmax(i_d.detach(), h_d.detach())
        assert th.equal(rm.cpu(), th.maximum(inp.abs().max(1).values, h.abs().max(1).values))
        out = ops.gru_cell(i_d, h_d, cell, rowmax=rm)
        got = th.autograd.grad((out * w.cuda()).sum(), [i_d, h_d] + list(cell.parameters()))
        with th.no_grad():
            out_x3 = ops.gru_cell(inp.cuda(), h.cuda(), cell)
            out_ng = ops.gru_cell(inp.cuda(), h.cuda(), cell, rowmax=rm)
            ops.GRU_FUSED = False
            ops.GEMM_X3 = False
            out_vendor = ops.gru_cell(inp.cuda(), h.cuda(), cell)
    finally:
        ops.GRU_FUSED, ops.GEMM_X3, ops.GRU_FUSED_MIN_ROWS = True, True, min_rows
    assert th.equal(out_ng, out.detach()) and not th.equal(out_x3, out.detach()), "the f16x2 cell did not run"
    assert_close(out, ref, 1e-5, "h' (f16x2 cell)")
    for a, b, b32, nm in zip(got, gref, g32, ["d_inp", "d_h", "dW_ih", "dW_hh", "db_ih", "db_hh"]):
        grad_close(a, b, f"K4 f16x2 N={N} K={K_in} H={H}: {nm}", ref32=b32)
    rows = [_cell_error_row("f16x2", out.detach(), ref.detach()), _cell_error_row("bf16x3", out_x3, ref.detach()),
            _cell_error_row("vendor fp32 GEMMs + gates", out_vendor, ref.detach())]
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "gpurun_out", "h2_errors.jsonl"), "a") as f:
            f.write(json.dumps(dict(test="cell model-like", N=N, K_in=K_in, H=H, rows=rows)) + "\n")
    except OSError:
        pass
    # not above the other fp32-grade paths: 1.25 x covers the scatter between two roundings of the same size on 10^5..10^6 outputs
    assert rows[0]["mean"] <= 1.25 * max(rows[1]["mean"], rows[2]["mean"]), rows
    assert rows[0]["max"] <= 2.0 * max(rows[1]["max"], rows[2]["max"]), rows


@pytest.mark.parametrize("case", ["in-row range 2^+-30", "rows at 2^-100", "rows at 2^100", "one huge element per row", "zero rows"])
def test_gru_cell_f16x2_operand_range(case):
    """The f16x2 cell where its scaling is exercised: elements 2^60 apart inside one row (the small ones lose their low term to f16's
    exponent range - bounded by 2^-39 of the row maximum), whole rows near the ends of fp32's range (the scale exponent moves, nothing
    else), one dominant element per row, all-zero rows; float64 reference, error measured like every cell's and held to grad_close's
    rule against what ATen's fp32 cell delivers on the same data."""
    from uav_bs_ctrl_amd import ops
    N, K_in, H = 2048, 320, 256
    gen = th.Generator().manual_seed(21)
    cell = th.nn.GRUCell(K_in, H)
    c64 = th.nn.GRUCell(K_in, H).double()
    c64.load_state_dict({k: v.double() for k, v in cell.state_dict().items()})
    inp, h = th.randn(N, K_in, generator=gen), th.tanh(th.randn(N, H, generator=gen))
    if case == "in-row range 2^+-30":
        inp = inp * th.exp2(th.randint(-30, 31, (N, K_in), generator=gen).float())
    elif case == "rows at 2^-100":
        inp, h = inp * 2.0 ** -100, h * 2.0 ** -100
    elif case == "rows at 2^100":
        inp = inp * 2.0 ** 100
    elif case == "one huge element per row":
        inp[th.arange(N), th.randint(0, K_in, (N,), generator=gen)] = 3.0e4
    elif case == "zero rows":
        inp[::3] = 0.0
        h[::3] = 0.0
    with th.no_grad():
        ref = c64(inp.double(), h.double())
        ref32 = cell(inp, h)
        cell = cell.cuda()
        rm = ops.row_absmax(inp.cuda(), h.cuda())
        ops.KERNEL_TIMER.reset(enabled=True)
        out = ops.gru_cell(inp.cuda(), h.cuda(), cell, rowmax=rm)
        work = ops.KERNEL_TIMER.summary()["gru_cell_fwd"]["work"]
        ops.KERNEL_TIMER.reset(enabled=False)
    assert work and work[-1][3] == "f16x2", "the f16x2 cell did not run"
    assert bool(th.isfinite(out).all())
    grad_close(out, ref, f"K4 f16x2 operand range ({case}): h'", ref32=ref32)


def test_gru_cell_f16x2_non_finite_rows_and_too_small_bounds_yield_nan_never_a_number():
    """The documented contract of csrc/gru_h2.hip: a row of the cell's operand that holds Inf / NaN gives NaN outputs for THAT agent
    only, and a caller's row bound that is too small (f16 overflow) gives NaN as well - never a finite wrong value."""
    from uav_bs_ctrl_amd import ops
    N, K_in, H = 1024, 320, 256
    gen = th.Generator().manual_seed(22)
    cell = th.nn.GRUCell(K_in, H).cuda()
    inp, h = th.randn(N, K_in, generator=gen).cuda(), th.tanh(th.randn(N, H, generator=gen)).cuda()
    inp[5, 17] = float("inf")
    inp[9, 300] = float("nan")
    h[11, 3] = -float("inf")
    with th.no_grad():
        rm = ops.row_absmax(inp, h)
        assert bool(th.isinf(rm[[5, 9, 11]]).all())
        out = ops.gru_cell(inp, h, cell, rowmax=rm)
        clean = th.ones(N, dtype=th.bool, device="cuda")
        clean[[5, 9, 11]] = False
        assert bool(th.isnan(out[~clean]).all()) and bool(th.isfinite(out[clean]).all())
        good_in, h = th.randn(N, K_in, generator=gen).cuda() * 100.0, th.tanh(th.randn(N, H, generator=gen)).cuda()
        rm2 = ops.row_absmax(good_in, h)
        rm2[7] = rm2[7] * 2.0 ** -8            # a bound 256 x too small: the row's largest elements overflow f16
        out2 = ops.gru_cell(good_in, h, cell, rowmax=rm2)
        assert bool(th.isnan(out2[7]).any()) and bool(th.isfinite(out2[th.arange(N, device="cuda") != 7]).all())


@pytest.mark.parametrize("train", [False, True])
def test_tarmac_step_on_the_f16x2_cell_equals_the_bf16x3_step_and_the_message_kernel_hands_over_the_row_maxima(train, monkeypatch):
    """ops.tarmac_step at exp3 sizes: the fused message launch writes max(|x|, |c|, |h|) per agent (checked against torch), the cell
    behind it runs csrc/gru_h2.hip, and q / h' (and, training, every gradient the step returns) equal the bf16x3 step's to 1e-5."""
    from uav_bs_ctrl_amd import ops
    net = agent_from_params(default_init_params(EXP3, seed=4), EXP3)
    g = to_batch(synth_graph(256, 8, 20, "env", seed=5))
    N = 256 * 8
    gen = th.Generator().manual_seed(6)
    x = th.relu(th.randn(N, 256, generator=gen)).cuda()
    h = th.tanh(th.randn(N, 256, generator=gen)).cuda()
    seen = {}
    orig = ops._gru_cell_launch

    def spy(*a, **k):
        if k.get("rowmax") is not None:
            inp2 = k.get("inp2")
            pieces = [a[0]] + ([inp2] if inp2 is not None else []) + [a[1]]
            seen["rowmax"], seen["want"] = k["rowmax"].clone(), th.cat([p.abs().max(1, keepdim=True).values for p in pieces], 1).max(1).values
        return orig(*a, **k)
    monkeypatch.setattr(ops, "_gru_cell_launch", spy)

    def run(h2):
        monkeypatch.setattr(ops, "GRU_H2", h2)
        xx, hh = x.clone().requires_grad_(train), h.clone().requires_grad_(train)
        with th.enable_grad() if train else th.no_grad():
            q, hn = net._tarmac_step(g.fresh(), xx, hh)       # the agent's own call of ops.tarmac_step (gnn_agents.py:351)
            grads = ()
            if train:
                params = [p for p in list(net.f_comm.parameters()) + list(net.f_out.parameters())]
                grads = th.autograd.grad((q * q).sum() + hn.sum(), [xx, hh] + params, allow_unused=True)
        return q.detach(), hn.detach(), grads
    q1, h1, g1 = run(True)
    assert "rowmax" in seen, "the f16x2 cell was not dispatched"
    assert th.equal(seen["rowmax"], seen["want"]), "row maxima of the message kernel differ from max(|x|, |c|, |h|)"
    seen.clear()
    q0, h0, g0 = run(False)
    assert "rowmax" not in seen
    assert_close(q1, q0, 1e-5, "q: f16x2 vs bf16x3 step")
    assert_close(h1, h0, 1e-5, "h': f16x2 vs bf16x3 step")
    scale = max([float(b.abs().max()) for b in g0 if b is not None] + [0.0])
    for i, (a, b) in enumerate(zip(g1, g0)):
        if a is not None:     # (floor: analytically zero gradients - d f_sign.bias - are rounding noise on both sides)
            assert_close(a, b, 2e-5, f"gradient {i}: f16x2 vs bf16x3 step", floor=1e-6 * scale)


@pytest.mark.parametrize("M,K1,K2,N,acc,relu,transpose", [(16384, 768, 0, 256, True, False, True), (16640, 768, 96, 256, False, False, True),
                                                          (33001, 256, 0, 512, False, True, False), (33000, 64, 32, 128, True, True, True)])
def test_gemm_f16x2_vs_float64_and_the_other_gemms(M, K1, K2, N, acc, relu, transpose):
    """csrc/gemm_h2.hip against float64: one and two sources, accumulate / ReLU epilogues, both weight orientations, ragged row
    tiles; error measured like test_gemm_bf16x3_vs_float64 (|err| / sum_k |a b|) and held to the bf16x3 kernel's and the vendor fp32
    GEMM's on the same data (gradient-like operands: rows whose magnitudes span six orders)."""
    import json
    import os
    from uav_bs_ctrl_amd import ops
    gen = th.Generator().manual_seed(M + N + K1)
    K = K1 + K2
    a = (th.randn(M, K, generator=gen) * th.exp2(th.randint(-20, 1, (M, 1), generator=gen).float())).cuda()
    W = (0.1 * th.randn(K, N, generator=gen)).cuda() if transpose else (0.1 * th.randn(N, K, generator=gen)).cuda()
    bias = None if transpose else (0.1 * th.randn(N, generator=gen)).cuda()
    y0 = (1e-3 * th.randn(M, N, generator=gen)).cuda() if acc else None
    B64 = (W.double() if transpose else W.double().t())            # [K, N]
    ref = a.double() @ B64
    den = a.double().abs() @ B64.abs()
    if bias is not None:
        ref, den = ref + bias.double(), den + bias.double().abs()
    if acc:
        ref, den = ref + y0.double(), den + y0.double().abs()
    if relu:
        ref = ref.clamp_min(0)
    a1, a2 = (a[:, :K1].contiguous(), a[:, K1:].contiguous()) if K2 else (a, None)
    rm1 = ops.row_absmax(a1)
    rm2 = ops.row_absmax(a2) if K2 else None
    assert ops.gemm_h2_supported(a1, N, K)
    if K2:
        out = ops.gemm_h2(a1, W[:K1], rm1, True, out=y0.clone() if acc else None, accumulate=acc, relu=relu, a2=a2, W2=W[K1:], rowmax2=rm2)
    else:
        out = ops.gemm_h2(a1, W, rm1, transpose, bias=bias, out=y0.clone() if acc else None, accumulate=acc, relu=relu)
    x3 = ops.gemm_x3(a, W, transpose, bias=bias, out=y0.clone() if acc else None, accumulate=acc, relu=relu)
    vend = a @ (W if transpose else W.t())
    if bias is not None:
        vend = vend + bias
    if acc:
        vend = vend + y0
    if relu:
        vend = vend.clamp_min(0)
    rows = []
    for tag, o in (("f16x2", out), ("bf16x3", x3), ("vendor fp32", vend)):
        e = (o.double() - ref).abs() / den.clamp_min(1e-300)
        e = e[den > 0]
        rows.append(dict(what=tag, max=float(e.max()), mean=float(e.mean())))
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "gpurun_out", "h2_errors.jsonl"), "a") as f:
            f.write(json.dumps(dict(test="gemm", M=M, K1=K1, K2=K2, N=N, acc=acc, relu=relu, rows=rows)) + "\n")
    except OSError:
        pass
    assert rows[0]["max"] < 4e-7 and rows[0]["mean"] < 4e-8, rows          # the absolute bar of test_gemm_bf16x3_vs_float64
    assert rows[0]["mean"] <= 1.25 * max(rows[1]["mean"], rows[2]["mean"]), rows
    assert rows[0]["max"] <= 2.0 * max(rows[1]["max"], rows[2]["max"]), rows


@pytest.mark.parametrize("M,K1,K2,N", [(33000, 768, 96, 256), (16385, 64, 32, 512), (65536, 256, 160, 128)])
def test_gemm_f16x2_takes_the_row_maxima_of_its_second_source_itself(M, K1, K2, N):
    """uavgnn_gemm_nt_h2_rm2: the row maxima of the second source taken inside the launch (d_proj of the recurrent step: no producer bounds
    it) - the product is bit-identical to the launch that is handed uavgnn_row_absmax(X2), the maxima it writes ARE uavgnn_row_absmax(X2)
    (rows past the last full 256-row block, a row holding Inf and one holding NaN included: Inf there, and only there), accumulate mode."""
    from uav_bs_ctrl_amd import ops
    gen = th.Generator().manual_seed(M + K2)
    a = (th.randn(M, K1, generator=gen) * 0.3).cuda()
    a2 = (th.randn(M, K2, generator=gen) * th.exp2(th.randint(-20, 6, (M, 1), generator=gen).float())).cuda()
    a2[5, 3], a2[M - 1, K2 - 1] = float("inf"), float("nan")
    W, W2 = (th.randn(K1, N, generator=gen) / K1 ** 0.5).cuda(), (th.randn(K2, N, generator=gen) / K2 ** 0.5).cuda()
    rm = ops.row_absmax(a)
    rm2 = ops.row_absmax(a2)
    assert th.equal(rm2, a2.abs().amax(1).nan_to_num(nan=float("inf"), posinf=float("inf")))
    assert ops.gemm_h2_supported(a, N, K1 + K2)
    with ops.frozen_weights():
        ref = ops.gemm_h2(a, W, rm, True, a2=a2, W2=W2, rowmax2=rm2)
        out_rm = th.full((M,), -1.0, device="cuda")
        got = ops.gemm_h2(a, W, rm, True, a2=a2, W2=W2, rowmax2_out=out_rm)
        th.cuda.synchronize()
        assert th.equal(out_rm, rm2)
        assert th.equal(got.isnan(), ref.isnan()) and th.equal(got.nan_to_num(nan=0.0), ref.nan_to_num(nan=0.0))
        assert bool(got[5].isnan().all()) and bool(got[M - 1].isnan().all()) and not bool(got[6:M - 1].isnan().any())
        y0 = th.randn(M, N, generator=gen).cuda()
        acc_ref, acc_got = y0.clone(), y0.clone()
        ops.gemm_h2(a, W, rm, True, out=acc_ref, accumulate=True, a2=a2, W2=W2, rowmax2=rm2)
        ops.gemm_h2(a, W, rm, True, out=acc_got, accumulate=True, a2=a2, W2=W2, rowmax2_out=th.empty(M, device="cuda"))
        assert th.equal(acc_got.nan_to_num(nan=0.0), acc_ref.nan_to_num(nan=0.0))


def test_row_maxima_of_the_gate_gradient_and_relu_backward_kernels_are_exact():
    """uavgnn_gru_gates_bwd_fused_sums_rowmax / uavgnn_relu_bwd_colsum_rowmax: same outputs as the kernels without the row maxima, bit
    for bit, and row_absmax == max |.| over the rows they wrote."""
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    N, H, A = 5000, 256, 9
    gen = th.Generator().manual_seed(31)
    pre, h, dh = (th.randn(N, 4 * H, generator=gen).cuda(), th.tanh(th.randn(N, H, generator=gen)).cuda(), th.randn(N, H, generator=gen).cuda())
    dq, Wo = th.randn(N, A, generator=gen).cuda(), th.randn(A, H, generator=gen).cuda()
    G = lib.uavgnn_gru_gates_bwd_sum_rows(N, H)
    outs = []
    for rm in (False, True):
        d_gi, d_gh, d_h = th.empty(N, 3 * H, device="cuda"), th.empty(N, 3 * H, device="cuda"), th.empty(N, H, device="cuda")
        sums, rowmax = th.empty(G, 4 * H, device="cuda"), th.full((N,), -1.0, device="cuda")
        args = (pre.data_ptr(), h.data_ptr(), dh.data_ptr(), dq.data_ptr(), A, Wo.data_ptr(), N, H, d_gi.data_ptr(), d_gh.data_ptr(),
                d_h.data_ptr(), sums.data_ptr())
        if rm:
            L.check(lib.uavgnn_gru_gates_bwd_fused_sums_rowmax(*args, rowmax.data_ptr(), L.stream()), "rowmax")
        else:
            L.check(lib.uavgnn_gru_gates_bwd_fused_sums(*args, L.stream()), "plain")
        outs.append((d_gi, d_gh, d_h, sums, rowmax))
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert th.equal(a, b)
    assert th.equal(outs[1][4], th.maximum(outs[1][0].abs().max(1).values, outs[1][1].abs().max(1).values))
    assert lib.uavgnn_gru_gates_bwd_fused_sums_rowmax(pre.data_ptr(), h.data_ptr(), dh.data_ptr(), None, 0, None, 64, 128, d_gi.data_ptr(),
                                                      d_gh.data_ptr(), d_h.data_ptr(), sums.data_ptr(), rowmax.data_ptr(), L.stream()) == L.UAVGNN_EUNSUPPORTED
    n, C, S = 5003, 256, 8
    dy, y = th.randn(n, C, generator=gen).cuda(), th.randn(n, C, generator=gen).cuda()
    o0, o1 = th.empty(n, C, device="cuda"), th.empty(n, C, device="cuda")
    p0, p1, rmx = th.zeros(S, C, device="cuda"), th.zeros(S, C, device="cuda"), th.full((n,), -1.0, device="cuda")
    L.check(lib.uavgnn_relu_bwd_colsum(dy.data_ptr(), C, y.data_ptr(), C, o0.data_ptr(), C, n, C, p0.data_ptr(), S, L.stream()), "plain")
    L.check(lib.uavgnn_relu_bwd_colsum_rowmax(dy.data_ptr(), C, y.data_ptr(), C, o1.data_ptr(), C, n, C, p1.data_ptr(), S, rmx.data_ptr(),
                                              L.stream()), "rowmax")
    assert th.equal(o0, o1) and th.equal(p0, p1) and th.equal(rmx, o1.abs().max(1).values)
    assert lib.uavgnn_relu_bwd_colsum_rowmax(dy.data_ptr(), C, y.data_ptr(), C, o1.data_ptr(), C, n, 128, p1.data_ptr(), S, rmx.data_ptr(),
                                             L.stream()) == L.UAVGNN_EUNSUPPORTED


@pytest.mark.parametrize("n,Mo,Ko,views,bounds", [(65536, 768, 320, False, "exact"), (32768, 256, 512, True, "exact"), (262144, 768, 256, False, "global"),
                                                  (4096, 260, 132, False, "exact")])
def test_gemm_tn_f16x2_weight_gradient_vs_float64(n, Mo, Ko, views, bounds):
    """csrc/gemm_tn_h2.hip (dW = dY^T X through LDS transposing reads, f16x2 arithmetic) against float64: strided row views, ragged output
    tiles, partial sums over row chunks (+ accumulate), the column maxima of uavgnn_col_absmax - and the ONE global bound per operand the
    learner uses (row maxima left by the producers), with columns 2^-12 below it; error held to the vendor fp32 split-K GEMM's on the
    same data."""
    import json
    import os
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    gen = th.Generator().manual_seed(n + Mo)
    dy = (th.randn(n, Mo + 4, generator=gen) * th.exp2(th.randint(-14, 1, (n, 1), generator=gen).float()) * 1e-3).cuda()
    x = th.relu(th.randn(n, Ko + 8, generator=gen)).cuda()
    if bounds == "global":     # a quarter of the columns far below the tensor's maximum
        dy[:, ::4] *= 2.0 ** -12
        x[:, 1::4] *= 2.0 ** -12
    if views:
        dy, x = dy[:, :Mo], x[:, :Ko]
    else:
        dy, x = dy[:, :Mo].contiguous(), x[:, :Ko].contiguous()
    assert lib.uavgnn_gemm_tn_h2_supported(n, Mo, Ko)
    if bounds == "exact":
        cy, cx = th.empty(Mo, device="cuda"), th.empty(Ko, device="cuda")
        L.check(lib.uavgnn_col_absmax(dy.data_ptr(), dy.stride(0), n, Mo, cy.data_ptr(), L.stream()), "col_absmax")
        L.check(lib.uavgnn_col_absmax(x.data_ptr(), x.stride(0), n, Ko, cx.data_ptr(), L.stream()), "col_absmax")
        assert th.equal(cy, dy.abs().max(0).values) and th.equal(cx, x.abs().max(0).values)
    else:
        cy, cx = dy.abs().max().expand(Mo).contiguous(), x.abs().max().expand(Ko).contiguous()
    S = lib.uavgnn_gemm_tn_h2_chunks(n, Mo, Ko)
    assert S >= 1
    part = th.full((S, Mo, Ko), float("nan"), device="cuda")
    args = (dy.data_ptr(), dy.stride(0), Mo, x.data_ptr(), x.stride(0), Ko, n, cy.data_ptr(), cx.data_ptr(), part.data_ptr(), S)
    L.check(lib.uavgnn_gemm_tn_h2(*args, 0, L.stream()), "gemm_tn_h2")
    got = part.sum(0)
    L.check(lib.uavgnn_gemm_tn_h2(*args, 1, L.stream()), "gemm_tn_h2 accumulate")
    assert_close(part.sum(0), 2 * got, 1e-6, "accumulate doubles the partials")
    ref = dy.double().t() @ x.double()
    den = dy.double().abs().t() @ x.double().abs()
    Sv = 64
    vend = th.bmm(dy.contiguous().view(Sv, n // Sv, -1).transpose(1, 2), x.contiguous().view(Sv, n // Sv, -1)).sum(0)
    rows = []
    for tag, o in (("f16x2", got), ("vendor fp32 split-K", vend)):
        e = (o.double() - ref).abs() / den.clamp_min(1e-300)
        rows.append(dict(what=tag, max=float(e.max()), mean=float(e.mean())))
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "gpurun_out", "h2_errors.jsonl"), "a") as f:
            f.write(json.dumps(dict(test="gemm_tn", n=n, Mo=Mo, Ko=Ko, bounds=bounds, rows=rows)) + "\n")
    except OSError:
        pass
    assert_close(got, ref, 1e-5, "dW (f16x2)")
    # the absolute bar of test_gemm_bf16x3_vs_float64, and not above the vendor's split-K GEMM where the row chunks are comparable (the
    # vendor reference sums 64 short chunks: on a few thousand rows its chains are 8 x shorter than this kernel's 512-row chunks)
    assert rows[0]["max"] < 4e-7 and rows[0]["mean"] < 4e-8, rows
    if n >= 32768:
        assert rows[0]["mean"] <= 1.5 * rows[1]["mean"] and rows[0]["max"] <= 3.0 * rows[1]["max"], rows
    # ... and bit-reproducible
    part2 = th.empty_like(part)
    L.check(lib.uavgnn_gemm_tn_h2(dy.data_ptr(), dy.stride(0), Mo, x.data_ptr(), x.stride(0), Ko, n, cy.data_ptr(), cx.data_ptr(), part2.data_ptr(),
                                  S, 0, L.stream()), "gemm_tn_h2")
    assert th.equal(part2.sum(0), got)


@pytest.mark.parametrize("n,Mo,Ko", [(65536, 260, 132)])
def test_gemm_tn_f16x2_global_bound_column_ladder(n, Mo, Ko):
    """csrc/gemm_tn_h2.hip under ONE global bound per operand, as WeightGradSink.end_sequence passes it, with columns 2^-17, 2^-24, 2^-30
    and 2^-40 below that bound: every entry within the derived floor |dW - ref| <= A sum|dy||x| + B_FLOOR (B_y sum|x| + B_x sum|dy|)
    against float64 (constants and derivation: tests/test_f16x2_emulation.py; A = A_GPU includes the fp32 accumulation)."""
    import json
    import os
    from tests.test_f16x2_emulation import A_GPU, LADDER, derived_bound, ladder_operands
    from tests.util import _GRAD_LOG
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    assert lib.uavgnn_gemm_tn_h2_supported(n, Mo, Ko)
    dy_np, x_np = ladder_operands(n, Mo, Ko, seed=5)
    dy, x = th.from_numpy(dy_np).cuda(), th.from_numpy(x_np).cuda()
    cy, cx = dy.abs().max().expand(Mo).contiguous(), x.abs().max().expand(Ko).contiguous()
    S = lib.uavgnn_gemm_tn_h2_chunks(n, Mo, Ko)
    part = th.full((S, Mo, Ko), float("nan"), device="cuda")
    L.check(lib.uavgnn_gemm_tn_h2(dy.data_ptr(), dy.stride(0), Mo, x.data_ptr(), x.stride(0), Ko, n, cy.data_ptr(), cx.data_ptr(),
                                  part.data_ptr(), S, 0, L.stream()), "gemm_tn_h2")
    got = part.sum(0).double().cpu().numpy()
    ref = dy_np.astype("float64").T @ x_np.astype("float64")
    bound = derived_bound(dy_np, x_np, float(cy[0]), float(cx[0]), A_GPU)
    ratio = abs(got - ref) / bound
    rows = {}
    for i, k in enumerate((0,) + LADDER):         # worst ratio per ladder rung (rows or columns of that rung)
        rows[f"2^-{k}"] = float(max(ratio[i::5, :].max(), ratio[:, i::5].max()))
    try:
        with open(os.path.join(os.path.dirname(_GRAD_LOG), "h2_errors.jsonl"), "a") as f:      # (the directory of the gradient-error log)
            f.write(json.dumps(dict(test="gemm_tn global-bound ladder", n=n, Mo=Mo, Ko=Ko, worst_ratio_to_floor=rows)) + "\n")
    except OSError:
        pass
    assert (ratio <= 1.0).all(), (f"f16x2 weight gradient outside the derived floor: {rows}; worst entry "
                                  f"{divmod(int(ratio.argmax()), Ko)}")


def test_time_batched_linear_relu_weight_gradient_on_the_f16x2_kernel(monkeypatch):
    """ops.linear_relu (f_aggr, gnn_agents.py:99-102) over 2^18 time-batched rows: the forward GEMM leaves the row maxima of its input, the
    ReLU-backward kernel those of the masked gradient, dx and dW run on the f16x2 kernels (csrc/gemm_h2.hip, csrc/gemm_tn_h2.hip) - against
    float64 under grad_close and against the bf16x3 / vendor path of rounds 3-5."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    n, K, C = 1 << 18, 512, 256
    gen = th.Generator().manual_seed(41)
    x = th.relu(th.randn(n, K, generator=gen)).cuda().requires_grad_(True)
    W = (0.05 * th.randn(C, K, generator=gen)).cuda().requires_grad_(True)
    b = (0.1 * th.randn(C, generator=gen)).cuda().requires_grad_(True)
    g = (th.randn(n, C, generator=gen) * 1e-3).cuda()
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    y = ops.linear_relu(x, W, b)
    dx, dW, db = th.autograd.grad(y, [x, W, b], g)
    monkeypatch.undo()
    assert {"uavgnn_gemm_nt_x3_rowmax", "uavgnn_relu_bwd_colsum_rowmax", "uavgnn_gemm_nt_h2", "uavgnn_gemm_tn_h2"} <= set(spy.names), sorted(set(spy.names))
    m = 16384      # float64 reference of y and dx on a prefix of the rows; dW / db on all rows in float64 on the device
    x64, W64, b64 = x.detach().double(), W.detach().double(), b.detach().double()
    pre64 = x64 @ W64.t() + b64
    y64 = th.relu(pre64)
    # the ReLU mask is a discontinuity of the gradient: a pre-activation within rounding of zero may fall on either side in fp32 (a handful of
    # 6.7e7 here, each moving one entry of dW by |g x| ~ 1e-3 of it).  The float64 reference takes the GPU's side after checking that every
    # disagreement sits ON the kink (the rule of test_learner_update_at_exp3_sizes_vs_oracle)
    mask = y.detach() > 0
    flips = mask != (pre64 > 0)
    assert int(flips.sum()) <= 1e-6 * flips.numel() + 2, int(flips.sum())
    if bool(flips.any()):
        assert float(pre64[flips].abs().max()) <= 1e-5 * float(pre64.abs().max())
    del pre64
    gm = g.double() * mask
    assert_close(y[:m], y64[:m], 1e-5, "y")
    assert_close(dx[:m], (gm @ W64)[:m], 1e-5, "dx (f16x2)")
    monkeypatch.setattr(ops, "GEMM_H2", False)
    y2 = ops.linear_relu(x, W, b)
    dx2, dW2, db2 = th.autograd.grad(y2, [x, W, b], g)
    grad_close(dW, gm.t() @ x64, "f_aggr dW on the f16x2 kernel, 2^18 rows", ref32=dW2)
    grad_close(db, gm.sum(0), "f_aggr db, 2^18 rows", ref32=db2)
    assert th.equal(y, y2)

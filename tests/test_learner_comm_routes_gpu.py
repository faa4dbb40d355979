"""`-m gpu`: the communication blocks that leave ``GnnAgent.step`` through the generic route ``self.f_comm(g["talk"], x, h)`` - BaseComm,
CommNet, EdgeConv and TarMAC with ``n_rounds`` = 2 - at exp3 sizes, on the kernels production dispatches there, against the float64
oracle (oracle/restatement.py; float32 for the error floor).  tests/test_gpu_parity.py covers the fused one-round TarMAC step,
tests/test_learner_comm_variants_gpu.py ``c`` = None / 'disc'; the fixtures (agent_base, agent_commnet, agent_econv, agent_tarmac_r2) stay
below every row threshold of uav_bs_ctrl_amd/ops.py.  Here: ``MultiAgentQLearner.accumulate`` on bench.py's sampled batches (the bf16x3
GRU cell on a concatenated / summed input without row maxima, the bf16x3 input-gradient products from 4 096 rows, EdgeConv's four strided
column slices of one parameter, TarMAC's per-step ``th.cat`` weight under ``frozen_weights()``, the uniform talk aggregation at M = 256,
``_TimeSplit.backward``'s stray-gradient copy), and ONE agent step on ragged 16-agent graphs through both talk kernel families.
Helpers: tests/gpu_util.py."""
import pytest
import torch as th

from oracle import restatement as R
from tests.gpu_util import (EXP3, UPDATE_CASES, _exp3_learner_and_sequence, _LibSpy, _oracle_at_gpu_branch, _oracle_update, _ScriptedRelu,
                            agent_from_params, default_init_params, synth_graph, to_batch)
from tests.test_learner_comm_variants_gpu import _expected_dispatch, _grad_ratio, _record
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 0.0       # as tests/test_gpu_parity.py: no blanket absolute floor
VARIANTS = [("base", 1), ("commnet", 1), ("commnet", 2), ("econv", 1), ("econv", 2), ("tarmac", 2)]
VARIANT_IDS = [f"{c}-r{r}" for c, r in VARIANTS]


def _expected_routes_dispatch(c, N, T, M, dist):
    """(C-ABI entries that must be called, entries that must NOT be) for one accumulate of variant c on N agents x (T + 1) steps - from
    uav_bs_ctrl_amd/ops.py (line numbers: of the commit that added this test).  The number of rounds changes how often an entry is
    called, not which."""
    # --- the time-batched encoder and the recurrent cell: what `_expected_dispatch` derives for an agent without a communication block.
    # The encoder does not depend on the block.  The cell: every block ends in agents/gnn_agents.py:_gru -> ops.gru_cell(inp, h, cell)
    # with rowmax=None (ops.py:577) - gru_cell_supported from GRU_FUSED_MIN_ROWS = 1024 rows (ops.py:363-368; K_in = 320 for the
    # th.cat of x and a 64-wide message, K_in = 256 for CommNet's sum), _gru_cell_launch without row maxima takes the bf16x3 entries
    # uavgnn_gru_split_weights / uavgnn_gru_cell_fwd_x3_opts (ops.py:482-483), _GruCellFused.backward the plain gate entry
    # uavgnn_gru_gates_bwd_fused (ops.py:549 -> :520: no sums, no head).  From 4096 rows d h += d_gh W_hh runs on uavgnn_gemm_nt_x3
    # (ops.py:552 -> _mm_nn :764, gemm_x3_supported :710-712: 256 outputs), so do CommNet's d inp (256 outputs; the 320 of the other
    # blocks are no multiple of 128: vendor GEMM) and its c_mod (ops.linear -> _mm_nt, ops.py:752)
    expect, forbid = _expected_dispatch(None, N, T, M, dist)
    # --- the talk relation.  bench.py's batches carry graph_off and the hint of 8 agents per graph, so ops.talk_attention picks the
    # per-graph kernels (ops.py:317 _talk_env -> _launch_talk_fwd :244-248): mean mode over M = 64 (base, econv), M = 256 (commnet's h),
    # attention with K = 16 (tarmac's second and first round alike)
    expect |= {"uavgnn_talk_attn_env_fwd"}
    forbid -= {"uavgnn_talk_attn_env_bwd"}
    if c == "commnet":      # the aggregated h is detached (agents/gnn_agents.py:246): autograd never enters _TalkAttention.backward
        forbid |= {"uavgnn_talk_attn_env_bwd"}
    else:                   # _TalkAttention.backward -> _launch_talk_bwd, env branch (ops.py:258-262)
        expect |= {"uavgnn_talk_attn_env_bwd"}
    # the per-destination kernels (ops.py:250 / :266: batches without graph_off) and DiscreteComm's
    forbid |= {"uavgnn_talk_attn_fwd", "uavgnn_talk_attn_bwd", "uavgnn_disc_comm_fwd", "uavgnn_disc_comm_bwd"}
    return expect, forbid


def _accumulate_spied(learner, batch, monkeypatch):
    """(out, flat gradients, called C-ABI entries, (rows, K, outputs) of every bf16x3 NT GEMM, staged steps per ``end_sequence``) of one
    eager ``learner.accumulate``."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    staged = []
    orig_end = ops.WeightGradSink.end_sequence

    def end_spy(self):
        staged.append(0 if self.seq is None else len(self.seq.bwd_steps))
        return orig_end(self)
    monkeypatch.setattr(ops.WeightGradSink, "end_sequence", end_spy)
    out = learner.accumulate(dict(batch))
    flat = learner.grads.flat.clone()
    monkeypatch.undo()
    # include/uavgnn.h: uavgnn_gemm_nt_x3(X, ldx, M, K, planes, N, ...)
    x3 = {(a[2], a[3], a[5]) for name, a in spy.calls if name == "uavgnn_gemm_nt_x3"}
    return out, flat, set(spy.names), x3, staged


@pytest.mark.parametrize("c,r", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("dist", ["env", "dense"])
@pytest.mark.parametrize("label,B,n,M,T", UPDATE_CASES[:2])
def test_learner_update_comm_route_vs_oracle(label, B, n, M, T, dist, c, r, monkeypatch):
    """``learner.accumulate`` for base / commnet / econv / two-round tarmac on bench.py's sampled batches, at 1 280 rows (above the
    1 024-row cell threshold) and 4 096 rows (at the bf16x3 GEMM threshold): the dispatched C-ABI set, LossQ and every Q value at 1e-5
    against float64, every slice of the flat gradient buffer under ``grad_close`` - at the branch the HIP path took for the double-Q
    argmax and the encoder's ReLUs - and the captured ``GraphedCycle`` replay bit-identical to the eager run.  (The 16 384-row case of
    UPDATE_CASES is left out: without a producer's row maxima no route here has a threshold above 4 096.)"""
    from uav_bs_ctrl_amd.graphs import GraphedCycle
    what = f"c={c} r={r} {label} {dist}"
    learner, batch = _exp3_learner_and_sequence(B, n, M, T, dist, seed=3, c=c, n_rounds=r)
    N = B * n
    out, flat, called, x3, staged = _accumulate_spied(learner, batch, monkeypatch)
    expect, forbid = _expected_routes_dispatch(c, N, T, M, dist)
    _record("comm_routes_dispatch.jsonl", dict(case=what, called=sorted(called), gemm_nt_x3=sorted(x3)))
    # --- the dispatch
    assert expect <= called, f"{what}: production kernels not dispatched: {sorted(expect - called)}"
    assert not (forbid & called), f"{what}: re-routed to {sorted(forbid & called)}"
    assert staged and max(staged) == 0, f"{what}: the time-batched staging serves only the fused TarMAC step: {staged}"
    # the entry's NAME is in every set (the encoder's f_aggr runs on it over the (T + 1) N and T N rows of the time-batched graphs): the
    # per-step products are told by their N rows - from 4096 rows d h += d_gh W_hh [N, 3H] x [3H, H] (CommNet's d inp has the same shape),
    # CommNet's c_mod [N, H] x [H, H], and d x of the message projections through a STRIDED column slice of their weight
    # (_LinearSplitK._grads, ops.py:1013 -> _mm_nn: [N, 64] x W[:, :H] of f_msg's [64, 2H] / [64, 4H], [N, 96] x the [96, 2H] cat of
    # TarMAC's three); none below
    H, msg, key = EXP3["hidden_size"], EXP3["msg_size"], EXP3["key_size"]
    per_step = {s for s in x3 if s[0] == N}
    want = {(N, 3 * H, H), (N, H, H) if c == "commnet" else (N, msg + 2 * key if c == "tarmac" else msg, H)} if N >= 4096 else set()
    assert want <= per_step and (N >= 4096 or not per_step), f"{what}: per-step bf16x3 GEMMs {sorted(per_step)}, expected {sorted(want)}"
    # --- oracle, float64 (float32 for the error floor), at the branch the HIP path took
    stats = {}
    l64, _, g64, l32, g32 = _oracle_at_gpu_branch(learner, batch, out["QVals"].detach().cpu(), T, N, what, cfg=dict(EXP3, c=c, n_rounds=r),
                                                  stats=stats)
    print(f"{what}: decisions {stats}")
    assert_close(out["LossQ"], l64, 1e-5, f"{what}: LossQ")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    worst, fails = (0.0, ""), []
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        got = flat[o:o + prm.numel()].view_as(prm)
        ratio = _grad_ratio(got, g64[k], g32[k])
        worst = max(worst, (ratio, k))
        print(f"{what}: grad {k}: {ratio:.3f} of grad_close's limit")
        try:
            grad_close(got, g64[k], f"learner.accumulate c={c} r={r} {label} {dist}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)
        except AssertionError as e:       # every parameter is measured before the first failure is raised
            fails.append(str(e))
    _record("comm_routes_oracle.jsonl",
            dict(kind="update", case=what, expect=sorted(expect), worst_grad_ratio=worst[0], worst_grad=worst[1], **stats))
    assert not fails, "\n".join(fails)
    # --- the same accumulate as ONE replayed hipGraph leaves the eager flat gradient buffer, bit for bit
    cyc = GraphedCycle(learner, lambda: learner.accumulate(batch))
    learner.grads.flat.fill_(float("nan"))
    out_g = cyc()
    th.cuda.synchronize()
    assert_close(out_g["LossQ"], l64, 1e-5, f"{what}: LossQ (graph replay)")
    assert th.equal(learner.grads.flat, flat), f"{what}: graph replay of accumulate differs from the eager run"


def test_two_round_tarmac_update_is_told_from_the_one_round_oracle():
    """Negative control of the comparison above: the Q values of the two-round TarMAC update (1 280 rows, D-env) must FAIL the 1e-5
    comparison with the float64 oracle run with ``n_rounds`` = 1 - the comparison sees the second round."""
    _, B, n, M, T = UPDATE_CASES[0]
    learner, batch = _exp3_learner_and_sequence(B, n, M, T, "env", seed=3, c="tarmac", n_rounds=2)
    q_gpu = learner.accumulate(dict(batch))["QVals"].detach().cpu()
    _, q64_one, _, _ = _oracle_update(learner, batch, th.float64, cfg=dict(EXP3, c="tarmac", n_rounds=1))
    with pytest.raises(AssertionError):
        assert_close(q_gpu, q64_one, 1e-5, "two-round Q values against the one-round oracle")


# ---------------------------------------------------------------------------------------------------------------------
# One agent step at exp3 model sizes on both talk kernel families
# ---------------------------------------------------------------------------------------------------------------------
STEP_B, STEP_N, STEP_M = 80, 16, 40     # 1 280 rows (above the cell threshold) in graphs of 16 agents: the NMAX = 16 per-graph kernels
TALK_P, TALK_SEED = 0.12, 11            # edge probability / generator seed of the hand-built talk relation


def _loss(q, h2, wq, wh):
    return (q * wq).sum() + (h2 * wh).sum()


def _sparse_talk(B, n, p, seed):
    """(talk_off [N + 1], talk_src [E]) of B graphs of n agents: edge i -> j with probability p, no self loops added (an agent may have
    no in-edge at all), every fifth graph without any edge, every third edge doubled (a parallel edge into the same destination)."""
    gen = th.Generator().manual_seed(seed)
    N = B * n
    adj = th.rand(B, n, n, generator=gen) < p          # adj[b, i, j]: edge i -> j
    adj[3::5] = False
    b, i, j = adj.nonzero(as_tuple=True)
    src, dst = b * n + i, b * n + j
    keep = th.arange(src.numel())
    idx = th.cat([keep, keep[::3]])
    src, dst = src[idx], dst[idx]
    o = th.argsort(dst * N + src)                      # CSC: by destination, parallel edges next to each other
    src, dst = src[o], dst[o]
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(th.bincount(dst, minlength=N), 0)
    return off, src.to(th.int32)


@pytest.fixture(scope="module")
def step_graph():
    """The arrays of the single-step batch (host), checked for what they are meant to exercise before any GPU work."""
    B, n, M = STEP_B, STEP_N, STEP_M
    N = B * n
    g = synth_graph(B, n, M, "ragged", seed=5)
    g["talk_off"], g["talk_src"] = _sparse_talk(B, n, TALK_P, TALK_SEED)
    off, src = g["talk_off"].long(), g["talk_src"].long()
    deg = off[1:] - off[:-1]
    dst = th.repeat_interleave(th.arange(N), deg)
    assert bool((src // n == dst // n).all()), "talk edges leave their graph"
    assert int((deg == 0).sum()) >= 0.05 * N, "too few agents without a talk in-edge (EdgeConv's has_in mask, the mean over an empty set)"
    assert int((deg.view(B, n).sum(1) == 0).sum()) >= 1, "no graph without any talk edge"
    pair = dst * N + src
    assert bool((pair[1:] == pair[:-1]).any()), "no destination with a duplicate in-edge"
    assert int(deg.max()) > 1 and N >= 1024
    gen = th.Generator().manual_seed(99)
    h = 0.5 * th.randn(N, 256, generator=gen)
    wq, wh = th.randn(N, 9, generator=gen), th.randn(N, 256, generator=gen) / 16
    return g, h, wq, wh


KINK_MARGIN = 2.0 ** -20     # see _off_the_leaky_relu_kink


def _off_the_leaky_relu_kink(g, p64, seed):
    """(copy of g whose GATv2 score pre-activations stay clear of the LeakyReLU kink, source rows re-drawn).  The gradient is
    discontinuous where z = fc_src(x_u) + fc_dst(x_v) crosses zero (the slope of the score's LeakyReLU jumps from 0.2 to 1), and the
    gradient of fc_dst is a sum over the in-edges that cancels almost entirely (a constant added to every in-edge's score leaves the
    softmax as it is), so ONE element of 6.6 x 10^6 evaluated on the other side moves one unit of d fc_dst.bias by 1e-4 ... 1e-3 of the
    tensor's scale: seen with the reference alone (float32 against float64 oracle, c = 'commnet', unit 215: |z64| = 6e-9 of the scale)
    and on the HIP path (c = 'econv', unit 92: |z64| = 4e-9).  Unlike the ReLUs the slope a kernel took cannot be read off its output,
    so the INPUTS keep away from the kink: every source row with an element |z64| <= 2^-20 sum |terms| is drawn again from the
    distribution of gpu_util.synth_graph.  The margin is what an fp32 evaluation of z can be off by: at most 8 terms (4 + 2 features,
    2 biases) added in fp32 (8 x 2^-24 of sum |terms|), each product on the bf16x3 matrix-core path short of its exact value by at
    most 2^-23 (csrc/gatv2_hetero.hip) - 10 x 2^-24 < 2^-20."""
    g = dict(g)
    gen = th.Generator().manual_seed(seed)
    lin = th.nn.functional.linear
    x_dst, redrawn = g["x_a"].double(), 0
    for rel, xk, ok in (("seen", "x_gt", "seen_off"), ("near", "x_ubs", "near_off")):
        pr = R.sub(p64, f"enc.f_conv.{rel}")
        Ws, bs, Wd, bd = (pr[k].double() for k in ("fc_src.weight", "fc_src.bias", "fc_dst.weight", "fc_dst.bias"))
        dst = R.seg_ids(g[ok])
        zd, ad = lin(x_dst, Wd, bd).index_select(0, dst), lin(x_dst.abs(), Wd.abs(), bd.abs()).index_select(0, dst)
        g[xk] = g[xk].clone()
        for _ in range(8):
            xs = g[xk].double()
            z, mag = lin(xs, Ws, bs) + zd, lin(xs.abs(), Ws.abs(), bs.abs()) + ad
            rows = ((z.abs() <= KINK_MARGIN * mag).any(1)).nonzero().flatten()
            if rows.numel() == 0:
                break
            redrawn += rows.numel()
            new = th.rand(rows.numel(), xs.shape[1], generator=gen) * 2 - 1
            if rel == "seen":
                new[:, 2:] = th.rand(rows.numel(), 2, generator=gen)
            g[xk][rows] = new
        else:
            raise AssertionError(f"{rel}: score pre-activations still on the LeakyReLU kink after 8 passes")
    return g, redrawn


def _step_oracle(g, h, wq, wh, p64, cfg, dtype, masks=None):
    """(q, h', gradients by parameter name + "__h__", ReLU pre-activations in call order) of R.gnn_agent_forward + ``_loss`` on the CPU;
    masks: {call index: activation pattern} prescribed to the encoder's three ReLUs (gpu_util._ScriptedRelu)."""
    pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p64.items()}
    gg = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g.items()}
    hh = h.detach().clone().to(dtype).requires_grad_(True)
    script, real = _ScriptedRelu(masks), R.F
    R.F = script
    try:
        q, h2 = R.gnn_agent_forward(gg, hh, pp, cfg)
    finally:
        R.F = real
    gr = th.autograd.grad(_loss(q, h2, wq.to(dtype), wh.to(dtype)), list(pp.values()) + [hh])
    return q.detach(), h2.detach(), dict(zip(list(pp) + ["__h__"], gr)), script.pre


def _step_oracle_at_gpu_branch(net, hb, g, h, wq, wh, p64, cfg, what, stats):
    """float64 and float32 oracle of the single step at the ReLU pattern the HIP encoder took (the second discontinuity that
    gpu_util._oracle_at_gpu_branch handles, under the same caps: a flipped element sits within 1e-5 of the tensor's scale of the kink,
    at most 1e-5 of the elements + 2 flip); forward values are compared by the caller with float64's OWN branch."""
    from uav_bs_ctrl_amd import ops
    q64, h64, g64, pre64 = _step_oracle(g, h, wq, wh, p64, cfg, th.float64)
    enc = net.enc
    with th.no_grad():
        rels = []
        for et in ("seen", "near"):
            x_src, off = hb.relation_segments(et)
            rels.append((x_src, off, hb.relation_order(et), enc.f_conv[et]))
        k1 = ops.hetero_gatv2(hb.agent_feat(), enc._n_heads, rels)
        x = ops.linear_relu(k1, enc.f_aggr[0].weight, enc.f_aggr[0].bias)
    H = x.shape[1]
    k1, x = (k1 > 0).cpu(), (x > 0).cpu()
    masks = {0: k1[:, :H], 1: k1[:, H:], 2: x}
    flips, margin = 0, 0.0
    for i, m in masks.items():
        pre = pre64[i].reshape(m.shape)
        flipped = (pre > 0) != m
        if bool(flipped.any()):
            flips += int(flipped.sum())
            assert float(pre[flipped].abs().max()) <= 1e-5 * float(pre.abs().max()), \
                f"{what}: ReLU pattern of call {i} differs from float64's away from the kink"
            margin = max(margin, float(pre[flipped].abs().max()) / float(pre.abs().max()))
    total = sum(m.numel() for m in masks.values())
    assert flips <= 1e-5 * total + 2, f"{what}: {flips} ReLU elements flipped"
    stats.update(relu=flips, relu_total=total, relu_margin=margin)
    if flips:
        _, _, g64, _ = _step_oracle(g, h, wq, wh, p64, cfg, th.float64, masks)
    _, _, g32, _ = _step_oracle(g, h, wq, wh, p64, cfg, th.float32, masks)
    return q64, h64, g64, g32


@pytest.mark.parametrize("c,r", VARIANTS, ids=VARIANT_IDS)
def test_agent_step_comm_route_on_both_talk_kernel_families_vs_oracle(c, r, step_graph):
    """ONE step of the agent at exp3 model sizes on 80 ragged graphs of 16 agents whose sparse talk relation leaves agents (and whole
    graphs) without in-edges and carries parallel edges: with ``graph_off`` (per-graph talk kernels, NMAX = 16) and without
    (per-destination kernels, transposed CSC in the backward).  q and h' at 1e-5 against float64, every parameter gradient and d h under
    ``grad_close``, the two families within 2e-6 of each other, the no-grad forward (rollout / target network) bit-identical to the
    training forward."""
    from uav_bs_ctrl_amd import ops
    g, h, wq, wh = step_graph
    cfg = dict(EXP3, c=c, n_rounds=r)
    what = f"step c={c} r={r}"
    p64 = default_init_params(cfg, seed=1)
    g, redrawn = _off_the_leaky_relu_kink(g, p64, seed=17)       # (per variant: the biases of the encoder differ between them)
    net = agent_from_params(p64, cfg)
    M_talk, K_talk = (256 if c == "commnet" else 64), (16 if c == "tarmac" else 0)
    g_env = to_batch(g)
    g_dst = to_batch({k: v for k, v in g.items() if k != "graph_off"})
    assert ops._talk_env(g_env, M_talk, K_talk) is not None and g_env.hints["max_graph_agents"] == STEP_N
    assert ops._talk_env(g_dst, M_talk, K_talk) is None
    stats = dict(kink_rows_redrawn=redrawn)
    q64, h64, g64, g32 = _step_oracle_at_gpu_branch(net, g_env.fresh(), g, h, wq, wh, p64, cfg, what, stats)
    print(f"{what}: decisions {stats}")
    outs, worst, fails = [], (0.0, ""), []
    names = [k for k, _ in net.named_parameters()]
    for fam, hb in (("per graph", g_env), ("per destination", g_dst)):
        hd = h.cuda().requires_grad_(True)
        q, h2 = net(hb, hd)
        with th.no_grad():
            q_ng, h2_ng = net(hb.fresh(), h.cuda())
        assert th.equal(q_ng, q) and th.equal(h2_ng, h2), f"{what} {fam}: the no-grad forward differs from the training forward"
        assert_close(q, q64, 1e-5, f"{what} {fam}: q")
        assert_close(h2, h64, 1e-5, f"{what} {fam}: h'")
        gr = th.autograd.grad(_loss(q, h2, wq.cuda(), wh.cuda()), list(net.parameters()) + [hd])
        for k, got in zip(names + ["__h__"], gr):
            ratio = _grad_ratio(got, g64[k], g32[k])
            worst = max(worst, (ratio, f"{k} ({fam})"))
            print(f"{what} {fam}: grad {k}: {ratio:.3f} of grad_close's limit")
            try:
                grad_close(got, g64[k], f"{what} {fam}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)
            except AssertionError as e:       # every gradient is measured before the first failure is raised
                fails.append(str(e))
        outs.append((q.detach(), h2.detach()))
    _record("comm_routes_oracle.jsonl", dict(kind="step", case=what, worst_grad_ratio=worst[0], worst_grad=worst[1], **stats))
    assert not fails, "\n".join(fails)
    # the backward of the per-graph kernels never builds the transposed CSC; that of the per-destination kernels does, unless nothing
    # that is aggregated carries a gradient (CommNet)
    assert "talkT" not in g_env._cache
    assert ("talkT" in g_dst._cache) == (c != "commnet")
    assert_close(outs[0][0], outs[1][0], 2e-6, f"{what}: q per graph vs per destination")
    assert_close(outs[0][1], outs[1][1], 2e-6, f"{what}: h' per graph vs per destination")

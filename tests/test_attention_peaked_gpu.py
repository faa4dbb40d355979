"""`-m gpu`: every kernel that contains a segment softmax against the float64 oracle where a trained policy puts it - per-destination
score spreads of 8 .. 30 (`peaked`) and 60 .. 250 (`saturated`) natural-log units instead of the 0.1 .. 0.5 of a fresh initialisation
- and on the structured cases of tests/attention_cases.py (`winner_at`, `offset`, `ties`, `deg1`).  Inputs and references come from
that module (checked on the CPU by tests/test_attention_cases_host.py).

Tolerance: the rule of tests/util.py::grad_close for outputs as well as gradients - 1e-5 of max|ref| + |ref_i| where fp32 can hold it,
else 4 x the float32 CPU oracle's own error against float64 on the same tensor - and every kernel output is asserted finite first.
The K1 backward kernels may take the other side of a z within rounding of zero than float64 does: their gradients get, per element,
the sign-tie allowance of tests/k1_closed_form.py on top (at most 1e-4 of the (edge, channel) pairs count, host test)."""
import pytest
import torch as th

from tests import attention_cases as AC
from tests.gpu_util import agent_from_params, make_args, to_batch
from tests.k1_closed_form import NAMES, float64_closed_form_ragged
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu

H = AC.H
VID = AC.variant_id


def _held(actual, ref64, ref32, what, base=None, allow=None):
    """Finite, and within the rule of grad_close of float64.  allow: per-element allowance taken off the error first (sign ties)."""
    assert bool(th.isfinite(actual).all()), f"{what}: non-finite kernel output"
    a = actual.detach().double().cpu().reshape(ref64.shape)
    if allow is not None:
        err = a - ref64.double()
        a = ref64.double() + th.sign(err) * (err.abs() - allow.double().cpu()).clamp_min(0.0)
    return grad_close(a, ref64, what, ref32=ref32, base=base)


# ---------------------------------------------------------------------------------------------------------------------
# K1 forward

def _k1_forward_abi(c, entry):
    """One relation through a C-ABI entry point: (rows [N, H], saved weights [E, 4]) on the GPU."""
    from uav_bs_ctrl_amd import _lib as L
    dev = "cuda"
    x_src, x_dst, off = c.x_src.to(dev).contiguous(), c.x_dst.to(dev).contiguous(), c.off.to(dev)
    prm = [t.to(dev).contiguous() for t in AC.prm_list(c.p)]
    out = th.full((c.N, H), float("nan"), device=dev)
    a_save = th.full((max(c.E, 1), 4), float("nan"), device=dev)
    rc = getattr(L.lib(), entry)(L.ptr(x_src) if c.E else None, c.E, x_src.shape[1], x_dst.data_ptr(), 2, off.data_ptr(), None, c.N,
                                 *[t.data_ptr() for t in prm], 4, 64, 0.2, out.data_ptr(), H, a_save.data_ptr(), L.stream())
    assert rc == 0, (entry, rc)
    th.cuda.synchronize()
    return out, a_save[:c.E], dict(x_src=x_src, x_dst=x_dst, off=off, prm=prm)


def _check_k1_forward(c, out, a, what):
    _held(out, c.out64, c.out32, f"{what}: rows")
    if c.E:
        _held(a, c.a64, c.a32, f"{what}: attention weights")
        dst = th.repeat_interleave(th.arange(c.N), c.deg)
        sums = th.zeros(c.N, 4, dtype=th.float64).index_add_(0, dst, a.detach().double().cpu())
        assert_close(sums[c.deg > 0], th.ones_like(sums[c.deg > 0]), 1e-6, f"{what}: attention weights sum to one per destination")
    one = th.nonzero(c.deg == 1).flatten()
    if one.numel():        # exp2(0) x rcp(1): a single in-edge weighs exactly 1
        assert bool((a.cpu()[c.off[one].long()] == 1.0).all()), f"{what}: the weight of a single in-edge is not exactly 1.0f"
    assert bool((out[(c.deg == 0).to(out.device)] >= 0).all())


@pytest.mark.parametrize("variant", AC.K1_FORWARD_VARIANTS, ids=VID)
@pytest.mark.parametrize("entry", ["uavgnn_gatv2_fwd_valu", "uavgnn_gatv2_fwd_mfma", "uavgnn_gatv2_fwd"])
def test_k1_forward_entry_points_at_peaked_and_saturated_scores(entry, variant):
    """`seen` (F = 4, 0 .. 80 in-edges) and `near` (F = 2, 7 in-edges; uavgnn_gatv2_fwd sends it to gatv2_small) at N = 320 through the
    VALU kernel, the row-tile kernel and the automatic choice; `winner_at` for the 16-edge pass of the row-tile kernels."""
    for c in AC.k1_forward_pair(variant, 16):
        out, a, _ = _k1_forward_abi(c, entry)
        _check_k1_forward(c, out, a, f"{entry} {c.name}")


def _fused_relations(seen, near):
    from uav_bs_ctrl_amd import HeteroBatch
    from uav_bs_ctrl_amd.agents.gnn_agents import GATv2Conv
    hb = HeteroBatch.from_arrays(x_a=seen.x_dst, x_gt=seen.x_src, seen_off=seen.off, x_ubs=near.x_src, near_off=near.off).to("cuda")
    rels = []
    for et, c, F in (("seen", seen, 4), ("near", near, 2)):
        conv = GATv2Conv((F, 2), 64, 4)
        conv.load_state_dict(c.p)
        xs, off = hb.relation_segments(et)
        rels.append((xs, off, hb.relation_order(et), conv.cuda()))
    return hb, rels


def _fused_launch(seen, near, what):
    """ops.hetero_gatv2 in training mode: rows of both relations and the attention weights its backward will read."""
    from uav_bs_ctrl_amd import ops
    hb, rels = _fused_relations(seen, near)
    ops.KERNEL_TIMER.reset(enabled=True)
    try:
        out = ops.hetero_gatv2(hb.agent_feat(), 4, rels)
        names = set(ops.KERNEL_TIMER.summary())
    finally:
        ops.KERNEL_TIMER.enabled = False
    assert "gatv2_hetero_fwd" in names, f"{what}: the fused launch was not taken ({names})"
    saved = out.grad_fn.saved_tensors            # x_dst, then per relation x_src, seg_off, order, six parameters, a_save; the output
    for i, c in enumerate((seen, near)):
        a = saved[1 + i * 10 + 9]
        assert a.shape == (max(c.E, 1), 4)
        _check_k1_forward(c, out.detach()[:, i * H:(i + 1) * H], a[:c.E], f"{what}: {c.name}")
    return out


FUSED_FORMS = ["default", "fp32-mfma", "prepared-image", "row-maxima"]


@pytest.mark.parametrize("variant", AC.K1_FORWARD_VARIANTS, ids=VID)
@pytest.mark.parametrize("form", FUSED_FORMS)
def test_fused_k1_forward_at_peaked_and_saturated_scores(form, variant, monkeypatch):
    """The fused launch of both relations (gatv2_hetero.hip; 8-edge passes) with the bf16x3 score GEMM, with the fp32-MFMA source
    (gatv2_hetero_f32.hip), from the prepared parameter image, and with row maxima (which must be the maxima of the rows it wrote)."""
    from uav_bs_ctrl_amd import ops
    seen, near = AC.k1_forward_pair(variant, 8)
    what = f"fused K1 [{form}]"
    if form == "fp32-mfma":
        monkeypatch.setattr(ops, "K1_BF16Z", False)
    if form == "row-maxima":
        monkeypatch.setattr(ops, "K1_ROWMAX_MIN_ROWS", 64)
    if form == "prepared-image":
        with ops.frozen_weights():
            out = _fused_launch(seen, near, what)
    else:
        out = _fused_launch(seen, near, what)
    rm = getattr(out, "_uavgnn_rowmax", None)
    assert (rm is not None) == (form == "row-maxima"), f"{what}: row maxima {'missing' if rm is None else 'unexpected'}"
    if rm is not None:
        assert th.equal(rm[0], out.detach()[:, H:].max(1).values), f"{what}: row maxima of the `near` half"
        assert th.equal(rm[1], out.detach()[:, :H].max(1).values), f"{what}: row maxima of the `seen` half"


def test_fused_k1_forward_isolated_destinations_under_saturated_scores():
    """The "env" degree distribution (94 % of the destinations see nothing) under saturated scores, fused and per relation."""
    seen, near = AC.k1_forward_pair(("saturated", None, None), 8, dist="env", seed=12)
    _fused_launch(seen, near, "fused K1, env degrees")
    for entry in ("uavgnn_gatv2_fwd_valu", "uavgnn_gatv2_fwd"):
        out, a, _ = _k1_forward_abi(seen, entry)
        _check_k1_forward(seen, out, a, f"{entry} {seen.name}")


# ---------------------------------------------------------------------------------------------------------------------
# K1 backward

def _k1_backward(c, entry, what):
    """Forward (automatic choice) and backward of one relation through the C ABI; the seven gradients against float64 autograd of the
    restatement, differentiated at the ReLU branch the forward took, with the sign-tie allowance of the closed form."""
    from uav_bs_ctrl_amd import _lib as L
    out, a_save, t = _k1_forward_abi(c, "uavgnn_gatv2_fwd")
    _check_k1_forward(c, out, a_save, f"{what}: forward")
    lib, F = L.lib(), c.x_src.shape[1]
    d_out = c.d_out.cuda()
    wsb = lib.uavgnn_gatv2_bwd_workspace_bytes(F, H)
    ws = th.empty(wsb // 4, device="cuda")
    g = [th.full_like(p, float("nan")) for p in t["prm"]]
    a_full = a_save if c.E else th.zeros(1, 4, device="cuda")
    rc = getattr(lib, entry)(L.ptr(t["x_src"]), c.E, F, t["x_dst"].data_ptr(), 2, t["off"].data_ptr(), None, c.N,
                             *[p.data_ptr() for p in t["prm"][:5]], 4, 64, 0.2, out.data_ptr(), d_out.data_ptr(), H, a_full.data_ptr(),
                             *[x.data_ptr() for x in g], ws.data_ptr(), wsb, L.stream())
    assert rc == 0, (entry, rc)
    th.cuda.synchronize()
    mask = (out > 0).cpu()
    ref64, ref32 = AC.k1_grads(c, c.d_out, mask, th.float64), AC.k1_grads(c, c.d_out, mask, th.float32)
    data = dict(x_src=c.x_src, x_dst=c.x_dst, out=out.cpu(), d_out=c.d_out, a_save=a_save.cpu(), prm=AC.prm_list(c.p), N=c.N)
    _, tie = float64_closed_form_ragged(data, c.off)
    for nm, got, r64, r32, al in zip(NAMES, g, ref64, ref32, tie):
        _held(got, r64, r32, f"{what}: {nm}", allow=al)
    return g


BWD_VARIANTS = AC.K1_BACKWARD_VARIANTS
BWD_IDS = [VID(v + (None,)) for v in BWD_VARIANTS]


@pytest.mark.parametrize("variant", BWD_VARIANTS, ids=BWD_IDS)
@pytest.mark.parametrize("kind", ["generic-sparse", "generic-dense"])
def test_k1_backward_generic_kernel_at_peaked_and_saturated_scores(kind, variant):
    """uavgnn_gatv2_bwd_generic below and above a mean in-degree of 16 (its two instantiations)."""
    _k1_backward(AC.k1_backward_case(kind, variant), "uavgnn_gatv2_bwd_generic", f"generic K1 backward, {kind} {VID(variant + (None,))}")


@pytest.mark.parametrize("variant", BWD_VARIANTS, ids=BWD_IDS)
def test_k1_backward_pair_kernel_at_peaked_and_saturated_scores(variant):
    """gatv2_bwd_pair_kernel: F = 2, at most 8 in-edges on average, an odd number of destinations."""
    _k1_backward(AC.k1_backward_case("pair", variant), "uavgnn_gatv2_bwd", f"pair K1 backward {VID(variant + (None,))}")


@pytest.mark.parametrize("variant", BWD_VARIANTS, ids=BWD_IDS)
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "per-destination"])
def test_k1_backward_matrix_core_kernels_at_peaked_and_saturated_scores(resident, variant, monkeypatch):
    """The matrix-core backward (F = 4, 16 .. 128 in-edges, N = 300) with resident accumulators and draining them per destination."""
    if not resident:
        monkeypatch.setenv("UAVGNN_K1_BWD_RESIDENT", "0")
    _k1_backward(AC.k1_backward_case("mfma", variant), "uavgnn_gatv2_bwd",
                 f"matrix-core K1 backward ({'resident' if resident else 'per destination'}) {VID(variant + (None,))}")


# ---------------------------------------------------------------------------------------------------------------------
# K3b

def _check_k3(c, g, what, weights=True):
    from uav_bs_ctrl_amd import ops
    sd, qd, vd = (t.cuda().requires_grad_(True) for t in (c.s, c.q, c.v))
    out = ops.talk_attention(sd, qd, vd, g, 1.0 / c.K)
    E = int(c.src.numel())
    a = out.grad_fn.saved_tensors[-1][:E].clone()          # the weights the backward will read (gone once it has run)
    got = th.autograd.grad((out * c.w.cuda()).sum(), [sd, qd, vd])
    _held(out, c.c64, c.c32, f"{what}: c")
    if E:
        assert bool(th.isfinite(a).all()), f"{what}: non-finite attention weights"
        if weights:
            _held(a, c.a64[:, 0], c.a32[:, 0], f"{what}: attention weights")
        one = th.nonzero(c.deg == 1).flatten()
        if one.numel():
            assert bool((a.cpu()[c.off[one].long()] == 1.0).all()), f"{what}: the weight of a single in-edge is not exactly 1.0f"
    for nm, a_, r64, r32 in zip(("d_s", "d_q", "d_v"), got, c.g64, c.g32):
        _held(a_, r64, r32, f"{what}: {nm}")


def _k3_dst_params():
    return [pytest.param(sh, v, id=f"N{sh[0]}-deg{sh[1]}-K{sh[2]}-M{sh[3]}-{VID(v)}") for sh in AC.K3_DST_SHAPES for v in AC.k3_dst_variants(sh)]


@pytest.mark.parametrize("shape,variant", _k3_dst_params())
def test_talk_attention_per_destination_kernels_at_peaked_and_saturated_scores(shape, variant):
    from uav_bs_ctrl_amd import HeteroBatch, ops
    c = AC.k3_dst_case(shape, variant)
    g = HeteroBatch.from_arrays(x_a=th.zeros(c.N, 2), talk_off=c.off, talk_src=c.src).to("cuda")
    assert ops._talk_env(g, c.M, c.K) is None
    _check_k3(c, g, f"K3b {c.name}")


@pytest.mark.parametrize("variant", AC.K3_ENV_VARIANTS, ids=VID)
@pytest.mark.parametrize("i", range(len(AC.K3_ENV_SHAPES)))
def test_talk_attention_per_graph_kernels_at_peaked_and_saturated_scores(i, variant):
    from uav_bs_ctrl_amd import HeteroBatch, ops
    c = AC.k3_env_case(i, variant)
    g = HeteroBatch.from_arrays(x_a=th.zeros(c.N, 2), talk_off=c.off, talk_src=c.src, graph_off=c.bounds, device="cuda")
    assert ops._talk_env(g, c.M, c.K) is not None
    # `ties` repeats sources inside a segment: the per-graph kernels' dense attention matrix adds parallel edges up, so their saved
    # weights are compared on the simple graphs only (c and the gradients on all)
    _check_k3(c, g, f"K3b {c.name}", weights=variant[1] != "ties")


# ---------------------------------------------------------------------------------------------------------------------
# the fused message step, DiscreteComm, the whole agent

def _named_grads(net, extra):
    g = {k: p.grad for k, p in net.named_parameters()}
    g.update(extra)
    return g


@pytest.mark.parametrize("regime", ["peaked", "saturated"])
@pytest.mark.parametrize("M,K,Hh", [(64, 16, 256), (72, 14, 64)], ids=["wavefront-pair-kernel", "one-wavefront-kernel"])
def test_tarmac_step_at_peaked_and_saturated_scores(M, K, Hh, regime, monkeypatch):
    """ops.tarmac_step on a 40 x 8 complete-talk batch through both kernels of tarmac_msg.hip (M + 2K = 96: the wavefront-pair kernel;
    100: the one-wavefront kernel), forward and backward, against R.tarmac + the Q head."""
    from uav_bs_ctrl_amd import ops
    c = AC.tarmac_case(regime, M, K, Hh)
    taken = []
    orig = ops._launch_tarmac_msg
    monkeypatch.setattr(ops, "_launch_tarmac_msg", lambda *a, **k: (taken.append(1), orig(*a, **k))[1])
    net = agent_from_params(c.p, c.cfg)
    xd, hd = c.x.cuda().requires_grad_(True), c.h.cuda().requires_grad_(True)
    q, h2 = net.step(to_batch(c.g), xd, hd)
    assert taken, "the fused message launch was not taken"
    what = f"tarmac_step {regime} M={M} K={K}"
    _held(q, c.q64, c.q32, f"{what}: q")
    _held(h2, c.h64, c.h32, f"{what}: h'")
    ((q * c.wq.cuda()).sum() + (h2 * c.wh.cuda()).sum()).backward()
    grads = _named_grads(net, {"__x__": xd.grad, "__h__": hd.grad})
    for k, r64 in c.g64.items():
        _held(grads[k], r64, c.g32[k], f"{what}: grad {k}")


@pytest.mark.parametrize("regime", ["peaked", "saturated"])
def test_disc_comm_at_peaked_and_saturated_logits(regime):
    """DiscreteComm (disc_comm.hip's two-way softmax, forward and backward) under fixed Gumbel noise against R.disc_comm."""
    from uav_bs_ctrl_amd.agents.gnn_agents import DiscreteComm
    c = AC.disc_case(regime)
    comm = DiscreteComm(make_args(c.cfg))
    comm.load_state_dict(c.p)
    comm = comm.cuda()
    comm.gumbel = c.gum.cuda()
    xd, hd = c.x.cuda().requires_grad_(True), c.h.cuda().requires_grad_(True)
    h2 = comm(to_batch(c.g), xd, hd)
    what = f"disc_comm {regime}"
    _held(h2, c.h64, c.h32, f"{what}: h'")
    (h2 * c.w.cuda()).sum().backward()
    grads = _named_grads(comm, {"__x__": xd.grad, "__h__": hd.grad})
    for k, r64 in c.g64.items():
        _held(grads[k], r64, c.g32[k], f"{what}: grad {k}")


def test_whole_agent_step_with_peaked_attention():
    """The exp3 GnnAgent at B = 40, n = 8, M = 80 ragged with the encoder's attn vectors and TarMAC's f_sign / f_que scaled into
    `peaked`: Q values, h' and every parameter gradient against R.gnn_agent_forward."""
    c = AC.agent_case("peaked")
    net = agent_from_params(c.p, c.cfg)
    hd = c.h.cuda().requires_grad_(True)
    q, h2 = net(to_batch(c.g), hd)
    _held(q, c.q64, c.q32, "peaked agent: q")
    _held(h2, c.h64, c.h32, "peaked agent: h'")
    ((q * c.wq.cuda()).sum() + (h2 * c.wh.cuda()).sum()).backward()
    grads = _named_grads(net, {"__h__": hd.grad})
    for k, r64 in c.g64.items():
        _held(grads[k], r64, c.g32[k], f"peaked agent: grad {k}")

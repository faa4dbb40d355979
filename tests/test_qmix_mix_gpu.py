"""`-m gpu`: the QMIX mixing kernels (csrc/qmix.hip) against the torch formulation of agents/qmix.py evaluated in float64 on the CPU -
first the two kernels alone on a given projection, then the module and the learner's update through them.  Tolerance: the parity rule
of BASELINE section 4 (tests.util.assert_close / grad_close)."""
import copy
import math
import types

import numpy as np
import pytest
import torch as th

from oracle.closed_form import closed_form_tensor
from tests.util import GOLDEN, assert_close, grad_close

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 32), (37, 8, 32), (1600, 8, 32), (37, 3, 5), (5, 16, 128), (130, 1, 1)]


def _kernel_inputs(rows, n, e):
    gen = th.Generator().manual_seed(100 * rows + 10 * n + e)
    f = lambda *s: th.randn(*s, generator=gen, dtype=th.float32)   # noqa: E731
    proj, qs, g, v2w, v2b = f(rows, (n + 3) * e), f(rows, n), f(rows), f(e), f(1)
    # exact zeros under the two abs and the ReLU (sign(0) = 0, [0 > 0] = 0)
    planted = [(0, (n - 1) * e + e // 2), (rows // 2, n * e + e - 1), (rows - 1, (n + 2) * e)]
    for r, c in planted:
        proj[r, c] = 0.0
    return proj, qs, g, v2w, v2b, planted


def _run_kernels(proj, qs, g, v2w, v2b, n, e, q_tot=None, d_proj=None):
    """Both entries on NaN-poisoned outputs: (q_tot, d_proj, d_qs, partials).  q_tot / d_proj: NaN-filled views to write into instead
    (any base address, any row stride); proj may be a column view as well - both row strides go to the C ABI as they are."""
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    rows = proj.shape[0]
    nan = lambda *s: th.full(s, float("nan"), dtype=th.float32, device="cuda")   # noqa: E731
    G = lib.uavgnn_qmix_mix_bwd_partials(rows, e)
    assert G >= 1
    q_tot = nan(rows) if q_tot is None else q_tot
    d_proj = nan(*proj.shape) if d_proj is None else d_proj
    assert proj.stride(1) == d_proj.stride(1) == 1 and d_proj.shape == proj.shape and q_tot.shape == (rows,) and q_tot.is_contiguous()
    d_qs, part = nan(rows, n), nan(G, e + 1)
    L.check(lib.uavgnn_qmix_mix_fwd(proj.data_ptr(), proj.stride(0), qs.data_ptr(), v2w.data_ptr(), v2b.data_ptr(), rows, n, e,
                                    q_tot.data_ptr(), L.stream()), "uavgnn_qmix_mix_fwd")
    L.check(lib.uavgnn_qmix_mix_bwd(proj.data_ptr(), proj.stride(0), qs.data_ptr(), g.data_ptr(), v2w.data_ptr(), rows, n, e,
                                    d_proj.data_ptr(), d_proj.stride(0), d_qs.data_ptr(), part.data_ptr(), G, L.stream()),
            "uavgnn_qmix_mix_bwd")
    th.cuda.synchronize()
    return q_tot, d_proj, d_qs, part


def _check_against_float64(rows, n, e):
    """Forward and backward at one shape against ``mix_torch`` in float64; returns the partials [G, e + 1] of the first run."""
    from uav_bs_ctrl_amd.agents.qmix import mix_torch
    proj, qs, g, v2w, v2b, planted = _kernel_inputs(rows, n, e)
    # the oracle takes the SAME fp32 projection as a leaf: no sign or ReLU decision can differ between the two sides
    p64, q64 = proj.double().requires_grad_(True), qs.double().requires_grad_(True)
    w64, b64 = v2w.double().view(1, e).requires_grad_(True), v2b.double().requires_grad_(True)
    y64 = mix_torch(p64, q64, n, e, w64, b64).view(-1)
    pre = (q64.detach().unsqueeze(2) * p64.detach()[:, :n * e].view(rows, n, e).abs()).sum(1) + p64.detach()[:, (n + 1) * e:(n + 2) * e]
    vh = p64.detach()[:, (n + 2) * e:]
    assert bool((pre > 0).any()) and bool((pre < 0).any()), "pre has one sign only"
    assert bool((vh > 0).any()) and bool((vh < 0).any()), "v_hid has one sign only"
    ref = th.autograd.grad((y64 * g.double()).sum(), [p64, q64, w64, b64])
    dev = [t.cuda() for t in (proj, qs, g, v2w, v2b)]
    q_tot, d_proj, d_qs, part = _run_kernels(*dev, n, e)
    for name, t in (("q_tot", q_tot), ("d_proj", d_proj), ("d_qs", d_qs), ("partials", part)):
        assert bool(th.isfinite(t).all()), f"{name}: an element was not written (NaN poison left) or is not finite"
    tot = part.sum(0)
    assert_close(q_tot, y64, 1e-5, "q_tot")
    assert_close(d_proj, ref[0], 1e-5, "d_proj")
    assert_close(d_qs, ref[1], 1e-5, "d_qs")
    assert_close(tot[:e], ref[2].view(e), 1e-5, "d_v2w")
    assert_close(tot[e:], ref[3], 1e-5, "d_v2b")
    for r, c in planted:
        assert float(d_proj[r, c]) == 0.0 and float(ref[0][r, c]) == 0.0, f"planted zero at ({r}, {c})"
    again = _run_kernels(*dev, n, e)
    for name, a, b in zip(("q_tot", "d_proj", "d_qs", "partials"), (q_tot, d_proj, d_qs, part), again):
        assert th.equal(a, b), f"{name}: two runs differ"
    return part


@pytest.mark.parametrize("rows,n,e", SHAPES)
def test_kernels_against_float64_on_the_same_projection(rows, n, e):
    _check_against_float64(rows, n, e)


def _lane_group(e):
    """EP of csrc/qmix.hip: the next power of two >= e, at most 64 lanes per row (e > 64: two columns per lane)."""
    ep = 1
    while ep < e and ep < 64:
        ep *= 2
    return ep


def _rows_per_workgroup(e):
    return 4 * (64 // _lane_group(e))      # 4 wavefronts of 64 / EP rows


# rows > 2048 workgroups x rows per workgroup: the grid-stride loop makes a second (third) pass and the last pass is ragged.
#   (32781, 8, 32)  EP 32, 8 rows per workgroup: two full passes of 16 384 rows + 13 rows (workgroup 0 whole, workgroup 1 five of eight)
#   (16387, 2, 128) EP 64 x 2 columns, 4 rows: two full passes of 8192 + 3 rows of workgroup 0
#   (65575, 3, 5)   EP 8, 32 rows: one full pass of 65 536 + 39 rows (workgroup 0 whole, workgroup 1 seven of 32)
#   (524545, 1, 1)  EP 1, 256 rows: one full pass of 524 288 + 257 rows (workgroup 0 whole, workgroup 1 one row)
PAST_THE_CAP = [(32781, 8, 32), (16387, 2, 128), (65575, 3, 5), (524545, 1, 1)]


@pytest.mark.parametrize("rows,n,e", PAST_THE_CAP)
def test_kernels_past_the_grid_cap(rows, n, e):
    """Workgroups that walk more than one block of rows: the d V[2] sums carried across the passes, w / dpre / qv set up again per
    pass, and a last pass with dead rows - everything ``_check_against_float64`` asserts, d_v2w / d_v2b from the partials included."""
    from uav_bs_ctrl_amd import _lib as L
    G = L.lib().uavgnn_qmix_mix_bwd_partials(rows, e)
    per = _rows_per_workgroup(e)
    assert G * per < rows, f"{G} workgroups x {per} rows cover all {rows} rows in one pass: the case no longer reaches the loop"
    assert rows % (G * per) % per != 0, "the last pass is not ragged"
    part = _check_against_float64(rows, n, e)
    assert part.shape == (G, e + 1)


LAYOUTS = [(8, 33), (8, 64), (8, 65), (3, 96), (16, 127), (16, 16), (5, 16), (16, 8), (16, 2), (9, 4), (16, 1)]


@pytest.mark.parametrize("n,e", LAYOUTS)
@pytest.mark.parametrize("rows", [37, 300])
def test_kernels_on_every_lane_layout(rows, n, e):
    """The (EP, CPL) arms of ``dispatch`` and both arms of the d_qs store that SHAPES does not instantiate: dead lanes at EP = 64, a
    second column that is dead from some lane on, n == EP / n < EP / n > EP around kMaxAgents = 16, EP = 2 and EP = 4."""
    _check_against_float64(rows, n, e)


def _off_by_one_float(t):
    """A copy of t that starts one float into its storage."""
    s = th.full((t.numel() + 1,), float("nan"), dtype=t.dtype, device=t.device)
    v = s[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() == s.data_ptr() + 4
    return v


def _column_view(rows, width, left, right, fill=None):
    """([rows, width] column view, its [rows, left + width + right] NaN-filled storage)."""
    s = th.full((rows, left + width + right), float("nan"), dtype=th.float32, device="cuda")
    v = s[:, left:left + width]
    if fill is not None:
        v.copy_(fill)
    return v, s


@pytest.mark.parametrize("rows,n,e", [(37, 3, 5), (300, 8, 32)])
def test_kernels_take_row_strides_and_unaligned_bases(rows, n, e):
    """The C ABI's ld_proj / ld_dproj beyond (n + 3) e and dword-aligned base addresses: the same bits as the contiguous run, and not
    one float outside the [rows, (n + 3) e] window of d_proj's storage touched."""
    proj, qs, g, v2w, v2b, _ = (t.cuda() if isinstance(t, th.Tensor) else t for t in _kernel_inputs(rows, n, e))
    want = _run_kernels(proj, qs, g, v2w, v2b, n, e)
    w = (n + 3) * e
    proj_v, _ = _column_view(rows, w, 3, 4, fill=proj)                 # 7 floats wider, NaN around the window
    d_proj_v, d_store = _column_view(rows, w, 5, 6)                    # another width
    q_tot_v = _off_by_one_float(th.full((rows,), float("nan"), device="cuda"))
    assert proj_v.stride(0) == w + 7 and d_proj_v.stride(0) == w + 11 and proj_v.data_ptr() % 16 != 0
    got = _run_kernels(proj_v, *(_off_by_one_float(t) for t in (qs, g, v2w, v2b)), n, e, q_tot=q_tot_v, d_proj=d_proj_v)
    for name, a, b in zip(("q_tot", "d_proj", "d_qs", "partials"), want, got):
        assert bool(th.isfinite(b).all()), f"{name}: an element was not written, or a padding column was read"
        assert th.equal(a, b), f"{name}: the strided run differs from the contiguous one"
    assert bool(th.isnan(d_store[:, :5]).all()) and bool(th.isnan(d_store[:, 5 + w:]).all()), "a padding column of d_proj was written"


RUNG = 16
RUNG_B1 = [-60.0, -20.0, -1.0, -1e-3, -1e-7, 0.0, 1e-7, 1.0, 50.0]      # pre == c exactly (qs = 0); exp(-60) is a normal fp32 number
RUNG_SCALE = [-10, 0, 5]


def test_kernels_over_the_range_of_the_elu():
    """ELU / expm1f / expf away from randn scale, n = 8, e = 32, rungs of 16 rows: ``pre`` exactly c for nine values of c (qs = 0, the b1
    block = c: no cancellation, the same number in both precisions), then the whole of proj and qs scaled by 2^-10, 1, 2^5.  Every rung
    and every column block of d_proj is judged against ITS OWN maximum (one assert_close over the tensor would judge the rung at c = -60
    by the rung at 2^5); the rule stays 1e-5.  mix_torch in fp32 on the CPU needs at most 2.0e-6 on any (rung, block) of these inputs."""
    from uav_bs_ctrl_amd.agents.qmix import mix_torch
    n, e = 8, 32
    rows = RUNG * (len(RUNG_B1) + len(RUNG_SCALE))
    proj, qs, g, v2w, v2b, _ = _kernel_inputs(rows, n, e)
    tags = []
    for i, c in enumerate(RUNG_B1):
        s = slice(i * RUNG, (i + 1) * RUNG)
        qs[s] = 0.0
        proj[s, (n + 1) * e:(n + 2) * e] = c
        tags.append(f"pre = {c:g}")
    for i, k in enumerate(RUNG_SCALE):
        s = slice((len(RUNG_B1) + i) * RUNG, (len(RUNG_B1) + i + 1) * RUNG)
        proj[s] *= 2.0 ** k
        qs[s] *= 2.0 ** k
        tags.append(f"scale 2^{k}")
    p64, q64 = proj.double().requires_grad_(True), qs.double().requires_grad_(True)
    y64 = mix_torch(p64, q64, n, e, v2w.double().view(1, e), v2b.double()).view(-1)
    dp64, dq64 = th.autograd.grad((y64 * g.double()).sum(), [p64, q64])
    q_tot, d_proj, d_qs, part = _run_kernels(*(t.cuda() for t in (proj, qs, g, v2w, v2b)), n, e)
    for name, t in (("q_tot", q_tot), ("d_proj", d_proj), ("d_qs", d_qs), ("partials", part)):
        assert bool(th.isfinite(t).all()), f"{name}: an element was not written (NaN poison left) or is not finite"
    blocks = dict(w1=slice(0, n * e), w_final=slice(n * e, (n + 1) * e), b1=slice((n + 1) * e, (n + 2) * e),
                  v_hid=slice((n + 2) * e, (n + 3) * e))
    for i, tag in enumerate(tags):
        s = slice(i * RUNG, (i + 1) * RUNG)
        assert_close(q_tot[s], y64[s], 1e-5, f"{tag}: q_tot")
        assert_close(d_qs[s], dq64[s], 1e-5, f"{tag}: d_qs")
        for k, b in blocks.items():
            assert_close(d_proj[s, b], dp64[s, b], 1e-5, f"{tag}: d_proj block {k}")


@pytest.mark.parametrize("rows,n,e", [(37, 3, 5), (37, 8, 32), (37, 16, 16)])
def test_rows_of_a_wavefront_do_not_mix(rows, n, e):
    """64 / EP rows share a wavefront (8, 2 and 4 here) and their sums are xor-shuffles: a row of NaN in proj and qs - first, middle,
    last - must leave every other row of the three outputs bit-identical to the clean run, and every partial row but its workgroup's.
    In the poisoned row q_tot, d_qs and the w1 | w_final | b1 blocks of d_proj are NaN; the v_hid block is a ReLU mask times values of
    other inputs and is not NaN by either formulation."""
    proj, qs, g, v2w, v2b, _ = (t.cuda() if isinstance(t, th.Tensor) else t for t in _kernel_inputs(rows, n, e))
    clean = _run_kernels(proj, qs, g, v2w, v2b, n, e)
    per = _rows_per_workgroup(e)
    for r in (0, rows // 2, rows - 1):
        p, q = proj.clone(), qs.clone()
        p[r], q[r] = float("nan"), float("nan")
        q_tot, d_proj, d_qs, part = _run_kernels(p, q, g, v2w, v2b, n, e)
        others = th.arange(rows, device="cuda") != r
        for name, a, b in zip(("q_tot", "d_proj", "d_qs"), clean, (q_tot, d_proj, d_qs)):
            assert th.equal(a[others], b[others]), f"row {r} poisoned: {name} changed in another row"
        assert bool(th.isnan(q_tot[r])) and bool(th.isnan(d_qs[r]).all()) and bool(th.isnan(d_proj[r, :(n + 2) * e]).all()), \
            f"row {r} poisoned: its own outputs are not NaN"
        other_groups = th.arange(part.shape[0], device="cuda") != r // per
        assert th.equal(clean[3][other_groups], part[other_groups]), f"row {r} poisoned: a partial row of another workgroup changed"


def _fixture_case():
    z = np.load(f"{GOLDEN}/qmixer.npz")
    from uav_bs_ctrl_amd.agents.qmix import QMixer
    T, B, n = z["qs"].shape
    mix = QMixer(z["states"].shape[-1], n, types.SimpleNamespace(embed_dim=8))
    with th.no_grad():
        for i, (k, p) in enumerate(mix.named_parameters()):
            p.copy_(closed_form_tensor(p.shape, 1.0 + i * math.pi / 7, 0.1 if p.dim() == 1 else 0.25, th.float64))
    f = lambda k: th.as_tensor(z[k]).float()   # noqa: E731
    return mix, f("qs"), f("states"), f("w")


def _seeded_case():
    """(T, B) = (5, 7), n = 8, e = 32, S = 22.  Seed 354: of the seeds 0..599, tried on the CPU, the one whose projection keeps the elements under
    an abs or the ReLU furthest from zero (1.9e-4 max|proj|; the test asserts 1e-4)."""
    from uav_bs_ctrl_amd.agents.qmix import QMixer
    th.manual_seed(354)
    mix = QMixer(22, 8, types.SimpleNamespace(embed_dim=32))
    states = th.randn(5, 7, 22)
    return mix, th.randn(5, 7, 8), states, th.randn(5, 7, 1)


def _grads(mix, qs, states, w):
    qs = qs.clone().requires_grad_(True)
    y = mix(qs, states)
    return y.detach(), th.autograd.grad((y * w).sum(), list(mix.parameters()) + [qs])


@pytest.mark.parametrize("case", ["fixture", "seeded"])
def test_module_on_the_gpu_against_float64(case, monkeypatch):
    mix32, qs, states, w = _fixture_case() if case == "fixture" else _seeded_case()
    n, e = mix32.n_agents, mix32.embed_dim
    mix64 = copy.deepcopy(mix32).double()
    heads = (mix64.hyper_w_1, mix64.hyper_w_final, mix64.hyper_b_1, mix64.V[0])
    with th.no_grad():
        proj = th.nn.functional.linear(states.double().reshape(-1, states.shape[-1]), th.cat([m.weight for m in heads], 0),
                                       th.cat([m.bias for m in heads], 0))
    kinks = th.cat([proj[:, :(n + 1) * e], proj[:, (n + 2) * e:]], 1)
    assert float(kinks.abs().min()) > 1e-4 * float(proj.abs().max()), "an element under an abs / the ReLU sits on its kink"
    y64, g64 = _grads(mix64, qs.double(), states.double(), w.double())
    y32, g32 = _grads(mix32, qs, states, w)
    mixg = copy.deepcopy(mix32).cuda()
    from tests.gpu_util import _LibSpy
    from uav_bs_ctrl_amd import _lib as L
    spy = _LibSpy(L.lib())
    with monkeypatch.context() as mp:
        mp.setattr(L, "lib", lambda: spy)
        yg, gg = _grads(mixg, qs.cuda(), states.cuda(), w.cuda())
    assert [c[0] for c in spy.calls if "qmix_mix" in c[0] and "partials" not in c[0]] == ["uavgnn_qmix_mix_fwd", "uavgnn_qmix_mix_bwd"]
    grad_close(yg, y64, f"{case}: q_tot", ref32=y32)
    names = [k for k, _ in mix32.named_parameters()] + ["qs"]
    for k, a, r64, r32 in zip(names, gg, g64, g32):
        grad_close(a, r64, f"{case}: grad {k}", ref32=r32)


def test_learner_update_with_a_mixer_launches_the_kernels(monkeypatch):
    from tests.gpu_util import _LibSpy
    from tests.test_replay_mixer import _qmix_learner
    from uav_bs_ctrl_amd import _lib as L
    learner, batch, _, _ = _qmix_learner("cuda", th.float32)
    spy = _LibSpy(L.lib())
    with monkeypatch.context() as mp:
        mp.setattr(L, "lib", lambda: spy)
        out = learner.update(batch)
    th.cuda.synchronize()
    calls = [c[0] for c in spy.calls]
    assert calls.count("uavgnn_qmix_mix_fwd") == 2 and calls.count("uavgnn_qmix_mix_bwd") == 1
    assert bool(th.isfinite(out["LossQ"]))


def test_unsupported_embed_dim_takes_the_torch_formulation(monkeypatch):
    from tests.gpu_util import _LibSpy
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.agents.qmix import QMixer
    th.manual_seed(5)
    mix32 = QMixer(11, 3, types.SimpleNamespace(embed_dim=129))
    qs, states = th.randn(2, 3, 3), th.randn(2, 3, 11)
    y64 = copy.deepcopy(mix32).double()(qs.double(), states.double())
    spy = _LibSpy(L.lib())
    with monkeypatch.context() as mp:
        mp.setattr(L, "lib", lambda: spy)
        yg = copy.deepcopy(mix32).cuda()(qs.cuda(), states.cuda())
    assert not [c for c in spy.calls if "qmix" in c[0]]
    assert_close(yg, y64, 1e-5, "q_tot at e = 129")

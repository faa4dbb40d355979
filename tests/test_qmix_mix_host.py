"""The QMIX mixing kernels' contract without a GPU: the argument codes of the three C-ABI entries (csrc/qmix.hip) and the backward
formulas the kernel is asked to compute, written out in float64 and held against autograd of the torch formulation
(``agents.qmix.mix_torch``) on the reference fixture tests/golden/qmixer.npz.  The kernels themselves: tests/test_qmix_mix_gpu.py."""
import math
import types

import numpy as np
import torch as th

from oracle.closed_form import closed_form_tensor
from tests.util import GOLDEN, assert_close
from uav_bs_ctrl_amd import _lib
from uav_bs_ctrl_amd.agents.qmix import QMixer, mix_torch
from uav_bs_ctrl_amd.build import build_lib


def test_argument_codes_of_the_mixing_entries():
    build_lib()
    L = _lib.lib()
    # NULL operands: UAVGNN_EINVAL whatever the shape
    assert L.uavgnn_qmix_mix_fwd(None, 11 * 32, None, None, None, 4, 8, 32, None, None) == _lib.UAVGNN_EINVAL
    assert L.uavgnn_qmix_mix_bwd(None, 11 * 32, None, None, None, 4, 8, 32, None, 11 * 32, None, None, 1, None) == _lib.UAVGNN_EINVAL
    # unsupported shapes (rows = 0: nothing would be launched or dereferenced, so any non-NULL address will do)
    p = 4096
    for n, e in ((17, 32), (8, 129), (8, 0), (0, 32)):
        ld = max((n + 3) * e, 1)
        assert L.uavgnn_qmix_mix_fwd(p, ld, p, p, p, 0, n, e, p, None) == _lib.UAVGNN_EUNSUPPORTED, (n, e)
        assert L.uavgnn_qmix_mix_bwd(p, ld, p, p, p, 0, n, e, p, ld, p, p, 1, None) == _lib.UAVGNN_EUNSUPPORTED, (n, e)
    # rows == 0 on a supported shape: success without a launch; a row stride shorter than the row, or a foreign G: UAVGNN_EINVAL
    assert L.uavgnn_qmix_mix_fwd(p, 11 * 32, p, p, p, 0, 8, 32, p, None) == 0
    assert L.uavgnn_qmix_mix_bwd(p, 11 * 32, p, p, p, 0, 8, 32, p, 11 * 32, p, p, L.uavgnn_qmix_mix_bwd_partials(0, 32), None) == 0
    assert L.uavgnn_qmix_mix_fwd(p, 11 * 32 - 1, p, p, p, 0, 8, 32, p, None) == _lib.UAVGNN_EINVAL
    assert L.uavgnn_qmix_mix_bwd(p, 11 * 32, p, p, p, 0, 8, 32, p, 11 * 32, p, p, 7, None) == _lib.UAVGNN_EINVAL
    # the number of partial rows: positive, a function of the shape only, never more than one workgroup per row group
    for rows, e in ((0, 32), (1, 32), (37, 5), (1600, 32), (204800, 32), (5, 128), (130, 1)):
        G = L.uavgnn_qmix_mix_bwd_partials(rows, e)
        assert G >= 1 and G == L.uavgnn_qmix_mix_bwd_partials(rows, e), (rows, e)
        assert G <= max(rows, 1)
    assert L.uavgnn_qmix_mix_bwd_partials(204800, 32) > L.uavgnn_qmix_mix_bwd_partials(8, 32)
    assert L.uavgnn_qmix_mix_bwd_partials(8, 129) == _lib.UAVGNN_EUNSUPPORTED


def mix_backward_formulas(proj, qs, g, v2w, n, e):
    """(d_proj, d_qs, d_v2w, d_v2b) of q_tot = mix(proj, qs) under the upstream gradient g [rows], as csrc/qmix.hip computes them."""
    rows = proj.shape[0]
    w1, wf, b1, vh = proj.split((n * e, e, e, e), 1)
    w1 = w1.view(rows, n, e)
    pre = (qs.unsqueeze(2) * w1.abs()).sum(1) + b1
    hid = th.where(pre > 0, pre, th.expm1(pre))
    g = g.view(rows, 1)
    d_wf = g * hid * th.sign(wf)                                    # sign(0) = 0
    d_vh = g * v2w.view(1, e) * (vh > 0).to(proj.dtype)
    d_pre = g * wf.abs() * th.where(pre > 0, th.ones_like(pre), th.exp(pre))
    d_w1 = d_pre.unsqueeze(1) * qs.unsqueeze(2) * th.sign(w1)
    d_qs = (d_pre.unsqueeze(1) * w1.abs()).sum(2)
    d_proj = th.cat([d_w1.reshape(rows, n * e), d_wf, d_pre, d_vh], 1)
    return d_proj, d_qs, (g * vh.clamp_min(0)).sum(0), g.sum().view(1)


def test_backward_formulas_equal_autograd_of_the_torch_formulation_on_the_reference_fixture():
    z = np.load(f"{GOLDEN}/qmixer.npz")
    T, B, n = z["qs"].shape
    S, e = z["states"].shape[-1], 8
    mix = QMixer(S, n, types.SimpleNamespace(embed_dim=e)).double()
    with th.no_grad():
        for i, (k, p) in enumerate(mix.named_parameters()):
            p.copy_(closed_form_tensor(p.shape, 1.0 + i * math.pi / 7, 0.1 if p.dim() == 1 else 0.25, th.float64))
    heads = (mix.hyper_w_1, mix.hyper_w_final, mix.hyper_b_1, mix.V[0])
    qs, states = th.as_tensor(z["qs"]).reshape(-1, n), th.as_tensor(z["states"]).reshape(-1, S)
    with th.no_grad():
        proj = th.nn.functional.linear(states, th.cat([m.weight for m in heads], 0), th.cat([m.bias for m in heads], 0))
        # the split formulation on this proj IS the fixture's mixer
        assert_close(mix_torch(proj, qs, n, e, mix.V[2].weight, mix.V[2].bias).view(T, B, 1), th.as_tensor(z["y"]), 1e-12, "q_tot")
        planted = [(3, 2 * e + 5), (7, n * e + 1), (11, (n + 2) * e + 6), (0, 0)]        # w1 (agent 2), w_final, v_hid, w1
        for r, c in planted:
            proj[r, c] = 0.0
    pre = (qs.unsqueeze(2) * proj[:, :n * e].view(-1, n, e).abs()).sum(1) + proj[:, (n + 1) * e:(n + 2) * e]
    vh = proj[:, (n + 2) * e:]
    assert bool((pre > 0).any()) and bool((pre < 0).any()) and bool((vh > 0).any()) and bool((vh < 0).any())
    proj.requires_grad_(True), qs.requires_grad_(True)
    g = th.as_tensor(z["w"]).reshape(-1)
    y = mix_torch(proj, qs, n, e, mix.V[2].weight, mix.V[2].bias)
    ref = th.autograd.grad((y.view(-1) * g).sum(), [proj, qs, mix.V[2].weight, mix.V[2].bias])
    got = mix_backward_formulas(proj.detach(), qs.detach(), g, mix.V[2].weight.detach().view(-1), n, e)
    for name, a, b in zip(("d_proj", "d_qs", "d_v2w", "d_v2b"), got, ref):
        assert_close(a.reshape(b.shape), b, 1e-12, name)
    for r, c in planted:
        assert float(ref[0][r, c]) == 0.0 and float(got[0][r, c]) == 0.0, f"planted zero at ({r}, {c})"

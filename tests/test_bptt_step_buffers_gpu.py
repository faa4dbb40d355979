"""`-m gpu`: the backward of the recurrent step with ONE packed gate-gradient buffer G = [dn_h | dr | dz | dn_i] (`UAVGNN_G4`, the packed
mode of ``uavgnn_gru_gates_bwd_fused_sums_rowmax``) and d c = d_gi W_ih[:, H:] on the 128 x 64-tile f16x2 kernel (`UAVGNN_DC_H2`,
``uavgnn_gemm_nt_h2_n64``).

The two switches are read when ``uav_bs_ctrl_amd.ops`` is imported, so every arm of an A/B runs in a child process of its own (this
file run as a script: ``python tests/test_bptt_step_buffers_gpu.py <cases> <out.pt>`` under the arm's environment) and hands its tensors
back through a file.  The packed buffer changes where numbers are stored, not how they are computed: every comparison of the two layouts
is ``torch.equal``.  The new product is held to float64 with the measure and the bounds of
``test_gemm_f16x2_vs_float64_and_the_other_gemms`` (|err| / sum_k |a_k b_k|), against the vendor fp32 product on the same data."""
import json
import os
import subprocess
import sys

import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TN_ROWS = 4096      # GEMM_TN_MIN_ROWS of the 16384-row cases (as tests/test_gpu_parity.py: the sequence's f16x2 weight gradients run)
B, NA, T = 2048, 8, 1          # the "16384 rows" case of tests/gpu_util.py: UPDATE_CASES


# ---------------------------------------------------------------------------------------------------------------------
# child process: one arm of the switches
# ---------------------------------------------------------------------------------------------------------------------
def _learner_and_chunks(rho, hidden=256, msg=64, M_gt=6, Bc=B, Tc=T, seed=3):
    """The exp3 learner of test_learner_update_at_exp3_sizes_vs_oracle (tests/gpu_util.py: _exp3_learner_and_sequence) with `hidden` /
    `msg` overridable, and `rho` distinct sampled chunks."""
    import bench
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    th.manual_seed(seed)
    args = bench.exp3_args("cuda")
    args.hidden_size, args.msg_size = hidden, msg
    learner = MultiAgentQLearner(dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=9, n_agents=NA, episode_limit=Tc), args)
    gen = th.Generator(device="cuda").manual_seed(1000 + seed)
    with th.no_grad():
        for prm in learner.policy_net.parameters():
            if prm.dim() == 1:
                prm.add_(0.05 * th.randn(prm.shape, device="cuda", generator=gen))
        for pt, pp in zip(learner.target_net.parameters(), learner.policy_net.parameters()):
            pt.copy_(pp + 0.02 * pp.abs().mean() * th.randn(pp.shape, device="cuda", generator=gen))
    learner.invalidate_weight_cache()
    chunks = []
    for i in range(rho):
        b = bench.make_sequence(Bc, NA, M_gt, Tc, "dense", th.device("cuda"), seed=7 + seed + 13 * i, distinct=2)
        b["h0"] = 0.1 * th.randn(Bc * NA, hidden, device="cuda", generator=gen)          # stored hidden states, not zeros
        b["h1"] = 0.1 * th.randn(Bc * NA, hidden, device="cuda", generator=gen)
        chunks.append(b)
    return learner, chunks


def _flat_params(net):
    return th.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu()


def _error_rows(out, vend, a, W):
    """|err| / sum_k |a_k b_k| of the f16x2 product and of the vendor fp32 product against float64 (tests/test_gpu_parity.py)."""
    ref = a.double() @ W.double()
    den = a.double().abs() @ W.double().abs()
    rows = []
    for tag, o in (("f16x2 128x64", out), ("vendor fp32", vend)):
        e = (o.double() - ref).abs() / den.clamp_min(1e-300)
        e = e[den > 0]
        rows.append(dict(what=tag, max=float(e.max()), mean=float(e.mean())))
    return rows


def _child_update(rho, hidden=256, msg=64):
    """accumulate + optimizer step under the library spy; the torch side (th.mm shapes) is recorded too."""
    from tests.gpu_util import _LibSpy
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    learner, chunks = _learner_and_chunks(rho, hidden, msg)
    ops.GEMM_TN_MIN_ROWS = TN_ROWS
    real_lib, real_mm = L.lib, th.mm
    spy = _LibSpy(real_lib())
    mms = []

    def mm_spy(a, b, *rest, **kw):
        mms.append((tuple(a.shape), tuple(b.shape)))
        return real_mm(a, b, *rest, **kw)
    L.lib, th.mm = (lambda: spy), mm_spy
    try:
        out = learner.accumulate(chunks if rho > 1 else chunks[0])
    finally:
        L.lib, th.mm = real_lib, real_mm
    flat = learner.grads.flat.clone().cpu()
    learner.apply()
    th.cuda.synchronize()
    gate = [a for nm, a in spy.calls if nm == "uavgnn_gru_gates_bwd_fused_sums_rowmax"]
    return dict(flat=flat, loss=out["LossQ"].detach().cpu(), policy=_flat_params(learner.policy_net), target=_flat_params(learner.target_net),
                called=sorted(set(nm for nm, _ in spy.calls)), mms=mms,
                packed_gate_calls=sum(1 for a in gate if a[8] == a[9] + 4 * a[7]), gate_calls=len(gate),
                n64_shapes=sorted({(a[2], a[6], a[3]) for nm, a in spy.calls if nm == "uavgnn_gemm_nt_h2_n64"}),
                tn_shapes=sorted({(a[2], a[5]) for nm, a in spy.calls if nm == "uavgnn_gemm_tn_h2"}))


def _child_c3_dc():
    """The d c product of one backward step of a C3-size update (N = 32 768 rows, H = 256, M = 64) on its own operands: the d_gi the gate
    kernel wrote and the learner's W_ih - against float64 and the vendor product."""
    from uav_bs_ctrl_amd import ops
    learner, chunks = _learner_and_chunks(1, M_gt=80, Bc=4096, Tc=2)
    taken, real = [], ops.gemm_h2_n64

    def keep(a, W, rowmax, out=None):
        y = real(a, W, rowmax, out=out)
        taken.append((a.detach().clone(), W.detach().clone(), y.detach().clone(), a.stride(0)))
        return y
    ops.gemm_h2_n64 = keep
    try:
        learner.accumulate(chunks[0])
    finally:
        ops.gemm_h2_n64 = real
    assert len(taken) == 3, f"{len(taken)} d c products on the 128 x 64-tile kernel in a T + 1 = 3 step sequence"
    a, W, y, ld = taken[-1]          # time step 0, the last of the backward: its d h' carries the whole sequence (the Q values of step
    #                                  T only pick the double-Q action: that step's gate gradients are zero)
    rows = _error_rows(y, th.mm(a, W), a, W)
    return dict(rows=rows, shape=(tuple(a.shape), tuple(W.shape)), ld=ld)


def _child_main(cases, out_path):
    res = {}
    for c in cases.split(","):
        if c == "rho1":
            res[c] = _child_update(1)
        elif c == "rho2":
            res[c] = _child_update(2)
        elif c == "h128":
            res[c] = _child_update(1, hidden=128)
        elif c == "m32":
            res[c] = _child_update(1, msg=32)
        elif c == "c3_dc":
            res[c] = _child_c3_dc()
        else:
            raise ValueError(c)
    th.save(res, out_path)


# ---------------------------------------------------------------------------------------------------------------------
# parent
# ---------------------------------------------------------------------------------------------------------------------
_ARMS = {}


def _arm(g4, dc, cases, tmp_path_factory):
    """Results of `cases` under UAVGNN_G4 = g4, UAVGNN_DC_H2 = dc (None: the variable is unset - the defaults), one child per arm."""
    key = (g4, dc, cases)
    if isinstance(_ARMS.get(key), str):      # the arm failed before: not started again
        pytest.fail(_ARMS[key])
    if key not in _ARMS:
        env = {k: v for k, v in os.environ.items() if k not in ("UAVGNN_G4", "UAVGNN_DC_H2")}
        if g4 is not None:
            env["UAVGNN_G4"] = g4
        if dc is not None:
            env["UAVGNN_DC_H2"] = dc
        out = str(tmp_path_factory.mktemp("bptt_step") / "arm.pt")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), cases, out], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=900)
        if r.returncode != 0:
            _ARMS[key] = f"child (G4={g4}, DC_H2={dc}, {cases}) failed with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
            pytest.fail(_ARMS[key])
        _ARMS[key] = th.load(out)
    return _ARMS[key]


def _packed(tmp_path_factory):
    return _arm("1", "0", "rho1,rho2", tmp_path_factory)


def _plain(tmp_path_factory):
    return _arm("0", "0", "rho1,rho2,h128,m32", tmp_path_factory)


def _defaults(tmp_path_factory):
    return _arm(None, None, "rho1,h128,m32,c3_dc", tmp_path_factory)


@pytest.mark.parametrize("case", ["rho1", "rho2"])
def test_packed_gate_gradient_buffer_leaves_the_update_bit_identical(case, tmp_path_factory):
    """Part A: one ``learner.accumulate`` + optimizer step at exp3 sizes (16 384 rows; rho = 1, and rho = 2: stage buffers and sink slots
    reused across chunks), UAVGNN_G4=1 against UAVGNN_G4=0, both with the vendor d c product: the flat gradient buffer, the loss and
    both parameter sets after the step are bit-identical.  No tolerance - the arithmetic is unchanged."""
    new, old = _packed(tmp_path_factory)[case], _plain(tmp_path_factory)[case]
    assert new["gate_calls"] > 0 and new["packed_gate_calls"] == new["gate_calls"], (new["packed_gate_calls"], new["gate_calls"])
    assert old["gate_calls"] == new["gate_calls"] and old["packed_gate_calls"] == 0
    assert not new["n64_shapes"] and not old["n64_shapes"]
    assert (768, 320) in new["tn_shapes"] and (768, 256) in new["tn_shapes"], new["tn_shapes"]
    assert bool(th.isfinite(new["flat"]).all())
    ne = int((new["flat"] != old["flat"]).sum())
    assert th.equal(new["flat"], old["flat"]), f"{case}: {ne} of {new['flat'].numel()} gradient elements differ, max |diff| " \
                                               f"{float((new['flat'] - old['flat']).abs().max()):.3e}"
    assert th.equal(new["loss"], old["loss"])
    assert th.equal(new["policy"], old["policy"]) and th.equal(new["target"], old["target"])


@pytest.mark.parametrize("N,head", [(5000, True), (40000, False), (257, True)])
def test_packed_gate_call_stores_every_gate_gradient_once(N, head):
    """The packed call (d_gi == d_gh + H) against the plain call on the same inputs: G = [dn_h | dr | dz | dn_i] holds the columns of d_gi /
    d_gh bit for bit, row_absmax, col_sums and d_h are equal, and nothing outside G's [N, 4H] is written (guard rows on both sides)."""
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    H, A, GUARD, MARK = 256, 9, 4, -7.25
    gen = th.Generator().manual_seed(N)
    pre, h, dh = (th.randn(N, 4 * H, generator=gen).cuda(), th.tanh(th.randn(N, H, generator=gen)).cuda(), th.randn(N, H, generator=gen).cuda())
    dq, Wo = th.randn(N, A, generator=gen).cuda(), th.randn(A, H, generator=gen).cuda()
    R = lib.uavgnn_gru_gates_bwd_sum_rows(N, H)
    d_gi, d_gh = th.full((N, 3 * H), MARK, device="cuda"), th.full((N, 3 * H), MARK, device="cuda")
    buf = th.full((N + 2 * GUARD, 4 * H), MARK, device="cuda")
    G = buf[GUARD:GUARD + N]
    outs = []
    for gi_ptr, gh_ptr in ((d_gi.data_ptr(), d_gh.data_ptr()), (G.data_ptr() + 4 * H, G.data_ptr())):
        d_h, sums, rowmax = th.full((N, H), MARK, device="cuda"), th.full((R, 4 * H), MARK, device="cuda"), th.full((N,), -1.0, device="cuda")
        L.check(lib.uavgnn_gru_gates_bwd_fused_sums_rowmax(pre.data_ptr(), h.data_ptr(), dh.data_ptr(), dq.data_ptr() if head else None,
                                                           A if head else 0, Wo.data_ptr() if head else None, N, H, gi_ptr, gh_ptr,
                                                           d_h.data_ptr(), sums.data_ptr(), rowmax.data_ptr(), L.stream()), "gate kernel")
        outs.append((d_h, sums, rowmax))
    th.cuda.synchronize()
    for a, b, what in zip(outs[0], outs[1], ("d_h", "col_sums", "row_absmax")):
        assert th.equal(a, b), what
    assert th.equal(G[:, :H], d_gh[:, 2 * H:]), "dn_h"
    assert th.equal(G[:, H:3 * H], d_gi[:, :2 * H]) and th.equal(G[:, H:3 * H], d_gh[:, :2 * H]), "dr | dz"
    assert th.equal(G[:, 3 * H:], d_gi[:, 2 * H:]), "dn_i"
    assert th.equal(outs[1][2], G.abs().max(1).values)
    assert bool((buf[:GUARD] == MARK).all()) and bool((buf[GUARD + N:] == MARK).all()), "the packed call wrote outside [N, 4H]"
    assert not bool((G == MARK).any())


DC_ROWS = []


def _dump_rows():
    """The error rows as JSON in the directory UAVGNN_ERROR_TABLE_DIR names (profiles/bptt_step_error_table.json is a copy); unset: not kept."""
    d = os.environ.get("UAVGNN_ERROR_TABLE_DIR")
    if not d:
        return
    try:
        with open(os.path.join(d, "bptt_step_error_table.json"), "w") as f:
            json.dump(DC_ROWS, f, indent=1)
    except OSError:
        pass


def _assert_dc_bounds(rows, what):
    print(what, rows)
    assert rows[0]["max"] < 4e-7 and rows[0]["mean"] < 4e-8, (what, rows)          # the absolute bar of test_gemm_f16x2_vs_float64_...
    assert rows[0]["mean"] <= 1.25 * rows[1]["mean"], (what, rows)                  # ... and relative to the vendor product
    assert rows[0]["max"] <= 2.0 * rows[1]["max"], (what, rows)


@pytest.mark.parametrize("M", [32768, 33001])
def test_dc_product_on_128x64_tiles_vs_float64(M):
    """Part B on the gradient-like operands of test_gemm_f16x2_vs_float64_and_the_other_gemms (rows whose magnitudes span six orders): K =
    768, 64 output columns, the activation a [M, 768] view of a [M, 1024] buffer (the packed gate-gradient layout), the weight a
    64-column view of a [768, 320] matrix; a ragged last row tile; rows outside the product untouched."""
    from uav_bs_ctrl_amd import ops
    K, N = 768, 64
    gen = th.Generator().manual_seed(M + N + K)
    buf = th.randn(M, 1024, generator=gen).cuda()
    buf[:, 256:] *= th.exp2(th.randint(-20, 1, (M, 1), generator=gen).float()).cuda()
    a = buf[:, 256:]
    W = (0.1 * th.randn(K, 320, generator=gen)).cuda()[:, 256:]
    rm = ops.row_absmax(a.contiguous())
    assert ops.gemm_h2_n64_supported(a, N, K)
    ybuf = th.full((M + 8, N), -7.25, device="cuda")
    out = ops.gemm_h2_n64(a, W, rm, out=ybuf[4:4 + M])
    th.cuda.synchronize()
    assert bool((ybuf[:4] == -7.25).all()) and bool((ybuf[4 + M:] == -7.25).all()), "rows outside [M, 64] written"
    ac, Wc = a.contiguous(), W.contiguous()
    rows = _error_rows(out, th.mm(ac, Wc), ac, Wc)
    DC_ROWS.append(dict(test="gradient-like operands", M=M, K=K, N=N, ldx=1024, rows=rows))
    _dump_rows()
    _assert_dc_bounds(rows, f"M={M}")
    # the columns are those of the 256 x 128-tile kernel, bit for bit (same split, same order over K)
    W4 = th.cat((Wc, Wc), 1)
    if ops.gemm_h2_supported(a, 128, K):
        big = ops.gemm_h2(a, W4, rm, True)
        assert th.equal(big[:, :64], out) and th.equal(big[:, 64:], out)


def test_dc_product_on_the_steps_own_operands_at_c3(tmp_path_factory):
    """Part B on d_gi / W_ih of a backward step of a C3-size update (N = 32 768, taken inside the default arm's child)."""
    r = _defaults(tmp_path_factory)["c3_dc"]
    assert r["shape"] == ((32768, 768), (768, 64)) and r["ld"] == 1024, r
    DC_ROWS.append(dict(test="step operands at C3 (d_gi of time step 0, W_ih[:, H:])", M=32768, K=768, N=64, ldx=r["ld"], rows=r["rows"]))
    _dump_rows()
    _assert_dc_bounds(r["rows"], "C3 step")


def test_default_dispatch_takes_the_packed_buffer_and_the_new_dc_kernel(tmp_path_factory):
    """With the defaults the update at 16 384 rows calls the packed gate kernel and uavgnn_gemm_nt_h2_n64 for d c, no [N, 768] x [768, 64]
    torch.mm, and still every entry test_learner_update_at_exp3_sizes_vs_oracle pins."""
    r = _defaults(tmp_path_factory)["rho1"]
    N = B * NA
    assert r["gate_calls"] == T + 1 and r["packed_gate_calls"] == T + 1, r
    assert r["n64_shapes"] == [(N, 64, 768)], r["n64_shapes"]
    assert not [s for s in r["mms"] if s == ((N, 768), (768, 64))], r["mms"]
    assert {"uavgnn_gru_gates_bwd_fused_sums_rowmax", "uavgnn_gemm_nt_h2_rm2", "uavgnn_talk_attn_env_bwd", "uavgnn_gemm_nt_h2",
            "uavgnn_gemm_tn_h2", "uavgnn_gemm_nt_h2_n64"} <= set(r["called"])
    assert {(768, 320), (768, 256)} <= {tuple(s) for s in r["tn_shapes"]}
    # the packed layout with the vendor d c is the plain update bit for bit (above); the f16x2 d c moves the gradients inside fp32 noise
    old = _plain(tmp_path_factory)["rho1"]
    d = (r["flat"] - old["flat"]).abs().max() / old["flat"].abs().max()
    print("default vs (G4=0, DC_H2=0): max |d grad| / max |grad| =", float(d))
    assert float(d) < 1e-5


@pytest.mark.parametrize("case", ["h128", "m32"])
def test_fallback_shapes_keep_the_old_path_bit_for_bit(case, tmp_path_factory):
    """H = 128 (no row maxima from the gate kernel) and M = 32 (no 64-column tile): the defaults take two gate-gradient buffers / the
    vendor d c product and equal the run with both switches off."""
    new, old = _defaults(tmp_path_factory)[case], _plain(tmp_path_factory)[case]
    N = B * NA
    assert not new["n64_shapes"], new["n64_shapes"]
    if case == "h128":
        assert new["packed_gate_calls"] == 0
    else:
        assert [s for s in new["mms"] if s == ((N, 768), (768, 32))], "d c of the M = 32 step not on the vendor GEMM"
        assert [s for s in old["mms"] if s == ((N, 768), (768, 32))]
    assert th.equal(new["loss"], old["loss"])
    if case == "h128":
        assert th.equal(new["flat"], old["flat"])
        assert th.equal(new["policy"], old["policy"]) and th.equal(new["target"], old["target"])
    else:
        # M = 32 keeps the packed buffer (Part A is bit-exact whatever M); its d c stays on the vendor GEMM
        assert new["packed_gate_calls"] == new["gate_calls"] > 0
        assert th.equal(new["flat"], old["flat"])
        assert th.equal(new["policy"], old["policy"]) and th.equal(new["target"], old["target"])


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])

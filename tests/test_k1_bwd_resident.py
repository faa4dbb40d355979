"""`-m gpu`: the K1 backward of the dense matrix-core class (F_src 4, nh 4, D 64; destinations with 16 .. 128 in-edges) with its
accumulators resident over all destinations of a wavefront (gatv2_bwd_resident_kernel, csrc/gatv2_bwd_mfma.hip) against the generic
backward on the same inputs, under the rule of the per-destination kernel's test (every element within 2e-5 of max|ref|, at most 8
per tensor within 1e-3: the two arithmetics of z may disagree on the sign of a z within rounding of zero), and bit-exact over
repeated launches.  At the flagship size (51 steps x 32 768 agents, 80 in-edges each: hundreds of destinations per wavefront) every
gradient is also held to a float64 evaluation of the same closed form, next to the per-destination kernel
(UAVGNN_K1_BWD_RESIDENT=0) on the same inputs."""
import json
import os

import pytest
import torch as th

from tests.k1_closed_form import float64_closed_form as _float64_closed_form

pytestmark = pytest.mark.gpu

H = 256
NAMES = ["dW_s", "db_s", "dW_d", "db_d", "dattn", "dW_r", "db_r"]
SLOPE = 0.2


def _problem(deg, seed, ld_out=512):
    """Forward of one `seen`-shaped relation with the given in-degrees on the GPU; returns run(fn) -> the seven gradients."""
    from uav_bs_ctrl_amd import _lib as L
    N = int(deg.numel())
    dev = "cuda"
    off = th.zeros(N + 1, dtype=th.int64)
    off[1:] = th.cumsum(deg.to(th.int64), 0)
    E = int(off[-1])
    assert E >= 16 * N, "the matrix-core path is chosen for a mean in-degree of 16 or more"
    gen = th.Generator(device=dev).manual_seed(seed)
    x_src = th.rand(E, 4, generator=gen, device=dev) * 2 - 1
    x_dst = th.rand(N, 2, generator=gen, device=dev)
    prm = [0.5 * th.randn(s, generator=gen, device=dev) for s in ((H, 4), (H,), (H, 2), (H,), (H,), (H, 2), (H,))]
    out = th.empty(N, ld_out, device=dev)
    a_save = th.empty(E, 4, device=dev)
    lib, st, offd = L.lib(), L.stream(), off.to(th.int32).to(dev)
    rc = lib.uavgnn_gatv2_fwd(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), None, N, *[t.data_ptr() for t in prm],
                              4, 64, SLOPE, out.data_ptr(), ld_out, a_save.data_ptr(), st)
    assert rc == 0
    d_out = th.randn(N, ld_out, generator=gen, device=dev)
    wsb = lib.uavgnn_gatv2_bwd_workspace_bytes(4, H)
    ws = th.empty(wsb // 4, device=dev)

    def run(fn):
        g = [th.full_like(t, float("nan")) for t in prm]
        rc = fn(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), None, N, *[t.data_ptr() for t in prm[:5]], 4, 64,
                SLOPE, out.data_ptr(), d_out.data_ptr(), ld_out, a_save.data_ptr(), *[t.data_ptr() for t in g], ws.data_ptr(), wsb,
                st)
        assert rc == 0, rc
        th.cuda.synchronize()
        return g

    data = dict(x_src=x_src, x_dst=x_dst, prm=prm, out=out, d_out=d_out, a_save=a_save, N=N)
    return run, lib, data


def _per_destination(monkeypatch, run, lib):
    with monkeypatch.context() as mp:
        mp.setenv("UAVGNN_K1_BWD_RESIDENT", "0")
        return run(lib.uavgnn_gatv2_bwd)


def _agree(g_new, g_ref, what):
    for a, b, nm in zip(g_new, g_ref, NAMES):
        assert bool(th.isfinite(a).all()), f"{nm}: {what}"
        scale = float(b.abs().max())
        err = (a - b).abs()
        loose = int((err > 2e-5 * scale).sum())
        assert loose <= 8 and float(err.max()) <= 1e-3 * scale, (
            f"{nm} ({what}): {loose} elements beyond 2e-5 of max|ref|, worst {float(err.max()) / scale:.3e} of max|ref|")


def _repeatable(run, fn, first, reps):
    for rep in range(reps):
        again = run(fn)
        for a, c, nm in zip(first, again, NAMES):
            assert th.equal(a, c), f"{nm}: resident backward not bit-reproducible (launch {rep + 2})"


@pytest.mark.parametrize("d", [16, 17, 31, 32, 33, 80, 127, 128])
def test_resident_k1_backward_exact_degrees(monkeypatch, d):
    """Every destination with exactly d in-edges: the edge-tile tails (16, 17, 31 .. 33), the flagship's 80 and both ends of the
    class; 8192 destinations put four of them on every wavefront of the 512-workgroup grid."""
    run, lib, _ = _problem(th.full((8192,), d, dtype=th.int64), seed=d)
    g_new, g_gen = run(lib.uavgnn_gatv2_bwd), run(lib.uavgnn_gatv2_bwd_generic)
    _repeatable(run, lib.uavgnn_gatv2_bwd, g_new, 4)
    _agree(g_new, g_gen, f"resident vs generic, degree {d}")
    _agree(g_new, _per_destination(monkeypatch, run, lib), f"resident vs per-destination, degree {d}")


@pytest.mark.parametrize("N,lo,hi,seed", [(6001, 0, 140, 1), (20000, 0, 40, 2), (9000, 120, 200, 3), (16384, 10, 22, 4)])
def test_resident_k1_backward_mixed_classes(monkeypatch, N, lo, hi, seed):
    """Degrees below 16 and above 128 (the packed-FMA launch behind the matrix-core one) mixed with the class, zero in-degrees
    included; the sum of the two launches' partial rows against the generic kernel."""
    gen = th.Generator().manual_seed(seed)
    deg = th.randint(lo, hi + 1, (N,), generator=gen)
    deg[: N // 8] = 20   # keep the mean in-degree at 16 or more (the matrix-core dispatch) for the low mixes
    deg[N // 8: N // 4] = 100
    run, lib, _ = _problem(deg, seed=100 + seed)
    g_new, g_gen = run(lib.uavgnn_gatv2_bwd), run(lib.uavgnn_gatv2_bwd_generic)
    _repeatable(run, lib.uavgnn_gatv2_bwd, g_new, 4)
    _agree(g_new, g_gen, "resident vs generic, mixed classes")
    _agree(g_new, _per_destination(monkeypatch, run, lib), "resident vs per-destination, mixed classes")


def _vs_generic(g, g_gen):
    """(elements beyond 2e-5 of max|ref|, worst error / max|ref|) per gradient."""
    rows = {}
    for a, b, nm in zip(g, g_gen, NAMES):
        scale = float(b.abs().max())
        err = (a - b).abs()
        rows[nm] = (int((err > 2e-5 * scale).sum()), float(err.max()) / scale)
    return rows


def test_resident_k1_backward_at_the_flagship_size_vs_float64(monkeypatch):
    """51 x 32 768 destinations with 80 in-edges each (the bench's dense `seen` relation): every wavefront accumulates over ~800
    destinations.  Bit-exact repeats; per gradient, error against float64 no worse than 1.5x the per-destination kernel's on the
    same inputs, and within 2e-5 of max|ref| once the sign-tie allowance of each element is granted.  The 8-element rule of the
    small sizes does not scale to 3.4e10 (edge, channel) pairs: there the per-destination kernel and the generic kernel differ
    from each other, and from float64, by more than 2e-5 of max|ref| in dW_s / db_s / dW_d / db_d (sign ties of z); at this size
    the resident, the per-destination and the generic kernel are all held to float64 under the same allowance instead."""
    deg = 80
    N = 51 * 32768
    run, lib, data = _problem(th.full((N,), deg, dtype=th.int64), seed=7, ld_out=H)
    g_new = run(lib.uavgnn_gatv2_bwd)
    _repeatable(run, lib.uavgnn_gatv2_bwd, g_new, 2)
    g_old = _per_destination(monkeypatch, run, lib)
    assert any(not th.equal(a, b) for a, b in zip(g_new, g_old)), "the A/B switch selects a different kernel"
    g_gen = run(lib.uavgnn_gatv2_bwd_generic)
    ref, tie = _float64_closed_form(data, deg)
    gen_new, gen_old = _vs_generic(g_new, g_gen), _vs_generic(g_old, g_gen)
    table = {}
    for a, b, c, r, t, nm in zip(g_new, g_old, g_gen, ref, tie, NAMES):
        scale = float(r.abs().max())
        row = {"max_abs_ref": scale, "tie_allowance_rel_max": float(t.max()) / scale}
        for kn, g in (("resident", a), ("per_destination", b), ("generic", c)):
            err = (g.double() - r).abs()
            row[kn + "_err_rel_max"] = float(err.max()) / scale
            row[kn + "_err_beyond_ties_rel_max"] = float((err - t).max()) / scale
        row.update({"resident_vs_generic_beyond_2e-5": gen_new[nm][0], "resident_vs_generic_worst_rel": gen_new[nm][1],
                    "per_destination_vs_generic_beyond_2e-5": gen_old[nm][0], "per_destination_vs_generic_worst_rel": gen_old[nm][1]})
        table[nm] = row
    print("K1_BWD_RESIDENT_ERROR_TABLE " + json.dumps(table))
    path = os.environ.get("UAVGNN_K1_BWD_ERROR_TABLE")
    if path:
        with open(path, "w") as f:
            json.dump({"N": N, "deg": deg, "errors_vs_float64": table}, f, indent=1)
    for nm, row in table.items():
        assert row["resident_err_rel_max"] <= 1.5 * row["per_destination_err_rel_max"], (nm, row)
        for kn in ("resident", "per_destination", "generic"):
            assert row[kn + "_err_beyond_ties_rel_max"] <= 2e-5, (nm, kn, row)

#!/usr/bin/env python
"""Repeatability and A/B probe of the K1 backward (`seen` shape: F_src 4, nh 4, D 64) through the C-ABI.

    CASES="[(4096,64,64),(8192,16,130)]" REPS=100 python tools/k1_bwd_repro.py       launches per case that differ from the first
    REL=1  ... per-gradient difference between uavgnn_gatv2_bwd (matrix cores for mean degree >= 16) and the generic kernel
    ROWS=1 ... which workgroups' partial rows differ between launches, and in which gradient segment
    TIME=1 ... 20 extra launches of each entry (for rocprofv3 --kernel-trace)
    UAVGNN_K1_BWD_MFMA=0 sends every destination through the packed-FMA kernel.

    python tools/k1_bwd_repro.py --deg 80 [--n 1671168] [--launches 20]      timing run: the data is made on the GPU, only
    uavgnn_gatv2_bwd is launched (for rocprofv3 --kernel-trace); --deg D or LO..HI (uniform), e.g. 80, 96, 16..52.  The A/B
    switches of the launcher (UAVGNN_K1_BWD_RESIDENT / _PREFETCH / _HALFTRIP) select the kernel.

This is the script that located the gfx950 packed-fp32 / bf16-MFMA hazard (tools/ubench/mfma_pk_hazard.hip):
CASES are (destinations, min degree, max degree).
"""
import argparse, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th
from uav_bs_ctrl_amd import _lib as L
ap = argparse.ArgumentParser()
ap.add_argument("--deg", help="timing run at this in-degree: D, or LO..HI for a uniform mix")
ap.add_argument("--n", type=int, default=51 * 32768, help="destinations of the timing run (default: the bench's 51 x 32768)")
ap.add_argument("--launches", type=int, default=20)
args = ap.parse_args()
def timing_run(lo, hi, N, launches):
    dev = "cuda"; gen = th.Generator(device=dev).manual_seed(11); H = 256
    deg = th.randint(lo, hi + 1, (N,), generator=gen, device=dev)
    off = th.zeros(N + 1, dtype=th.int64, device=dev); off[1:] = th.cumsum(deg, 0); E = int(off[-1]); offd = off.to(th.int32)
    x_src = th.rand(E, 4, generator=gen, device=dev) * 2 - 1; x_dst = th.rand(N, 2, generator=gen, device=dev)
    prm = [0.5 * th.randn(s, generator=gen, device=dev) for s in ((H, 4), (H,), (H, 2), (H,), (H,), (H, 2), (H,))]
    out = th.empty(N, H, device=dev); a_save = th.empty(E, 4, device=dev); lib, st = L.lib(), L.stream()
    assert lib.uavgnn_gatv2_fwd(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), None, N, *[t.data_ptr() for t in prm], 4, 64, 0.2, out.data_ptr(), H, a_save.data_ptr(), st) == 0
    d_out = th.randn(N, H, generator=gen, device=dev)
    wsb = lib.uavgnn_gatv2_bwd_workspace_bytes(4, H); ws = th.empty(wsb // 4, device=dev)
    g = [th.empty_like(t) for t in prm]
    ev = [th.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    for i in range(launches + 1):
        ev[i].record()
        if i < launches:
            assert lib.uavgnn_gatv2_bwd(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), None, N, *[t.data_ptr() for t in prm[:5]], 4, 64, 0.2, out.data_ptr(), d_out.data_ptr(), H, a_save.data_ptr(), *[t.data_ptr() for t in g], ws.data_ptr(), wsb, st) == 0
    th.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(2, launches))   # the first two launches are warm-up
    print(f"k1_bwd N {N} deg {lo}..{hi} E {E}: whole backward (3 kernels) per launch ms min {ms[0]:.3f} p50 {ms[len(ms) // 2]:.3f} max {ms[-1]:.3f}"
          f" ; checksum {float(sum(t.double().sum() for t in g)):.9e}")
if args.deg:
    lo, _, hi = args.deg.partition("..")
    timing_run(int(lo), int(hi or lo), args.n, args.launches)
    sys.exit(0)
def case(N, lo, hi, seed):
    gen = th.Generator().manual_seed(seed)
    deg = th.randint(lo, hi + 1, (N,), generator=gen)
    off = th.zeros(N + 1, dtype=th.int32); off[1:] = th.cumsum(deg, 0); E = int(off[-1]); dev = "cuda"
    x_src = (th.rand(max(E, 1), 4, generator=gen) * 2 - 1).to(dev); x_dst = th.rand(N, 2, generator=gen).to(dev)
    H = 256
    prm = [(0.5 * th.randn(s, generator=gen)).to(dev) for s in ((H, 4), (H,), (H, 2), (H,), (H,), (H, 2), (H,))]
    out = th.empty(N, 512, device=dev); a_save = th.empty(max(E, 1), 4, device=dev)
    lib, st, offd = L.lib(), L.stream(), off.to(dev)
    assert lib.uavgnn_gatv2_fwd(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), None, N, *[t.data_ptr() for t in prm], 4, 64, 0.2, out.data_ptr(), 512, a_save.data_ptr(), st) == 0
    d_out = th.randn(N, 512, generator=gen).to(dev)
    mode = os.environ.get("MASK", "")
    if mode == "first": d_out[2048:] = 0
    if mode == "second": d_out[:2048] = 0
    wsb = lib.uavgnn_gatv2_bwd_workspace_bytes(4, H); ws = th.empty(wsb // 4, device=dev)
    def run(fn):
        g = [th.full_like(t, float("nan")) for t in prm]
        assert fn(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), None, N, *[t.data_ptr() for t in prm[:5]], 4, 64, 0.2, out.data_ptr(), d_out.data_ptr(), 512, a_save.data_ptr(), *[t.data_ptr() for t in g], ws.data_ptr(), wsb, st) == 0
        th.cuda.synchronize(); return g
    return run, lib, ws
cases = eval(os.environ.get("CASES", "[(4096, 64, 64), (4096, 48, 48), (8192, 100, 128)]"))
for (N, lo, hi) in cases:
    run, lib, ws = case(N, lo, hi, 11)
    ref = run(lib.uavgnn_gatv2_bwd)
    gen_ = run(lib.uavgnn_gatv2_bwd_generic)
    nbad = 0
    for rep in range(int(os.environ.get("REPS", "6"))):
        b = run(lib.uavgnn_gatv2_bwd)
        if any(not th.equal(x, y) for x, y in zip(ref, b)):
            nbad += 1
    print(N, lo, hi, "nondeterministic runs:", nbad, "of", os.environ.get("REPS", "6"), "; max |mf - generic| db_s", float((ref[1] - gen_[1]).abs().max()))
    if os.environ.get("TIME"):
        for fn in (lib.uavgnn_gatv2_bwd, lib.uavgnn_gatv2_bwd_generic):
            for _ in range(20): run(fn)
    if os.environ.get("ROWS"):
        g = min((N + 3) // 4, 512); P = 256 * 12    # the library's grid of the matrix-core launch
        run(lib.uavgnn_gatv2_bwd); r0 = ws[: 2 * g * P].clone().view(2 * g, P)
        names = [("dW_s", 0, 1024), ("db_s", 1024, 1280), ("dW_d", 1280, 1792), ("db_d", 1792, 2048), ("datt", 2048, 2304), ("dW_r", 2304, 2816), ("db_r", 2816, 3072)]
        for rep in range(5):
            run(lib.uavgnn_gatv2_bwd); r1 = ws[: 2 * g * P].view(2 * g, P)
            bad = (r0 != r1)
            rows = bad.any(1).nonzero().flatten().tolist()
            print(" rep", rep, "rows differing:", rows[:12], "n", len(rows))
            for r in rows[:3]:
                for nm, a, b in names:
                    idx = bad[r, a:b].nonzero().flatten()
                    if len(idx):
                        ch = idx.tolist()
                        print("    row", r, nm, "count", len(ch), "idx", ch[:24], "maxdiff", float((r0[r, a:b] - r1[r, a:b]).abs().max()))
    if os.environ.get("REL"):
        a = run(lib.uavgnn_gatv2_bwd); b = run(lib.uavgnn_gatv2_bwd_generic)
        for x, y, nm in zip(a, b, ["dW_s", "db_s", "dW_d", "db_d", "dattn", "dW_r", "db_r"]):
            d = (x - y).abs()
            print("   ", nm, "max|d|", float(d.max()), "max|ref|", float(y.abs().max()), "rel-to-max", float(d.max() / y.abs().max()), "n(|d| > 1e-5 max)", int((d > 1e-5 * y.abs().max()).sum()), "of", d.numel())

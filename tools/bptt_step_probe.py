#!/usr/bin/env python
"""The five launches of ONE backward step of the recurrent TarMAC step at C3 size (N = 32 768 rows, H = 256, M = 64, K = 16), old
layout against new, microseconds per launch:

    gate gradients   two [N, 3H] buffers d_gi / d_gh            | ONE packed [N, 4H] buffer G = [dn_h | dr | dz | dn_i]
    d c              vendor fp32 GEMM d_gi W_ih[:, H:]          | uavgnn_gemm_nt_h2_n64 (f16x2, 128 x 64 tiles) on G[:, H:]
    attention bwd    uavgnn_talk_attn_env_bwd (the same launch on both sides: d c is a contiguous [N, M] either way)
    d h += d_gh W_hh one source, K = 768                        | two sources G[:, H:3H], G[:, :H] over [W_hh[:2H]; W_hh[2H:]]
    d x              [d_gi || d_proj] [W_ih_x; Wp_x], ldx = 768 | the same with d_gi = G[:, H:], ldx = 1024

The launches of a side run back to back in the step's order (so each finds in the last-level cache what its predecessor left, as in the
update), timed per launch with event pairs over `--reps` rounds; the medians are printed.  GPU box.

    python tools/bptt_step_probe.py [--reps 30]
"""
import argparse
import os
import statistics
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uav_bs_ctrl_amd import _lib as L, enable_tuned_gemms, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--N", type=int, default=32768)
a_ = ap.parse_args()
enable_tuned_gemms()
dev = th.device("cuda")
N, H, M, K, n = a_.N, 256, 64, 16, 8
lib, st = L.lib(), L.stream()
gen = th.Generator(device=dev).manual_seed(0)
rnd = lambda *s, scale=1.0: scale * th.randn(*s, device=dev, generator=gen)   # noqa: E731
pre, h, dh2 = rnd(N, 4 * H), th.tanh(rnd(N, H)), rnd(N, H, scale=1e-3)
dq, W_out = rnd(N, 9, scale=1e-3), rnd(9, H, scale=0.1)
W_ih, W_hh, Wp = rnd(3 * H, H + M, scale=0.05), rnd(3 * H, H, scale=0.05), rnd(M + 2 * K, 2 * H, scale=0.05)
proj, ld = rnd(N, M + 2 * K), M + 2 * K
off = th.arange(0, N * n + 1, n, dtype=th.int32, device=dev)
src = ((th.arange(N, device=dev) // n * n).repeat_interleave(n) + th.arange(n, device=dev).repeat(N)).to(th.int32)
go = th.arange(0, N + 1, n, dtype=th.int32, device=dev)
env = (go, N // n, n)
a_save = th.softmax(rnd(N, n), 1).reshape(-1).contiguous()
R = lib.uavgnn_gru_gates_bwd_sum_rows(N, H)
sums, rm_g, rm_p = th.empty(R, 4 * H, device=dev), th.empty(N, device=dev), th.empty(N, device=dev)
d_gi, d_gh, G = th.empty(N, 3 * H, device=dev), th.empty(N, 3 * H, device=dev), th.empty(N, 4 * H, device=dev)
d_proj, dx = th.empty(N, ld, device=dev), th.empty(N, H, device=dev)
dh = {"old": th.empty(N, H, device=dev), "new": th.empty(N, H, device=dev)}
d_c = {"old": th.empty(N, M, device=dev), "new": th.empty(N, M, device=dev)}


def gate(gi, gh, out_h):
    L.check(lib.uavgnn_gru_gates_bwd_fused_sums_rowmax(pre.data_ptr(), h.data_ptr(), dh2.data_ptr(), dq.data_ptr(), 9, W_out.data_ptr(), N, H,
                                                       gi.data_ptr(), gh.data_ptr(), out_h.data_ptr(), sums.data_ptr(), rm_g.data_ptr(), st), "gate")


def attn(dc):
    ops._launch_talk_bwd(env, proj.data_ptr() + 4 * M, ld, proj.data_ptr() + 4 * (M + K), ld, proj.data_ptr(), ld, K, M, off, src, None, N,
                         1.0 / K, a_save, dc.data_ptr(), M, d_proj.data_ptr() + 4 * M, ld, d_proj.data_ptr() + 4 * (M + K), ld,
                         d_proj.data_ptr(), ld)


STEPS = {
    "old": [("gate gradients", lambda: gate(d_gi, d_gh, dh["old"])),
            ("d c", lambda: th.mm(d_gi, W_ih[:, H:], out=d_c["old"])),
            ("d h += d_gh W_hh", lambda: ops.gemm_h2(d_gh, W_hh, rm_g, True, out=dh["old"], accumulate=True)),
            ("attention bwd", lambda: attn(d_c["old"])),
            ("d x", lambda: ops.gemm_h2(d_gi, W_ih[:, :H], rm_g, True, out=dx, a2=d_proj, W2=Wp[:, :H], rowmax2_out=rm_p))],
    "new": [("gate gradients", lambda: gate(G[:, H:], G, dh["new"])),
            ("d c", lambda: ops.gemm_h2_n64(G[:, H:], W_ih[:, H:], rm_g, out=d_c["new"])),
            ("d h += d_gh W_hh", lambda: ops.gemm_h2(G[:, H:3 * H], W_hh[:2 * H], rm_g, True, out=dh["new"], accumulate=True, a2=G[:, :H],
                                                     W2=W_hh[2 * H:])),
            ("attention bwd", lambda: attn(d_c["new"])),
            ("d x", lambda: ops.gemm_h2(G[:, H:], W_ih[:, :H], rm_g, True, out=dx, a2=d_proj, W2=Wp[:, :H], rowmax2_out=rm_p))],
}

with ops.frozen_weights():
    res = {}
    for side in ("old", "new", "old", "new"):          # two passes: the second's figures are printed
        steps = STEPS[side]
        for _ in range(3):
            for _, f in steps:
                f()
        th.cuda.synchronize()
        ev = [[(th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)) for _ in steps] for _ in range(a_.reps)]
        for r in range(a_.reps):
            for i, (_, f) in enumerate(steps):
                ev[r][i][0].record()
                f()
                ev[r][i][1].record()
        th.cuda.synchronize()
        res[side] = [statistics.median(ev[r][i][0].elapsed_time(ev[r][i][1]) * 1e3 for r in range(a_.reps)) for i in range(len(steps))]
    same_h = bool(th.equal(dh["old"], dh["new"]))
    e = (d_c["new"] - d_c["old"]).abs().max() / d_c["old"].abs().max()
print(f"N = {N}: microseconds per launch (median of {a_.reps}, event pairs: a launch boundary included)")
for i, (name, _) in enumerate(STEPS["old"]):
    print(f"  {name:18s} old {res['old'][i]:7.1f}   new {res['new'][i]:7.1f}")
print(f"  {'sum':18s} old {sum(res['old']):7.1f}   new {sum(res['new']):7.1f}")
print(f"d h of the two sides bit-identical: {same_h};  max |d c new - old| / max |d c| = {float(e):.2e}")

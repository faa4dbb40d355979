"""The first encoder layer of the flattened-observation agents: fused (csrc/flat_obs.hip, reading the padded pieces in place) against
``th.cat`` + ``ops.linear_relu`` (UAVGNN_FLAT_OBS_FUSED=0), forward and weight gradient, timed with HIP events (median of --reps).

    python tools/flat_obs_probe.py [--reps 20] [--out profiles/flat_obs_probe.txt]

Shapes: exp2's 4 x 4 maps (F = 31) and 8 x 80 (F = 423), H_out = 256, at 16 384 rows (rollout: B = 4096 x 4 agents) and 41 x 16 384
rows (time-batched, HotSpot episode_limit 40).  The forward's algorithmic bytes per row are 4F + 4 H_out; the fused weight gradient reads
dy once per 32-column slice of F (ceil(F / 32) (4 H_out) + 4F per row) plus its partials; the unfused legs add the [rows, F] concat
(written once, read again).  HBM share: against 8 TB/s.  For a kernel-level cross-check run it under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import math
import os
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uav_bs_ctrl_amd import ops  # noqa: E402

PEAK_GBS = 8000.0


def _time(fn, reps):
    for _ in range(3):
        fn()
    th.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2]


def _pieces(rows, n, M):
    g = th.Generator(device="cuda").manual_seed(rows + n)
    return tuple(th.rand(rows, k, device="cuda", generator=g) * 2 - 1 for k in (2, M * 5, (n - 1) * 3))


def _wgrad_fused(parts, dym, H, F):
    lib = ops.L.lib()
    n = dym.shape[0]
    S = lib.uavgnn_flat_obs_wgrad_chunks(n, H, F)
    part = th.empty((S, H, F), dtype=th.float32, device="cuda")
    ops.L.check(lib.uavgnn_flat_obs_wgrad(dym.data_ptr(), dym.stride(0), H, *ops._flat_src(parts), n, part.data_ptr(), S, 0,
                                          ops.L.stream()), "uavgnn_flat_obs_wgrad")
    return part.sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H = 256
    lines = [f"# flat_obs_probe: fused first encoder layer vs th.cat + linear_relu, H_out = {H}, median of {a.reps} (HIP events); "
             f"HBM share against {PEAK_GBS / 1000:.0f} TB/s of algorithmic bytes",
             f"{'case':<28}{'leg':<10}{'fused ms':>10}{'cat ms':>10}{'fused/cat':>10}{'fused GB/s':>12}{'HBM':>7}"]
    for (n, M) in ((4, 4), (8, 80)):
        for rows in (16384, 41 * 16384):
            parts = _pieces(rows, n, M)
            F = sum(p.shape[1] for p in parts)
            g = th.Generator(device="cuda").manual_seed(7)
            W = th.randn(H, F, device="cuda", generator=g) / math.sqrt(F)
            b = th.randn(H, device="cuda", generator=g) * 0.1
            dym = th.randn(rows, H, device="cuda", generator=g)
            with th.no_grad():
                t_f = _time(lambda: ops._FlatLinearReLU.apply(W, b, *parts), a.reps)
                t_c = _time(lambda: ops.linear_relu(th.cat(parts, 1), W, b), a.reps)
                w_f = _time(lambda: _wgrad_fused(parts, dym, H, F), a.reps)
                w_c = _time(lambda: ops._wgrad(dym, th.cat(parts, 1)), a.reps)
            case = f"{n}x{M} F={F} rows={rows}"
            fb = rows * (4 * F + 4 * H)
            S = ops.L.lib().uavgnn_flat_obs_wgrad_chunks(rows, H, F)
            wb = rows * (math.ceil(F / 32) * 4 * H + 4 * F) + 2 * S * H * F * 4
            for leg, tf, tc, by in (("forward", t_f, t_c, fb), ("wgrad", w_f, w_c, wb)):
                gbs = by / tf / 1e6
                lines.append(f"{case:<28}{leg:<10}{tf:>10.4f}{tc:>10.4f}{tf / tc:>10.2f}{gbs:>12.0f}{gbs / PEAK_GBS:>7.1%}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

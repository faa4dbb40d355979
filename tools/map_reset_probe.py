"""Reset of the device simulator with the map's own placements: the one-launch sampler (csrc/map_sample.hip) against what a user had
to write before it existed - the torch formulation of a DenseHotSpot placement that bench.py's end-to-end leg carries (`positions()`,
about 15 launches, group cells drawn with replacement) feeding ``env.reset(ubs, gts, generator=...)``, whose own ``rand`` / ``argsort``
draw the priorities.  Timed with HIP events around --inner back-to-back calls (median of --reps windows, legs alternating).

    python tools/map_reset_probe.py [--B 4096] [--map 8ubs] [--reps 15] [--inner 50] [--out profiles/map_reset_probe.txt]

Legs:
  sampler launch     uavgnn_map_sample alone, into the environment's state buffers
  sample + counter   the launch + the in-place device add of the reset counter (BatchedUbsCoverageEnv._sample_into)
  reset_from_map     sampler launch, counter add, five zero fills, the reset-time simulator launch
  torch placement    the torch formulation alone (positions + rand / argsort priorities)
  torch + reset      the torch formulation + env.reset(ubs, gts, prior): the copies, the zero fills and the same simulator launch
  env_step(NULL)     the reset-time simulator launch alone (common to both resets)
"""
import argparse
import os
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uav_bs_ctrl_amd import _lib as L  # noqa: E402
from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv  # noqa: E402


def _window(fn, inner):
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3                                    # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--map", default="8ubs")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("map_reset_probe needs the GPU: there is nothing to time without it")
    dev, B = th.device("cuda"), a.B
    env = BatchedUbsCoverageEnv.from_map(a.map, B, seed=1)
    mp, n, M = env.p, env.n_agents, env.n_gts
    gen = th.Generator(device=dev).manual_seed(1)
    grid, L_s, r = 200.0, int(mp.range_pos // 200) // 4, 4

    def torch_placement():                                   # bench.py positions() ("env" mode) + reset()'s priorities
        spot = th.randint(0, L_s, (B, 1, 2), device=dev, generator=gen).double() * (grid * r)
        grp = spot + th.randint(0, r, (B, M // 5, 2), device=dev, generator=gen).double() * grid
        gts = grp.repeat_interleave(5, 1) + 100.0 * (th.rand(B, M, 2, device=dev, generator=gen, dtype=th.float64) - 0.5)
        ubs = th.randint(0, int(mp.range_pos // 200), (B, n, 2), device=dev, generator=gen).double() * grid
        prior = th.argsort(th.rand(B, M, device=dev, generator=gen), dim=1)
        return ubs.clamp(0, mp.range_pos), gts.clamp(0, mp.range_pos).float(), prior

    def sampler_launch():
        fu, fg = env._map_fixed
        L.check(L.lib().uavgnn_map_sample(env._map_ic, env._map_fc, B, env.map_rng.data_ptr(), L.ptr(fu), L.ptr(fg),
                                          env.pos_ubs.data_ptr(), env.pos_gts.data_ptr(), env.prior.data_ptr(), L.stream()),
                "uavgnn_map_sample")

    legs = [("sampler launch", sampler_launch),
            ("sample + counter", lambda: env._sample_into(env.pos_ubs, env.pos_gts, env.prior)),
            ("reset_from_map", env.reset_from_map),
            ("torch placement", torch_placement),
            ("torch + reset", lambda: env.reset(*torch_placement())),
            ("env_step(NULL)", lambda: env._launch(None))]
    for _, fn in legs:                                       # warm every leg: code objects, allocator pools
        for _ in range(5):
            fn()
    th.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(a.reps):
        for name, fn in legs:
            us[name].append(_window(fn, a.inner))
    lines = [f"# map_reset_probe: map {a.map}, B = {B} (n = {n}, M = {M}); us per call, HIP events around {a.inner} back-to-back calls, "
             f"median [min .. max] of {a.reps} windows, legs alternating",
             f"{'leg':<20}{'median us':>12}{'min':>10}{'max':>10}"]
    med = {}
    for name, _ in legs:
        v = sorted(us[name])
        med[name] = v[len(v) // 2]
        lines.append(f"{name:<20}{med[name]:>12.1f}{v[0]:>10.1f}{v[-1]:>10.1f}")
    lines.append(f"reset_from_map / (torch + reset) = {med['reset_from_map'] / med['torch + reset']:.3f}; "
                 f"sampler launch / torch placement = {med['sampler launch'] / med['torch placement']:.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

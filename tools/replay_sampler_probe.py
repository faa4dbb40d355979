#!/usr/bin/env python
"""One draw of the device replay sampler: the one-workgroup kernel (uavgnn_replay_sample, csrc/replay.hip) at its largest ring of
65 536 slots against the many-workgroup call (uavgnn_replay_sample_wide, csrc/replay_wide.hip) at 65 536, 65 537, 2^18, 2^20 and 2^22
slots - every ring full, B = 32 and B = 4096.

    python tools/replay_sampler_probe.py [--draws 200] [--windows 7] [--out profiles/replay_sampler_wide_probe.txt]

Device events around a window of --draws back-to-back draws (>= 200) on one stream, after a warm-up of every shape; the arms ALTERNATE
inside each of the --windows rounds (>= 5) of one process; per arm the median and the range over its windows, in microseconds per draw.
One condition is checked (exit status 1 when it fails): a single workgroup looping over 2^20 slots would take 16 x the one-workgroup
kernel's time at 65 536, so the wide call at 2^20 slots has to take less than 16 x that kernel's median in the same run - otherwise
the parallel form has lost to the serial one.  Everything else is a measurement, not a threshold."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NARROW = 65536
WIDE_SLOTS = (65536, 65537, 1 << 18, 1 << 20, 1 << 22)
BATCHES = (32, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=200, help="draws per timed window (>= 200)")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per arm (>= 5)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if a.draws < 200 or a.windows < 5:
        ap.error("--draws >= 200 and --windows >= 5: a shorter window measures the clock")
    import torch as th

    from uav_bs_ctrl_amd import _lib as L
    if not th.cuda.is_available():
        raise SystemExit("replay_sampler_probe: no GPU - nothing is measured on the host")
    lib = L.lib()
    status = th.zeros(1, dtype=th.int32, device="cuda")
    arms = []                                           # (name, slots, B, draw(), launches per draw)
    for B in BATCHES:
        for wide, slots in [(False, NARROW)] + [(True, s) for s in WIDE_SLOTS]:
            state = th.tensor([0, slots], dtype=th.int64, device="cuda")
            rng = th.tensor([12345, 0], dtype=th.int64, device="cuda")
            idx = th.empty(B, dtype=th.int64, device="cuda")
            if wide:
                ws = th.empty(lib.uavgnn_replay_sample_wide_workspace_bytes(slots), dtype=th.uint8, device="cuda")

                def draw(state=state, rng=rng, idx=idx, ws=ws, slots=slots, B=B):
                    L.check(lib.uavgnn_replay_sample_wide(state.data_ptr(), rng.data_ptr(), slots, B, idx.data_ptr(), status.data_ptr(),
                                                          ws.data_ptr(), L.stream()), "uavgnn_replay_sample_wide")
            else:
                def draw(state=state, rng=rng, idx=idx, slots=slots, B=B):
                    L.check(lib.uavgnn_replay_sample(state.data_ptr(), rng.data_ptr(), slots, B, idx.data_ptr(), status.data_ptr(),
                                                     L.stream()), "uavgnn_replay_sample")
            arms.append((f"{'wide' if wide else 'narrow'} {slots:>8d} slots  B {B:>4d}", wide, slots, B, draw, 7 if wide else 1))
    for arm in arms:                                    # warm-up of every shape
        for _ in range(20):
            arm[4]()
    th.cuda.synchronize()
    assert int(status) == 0
    times = [[] for _ in arms]
    for _ in range(a.windows):
        for i, arm in enumerate(arms):                  # the arms alternate inside a round
            t0, t1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.draws):
                arm[4]()
            t1.record()
            t1.synchronize()
            times[i].append(1e3 * t0.elapsed_time(t1) / a.draws)
    assert int(status) == 0
    S = lib.uavgnn_replay_sample_wide_slots_per_workgroup()
    lines = [f"replay sampler, one draw: device events around {a.draws} back-to-back draws, {a.windows} windows per arm, arms alternating; "
             f"{th.cuda.get_device_name(0)}",
             f"wide: one workgroup per {S} slots of the capacity, 7 launches per draw at any size; narrow: 1 launch of one workgroup",
             f"{'arm':<36s} {'launches':>8s} {'workgroups':>10s} {'median us':>10s} {'min us':>9s} {'max us':>9s}"]
    med = {}
    for (name, wide, slots, B, _, launches), t in zip(arms, times):
        med[(wide, slots, B)] = statistics.median(t)
        lines.append(f"{name:<36s} {launches:>8d} {(slots + S - 1) // S if wide else 1:>10d} {statistics.median(t):>10.2f} {min(t):>9.2f} "
                     f"{max(t):>9.2f}")
    ok = True
    for B in BATCHES:
        w, n = med[(True, 1 << 20, B)], med[(False, NARROW, B)]
        good = w < 16 * n
        ok &= good
        lines.append(f"condition, B {B}: wide at 2^20 slots {w:.2f} us {'<' if good else '>='} 16 x narrow at 65 536 slots = {16 * n:.2f} us "
                     f"({w / n:.2f} x): {'met' if good else 'NOT MET'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

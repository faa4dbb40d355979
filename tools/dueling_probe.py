#!/usr/bin/env python
"""What ``dueling=True`` (run_exp3.py's `duel` axis) costs on the device path: exp3 TarMAC on three arms -

  plain        dueling=False (the headline configuration)
  duel-torch   dueling=True with ``ops.DUEL_FUSED = False``: the generic comm route and the torch formulation of the head
  duel-fused   dueling=True on the fused step, csrc/head.hip's dueling form and the folded weight in the backward

- as microseconds per ``act`` step and milliseconds per ``accumulate``, at bench.py's sizes (B = 4096, 8 x 80, T = 50, D-dense) and at the
reference's (32 environments); and the dueling kernel alone against ``uavgnn_head_fwd`` at N = 32 768, H = 256, 9 actions.

    python tools/dueling_probe.py [--rounds 5] [--sizes bench,ref] [--out profiles/dueling_probe.txt]

The arms alternate inside one process after a warm-up of each.  Every figure is a window of back-to-back iterations between two device
events divided by the iterations; --rounds windows per arm, reported as median [min .. max] - the spread to hold a difference against.
Measurements, not thresholds."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"bench": dict(B=4096, n=8, M=80, T=50, act_iters=20, acc_iters=2), "ref": dict(B=32, n=8, M=80, T=50, act_iters=50, acc_iters=3)}
ARMS = [("plain", False, True), ("duel-torch", True, False), ("duel-fused", True, True)]


def _window(fn, iters):
    import torch as th
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _stat(ms, scale=1.0, digits=3):
    s = sorted(scale * m for m in ms)
    return dict(median=round(s[len(s) // 2], digits), min=round(s[0], digits), max=round(s[-1], digits))


def learner_rows(name, size, rounds):
    import torch as th

    import bench
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    B, n, M, T = size["B"], size["n"], size["M"], size["T"]
    batch = bench.make_sequence(B, n, M, T, "dense", th.device("cuda"), seed=1234, distinct=4)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=9, n_agents=n, episode_limit=T)
    fns = {}
    for arm, dueling, fused in ARMS:
        th.manual_seed(0)
        args = copy.copy(bench.exp3_args("cuda"))
        args.dueling = dueling
        lr = MultiAgentQLearner(info, args)
        h = lr.init_hidden(B)

        def act(lr=lr, h=h, fused=fused):
            ops.DUEL_FUSED = fused
            lr.act(batch["obs"][0].fresh(), h, 0.05)

        def acc(lr=lr, fused=fused):
            ops.DUEL_FUSED = fused
            fb = dict(batch, obs=[g.fresh() for g in batch["obs"]], obs_all=batch["obs_all"].fresh(), obs_all_next=batch["obs_all_next"].fresh())
            lr.accumulate(fb)
        fns[arm] = (act, acc)
    for act, acc in fns.values():      # warm-up: allocator, weight planes of the rollout store, lazily built indices
        for _ in range(3):
            act()
        acc()
    th.cuda.synchronize()
    t_act, t_acc = {a: [] for a in fns}, {a: [] for a in fns}
    for _ in range(rounds):
        for arm, (act, acc) in fns.items():
            t_act[arm].append(_window(act, size["act_iters"]))
            t_acc[arm].append(_window(acc, size["acc_iters"]))
    ops.DUEL_FUSED = True
    rows = []
    for arm in fns:
        rows.append(dict(size=name, B=B, rows_per_step=B * n, T=T, arm=arm, windows=rounds, act_us=_stat(t_act[arm], 1e3, 1),
                         accumulate_ms=_stat(t_acc[arm])))
    med = {r["arm"]: (r["act_us"]["median"], r["accumulate_ms"]["median"]) for r in rows}
    rows.append(dict(size=name, what="ratios of medians (act, accumulate)",
                     fused_over_torch=[round(med["duel-fused"][i] / med["duel-torch"][i], 4) for i in (0, 1)],
                     fused_over_plain=[round(med["duel-fused"][i] / med["plain"][i], 4) for i in (0, 1)]))
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def kernel_rows(rounds, N=32768, H=256, A=9, iters=200):
    import torch as th

    from uav_bs_ctrl_amd import _lib as L
    lib, st = L.lib(), L.stream()
    g = th.Generator(device="cuda").manual_seed(1)
    h = th.randn(N, H, device="cuda", generator=g)
    W, b = 0.1 * th.randn(A + 1, H, device="cuda", generator=g), th.randn(A + 4, device="cuda", generator=g)
    q = th.empty(N, A, device="cuda")

    def plain():
        lib.uavgnn_head_fwd(h.data_ptr(), H, N, H, W.data_ptr(), H, b.data_ptr(), A, q.data_ptr(), A, st)

    def duel():
        lib.uavgnn_head_fwd_duel(h.data_ptr(), H, N, H, W.data_ptr(), H, W[A:].data_ptr(), b.data_ptr(), b[A:].data_ptr(), A, q.data_ptr(), A, st)
    for f in (plain, duel):
        _window(f, 20)
    ms = {"uavgnn_head_fwd": [], "uavgnn_head_fwd_duel": []}
    for _ in range(rounds):
        ms["uavgnn_head_fwd"].append(_window(plain, iters))
        ms["uavgnn_head_fwd_duel"].append(_window(duel, iters))
    rows = [dict(what=k, N=N, H=H, A=A, windows=rounds, iters_per_window=iters, us=_stat(v, 1e3, 2), bytes_h=N * H * 4) for k, v in ms.items()]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():   # noqa: D103
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="bench,ref")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = kernel_rows(a.rounds)
    for name in a.sizes.split(","):
        rows += learner_rows(name, SIZES[name], a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# dueling_probe: exp3 TarMAC (H = 256, 9 actions), D-dense batches; windows between device events, {a.rounds} per arm, arms "
                    "alternating; median [min .. max]\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

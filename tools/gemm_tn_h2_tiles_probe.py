#!/usr/bin/env python
"""The weight-gradient products of a C3 update (dW = dY^T X over 1 671 168 time-batched rows) on csrc/gemm_tn_h2.hip at each column-tile
width and chunk count in question: (width, S) arms alternated round by round, device-event time per launch -> p50 [min .. max] per arm,
and the partials of every arm against the 128-wide kernel's at the same S (bit patterns).  GPU box.
    python tools/gemm_tn_h2_tiles_probe.py [rows] [rounds]
    python tools/gemm_tn_h2_tiles_probe.py --one NAME WIDTH S [rows]      ten launches of one arm (for a counter run of its own)"""
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uav_bs_ctrl_amd import _lib as L  # noqa: E402

dev = th.device("cuda")
lib = L.lib()
# name -> (Mo, Ko, arms (width, S)); dWp runs as x^T d_proj (ops.WeightGradSink.step_grads)
PRODUCTS = {"dW_ih": (768, 320, ((128, 56), (160, 80), (160, 85), (128, 56))),
            "dW_hh": (768, 256, ((128, 80), (128, 85), (128, 80))),
            "dW_aggr": (256, 512, ((128, 128), (128, 128))),
            "dWp": (256, 96, ((128, 512), (96, 512), (128, 512)))}


def operands(n, Mo, Ko, gen):
    # gradient-like dY: rows whose magnitudes span four orders (time steps), activation-like X (tools/gemm_tn_h2_probe.py)
    dy = th.randn(n, Mo, device=dev, generator=gen) * th.exp2(th.randint(-14, 1, (n, 1), device=dev, generator=gen).float()) * 1e-3
    x = th.relu(th.randn(n, Ko, device=dev, generator=gen))
    return dy, x, dy.abs().amax(0), x.abs().amax(0)


def launch(dy, x, cy, cx, part, S, tj):
    L.check(lib.uavgnn_gemm_tn_h2_tj(dy.data_ptr(), dy.stride(0), dy.shape[1], x.data_ptr(), x.stride(0), x.shape[1], dy.shape[0],
                                     cy.data_ptr(), cx.data_ptr(), part.data_ptr(), S, 0, tj, L.stream()), "gemm_tn_h2_tj")


def main():
    argv = sys.argv[1:]
    gen = th.Generator(device=dev).manual_seed(0)
    if argv and argv[0] == "--one":
        name, tj, S = argv[1], int(argv[2]), int(argv[3])
        n = int(argv[4]) if len(argv) > 4 else 51 * 32768
        Mo, Ko, _ = PRODUCTS[name]
        dy, x, cy, cx = operands(n, Mo, Ko, gen)
        part = th.empty(S, Mo, Ko, device=dev)
        for _ in range(10):
            launch(dy, x, cy, cx, part, S, tj)
        th.cuda.synchronize()
        print(f"{name} width {tj} S {S}: 10 launches over {n} rows")
        return
    n = int(argv[0]) if argv else 51 * 32768
    rounds = int(argv[1]) if len(argv) > 1 else 7
    print(f"# dW = dY^T X over {n} rows; {rounds} rounds of 3 launches per arm, arms alternated; microseconds per launch")
    for name, (Mo, Ko, arms) in PRODUCTS.items():
        dy, x, cy, cx = operands(n, Mo, Ko, gen)
        parts = [th.empty(S, Mo, Ko, device=dev) for _, S in arms]
        times = [[] for _ in arms]
        for i, (tj, S) in enumerate(arms):      # warm-up, and the bits against the 128-wide kernel at the same S
            launch(dy, x, cy, cx, parts[i], S, tj)
        for r in range(rounds):
            for i, (tj, S) in enumerate(arms):
                e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    launch(dy, x, cy, cx, parts[i], S, tj)
                e1.record()
                th.cuda.synchronize()
                times[i].append(e0.elapsed_time(e1) / 3 * 1e3)
        for i, (tj, S) in enumerate(arms):
            t = sorted(times[i])
            note = ""
            if tj != 128:
                ref = th.empty(S, Mo, Ko, device=dev)
                launch(dy, x, cy, cx, ref, S, 128)
                note = "   partials == 128-wide at this S: " + str(bool(th.equal(ref.view(th.int32), parts[i].view(th.int32))))
            tiles = -(-Mo // 256) * -(-Ko // tj)
            print(f"{name:8s} [{Mo} x {Ko}] width {tj:3d} S {S:3d} ({tiles * S:3d} workgroups): p50 {t[len(t) // 2]:8.1f} [{t[0]:8.1f} .. {t[-1]:8.1f}]{note}")
        del dy, x, parts


if __name__ == "__main__":
    main()

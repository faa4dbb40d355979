#!/usr/bin/env python
"""The QMIX mixer on two arms - the torch formulation (UAVGNN_QMIX_FUSED=0: ``agents.qmix.mix_torch`` behind ``F.linear``) and the kernel
path (``ops.linear`` + ``ops.qmix_mix``, csrc/qmix.hip) - forward + backward of ONE mixer, and one ``GraphedEpisode`` replay with the
mixer off and on.

    python tools/qmix_probe.py [--rounds 5] [--window-ms 300] [--skip-episode] [--out profiles/qmix_probe.txt]

  mixer     n = 8, embed_dim = 32, state_dim = 336 at rows = 1600 (the reference's 50 x 32) and rows = 204 800 (bench.py's T B)
  episode   map '8ubs' (8 x 50, episode limit 50 = T), TarMAC, H = 256, 32 environments, batch 32

The two arms alternate inside one process (the switch is the module attribute the environment variable seeds), after a warm-up of both.
Every figure is a window of --window-ms of back-to-back iterations between two device events, divided by the iterations; --rounds
windows per arm, reported as median [min .. max] - the spread to hold a difference against.  Launches per iteration: the kernels one
forward + backward puts on the stream, counted by the profiler in a run of its own after the timing ('not measured' where the profiler
gives nothing).  Algorithmic bytes of the two kernels: forward rows ((n+3) e + n + 1) 4, backward rows (2 (n+3) e +
2 n + 1) 4; the share of 8 TB/s is of the kernels' spans (``ops.KERNEL_TIMER``), taken in a third run.  Measurements, not thresholds."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_AGENTS, EMBED, STATE_DIM = 8, 32, 336
HBM_BYTES_PER_S = 8e12
E, BATCH = 32, 32


def _window(fn, iters):
    import torch as th
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _stat(ms):
    s = sorted(ms)
    return dict(median_ms=round(s[len(s) // 2], 5), min_ms=round(s[0], 5), max_ms=round(s[-1], 5))


def _launches(fn):
    """Device kernels of one fn() as the profiler lists them; None when it lists none."""
    import torch as th
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        th.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            th.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as exc:   # noqa: BLE001 - a probe: the timing stands without the count
        print(f"# launches not measured: {type(exc).__name__}: {exc}", flush=True)
        return None


def mixer_rows(rows, rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.agents import qmix
    th.manual_seed(0)
    mix = qmix.QMixer(STATE_DIM, N_AGENTS, types.SimpleNamespace(embed_dim=EMBED)).cuda()
    T = 50
    B = rows // T
    g = th.Generator(device="cuda").manual_seed(1)
    qs = th.randn(T, B, N_AGENTS, device="cuda", generator=g).requires_grad_(True)
    states = th.randn(T, B, STATE_DIM, device="cuda", generator=g)
    w = th.randn(T, B, 1, device="cuda", generator=g)
    params = list(mix.parameters()) + [qs]

    def step():
        return th.autograd.grad((mix(qs, states) * w).sum(), params)

    def arm(fused):
        qmix.QMIX_FUSED = fused
        return step

    # the two arms agree (the parity tests hold them to float64; here: that the probe times the same function)
    ref = [t.clone() for t in arm(False)()]
    got = arm(True)()
    worst = max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(got, ref))
    iters = {}
    for fused in (False, True):
        for _ in range(3):
            arm(fused)()
        iters[fused] = max(10, int(window_ms / max(_window(arm(fused), 10), 1e-3)))
    ms = {False: [], True: []}
    for _ in range(rounds):
        for fused in (False, True):
            ms[fused].append(_window(arm(fused), iters[fused]))
    qmix.QMIX_FUSED = True
    ops.KERNEL_TIMER.reset(True, only=("qmix_mix_fwd", "qmix_mix_bwd"))
    for _ in range(20):
        step()
    spans = ops.KERNEL_TIMER.summary()
    ops.KERNEL_TIMER.reset(False)
    n, e = N_AGENTS, EMBED
    by = dict(qmix_mix_fwd=rows * ((n + 3) * e + n + 1) * 4, qmix_mix_bwd=rows * (2 * (n + 3) * e + 2 * n + 1) * 4)
    out = []
    for fused in (False, True):
        out.append(dict(what="mixer fwd+bwd", rows=rows, arm="kernels" if fused else "torch", iters_per_window=iters[fused], windows=rounds,
                        **_stat(ms[fused])))
    out.append(dict(what="mixer fwd+bwd", rows=rows, arm="kernels / torch", ratio_of_medians=round(out[1]["median_ms"] / out[0]["median_ms"], 4),
                    max_rel_diff_of_gradients=worst))
    for k, v in spans.items():
        med = sorted(v["ms"])[len(v["ms"]) // 2]
        out.append(dict(what=k, rows=rows, median_us=round(1e3 * med, 2), algorithmic_bytes=by[k],
                        share_of_8TBs=round(by[k] / (med * 1e-3) / HBM_BYTES_PER_S, 4)))
    for r in out:
        print(json.dumps(r), flush=True)
    return out, arm


def launch_rows(rows, arm):
    """After all timing (the profiler slows the host): the kernels one forward + backward of each arm puts on the stream."""
    out = [dict(what="mixer fwd+bwd launches", rows=rows, arm="kernels" if fused else "torch", launches=_launches(arm(fused)) or "not measured")
           for fused in (False, True)]
    for r in out:
        print(json.dumps(r), flush=True)
    return out


def episode_rows(rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd.graphs import GraphedEpisode
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    runs = {}
    for mixer in (False, True):
        th.manual_seed(0)
        env = BatchedUbsCoverageEnv.from_map("8ubs", E, seed=0)
        args = types.SimpleNamespace(device="cuda", hidden_size=256, c="tarmac", n_heads=4, n_layers=2, msg_size=64, key_size=16, n_rounds=1,
                                     dueling=False, mixer=mixer, embed_dim=EMBED, share_reward=mixer, double_q=True, lr=5e-4, gamma=0.99,
                                     polyak=0.999, max_seq_len=None, batch_size=BATCH, seed=0)
        info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit,
                    state_shape=env.state_dim)
        rb = SequenceReplay(8 * E, env.episode_limit, env.n_agents, env.n_gts, 256, n_envs=E, state_dim=env.state_dim, r_comm=env.p.r_comm,
                            rew_dim=1 if mixer else None, device_state=True, seed=0)
        runs[mixer] = (GraphedEpisode(MultiAgentQLearner(info, args), env, rb, BATCH, eps=(1.0, 0.05, 5e4)), rb, env)
    iters = {}
    for mixer, (ge, _, _) in runs.items():
        ge(), ge()
        iters[mixer] = max(2, int(window_ms / max(_window(ge, 2), 1e-3)))
    ms = {False: [], True: []}
    for _ in range(rounds):
        for mixer, (ge, _, _) in runs.items():
            ms[mixer].append(_window(ge, iters[mixer]))
    out = []
    for mixer, (ge, rb, env) in runs.items():
        rb.check()
        out.append(dict(what="GraphedEpisode replay, '8ubs', TarMAC, H = 256", mixer=mixer, envs=E, batch=BATCH, episode_limit=env.episode_limit,
                        state_dim=env.state_dim, iters_per_window=iters[mixer], windows=rounds, loss_finite=bool(th.isfinite(ge.out["LossQ"])),
                        **_stat(ms[mixer])))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():   # noqa: D103
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--skip-episode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, arms = [], {}
    for r in (1600, 204800):
        out, arms[r] = mixer_rows(r, a.rounds, a.window_ms)
        rows += out
    if not a.skip_episode:
        rows += episode_rows(a.rounds, a.window_ms)
    _write(a, rows)
    for r, arm in arms.items():
        rows += launch_rows(r, arm)
    _write(a, rows)


def _write(a, rows):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# qmix_probe: n = {N_AGENTS}, embed_dim = {EMBED}, state_dim = {STATE_DIM}; windows of {a.window_ms:.0f} ms between device "
                    f"events, {a.rounds} per arm, arms alternating; median [min .. max]\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

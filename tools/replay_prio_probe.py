#!/usr/bin/env python
"""The prioritised replay's launches against what they stand beside: one prioritised draw (four launches, csrc/replay_prio.hip) against
the uniform sampler's draw at the same capacity, one priority update, and one ``GraphedEpisode`` replay with the option off and on.

    python tools/replay_prio_probe.py [--rounds 5] [--window-ms 200] [--skip-episode] [--out profiles/replay_prio_probe.txt]

  draw      full rings of 65 536, 2^20 and 2^22 slots, B = 32 and 4096; priorities uniform over [1, 2^24); the uniform arm is
            uavgnn_replay_sample (65 536: one launch) / uavgnn_replay_sample_wide (above: seven launches)
  update    td [T, B, C] = [50, 32, 8] and [50, 4096, 8] on ascending indices of a ring of 2^20 slots
  episode   map '8ubs' (8 x 50, episode limit 50 = T), TarMAC, H = 256, 32 environments, batch 32, a ring of 256 sequences;
            prioritized = (0.6, 0.4, 0.9, 1e-3)

The arms alternate inside one process after a warm-up of both.  Every figure is a window of --window-ms of back-to-back iterations
between two device events, divided by the iterations; --rounds windows per arm, reported as median [min .. max] - the spread to hold a
difference against.  The "off" arm is the code every run took before the option existed.  Measurements, not thresholds."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, BATCH = 32, 32
PRIO = (0.6, 0.4, 0.9, 1e-3)


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


def _alternate(arms, rounds, window_ms, floor=10):
    """{name: [ms per iteration, one per window]} of the callables ``arms``, windows alternating between them."""
    iters = {}
    for name, fn in arms.items():
        for _ in range(3):
            fn()
        iters[name] = max(floor, int(window_ms / max(_window(fn, floor), 1e-4)))
    ms = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            ms[name].append(_window(fn, iters[name]))
    return ms, iters


def draw_rows(capacity, B, rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.replay import NARROW_SAMPLER_CAPACITY
    lib = L.lib()
    state = th.tensor([0, capacity], dtype=th.int64, device="cuda")
    rng = th.tensor([1, 0], dtype=th.int64, device="cuda")
    status = th.zeros(1, dtype=th.int32, device="cuda")
    idx = th.empty(B, dtype=th.int64, device="cuda")
    weights = th.empty(B, dtype=th.float32, device="cuda")
    prio = th.randint(1, 1 << 24, (capacity,), dtype=th.int32, device="cuda", generator=th.Generator(device="cuda").manual_seed(0))
    ws = th.empty(lib.uavgnn_replay_prio_workspace_bytes(capacity, B), dtype=th.uint8, device="cuda")
    wide = capacity > NARROW_SAMPLER_CAPACITY
    ws_u = th.empty(lib.uavgnn_replay_sample_wide_workspace_bytes(capacity), dtype=th.uint8, device="cuda") if wide else None

    def prioritised():
        L.check(lib.uavgnn_replay_prio_sample(state.data_ptr(), rng.data_ptr(), capacity, B, prio.data_ptr(), PRIO[1], idx.data_ptr(),
                                              weights.data_ptr(), status.data_ptr(), ws.data_ptr(), L.stream()), "prio_sample")

    def uniform():
        if wide:
            L.check(lib.uavgnn_replay_sample_wide(state.data_ptr(), rng.data_ptr(), capacity, B, idx.data_ptr(), status.data_ptr(),
                                                  ws_u.data_ptr(), L.stream()), "sample_wide")
        else:
            L.check(lib.uavgnn_replay_sample(state.data_ptr(), rng.data_ptr(), capacity, B, idx.data_ptr(), status.data_ptr(), L.stream()),
                    "sample")
    ms, iters = _alternate(dict(uniform=uniform, prioritised=prioritised), rounds, window_ms)
    assert int(status) == 0
    out = [dict(what="one draw", capacity=capacity, B=B, arm=name, launches={"uniform": 7 if wide else 1, "prioritised": 4}[name],
                iters_per_window=iters[name], windows=rounds, **_stat(ms[name])) for name in ms]
    out.append(dict(what="one draw", capacity=capacity, B=B, arm="prioritised / uniform",
                    ratio_of_medians=round(out[1]["median_ms"] / out[0]["median_ms"], 4)))
    for r in out:
        print(json.dumps(r), flush=True)
    return out


def update_rows(T, B, C, rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd import _lib as L
    lib, capacity = L.lib(), 1 << 20
    gen = th.Generator(device="cuda").manual_seed(1)
    td = th.randn(T, B, C, device="cuda", generator=gen)
    idx = th.sort(th.randint(0, capacity, (B,), device="cuda", generator=gen)).values
    prio = th.full((capacity,), 1 << 20, dtype=th.int32, device="cuda")
    top = th.full((1,), 1 << 20, dtype=th.int32, device="cuda")
    status = th.zeros(1, dtype=th.int32, device="cuda")

    def update():
        L.check(lib.uavgnn_replay_prio_update(td.data_ptr(), T, B, C, idx.data_ptr(), capacity, PRIO[0], PRIO[2], PRIO[3], prio.data_ptr(),
                                              top.data_ptr(), status.data_ptr(), L.stream()), "prio_update")
    ms, iters = _alternate(dict(update=update), rounds, window_ms)
    assert int(status) == 0
    med = sorted(ms["update"])[len(ms["update"]) // 2]
    by = 4 * T * B * C + 12 * B
    out = dict(what="one priority update", T=T, B=B, C=C, launches=1, iters_per_window=iters["update"], windows=rounds,
               algorithmic_bytes=by, GBs_at_median=round(by / (med * 1e-3) / 1e9, 2), **_stat(ms["update"]))
    print(json.dumps(out), flush=True)
    return [out]


def episode_rows(rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd.graphs import GraphedEpisode
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    runs = {}
    for on in (False, True):
        th.manual_seed(0)
        env = BatchedUbsCoverageEnv.from_map("8ubs", E, seed=0)
        args = types.SimpleNamespace(device="cuda", hidden_size=256, c="tarmac", n_heads=4, n_layers=2, msg_size=64, key_size=16, n_rounds=1,
                                     dueling=False, mixer=False, share_reward=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999,
                                     max_seq_len=None, batch_size=BATCH, seed=0)
        info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
        rb = SequenceReplay(8 * E, env.episode_limit, env.n_agents, env.n_gts, 256, n_envs=E, state_dim=0, r_comm=env.p.r_comm,
                            device_state=True, seed=0, prioritized=PRIO if on else None)
        runs["on" if on else "off"] = (GraphedEpisode(MultiAgentQLearner(info, args), env, rb, BATCH, eps=(1.0, 0.05, 5e4)), rb, env)
    ms, iters = _alternate({k: v[0] for k, v in runs.items()}, rounds, window_ms, floor=2)
    out = []
    for name, (ge, rb, env) in runs.items():
        rb.check()
        out.append(dict(what="GraphedEpisode replay, '8ubs', TarMAC, H = 256", prioritized=name, envs=E, batch=BATCH,
                        episode_limit=env.episode_limit, iters_per_window=iters[name], windows=rounds,
                        loss_finite=bool(th.isfinite(ge.out["LossQ"])), **_stat(ms[name])))
        print(json.dumps(out[-1]), flush=True)
    out.append(dict(what="GraphedEpisode replay", arm="on / off", ratio_of_medians=round(out[1]["median_ms"] / out[0]["median_ms"], 4)))
    print(json.dumps(out[-1]), flush=True)
    return out


def main():   # noqa: D103
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-episode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for capacity in (65536, 1 << 20, 1 << 22):
        for B in (32, 4096):
            rows += draw_rows(capacity, B, a.rounds, a.window_ms)
            _write(a, rows)
    for B in (32, 4096):
        rows += update_rows(50, B, 8, a.rounds, a.window_ms)
    _write(a, rows)
    if not a.skip_episode:
        rows += episode_rows(a.rounds, a.window_ms)
    _write(a, rows)


def _write(a, rows):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# replay_prio_probe: prioritized = {PRIO}; windows of {a.window_ms:.0f} ms between device events, {a.rounds} per arm, "
                    f"arms alternating; median [min .. max]\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

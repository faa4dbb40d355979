#!/usr/bin/env python
"""What the noisy-net Q head costs per rollout step, and what the one-launch form saves over a torch formulation of the same draw.

    python tools/noisy_head_probe.py [--rounds 5] [--window-ms 200] [--skip-episode] [--out profiles/noisy_head_probe.txt]

  head      at N = 256 and N = 32 768 rows, H = 256, A = 9, three arms:
              head_fwd         ``uavgnn_head_fwd``: the plain head (what the option is measured against)
              noisy_head_fwd   ``uavgnn_noisy_head_fwd``: one draw per row inside the launch, the noise never in memory
              torch            the same per-row draw in torch: ``randn`` for [N, H] and [N, A], f = sign sqrt|.|, two products
                               (``ops._noisy_head_torch``) - it materialises both noise tensors
  episode   one ``GraphedEpisode`` replay of map '8ubs' (8 x 50, episode limit 50 = T), TarMAC, H = 256, 32 environments, batch 32, with the
            option off and with noisy = 0.5

The arms alternate inside one process after a warm-up of all.  Every figure is a window of --window-ms of back-to-back iterations
between two device events, divided by the iterations; --rounds windows per arm, reported as median [min .. max] - the spread to hold a
difference against.  The head arms run eagerly: at N = 256 they measure the host's launch overhead as much as the device (one launch
against about ten).  Measurements, not thresholds."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from replay_prio_probe import _alternate, _stat  # noqa: E402

E, BATCH, H, A, SIGMA0 = 32, 32, 256, 9, 0.5


def head_rows(N, rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    lib, ext, st = L.lib(), L.ext(), L.stream()
    g = th.Generator(device="cuda").manual_seed(N)
    h = th.randn(N, H, device="cuda", generator=g)
    W, Ws = 0.1 * th.randn(A, H, device="cuda", generator=g), 0.03 * th.rand(A, H, device="cuda", generator=g)
    b, bs = th.randn(A, device="cuda", generator=g), 0.03 * th.rand(A, device="cuda", generator=g)
    rng = th.tensor([1, 0], dtype=th.int64, device="cuda")
    q = th.empty(N, A, device="cuda")

    def plain():
        L.check(lib.uavgnn_head_fwd(h.data_ptr(), H, N, H, W.data_ptr(), H, b.data_ptr(), A, q.data_ptr(), A, st), "uavgnn_head_fwd")

    def noisy():
        L.check(ext.uavgnn_noisy_head_fwd(h.data_ptr(), H, N, H, W.data_ptr(), Ws.data_ptr(), H, b.data_ptr(), bs.data_ptr(), A, rng.data_ptr(),
                                          q.data_ptr(), A, st), "uavgnn_noisy_head_fwd")
        rng[1:].add_(1)                 # the step advance of a rollout step belongs to the cost

    def torch_arm():
        f_in = ops.noisy_f(th.randn(N, H, device="cuda"))
        f_out = ops.noisy_f(th.randn(N, A, device="cuda"))
        return ops._noisy_head_torch(h, W, b, Ws, bs, f_in, f_out)
    ms, iters = _alternate({"head_fwd": plain, "noisy_head_fwd": noisy, "torch": torch_arm}, rounds, window_ms)
    rows = [dict(what="Q head", arm=k, N=N, H=H, A=A, iters_per_window=iters[k], windows=rounds, **_stat(v)) for k, v in ms.items()]
    med = {r["arm"]: r["median_ms"] for r in rows}
    rows.append(dict(what="ratios of medians", N=N, noisy_over_plain=round(med["noisy_head_fwd"] / med["head_fwd"], 4),
                     noisy_over_torch=round(med["noisy_head_fwd"] / med["torch"], 4),
                     noisy_minus_plain_us=round(1e3 * (med["noisy_head_fwd"] - med["head_fwd"]), 3), bytes_h=4 * N * H,
                     noise_bytes_torch_materialises=4 * N * (H + A)))
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def episode_rows(rounds, window_ms):
    import torch as th

    from uav_bs_ctrl_amd.graphs import GraphedEpisode
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.run import seed_comm_modules
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    runs = {}
    for name, noisy in (("off", None), ("on", SIGMA0)):
        th.manual_seed(0)
        env = BatchedUbsCoverageEnv.from_map("8ubs", E, seed=0)
        args = types.SimpleNamespace(device="cuda", hidden_size=H, c="tarmac", n_heads=4, n_layers=2, msg_size=64, key_size=16, n_rounds=1,
                                     dueling=False, mixer=False, share_reward=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999,
                                     max_seq_len=None, batch_size=BATCH, seed=0)
        info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
        rb = SequenceReplay(8 * E, env.episode_limit, env.n_agents, env.n_gts, H, n_envs=E, state_dim=0, r_comm=env.p.r_comm,
                            device_state=True, seed=0)
        learner = MultiAgentQLearner(info, args, noisy=noisy)
        seed_comm_modules(learner, 0)
        runs[name] = (GraphedEpisode(learner, env, rb, BATCH, eps=(1.0, 0.05, 5e4)), rb, env)
    ms, iters = _alternate({k: v[0] for k, v in runs.items()}, rounds, window_ms, floor=2)
    out = []
    for name, (ge, rb, env) in runs.items():
        rb.check()
        out.append(dict(what="GraphedEpisode replay, '8ubs', TarMAC, H = 256", noisy=name, envs=E, batch=BATCH,
                        episode_limit=env.episode_limit, rollout_steps=env.episode_limit, iters_per_window=iters[name], windows=rounds,
                        **_stat(ms[name])))
    med = {r["noisy"]: r["median_ms"] for r in out}
    steps = out[0]["rollout_steps"]
    out.append(dict(what="ratios of medians", on_over_off=round(med["on"] / med["off"], 4),
                    on_minus_off_us_per_rollout_step=round(1e3 * (med["on"] - med["off"]) / steps, 3),
                    note="the difference also holds the two folds and the transpose of the episode's update"))
    for r in out:
        print(json.dumps(r), flush=True)
    return out


def main():   # noqa: D103
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-episode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for N in (256, 32768):
        rows += head_rows(N, a.rounds, a.window_ms)
    if not a.skip_episode:
        rows += episode_rows(a.rounds, a.window_ms)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# noisy_head_probe: H = {H}, A = {A}; windows of {a.window_ms:g} ms between device events, {a.rounds} per arm, arms "
                    "alternating; median [min .. max] in ms per iteration\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

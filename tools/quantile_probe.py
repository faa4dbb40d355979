#!/usr/bin/env python
"""What the quantile-regression TD tail costs, against its torch formulation and against the bytes it must move.

    python tools/quantile_probe.py [--rounds 5] [--window-ms 200] [--skip-episode] [--out profiles/quantile_probe.txt]

  tail      the TD tail alone - select, loss and the select's backward - at 32 x 8 x T = 10 and 4096 x 8 x T = 50 (environments x agents x
            steps), A = 9, K = 8 / 32 / 64, n_step = 3, with importance weights, two arms:
              kernels   ``ops.qr_select`` -> ``ops.qr_loss`` -> backward (csrc/qr/quantile.hip: four launches)
              torch     ``ops.qr_select_torch`` -> ``ops.qr_loss_torch`` -> backward: the same arithmetic in torch ops, which materialises
                        [rows, K, K] several times (skipped at the large size for K = 64: 27 GB per intermediate)
            and the floor of the kernels' arm: the bytes the four launches must read and write over the HBM peak (8 TB/s)
  episode   one ``GraphedEpisode`` replay of map '8ubs' (8 x 50, episode limit 50 = T), TarMAC, H = 256, 32 environments, batch 32, with the
            option off and with quantiles = 32 (the generic step route and the wide head are part of the difference)

The arms alternate inside one process after a warm-up of all.  Every figure is a window of --window-ms of back-to-back iterations
between two device events, divided by the iterations; --rounds windows per arm, reported as median [min .. max].  Measurements, not
thresholds."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from replay_prio_probe import _alternate, _stat  # noqa: E402

E, BATCH, H, A, N_STEP, GAMMA = 32, 32, 256, 9, 3, 0.99
HBM_PEAK = 8.0e12       # bytes per second


def tail_bytes(T, N, K):
    """What the four launches must move: select reads both quantile tensors and writes the two rows and the means; the loss reads the two
    rows and writes g; the select's backward reads g and writes all of d theta_pol (rewards, dones, weights, td: below 1 %)."""
    rows = T * N
    select = 4 * ((2 * T + 1) * N * A * K + 2 * rows * K + (T + 1) * N * A)
    loss = 4 * 3 * rows * K
    bwd = 4 * (rows * K + (T + 1) * N * A * K)
    return select + loss + bwd, 4 * 3 * rows * K


def tail_rows(B, n, T, K, rounds, window_ms, with_torch=True):
    import torch as th

    from uav_bs_ctrl_amd import ops
    N = B * n
    g = th.Generator(device="cuda").manual_seed(K + T)
    pol = th.randn(T + 1, N, A, K, device="cuda", generator=g).requires_grad_(True)
    tgt = th.randn(T, N, A, K, device="cuda", generator=g)
    acts = th.randint(0, A, (T, N), device="cuda", generator=g)
    rews = th.randn(T, B, n, device="cuda", generator=g)
    dones = (th.rand(T, B, 1, device="cuda", generator=g) < 0.05).float()
    w = th.rand(B, device="cuda", generator=g) + 0.5
    ws = {}

    def run(select, loss, **kw):
        pol.grad = None
        theta_a, theta_next, _, _ = select(pol, tgt, acts, True)
        l, td = loss(theta_a.view(T, B, n, K), theta_next.view(T, B, n, K), rews, dones, w, GAMMA, N_STEP, 1.0, **kw)
        l.backward()
        return l.detach(), td, pol.grad

    def kernels():
        return run(ops.qr_select, ops.qr_loss, workspace=ws)

    def torch_arm():
        return run(ops.qr_select_torch, ops.qr_loss_torch)
    arms = {"kernels": kernels}
    if with_torch:
        arms["torch"] = torch_arm
        lk, tdk, gk = [t.clone() for t in kernels()]
        lt, tdt, gt = torch_arm()
        err = dict(loss=abs(float(lk) - float(lt)) / abs(float(lt)), td=float((tdk - tdt).abs().max() / tdt.abs().max()),
                   grad=float((gk - gt).abs().max() / gt.abs().max()))
    ms, iters = _alternate(arms, rounds, window_ms, floor=2)
    total, loss_only = tail_bytes(T, N, K)
    rows = [dict(what="quantile TD tail", arm=k, envs=B, agents=n, T=T, rows=T * N, A=A, K=K, n_step=N_STEP, iters_per_window=iters[k],
                 windows=rounds, **_stat(v)) for k, v in ms.items()]
    med = {r["arm"]: r["median_ms"] for r in rows}
    summary = dict(what="floor and ratios of medians", rows=T * N, K=K, bytes_moved=total, floor_ms_at_8TBps=round(1e3 * total / HBM_PEAK, 5),
                   kernels_over_floor=round(med["kernels"] / (1e3 * total / HBM_PEAK), 2), loss_launch_bytes=loss_only,
                   pairs=T * N * K * K)
    if with_torch:
        summary.update(kernels_over_torch=round(med["kernels"] / med["torch"], 4), intermediate_bytes_torch=4 * T * N * K * K,
                       max_rel_difference_to_torch=err)
    rows.append(summary)
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def loss_launch_rows(B, n, T, K, rounds, window_ms):
    """The loss launch alone (the VALU-bound one by count: about ten operations per pair)."""
    import torch as th

    from uav_bs_ctrl_amd import ops
    g = th.Generator(device="cuda").manual_seed(K)
    theta_a = th.randn(T, B, n, K, device="cuda", generator=g)
    theta_next = th.randn(T, B, n, K, device="cuda", generator=g)
    rews = th.randn(T, B, n, device="cuda", generator=g)
    dones = (th.rand(T, B, 1, device="cuda", generator=g) < 0.05).float()
    w = th.rand(B, device="cuda", generator=g) + 0.5
    ws, td = {}, th.empty(T, B, n, device="cuda")
    ms, iters = _alternate({"qr_loss": lambda: ops.qr_loss(theta_a, theta_next, rews, dones, w, GAMMA, N_STEP, 1.0, td_out=td, workspace=ws)},
                           rounds, window_ms)
    nbytes = 4 * 3 * T * B * n * K
    st = _stat(ms["qr_loss"])
    row = dict(what="uavgnn_qr_loss_fwd alone", rows=T * B * n, K=K, iters_per_window=iters["qr_loss"], windows=rounds, **st, bytes_moved=nbytes,
               floor_ms_at_8TBps=round(1e3 * nbytes / HBM_PEAK, 5), pairs=T * B * n * K * K,
               pairs_per_ns=round(T * B * n * K * K / (1e6 * st["median_ms"]), 2))
    print(json.dumps(row), flush=True)
    return [row]


def episode_rows(rounds, window_ms, K=32):
    import torch as th

    from uav_bs_ctrl_amd.graphs import GraphedEpisode
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.run import seed_comm_modules
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    runs = {}
    for name, quantiles in (("off", None), ("on", K)):
        th.manual_seed(0)
        env = BatchedUbsCoverageEnv.from_map("8ubs", E, seed=0)
        args = types.SimpleNamespace(device="cuda", hidden_size=H, c="tarmac", n_heads=4, n_layers=2, msg_size=64, key_size=16, n_rounds=1,
                                     dueling=False, mixer=False, share_reward=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999,
                                     max_seq_len=None, batch_size=BATCH, seed=0)
        info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
        rb = SequenceReplay(8 * E, env.episode_limit, env.n_agents, env.n_gts, H, n_envs=E, state_dim=0, r_comm=env.p.r_comm,
                            device_state=True, seed=0)
        learner = MultiAgentQLearner(info, args, quantiles=quantiles)
        seed_comm_modules(learner, 0)
        runs[name] = (GraphedEpisode(learner, env, rb, BATCH, eps=(1.0, 0.05, 5e4)), rb, env)
    ms, iters = _alternate({k: v[0] for k, v in runs.items()}, rounds, window_ms, floor=2)
    out = []
    for name, (ge, rb, env) in runs.items():
        rb.check()
        out.append(dict(what="GraphedEpisode replay, '8ubs', TarMAC, H = 256", quantiles=name if name == "off" else K, envs=E, batch=BATCH,
                        episode_limit=env.episode_limit, iters_per_window=iters[name], windows=rounds, **_stat(ms[name])))
    out.append(dict(what="ratio of medians", on_over_off=round(out[1]["median_ms"] / out[0]["median_ms"], 4),
                    note="off runs the fused TarMAC step; on runs the generic route (communication block, then the [A K, H] head) in the "
                         "rollout, the evaluation of both networks over the sequence and the quantile tail"))
    for r in out:
        print(json.dumps(r), flush=True)
    return out


def main():   # noqa: D103
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-episode", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    sizes = [(32, 8, 10)] + ([] if a.skip_large else [(4096, 8, 50)])
    for B, n, T in sizes:
        for K in (8, 32, 64):
            large = B * n * T > 1 << 20
            rows += tail_rows(B, n, T, K, a.rounds, a.window_ms, with_torch=not (large and K == 64))
            rows += loss_launch_rows(B, n, T, K, a.rounds, a.window_ms)
    if not a.skip_episode:
        rows += episode_rows(a.rounds, a.window_ms)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# quantile_probe: A = {A}, n_step = {N_STEP}; windows of {a.window_ms:g} ms between device events, {a.rounds} per arm, arms "
                    "alternating; median [min .. max] in ms per iteration\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

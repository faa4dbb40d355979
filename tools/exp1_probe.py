#!/usr/bin/env python
"""Experiment 1 on the device path: env-steps/s of the rollout (act -> stage -> step -> cache) and of the whole cycle (rollout of
max_seq_len steps + one update on 32 stored sequences) at BASELINE's configuration C1 (one UBS x 20 GTs, DRQN 'gnn' agent, H = 256,
4 heads, 32 parallel environments) and at 4096 parallel environments; the launch-to-launch time of the two kernels of
csrc/subs_env.hip alone at B = 1 / 32 / 4096; and - where the reference is importable (--reference PATH, with the stand-ins of
oracle/) - the reference environment's own ``step`` rate on the host, one instance, in the same run.

    python tools/exp1_probe.py [--envs 32 4096] [--steps 200] [--reference /path/to/uav_bs_ctrl] [--host-only]
    python tools/exp1_probe.py --ab [--agents gnn rnn] [--repeats 3]

--ab: the rows that decide the default of ``ops.GRU_SEQ`` at the reference's operating point (32 environments / 32 sequences x T = 10 x
H = 256 x 1 x 20), per agent: the update alone, the 10-step rollout and the cycle, each on three arms - `per-step` (ops.GRU_SEQ off and
``gather(time_batched=False)``: 2T + 1 separate forwards, the launch sequence of the commit before the sequence route - on THIS tree, whose
``DrqnGnnAgent.forward`` is ``step(encode())``; the baseline proper is that commit's own checkout running its own probe, recorded next to these rows
in profiles/exp1_probe.txt), `sequence` (the defaults, eager) and `graphed`
(``graphs.GraphedSingleUbsAct`` on the simulator's buffers / ``GraphedSingleUbsUpdate`` replayed) - every arm repeated --repeats times.

Measurements, not thresholds: host clock around work that ends in a device synchronise, after a warm-up of every shape."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C1 = dict(n_grps=4, gts_per_grp=5)      # 1 x 20
T_SEQ, UPDATE_BATCH = 10, 32            # algos/drqn/config.py: max_seq_len, batch_size


def reference_step_rate(path, steps):
    """envs/subs_cov/subs_cov.py imported unchanged: seconds per ``step`` of ONE environment on this host."""
    sys.path[:0] = [os.path.join(ROOT, "oracle", "gym_standin"), path]
    from envs.subs_cov.subs_cov import SingleUbsCoverageEnv
    np.random.seed(0)
    env = SingleUbsCoverageEnv(episode_limit=10 ** 9, record=False, **C1)
    env.reset()
    acts = np.random.default_rng(0).integers(0, env.n_actions, steps)
    for a in acts[:50]:
        env.step(int(a))
    t0 = time.perf_counter()
    for a in acts:
        env.step(int(a))
    dt = time.perf_counter() - t0
    return dict(what="reference SingleUbsCoverageEnv.step on the host (one instance, 1 x 20)", steps=int(steps),
                us_per_step=1e6 * dt / steps, env_steps_per_s=steps / dt)


def device_rates(B, steps):
    import torch as th

    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    p = SingleUbsParams(episode_limit=200, **C1)
    env = BatchedSingleUbsCoverageEnv(p, B, seed=0)
    args = types.SimpleNamespace(device="cuda", agent="gnn", hidden_size=256, n_heads=4, n_layers=2, max_seq_len=T_SEQ, gamma=0.99,
                                 polyak=0.999, batch_size=UPDATE_BATCH, lr=5e-4, anneal_lr=False, seed=0)
    learner = QLearner(env.get_env_info("gnn"), args)
    buf = SingleUbsSequenceReplay(max(2 * B, 2 * UPDATE_BATCH), T_SEQ, p.n_gts, 256, n_envs=B, device="cuda")
    state = dict(obs=env.reset(), h=learner.init_hidden(B), t=0)

    def rollout(n):
        for _ in range(n):
            obs, h = state["obs"], state["h"]
            a, h2 = learner.act(env.graph(), h, 0.1)
            buf.stage_obs(dict(gt=obs["gt"], agent=obs["agent"], h=h))
            obs, rew, done, info = env.step(a)
            learner.cache(buf, None, None, a, rew, obs, h2, done, info["BadMask"], staged=True)
            state["t"] += 1
            if state["t"] % p.episode_limit == 0:      # every environment ends at the limit: no host read of `done`
                obs, h2 = env.reset(), learner.init_hidden(B)
            state["obs"], state["h"] = obs, h2

    def cycle():
        rollout(T_SEQ)
        learner.update(buf.sample(UPDATE_BATCH, enc="gnn"))

    def timed(fn, reps):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        th.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    rollout(4 * T_SEQ)
    cycle(), cycle()
    n_roll = max(steps // T_SEQ, 1)
    t_roll = timed(lambda: rollout(T_SEQ), n_roll)
    t_cyc = timed(cycle, n_roll)
    return dict(what=f"device path, 1 x 20, DRQN gnn H=256, {B} parallel environments", envs=B, rollout_steps=n_roll * T_SEQ,
                rollout_ms_per_step=1e3 * t_roll / T_SEQ, rollout_env_steps_per_s=B * T_SEQ / t_roll,
                cycle_ms=1e3 * t_cyc, cycle_env_steps_per_s=B * T_SEQ / t_cyc, update_batch=UPDATE_BATCH, seq_len=T_SEQ)


def ab_rows(agent, repeats, iters=20):
    """[{phase, arm, ms: [one mean per repeat]}] for `agent` at the reference's operating point."""
    import torch as th

    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.graphs import GraphedSingleUbsAct, GraphedSingleUbsUpdate
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    B = UPDATE_BATCH
    p = SingleUbsParams(episode_limit=200, **C1)
    env = BatchedSingleUbsCoverageEnv(p, B, seed=0)
    args = types.SimpleNamespace(device="cuda", agent=agent, hidden_size=256, n_heads=4, n_layers=2, max_seq_len=T_SEQ, gamma=0.99,
                                 polyak=0.999, batch_size=UPDATE_BATCH, lr=5e-4, anneal_lr=False, seed=0)
    learner = QLearner(env.get_env_info(agent), args)
    buf = SingleUbsSequenceReplay(4 * B, T_SEQ, p.n_gts, 256, n_envs=B, device="cuda")
    state = dict(obs=env.reset(), h=learner.init_hidden(B), t=0)
    ga = GraphedSingleUbsAct(learner, B, p.n_gts, agent, obs=(env.out["obs_gt"], env.out["obs_agent"]))
    gu = GraphedSingleUbsUpdate(learner, B, T_SEQ, p.n_gts, agent)
    obs_in = (lambda: env.graph()) if agent == "gnn" else (lambda: env.observations()["flat"])

    def rollout(graphed):
        for _ in range(T_SEQ):
            obs, h = state["obs"], state["h"]
            if graphed:
                a, h2 = ga(None, None, h, 0.1)
                h2 = h2.clone()          # the graph's output buffer is overwritten by the next replay; the replay stores h AND h'
            else:
                a, h2 = learner.act(obs_in(), h, 0.1)
            buf.stage_obs(dict(gt=obs["gt"], agent=obs["agent"], h=h))
            obs, rew, done, info = env.step(a)
            learner.cache(buf, None, None, a, rew, obs, h2, done, info["BadMask"], staged=True)
            state["t"] += 1
            if state["t"] % p.episode_limit == 0:
                obs, h2 = env.reset(), learner.init_hidden(B)
            state["obs"], state["h"] = obs, h2

    def update(arm):
        idx = buf.sample_indices(UPDATE_BATCH)
        if arm == "graphed":
            return gu({k: v.index_select(0, idx) for k, v in buf.mem.items()})
        return learner.update(buf.gather(idx, agent, time_batched=arm == "sequence"))

    def timed(fn):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        th.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / iters
    for _ in range(4):
        rollout(False)
    rows = []
    phases = (("update", lambda arm: update(arm)), ("rollout of 10 steps", lambda arm: rollout(arm == "graphed")),
              ("cycle", lambda arm: (rollout(arm == "graphed"), update(arm))))
    for phase, fn in phases:
        for arm in ("per-step", "sequence", "graphed"):
            if phase.startswith("rollout") and arm == "sequence":
                continue                  # `act` has one eager path: the rollout gains from the capture only
            ops.GRU_SEQ = arm != "per-step"
            fn(arm), fn(arm)
            rows.append(dict(what=f"exp1 {agent}, 32 x T=10 x H=256, 1 x 20", phase=phase, arm=arm, iters=iters,
                             ms=[round(timed(lambda: fn(arm)), 4) for _ in range(repeats)]))
    ops.GRU_SEQ = True
    return rows


def kernel_times(reps=2000):
    """Launch-to-launch time of each kernel alone (back-to-back launches, one synchronise at the end)."""
    import torch as th

    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    out = []
    for B in (1, 32, 4096):
        env = BatchedSingleUbsCoverageEnv(SingleUbsParams(episode_limit=10 ** 9, **C1), B, seed=0)
        env.reset()
        a = th.randint(0, env.n_actions, (B,), device="cuda")
        bufs = env.sample_positions()
        row = dict(what="kernels of csrc/subs_env.hip alone, back-to-back launches", envs=B, launches=reps)
        for name, fn in (("step_us", lambda: env._launch(a)), ("sample_us", lambda: env._sample_into(*bufs))):
            for _ in range(20):
                fn()
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            th.cuda.synchronize()
            row[name] = 1e6 * (time.perf_counter() - t0) / reps
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[32, 4096])
    ap.add_argument("--steps", type=int, default=200, help="environment steps per timed window and configuration")
    ap.add_argument("--reference", default=None, help="checkout of the reference project (its host `step` rate is measured in this run)")
    ap.add_argument("--host-only", action="store_true", help="only the reference environment's host rate (no GPU needed)")
    ap.add_argument("--ab", action="store_true", help="per-step / sequence / graphed arms of update, rollout and cycle at 32 x T=10 x H=256")
    ap.add_argument("--agents", nargs="+", default=["gnn", "rnn"])
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.ab:
        for agent in a.agents:
            for r in ab_rows(agent, a.repeats):
                print(json.dumps(r), flush=True)
        return
    rows = []
    if a.reference and os.path.isdir(os.path.join(a.reference, "envs", "subs_cov")):
        rows.append(reference_step_rate(a.reference, max(a.steps, 2000)))
    else:
        rows.append(dict(what="reference SingleUbsCoverageEnv.step on the host", note="reference not importable here: not measured"))
    if not a.host_only:
        import torch as th
        if not th.cuda.is_available():
            raise SystemExit("exp1_probe: no GPU (there is no CPU fallback); --host-only measures the reference environment alone")
        rows += kernel_times()
        rows += [device_rates(B, a.steps) for B in a.envs]
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()

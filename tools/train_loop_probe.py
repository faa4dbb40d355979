#!/usr/bin/env python
"""env-steps/s of the TRAINING LOOP (run.py:81-99: act -> step -> cache, one update per sequence) at the reference's operating points,
on three arms:

  (a) eager, host-state replay      the loop as it stood before the replay state moved to the device: ``learner.act`` with a host
                                    epsilon, ``SequenceReplay.push`` committing at a Python ``head``, ``torch.randperm`` sampling,
                                    ``gather`` + ``learner.update`` - THE BASELINE
  (b) eager, device-state replay    ``graphs.Episode``: the same launches as (c), issued one by one
  (c) one graph per episode         ``graphs.GraphedEpisode``

  exp3   map '8ubs' (8 x 50, episode limit 50 = T), TarMAC, H = 256, 32 environments, batch 32
  exp1   n_grps = 4 x gts_per_grp = 5 (1 x 20, episode limit 200, T = 10), 'gnn' and 'rnn' agents, 32 environments, batch 32

and the one-launch batch gather (``gather_into``) against ``index_select`` per field + ``GraphedUpdate.load`` at B = 32 and B = 4096
(8 x 80, T = 50): microseconds and the fraction of 8 TB/s at 2 x the bytes moved.

    python tools/train_loop_probe.py [--episodes 6] [--repeats 3] [--skip-gather] [--out profiles/train_loop_probe.txt]

Measurements, not thresholds - nothing here switches on by default: host clock around work that ends in a device synchronise, after
a warm-up of every arm.  One JSON row per measurement; --out also writes them as a table."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, BATCH = 32, 32
EPS = (1.0, 0.05)
HBM_BYTES_PER_S = 8e12


def _timed(fn, reps):
    import torch as th
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    th.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def _exp3(device_state):
    import torch as th

    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(0)
    env = BatchedUbsCoverageEnv.from_map("8ubs", E, seed=0)
    args = types.SimpleNamespace(device="cuda", hidden_size=256, c="tarmac", n_heads=4, n_layers=2, msg_size=64, key_size=16, n_rounds=1,
                                 dueling=False, mixer=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999, max_seq_len=None,
                                 batch_size=BATCH, seed=0)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    rb = SequenceReplay(8 * E, env.episode_limit, env.n_agents, env.n_gts, 256, n_envs=E, r_comm=env.p.r_comm,
                        device_state=device_state, seed=0 if device_state else None)
    return MultiAgentQLearner(info, args), env, rb, 5e4


def _exp1(agent):
    def make(device_state):
        import torch as th

        from uav_bs_ctrl_amd.learner import QLearner
        from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
        from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
        th.manual_seed(0)
        p = SingleUbsParams(episode_limit=200, n_grps=4, gts_per_grp=5)
        env = BatchedSingleUbsCoverageEnv(p, E, seed=0)
        args = types.SimpleNamespace(device="cuda", agent=agent, hidden_size=256, n_heads=4, n_layers=2, max_seq_len=10, gamma=0.99,
                                     polyak=0.999, batch_size=BATCH, lr=5e-4, anneal_lr=False, seed=0)
        rb = SingleUbsSequenceReplay(64 * E, 10, p.n_gts, 256, n_envs=E, device_state=device_state, seed=0 if device_state else None)
        return QLearner(env.get_env_info(agent), args), env, rb, 2e5
    return make


def _host_state_episode(learner, env, rb, enc, decay, counter):
    """Arm (a): one episode of the loop with the replay state and the schedule on the host."""
    from uav_bs_ctrl_amd.graph import from_padded_obs
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv
    single = isinstance(env, BatchedSingleUbsCoverageEnv)
    n = 1 if single else env.n_agents
    obs = env.reset() if single else env.reset_from_map()
    h = learner.init_hidden(E)
    for _ in range(env.episode_limit // rb.T):
        for _ in range(rb.T):
            eps = max(EPS[1], EPS[0] - (EPS[0] - EPS[1]) / decay * counter[0])
            counter[0] += E
            if single:
                g = env.graph() if enc == "gnn" else obs["flat"]
                rb.stage_obs(dict(gt=obs["gt"], agent=obs["agent"], h=h))
            else:
                g = from_padded_obs(obs["gt"], obs["ubs"], obs["agent"], obs["d_u2u"], env.p.r_comm)
                rb.stage_obs(dict(gt=obs["gt"], ubs=obs["ubs"], agent=obs["agent"], d_u2u=obs["d_u2u"], h=h.view(E, n, -1)))
            a, h2 = learner.act(g, h, eps)
            obs, rew, done, info = env.step(a)
            if single:
                learner.cache(rb, None, None, a, rew, obs, h2, done, info["BadMask"], staged=True)
            else:
                learner.cache(rb, None, None, None, a, rew, obs, h2, None, done, info["BadMask"], staged=True)
            h = h2
        learner.update(rb.sample(BATCH, enc=enc))


def loop_rows(name, make, enc, episodes, repeats):
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    rows = []
    for arm in ("a: eager, host-state replay", "b: eager, device-state replay", "c: one graph per episode"):
        learner, env, rb, decay = make(not arm.startswith("a"))
        if arm.startswith("a"):
            counter = [0]
            run = lambda: _host_state_episode(learner, env, rb, enc, decay, counter)  # noqa: E731
        else:
            run = (Episode if arm.startswith("b") else GraphedEpisode)(learner, env, rb, BATCH, eps=(*EPS, decay), enc=enc)
        run(), run()
        steps = env.episode_limit * E
        secs = [_timed(run, episodes) for _ in range(repeats)]
        if not arm.startswith("a"):
            rb.check()
        rows.append(dict(what=name, arm=arm, envs=E, batch=BATCH, episode_limit=env.episode_limit, seq_len=rb.T, episodes=episodes,
                         ms_per_episode=[round(1e3 * s, 3) for s in secs], env_steps_per_s=[round(steps / s) for s in secs]))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def gather_rows(reps=20):
    import torch as th

    from uav_bs_ctrl_amd.graphs import GraphedUpdate
    from uav_bs_ctrl_amd.replay import SequenceReplay
    n, M, T, H = 8, 80, 50, 256
    rb = SequenceReplay(64, T, n, M, H, n_envs=1, device_state=True, seed=0)
    for v in rb.mem.values():
        v.copy_(th.randn(v.shape, device="cuda")) if v.dtype != th.int64 else v.random_(0, 9)
    rb.state.copy_(th.tensor([0, 64], device="cuda"))
    fake = types.SimpleNamespace(fused_tail=True, device=th.device("cuda"), args=types.SimpleNamespace(hidden_size=H, c="tarmac"))
    rows = []
    for B in (32, 4096):
        gu = GraphedUpdate(fake, B, T, n, M, capture=False)
        idx = th.randint(0, 64, (B,), device="cuda")
        moved = sum(t.numel() * t.element_size() for t in (gu.obs.gt, gu.obs.ubs, gu.obs.agent, gu.obs.d_u2u, gu.h0, gu.h1, gu.acts,
                                                           gu.rews, gu.dones))
        old = lambda: gu.load({k: v.index_select(0, idx) for k, v in rb.mem.items()})  # noqa: E731
        new = lambda: gu.load_from(rb, idx)  # noqa: E731
        old(), new()
        for arm, fn in (("index_select per field + load", old), ("gather_into (one launch)", new)):
            us = 1e6 * _timed(fn, reps)
            rows.append(dict(what="batch gather, 8 x 80, T = 50", arm=arm, B=B, bytes_moved=moved, us=round(us, 1),
                             fraction_of_8TBps_at_2x_bytes=round(2 * moved / (us * 1e-6) / HBM_BYTES_PER_S, 4)))
            print(json.dumps(rows[-1]), flush=True)
        del gu
        th.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=6, help="episodes per timed window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--points", nargs="+", default=["exp3", "exp1-gnn", "exp1-rnn"])
    ap.add_argument("--skip-gather", action="store_true")
    ap.add_argument("--out", default=None, help="also write the rows as a table")
    a = ap.parse_args()
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("train_loop_probe: no GPU (there is no CPU fallback)")
    rows = []
    if "exp3" in a.points:
        rows += loop_rows("exp3: '8ubs' 8 x 50, TarMAC, H = 256", _exp3, "gnn", a.episodes, a.repeats)
    for agent in ("gnn", "rnn"):
        if f"exp1-{agent}" in a.points:
            rows += loop_rows(f"exp1: 1 x 20, DRQN '{agent}', H = 256", _exp1(agent), agent, max(a.episodes // 2, 1), a.repeats)
    if not a.skip_gather:
        rows += gather_rows()
    if a.out:
        with open(a.out, "w") as f:
            f.write("training-loop probe (tools/train_loop_probe.py): MI355X, host clock around a device synchronise; arm (a) is the baseline\n\n")
            for r in rows:
                if "ms_per_episode" in r:
                    f.write(f"{r['what']:<44} {r['arm']:<34} ms/episode {r['ms_per_episode']}  env-steps/s {r['env_steps_per_s']}\n")
                else:
                    f.write(f"{r['what']:<44} {r['arm']:<34} B = {r['B']:<5} {r['us']:>10.1f} us  {r['bytes_moved'] / 1e6:9.1f} MB moved  "
                            f"{100 * r['fraction_of_8TBps_at_2x_bytes']:.1f} % of 8 TB/s at 2 x bytes\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""One ``test_agent()`` (run.py:63-74) at the reference's sizes, on three arms:

  (a) hand-written loop      reset, then per step a graph from the simulator's buffers, ``learner.act(o, h, 0.05)``, ``env.step`` - what a
                             caller had before ``graphs.Evaluation`` (it draws from the learner's generator) - THE BASELINE
  (b) graphs.Evaluation      the same steps with the in-kernel draws, eager
  (c) graphs.GraphedEvaluation   ... as one graph replay

  exp3   map '8ubs' (8 x 50, episode limit 50), TarMAC, H = 256, 10 evaluation environments x 1 round (num_test_episodes = 10)
  exp1   n_grps = 4 x gts_per_grp = 5 (1 x 20, episode limit 200), 'gnn' agent, H = 256, 10 environments x 1 round

    python tools/eval_probe.py [--runs 3] [--out profiles/eval_probe.txt]
    python tools/eval_probe.py --film [--runs 7] [--out profiles/eval_film_probe.txt]

--film: arm (c) alone, twice in one process - without a film and with ``film=Film(env, 10)`` (one more launch per reset and per step,
csrc/film.hip) -, the two graphs replayed alternately; per arm the launches a replay holds that the other does not.

Measurements, not thresholds: host clock around one call that ends in a device synchronise, after a warm-up call of every arm; ``runs``
runs per arm, the median reported.  One JSON row per arm; the table goes to --out (default profiles/eval_probe.txt)."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, EPS = 10, 0.05


def _exp3():
    import torch as th

    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(0)
    env = BatchedUbsCoverageEnv.from_map("8ubs", E, seed=1)
    args = types.SimpleNamespace(device="cuda", hidden_size=256, c="tarmac", n_heads=4, n_layers=2, msg_size=64, key_size=16, n_rounds=1,
                                 dueling=False, mixer=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999, max_seq_len=None,
                                 batch_size=32, seed=0)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    return MultiAgentQLearner(info, args), env, "gnn"


def _exp1():
    import torch as th

    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    th.manual_seed(0)
    env = BatchedSingleUbsCoverageEnv(SingleUbsParams(episode_limit=200, n_grps=4, gts_per_grp=5), E, seed=1)
    args = types.SimpleNamespace(device="cuda", agent="gnn", hidden_size=256, n_heads=4, n_layers=2, max_seq_len=10, gamma=0.99,
                                 polyak=0.999, batch_size=32, lr=5e-4, anneal_lr=False, seed=0)
    return QLearner(env.get_env_info("gnn"), args), env, "gnn"


def _act_loop(learner, env):
    """Arm (a): one round of run.py:63-74 for env.B environments around ``learner.act``."""
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv
    single = isinstance(env, BatchedSingleUbsCoverageEnv)

    def run():
        env.reset() if single else env.reset_from_map()
        h, info = learner.init_hidden(env.B), None
        for _ in range(env.episode_limit):
            a, h = learner.act(env.graph(), h, EPS)
            _, _, _, info = env.step(a)
        return info["EpRet"]
    return run


def rows_for(name, make, runs):
    import torch as th

    from uav_bs_ctrl_amd.graphs import Evaluation, GraphedEvaluation
    rows = []
    for arm in ("a: learner.act loop", "b: graphs.Evaluation", "c: graphs.GraphedEvaluation"):
        learner, env, enc = make()
        run = _act_loop(learner, env) if arm.startswith("a") else (Evaluation if arm.startswith("b") else GraphedEvaluation)(
            learner, env, E, eps=EPS, seed=0, enc=enc)
        run()
        ms = []
        for _ in range(runs):
            th.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            th.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        rows.append(dict(what=name, arm=arm, envs=E, episode_limit=env.episode_limit, ms=[round(m, 3) for m in ms],
                         median_ms=round(statistics.median(ms), 3)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def film_rows_for(name, make, runs):
    """GraphedEvaluation without and with a film, both built first and then replayed alternately (the same process, the same clocks)."""
    import torch as th

    from uav_bs_ctrl_amd.film import Film
    from uav_bs_ctrl_amd.graphs import GraphedEvaluation
    arms = {}
    for arm in ("c: GraphedEvaluation", "d: GraphedEvaluation(film=...)"):
        learner, env, enc = make()
        film = Film(env, E) if arm.startswith("d") else None
        arms[arm] = (GraphedEvaluation(learner, env, E, eps=EPS, seed=0, enc=enc, film=film), env, film)
        arms[arm][0]()
    ms = {arm: [] for arm in arms}
    for _ in range(runs):
        for arm, (run, _, _) in arms.items():
            th.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            th.cuda.synchronize()
            ms[arm].append(1e3 * (time.perf_counter() - t0))
    rows = []
    for arm, (_, env, film) in arms.items():
        if film is not None:
            film.check()
        rows.append(dict(what=name, arm=arm, envs=E, episode_limit=env.episode_limit, film_launches=0 if film is None else 1 + env.episode_limit,
                         ms=[round(m, 3) for m in ms[arm]], median_ms=round(statistics.median(ms[arm]), 3)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=None, help="timed calls per arm (default 3; 7 with --film)")
    ap.add_argument("--film", action="store_true", help="the graphed evaluation without and with a trajectory film")
    ap.add_argument("--points", nargs="+", default=["exp3", "exp1"])
    ap.add_argument("--out", default=None, help="the rows as a table ('' for none; default profiles/eval_probe.txt, "
                    "profiles/eval_film_probe.txt with --film)")
    a = ap.parse_args()
    if a.runs is None:
        a.runs = 7 if a.film else 3
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "eval_film_probe.txt" if a.film else "eval_probe.txt")
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("eval_probe: no GPU (there is no CPU fallback)")
    rows, rows_of = [], film_rows_for if a.film else rows_for
    if "exp3" in a.points:
        rows += rows_of("exp3: '8ubs' 8 x 50, TarMAC, H = 256", _exp3, a.runs)
    if "exp1" in a.points:
        rows += rows_of("exp1: 1 x 20, DRQN 'gnn', H = 256", _exp1, a.runs)
    if a.out:
        with open(a.out, "w") as f:
            if a.film:
                f.write("evaluation film probe (tools/eval_probe.py --film): one graphed test_agent() of 10 episodes without and with a "
                        "trajectory film, MI355X, host clock around a device synchronise, the two graphs replayed alternately\n\n")
            else:
                f.write("evaluation probe (tools/eval_probe.py): one test_agent() of 10 episodes, MI355X, host clock around a device "
                        "synchronise; arm (a) is the baseline\n\n")
            for r in rows:
                extra = f"   film launches {r['film_launches']}" if a.film else ""
                f.write(f"{r['what']:<40} {r['arm']:<32} median {r['median_ms']:>9.3f} ms   runs {r['ms']}{extra}\n")


if __name__ == "__main__":
    main()

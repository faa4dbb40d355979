#!/usr/bin/env python
"""A six-run series (``uav_bs_ctrl_amd.series``) at exp3 sizes, timed two ways:

  (a) one runner per run     per run directory a new ``PolicyRunner`` - simulator, learner, film, warm-up and capture of a
                             ``GraphedEvaluation`` - then one evaluation: what the loop costs when it is written by hand around
                             ``film.load_and_run_policy`` - THE BASELINE
  (b) one runner, reused     ``test_series``' way: the runner of the configuration is built for the first run, every later run loads its
                             checkpoint and its seeds in place and replays

  map '8ubs' (8 x 50, episode limit 50), TarMAC, H = 256, six seeds of one arm, 10 episodes on 10 evaluation environments, films written
  (``episode{k}/`` with its three CSV files, as ``test_series`` does).  The run directories are crafted: a freshly initialised learner's
  checkpoint and a ``config.json`` - the time of an evaluation does not depend on what the weights hold.

    python tools/series_probe.py [--repeats 2] [--out profiles/series_probe.txt]

Measurements, not thresholds: host clock around each run (``describe`` to the films on disk, ending in the device-to-host copies), after
one throw-away run that pays the process's first-use costs; the two arms alternate ``repeats`` times.  One JSON row per arm and repeat;
the table goes to --out."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS, EPISODES, CKPT = 6, 10, "checkpoint_epoch100.pt"
ARGS = dict(device="cuda", o="gnn", c="tarmac", share_reward=False, hidden_size=256, n_layers=2, n_heads=4, msg_size=64, key_size=16, n_rounds=1,
            lr=5e-4, gamma=0.99, polyak=0.999, double_q=True, dueling=False, mixer=False, steps_per_epoch=5000, epochs=100, update_after=5000,
            num_test_episodes=10, save_freq=10, decay_steps=5e4, batch_size=32, replay_size=5000, max_seq_len=None, anneal_lr=True)


def make_dirs(base):
    import torch as th

    from uav_bs_ctrl_amd import run as R
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    ns = R.check_args("exp3", ARGS)
    info = BatchedUbsCoverageEnv.from_map("8ubs", 1, seed=0).get_env_info("gnn")
    env_fn, env_kwargs = R._reference_env("exp3", "8ubs")
    dirs = []
    for seed in range(RUNS):
        d = os.path.join(base, "exp3_8ubs_gnn_tarmac", f"s{seed}")
        os.makedirs(d)
        th.manual_seed(seed)
        MultiAgentQLearner(info, ns).save_checkpoint(os.path.join(d, CKPT), dict(epoch=100, t=0))
        with open(os.path.join(d, "config.json"), "w") as f:
            f.write(R.config_text(dict(env_fn=env_fn, env_kwargs=env_kwargs, seed=seed, args=ns), "exp3_8ubs_gnn_tarmac"))
        dirs.append(d)
    return dirs


def one_series(dirs, out, reuse):
    """[seconds per run], {seed: table}."""
    from uav_bs_ctrl_amd import series as S
    secs, tables, runner = [], {}, None
    for d in dirs:
        t0 = time.perf_counter()
        desc = S.describe(d)
        if runner is None or not reuse:
            runner = S.PolicyRunner(desc, EPISODES)
        tables[desc.seed] = runner(os.path.join(d, CKPT), desc.seed, os.path.join(out, f"{desc.exp_name}_seed{desc.seed}"))
        secs.append(time.perf_counter() - t0)
    return secs, tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_probe.txt"), help="the rows as a table ('' for none)")
    a = ap.parse_args()
    import numpy as np
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("series_probe: no GPU (there is no CPU fallback)")
    arms = (("a: one runner per run", False), ("b: one runner, reused", True))
    rows, first = [], None
    with tempfile.TemporaryDirectory() as base:
        dirs = make_dirs(os.path.join(base, "logs"))
        one_series(dirs[:1], os.path.join(base, "throw_away"), False)
        for rep in range(a.repeats):
            for arm, reuse in arms:
                secs, tables = one_series(dirs, os.path.join(base, f"out_{rep}_{int(reuse)}"), reuse)
                first = first or tables
                same = all(np.array_equal(tables[s][k], first[s][k]) for s in first for k in first[s])
                rows.append(dict(arm=arm, repeat=rep, runs=len(dirs), s=[round(x, 3) for x in secs], s_per_run=round(sum(secs) / len(secs), 3),
                                 median_s=round(statistics.median(secs), 3), same_tables=bool(same)))
                print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("series probe (tools/series_probe.py): six runs of one arm - exp3 '8ubs' 8 x 50, TarMAC, H = 256 -, 10 episodes on 10 "
                    f"environments each, films written; {th.cuda.get_device_name()}, host clock per run; arm (a) is the baseline\n\n")
            for r in rows:
                f.write(f"{r['arm']:<24} repeat {r['repeat']}   {r['s_per_run']:>7.3f} s per run   median {r['median_s']:>7.3f} s   runs {r['s']}"
                        f"   tables equal to the first series' {r['same_tables']}\n")


if __name__ == "__main__":
    main()

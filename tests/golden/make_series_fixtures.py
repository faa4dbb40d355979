#!/usr/bin/env python
"""Generates tests/golden/series_reference.json: the two summary tables the REFERENCE's own ``test_series`` (test_policies.py:36-104)
writes - ``test_summary.csv`` and ``test_summary_t.csv`` - for made-up run directories and made-up per-run tables.  Data only, a few KB.

    python tests/golden/make_series_fixtures.py REFERENCE_TREE

``test_policies`` is imported unchanged over oracle/dgl_standin + oracle/gym_standin and the ``mpi4py`` stand-in of
make_run_fixtures.py (its imports pull in both ``run.py``, the learners and the logger).  The two entries of its ``TEST_FUNCTIONS`` are
replaced with a stub that evaluates nothing: it returns a seeded made-up DataFrame of ``n_episodes`` rows and records the order it was
called in (``os.walk`` visits directories in the file system's order: the recorded order is what the reference merged).  ``plt.show``
and ``plt.savefig`` are neutralised.  Skips when the reference tree is absent.

The directories (each holds a ``config.json`` and an empty checkpoint file):
    LOGDIRS[0]/s0, LOGDIRS[0]/s1     exp_name "arm_b", seeds 0 and 1     -> 2 * n_episodes episodes after the merge
    LOGDIRS[1]                       exp_name "arm_a", seed 5            -> n_episodes episodes (the shorter column: empty cells)
    LOGDIRS[0]/other                 no checkpoint file: not a run
"arm_b" is seen FIRST and sorts LAST: the column order of test_summary.csv (sorted) and of test_summary_t.csv (first seen) differ.

series_reference.json:  metrics, n_episodes, checkpoint, logdirs          the inputs of test_series
                        runs      [{dir (relative), exp_name, seed}]     the made-up directories
                        calls     [{dir, exp_name, seed, table: {key: [values]}}] in the order the stub was called
                        summary, summary_t                               the text of the two CSV files"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
KEYS = ("EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx", "ProbCollision")
METRICS = ["FairIdx", "EpRet", "TotalThroughput"]           # the caller's order: neither sorted nor the tables' own
N_EPISODES, CHECKPOINT = 3, "checkpoint_epoch7.pt"
LOGDIRS = ["grid_b", "grid_a"]
RUNS = [dict(dir="grid_b/s0", exp_name="arm_b", seed=0), dict(dir="grid_b/s1", exp_name="arm_b", seed=1),
        dict(dir="grid_a", exp_name="arm_a", seed=5)]


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "test_policies.py")):
        print("[make_series_fixtures] reference tree not given or not found: skipped")
        return
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, HERE)
    from make_run_fixtures import _mpi_standin
    _mpi_standin()
    sys.path[:0] = [os.path.join(ROOT, "oracle", "dgl_standin"), os.path.join(ROOT, "oracle", "gym_standin"), sys.argv[1]]
    import pandas as pd
    import test_policies as tp
    calls = []

    def stub(model_path, env_fn, env_kwargs, seed, args, n_episodes, output_dir):
        rel = os.path.relpath(os.path.dirname(model_path), base).replace(os.sep, "/")
        run = next(r for r in RUNS if r["dir"] == rel)
        assert os.path.isdir(output_dir) and os.path.basename(output_dir) == f"{run['exp_name']}_seed{seed}"
        rng = np.random.default_rng(1000 + 17 * seed + len(run["exp_name"]) + ord(run["exp_name"][-1]))
        table = {k: [float(v) for v in rng.normal(2.0, 3.0, n_episodes)] for k in KEYS}
        table["EpLen"] = [10.0] * n_episodes
        table["FairIdx"][0] = 0.1                             # a value whose repr is short, and one that needs 17 digits below
        table["EpRet"][-1] = 1.0 / 3.0
        calls.append(dict(dir=rel, exp_name=run["exp_name"], seed=seed, table=table))
        return pd.DataFrame(table)

    tp.TEST_FUNCTIONS = {k: stub for k in tp.TEST_FUNCTIONS}
    tp.plt.show = lambda *a, **k: None
    tp.plt.savefig = lambda *a, **k: None
    with tempfile.TemporaryDirectory() as base:
        for r in RUNS:
            d = os.path.join(base, r["dir"])
            os.makedirs(d)
            with open(os.path.join(d, "config.json"), "w") as f:
                json.dump(dict(exp_name=r["exp_name"], seed=r["seed"], env_fn="MultiUbsCoverageEnv",
                               env_kwargs=dict(map_id="debug", fair_service=True, avoid_collision=True),
                               args={"namespace(made_up)": dict(o="gnn", c="tarmac")}), f)
            open(os.path.join(d, CHECKPOINT), "w").close()
        os.makedirs(os.path.join(base, LOGDIRS[0], "other"))
        out_dir = os.path.join(base, "out")
        tp.test_series("madrqn", METRICS, [os.path.join(base, d) for d in LOGDIRS], CHECKPOINT, N_EPISODES, out_dir)
        texts = {}
        for key, name in (("summary", "test_summary.csv"), ("summary_t", "test_summary_t.csv")):
            with open(os.path.join(out_dir, name), newline="") as f:
                texts[key] = f.read()
    assert len(calls) == len(RUNS)
    out = dict(metrics=METRICS, n_episodes=N_EPISODES, checkpoint=CHECKPOINT, logdirs=LOGDIRS, runs=RUNS, calls=calls, **texts)
    path = os.path.join(HERE, "series_reference.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote series_reference.json:", os.path.getsize(path), "B; call order:", [c["dir"] for c in calls])
    print(texts["summary"])
    print(texts["summary_t"])


if __name__ == "__main__":
    main()

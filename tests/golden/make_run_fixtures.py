#!/usr/bin/env python
"""Generates tests/golden/run_dir_reference.json: the ``progress.txt`` the REFERENCE's own ``EpochLogger`` (utils/logx.py) writes for the
``store`` / ``log_tabular`` / ``dump_tabular`` calls of its two ``run.py`` (algos/madrqn/run.py:93-127, algos/drqn/run.py:88-123), and the
``config.json`` its ``save_config`` writes, for two epochs of made-up values.  Data only, a few KB.

    python tests/golden/make_run_fixtures.py REFERENCE_TREE

The reference's logger imports ``mpi4py``; where it is not installed a minimal single-process stand-in is put into ``sys.modules`` here
(rank 0 of 1: an all-reduce is a copy).  ``save_config`` is given the locals of ``train()`` that do not depend on the process - ``env_fn``,
``env_kwargs``, ``seed``, ``args`` - without ``logger``, whose text holds a memory address.

Per run.py (keys ``madrqn`` / ``drqn``):  epochs    [{"store": {key: [values]}, "scalars": {Epoch, Episode, TotalEnvInteracts, Time[, ExploreEps]}}]
                                          progress  the text of progress.txt
``config``: {"input": {env_fn, env_kwargs, seed, args, exp_name}, "text": the text of config.json}"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INFO = {"madrqn": ("EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx", "ProbCollision"),
        "drqn": ("EpRet", "EpLen", "AvgGlobalUtility", "FairIdx", "TotalThroughput")}
CONFIG_INPUT = dict(env_fn="MultiUbsCoverageEnv", env_kwargs=dict(map_id="debug", fair_service=True, avoid_collision=True), seed=20,
                    args=dict(device="cuda", c="tarmac", o="gnn", hidden_size=32, lr=1e-3, max_seq_len=None, anneal_lr=True, epochs=3,
                              decay_steps=200.0),
                    exp_name="made_up")


def _mpi_standin():
    try:
        import mpi4py  # noqa: F401
        return
    except ImportError:
        pass

    class _Comm:
        def Get_rank(self):
            return 0

        def Get_size(self):
            return 1

        def Allreduce(self, x, buff, op=None):
            buff[...] = x

        def Bcast(self, x, root=0):
            pass

    mod = types.ModuleType("mpi4py")
    mod.MPI = types.SimpleNamespace(COMM_WORLD=_Comm(), SUM="sum", MIN="min", MAX="max")
    sys.modules["mpi4py"] = mod


def _made_up_epochs(which, rng):
    out, episode, t = [], 0, 0
    for epoch in (1, 2):
        n_ep = 5 + epoch
        store = {k: [float(v) for v in rng.normal(3.0, 2.0, n_ep)] for k in INFO[which]}
        store["EpLen"] = [10.0] * n_ep
        store["LossQ"] = [float(v) for v in rng.uniform(0.0, 1.0, 7)]
        store["TestEpRet"] = [float(v) for v in rng.normal(5.0, 1.0, 4)]
        episode, t = episode + n_ep, t + 10 * n_ep
        scalars = dict(Epoch=epoch, Episode=episode, TotalEnvInteracts=t, Time=12.5 * epoch)
        if which == "drqn":
            scalars["ExploreEps"] = max(0.05, 1.0 - 0.95 / 200.0 * (t - 1))
        out.append(dict(store=store, scalars=scalars))
    return out


def _drive(EpochLogger, which, epochs, out_dir):
    """The logger calls of the run.py's main loop and end-of-epoch block, in their order."""
    logger = EpochLogger(output_dir=out_dir, exp_name="made_up")
    for e in epochs:
        st, sc = e["store"], e["scalars"]
        for i in range(len(st["EpRet"])):
            logger.store(**{k: st[k][i] for k in INFO[which]})
        for v in st["LossQ"]:
            logger.store(LossQ=v)
        for v in st["TestEpRet"]:
            logger.store(TestEpRet=v)
        logger.log_tabular("Epoch", sc["Epoch"])
        logger.log_tabular("Episode", sc["Episode"])
        logger.log_tabular("EpRet", with_min_and_max=True)
        logger.log_tabular("EpLen", average_only=True)
        logger.log_tabular("AvgGlobalUtility", with_min_and_max=True)
        if which == "madrqn":
            logger.log_tabular("TotalThroughput", average_only=True)
            logger.log_tabular("FairIdx", average_only=True)
            logger.log_tabular("ProbCollision", average_only=True)
        else:
            logger.log_tabular("FairIdx", average_only=True)
            logger.log_tabular("TotalThroughput", average_only=True)
        logger.log_tabular("TestEpRet", with_min_and_max=True)
        logger.log_tabular("TotalEnvInteracts", sc["TotalEnvInteracts"])
        logger.log_tabular("LossQ", average_only=True)
        if which == "drqn":
            logger.log_tabular("ExploreEps", sc["ExploreEps"])
        logger.log_tabular("Time", sc["Time"])
        logger.dump_tabular()
    logger.output_file.close()
    with open(os.path.join(out_dir, "progress.txt")) as f:
        return f.read()


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "utils")):
        raise SystemExit(__doc__)
    _mpi_standin()
    sys.path.insert(0, sys.argv[1])
    from utils.logx import EpochLogger
    rng = np.random.default_rng(5)
    out = {}
    for which in ("madrqn", "drqn"):
        epochs = _made_up_epochs(which, rng)
        with tempfile.TemporaryDirectory() as d:
            out[which] = dict(epochs=epochs, progress=_drive(EpochLogger, which, epochs, os.path.join(d, which)))
    with tempfile.TemporaryDirectory() as d:
        logger = EpochLogger(output_dir=os.path.join(d, "cfg"), exp_name=CONFIG_INPUT["exp_name"])
        cfg = CONFIG_INPUT
        logger.save_config(dict(env_fn=type(cfg["env_fn"], (), {}), env_kwargs=cfg["env_kwargs"], seed=cfg["seed"],
                                args=types.SimpleNamespace(**cfg["args"])))
        logger.output_file.close()
        with open(os.path.join(d, "cfg", "config.json")) as f:
            out["config"] = dict(input=cfg, text=f.read())
    with open(os.path.join(HERE, "run_dir_reference.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote run_dir_reference.json:", {k: len(json.dumps(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()

"""`-m gpu`: multi-step TD targets through ``Run`` at the smallest sizes of tests/run_args.py ('debug' map, 4 environments, batch 4):
``Run.create(..., returns=...)`` trains, ``config.json`` holds the key, ``Run.resume`` rebuilds a learner with the same option, and a run
without the option writes a ``config.json`` without the key."""
import json
import math

import pytest
import torch as th

from tests.run_args import small_args

pytestmark = pytest.mark.gpu

E, E_TEST, SEED = 4, 2, 3
PRIO = (0.6, 0.4, 0.9, 1e-3)


def _create(out, exp="exp3", env="debug", **kw):
    from uav_bs_ctrl_amd.run import Run
    return Run.create(exp, env, small_args(exp, epochs=2), str(out), exp_name="returns", seed=SEED, n_envs=E, n_test_envs=E_TEST, **kw)


def _loss_column(path):
    rows = [line.rstrip("\n").split("\t") for line in open(path / "progress.txt")]
    col = rows[0].index("LossQ")
    return [float(r[col]) for r in rows[1:]]


@pytest.mark.parametrize("prioritized", [None, PRIO], ids=["uniform", "prioritized"])
def test_a_run_with_lambda_returns_trains_and_resumes_with_the_option(tmp_path, prioritized):
    from uav_bs_ctrl_amd.run import Run
    run = _create(tmp_path / "on", returns=("lambda", 0.8), prioritized=prioritized, compact_replay=prioritized is not None)
    assert run.returns == ("lambda", 0.8) and run.learner.returns == ("lambda", 0.8)
    p0 = run.learner.flat.flat.clone()
    run.train(epochs=1)
    run.logger.close()
    cfg = json.loads((tmp_path / "on" / "config.json").read_text())["uav_bs_ctrl_amd"]
    assert cfg["returns"] == ["lambda", 0.8] and ("prioritized" in cfg) == (prioritized is not None)
    losses = _loss_column(tmp_path / "on")
    assert len(losses) == 1 and math.isfinite(losses[0]) and losses[0] > 0.0, losses
    assert not th.equal(run.learner.flat.flat, p0), "the epoch did not train"
    assert bool(th.isfinite(run.learner.flat.flat).all())
    params = run.learner.flat.flat.clone()
    del run
    back = Run.resume(str(tmp_path / "on"))
    assert back.returns == ("lambda", 0.8) and back.learner.returns == ("lambda", 0.8) and back.epoch == 1
    assert th.equal(back.learner.flat.flat, params)
    back.train()
    back.logger.close()
    assert back.epoch == 2 and all(math.isfinite(v) for v in _loss_column(tmp_path / "on"))


def test_nstep_on_exp1_and_a_run_without_the_option_writes_no_key(tmp_path):
    from uav_bs_ctrl_amd.run import Run
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    one = _create(tmp_path / "exp1", exp="exp1", env=SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10), returns=("nstep", 3))
    assert one.learner.returns == ("nstep", 3) and type(one.learner).__name__ == "QLearner"
    one.train(epochs=1)
    one.logger.close()
    assert json.loads((tmp_path / "exp1" / "config.json").read_text())["uav_bs_ctrl_amd"]["returns"] == ["nstep", 3]
    assert all(math.isfinite(v) for v in _loss_column(tmp_path / "exp1"))
    off = _create(tmp_path / "off")
    assert off.returns is None and off.learner.returns is None
    off.train(epochs=1)
    off.logger.close()
    assert "returns" not in json.loads((tmp_path / "off" / "config.json").read_text())["uav_bs_ctrl_amd"]
    del off
    back = Run.resume(str(tmp_path / "off"))
    assert back.returns is None and back.learner.returns is None
    back.logger.close()

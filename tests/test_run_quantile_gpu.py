"""`-m gpu`: the quantile-regression head through ``Run`` at the smallest sizes of tests/run_args.py ('debug' map, 4 environments, batch 4,
H = 64): ``Run.create(..., quantiles=8)`` beside ``prioritized`` and ``returns=("nstep", 3)`` trains, ``config.json`` and the checkpoints
carry what they must, a resumed run continues ``progress.txt`` where the uninterrupted one ends, ``series`` rebuilds the head from the
directory and evaluates it - and a run WITHOUT the option writes no key and the ``progress.txt`` it wrote before the option existed
(tests/golden/run_quantile_off_progress.txt: the rows of the same two-epoch run, recorded from the commit before this option, without
the wall-clock column)."""
import json
import math
import os

import pytest
import torch as th

from tests.run_args import small_args
from tests.test_run_gpu import _differences, _run_state, _without_time

pytestmark = pytest.mark.gpu

E, E_TEST, SEED, K = 4, 2, 3, 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_quantile_off_progress.txt")
OPTS = dict(quantiles=K, prioritized=(0.6, 0.4, 0.9, 1e-3), returns=("nstep", 3))


def _create(out, epochs=2, **kw):
    from uav_bs_ctrl_amd.run import Run
    return Run.create("exp3", "debug", small_args("exp3", epochs=epochs, hidden_size=64), str(out), exp_name="quantile", seed=SEED, n_envs=E,
                      n_test_envs=E_TEST, **kw)


def test_a_run_with_the_option_trains_resumes_and_is_evaluated_by_series(tmp_path):
    from uav_bs_ctrl_amd import series as S
    from uav_bs_ctrl_amd.agents.heads import QuantileLinear
    from uav_bs_ctrl_amd.run import Run
    whole = _create(tmp_path / "whole", epochs=4, **OPTS)
    lr = whole.learner
    A = whole.env.n_actions
    assert whole.quantiles == K and isinstance(lr.policy_net.f_out, QuantileLinear) and isinstance(lr.target_net.f_out, QuantileLinear)
    assert not hasattr(whole.args, "quantiles"), "the learner works on a copy of args"
    w0 = lr.policy_net.f_out.weight.detach().clone()
    whole.train()
    whole.logger.close()
    assert whole.interacts >= 200, "a few hundred steps"
    assert bool(th.isfinite(lr.flat.flat).all()) and not th.equal(lr.policy_net.f_out.weight, w0), "the quantile loss trains the head"
    out = tmp_path / "whole"
    ours = json.loads((out / "config.json").read_text())["uav_bs_ctrl_amd"]
    assert ours["quantiles"] == K and ours["returns"] == ["nstep", 3] and ours["prioritized"] == [0.6, 0.4, 0.9, 1e-3]
    ck = th.load(str(out / "checkpoint_epoch4.pt"), map_location="cpu")
    assert tuple(ck["model_state_dict"]["f_out.weight"].shape) == (A * K, 64) and tuple(ck["model_state_dict"]["f_out.bias"].shape) == (A * K,)
    head, rows = _without_time(out)
    losses = [float(r[head.index("LossQ")]) for r in rows]
    assert len(losses) == 4 and all(math.isfinite(v) and v > 0 for v in losses)
    want = _run_state(whole)
    del whole

    # killed after two epochs and resumed: ends bit for bit where the uninterrupted run ends, progress.txt continued
    part = _create(tmp_path / "part", epochs=4, **OPTS)
    part.train(epochs=2)
    part.logger.close()
    del part
    th.cuda.synchronize()
    th.manual_seed(12345)                                  # nothing of the resumed run may depend on the process's generator
    run = Run.resume(str(tmp_path / "part"))
    assert run.quantiles == K and run.epoch == 2 and isinstance(run.learner.policy_net.f_out, QuantileLinear)
    run.train()
    run.logger.close()
    assert not _differences(want, _run_state(run)), _differences(want, _run_state(run))
    assert _without_time(tmp_path / "part") == _without_time(out) and len(_without_time(tmp_path / "part")[1]) == 4
    del run

    # series rebuilds the head from the directory and evaluates the checkpoint on the quantile means
    d = S.describe(str(out), "cuda")
    assert d.args.quantiles == K and dict(d.key[2:])["quantiles"] == K
    runner = S.PolicyRunner(d, 4, n_envs=2)
    f_out = runner.learner.policy_net.f_out
    assert isinstance(f_out, QuantileLinear) and f_out.K == K and f_out.quantile_mode == "mean"
    path = str(out / "checkpoint_epoch4.pt")
    table = runner(path, 5)
    assert th.equal(f_out.weight.cpu(), ck["model_state_dict"]["f_out.weight"]), "the checkpoint loads into it"
    assert table and all(bool(th.isfinite(th.as_tensor(v, dtype=th.float64)).all()) for v in table.values())
    assert runner(path, 5).keys() == table.keys()


def test_a_run_without_the_option_writes_no_key_and_the_progress_it_wrote_before(tmp_path):
    from uav_bs_ctrl_amd import series as S
    off = _create(tmp_path / "off")
    assert off.quantiles is None and type(off.learner.policy_net.f_out) is th.nn.Linear and off.learner._quantile_heads == []
    off.train()
    off.logger.close()
    assert "quantiles" not in json.loads((tmp_path / "off" / "config.json").read_text())["uav_bs_ctrl_amd"]
    assert dict(S.describe(str(tmp_path / "off"), "cuda").key[2:])["quantiles"] is None
    head, rows = _without_time(tmp_path / "off")
    got = "\n".join("\t".join(r) for r in [[h for h in head if h != "Time"]] + rows) + "\n"
    with open(GOLDEN) as f:
        assert got == f.read(), "progress.txt of a run without the option changed"

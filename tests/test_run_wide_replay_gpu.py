"""`-m gpu`: ``uav_bs_ctrl_amd.run.Run`` on a replay ring beyond the one-workgroup sampler's 65 536 sequences (exp1, replay_size =
70 000, about 0.1 GB): the run samples through uavgnn_replay_sample_wide, inside the episode graph and eagerly, and both end in the same
state.  Sizes and helpers: tests/test_run_gpu.py."""
import numpy as np
import pytest

from tests.test_run_gpu import E, E_TEST, SEED, _differences, _rows, _run_state, _setup

pytestmark = pytest.mark.gpu

REPLAY_SIZE = 70_000


def _train(out, graphed):
    from uav_bs_ctrl_amd.run import Run
    exp, env, args = _setup("exp1-rnn", replay_size=REPLAY_SIZE, epochs=2)
    run = Run.create(exp, env, args, str(out), exp_name="exp1-wide-ring", seed=SEED, n_envs=E, n_test_envs=E_TEST, graphed=graphed)
    assert run.replay.capacity == REPLAY_SIZE and run.replay._sample_ws is not None, "the run does not use the wide sampler"
    run.train()
    run.logger.close()
    run.replay.check()
    head, rows = _rows(out)
    assert len(rows) == 2 and all(np.isfinite(float(r[head.index("LossQ")])) for r in rows), rows
    return _run_state(run)


def test_a_run_on_a_ring_of_70000_sequences_trains_graphed_and_eager_alike(tmp_path):
    graphed = _train(tmp_path / "graphed", True)
    assert graphed["rng"].tolist()[1] > 0 and int(graphed["status"]) == 0, "no update sampled"
    eager = _train(tmp_path / "eager", False)
    assert not _differences(graphed, eager), _differences(graphed, eager)

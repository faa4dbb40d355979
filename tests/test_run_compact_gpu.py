"""`-m gpu`: ``Run.create(..., compact_replay=True)`` - the driver on a ``replay.CompactSequenceReplay`` - at the sizes of
tests/test_run_gpu.py (map 'debug', T = 10, H = 32, 4 environments, batch 4, a ring of 8, two episode replays per epoch): the same
``progress.txt`` (but for ``Time``) and the same final checkpoint as the run on the full ring, bit for bit; interrupted after one epoch and
resumed it ends where the uninterrupted run ends; ``state.pt`` holds ``size x bytes_per_sequence`` bytes of ring; exp1 refuses the flag."""
import json

import pytest
import torch as th

from tests.run_args import small_args

pytestmark = pytest.mark.gpu

E, E_TEST, SEED, EPOCHS = 4, 2, 3, 2


def _create(out, **kw):
    from uav_bs_ctrl_amd.run import Run
    return Run.create("exp3", "debug", small_args("exp3", epochs=EPOCHS), str(out), exp_name="compact", seed=SEED, n_envs=E,
                      n_test_envs=E_TEST, **kw)


def _without_time(out):
    lines = (out / "progress.txt").read_text().split("\n")
    assert lines[-1] == ""
    head = lines[0].split("\t")
    i = head.index("Time")
    return head, [r[:i] + r[i + 1:] for r in (line.split("\t") for line in lines[1:-1])]


def _same(a, b, path="checkpoint"):
    """Walks two loaded checkpoints: tensors bit for bit, everything else by ==; returns the paths that differ."""
    if isinstance(a, th.Tensor):
        return [] if isinstance(b, th.Tensor) and a.shape == b.shape and a.dtype == b.dtype and th.equal(a, b) else [path]
    if isinstance(a, dict):
        if not isinstance(b, dict) or a.keys() != b.keys():
            return [path]
        return [p for k in a for p in _same(a[k], b[k], f"{path}.{k}")]
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return [path]
        return [p for i, (x, y) in enumerate(zip(a, b)) for p in _same(x, y, f"{path}[{i}]")]
    return [] if a == b else [path]


def _final(out):
    return th.load(out / f"checkpoint_epoch{EPOCHS}.pt", map_location="cpu", weights_only=False)


_CACHE = {}


def _whole(tmp_path_factory):
    """The uninterrupted two-epoch compact run, once per session: (directory, its parameters, its ring below `size`, bytes per sequence)."""
    if "run" not in _CACHE:
        out = tmp_path_factory.mktemp("compact") / "run"
        run = _create(out, compact_replay=True)
        run.train()
        run.logger.close()
        size = int(run.replay.state[1])
        _CACHE["run"] = (out, run.learner.flat.flat.clone(), {k: v[:size].clone() for k, v in run.replay.mem.items()},
                         run.replay.bytes_per_sequence, type(run.replay).__name__)
        del run
    return _CACHE["run"]


def test_the_compact_run_writes_the_rows_and_the_checkpoint_of_the_full_run(tmp_path, tmp_path_factory):
    out_c, params_c, _, _, ring = _whole(tmp_path_factory)
    assert ring == "CompactSequenceReplay"
    full = _create(tmp_path / "full")
    assert type(full.replay).__name__ == "SequenceReplay", "the default ring changed"
    full.train()
    full.logger.close()
    head_f, rows_f = _without_time(tmp_path / "full")
    head_c, rows_c = _without_time(out_c)
    assert head_f == head_c and len(rows_f) == EPOCHS
    assert rows_f == rows_c, "progress.txt differs beyond the Time column"
    loss = rows_f[-1][head_f.index("LossQ")]
    assert loss not in ("", "nan"), "the last epoch did not train: the comparison is vacuous"
    assert not _same(_final(tmp_path / "full"), _final(out_c))
    assert th.equal(full.learner.flat.flat, params_c)
    cfg_f, cfg_c = (json.loads((d / "config.json").read_text())["uav_bs_ctrl_amd"] for d in (tmp_path / "full", out_c))
    assert cfg_f["compact_replay"] is False and cfg_c["compact_replay"] is True


def test_a_resumed_compact_run_ends_where_the_uninterrupted_one_ends(tmp_path, tmp_path_factory):
    from uav_bs_ctrl_amd.run import Run
    out_w, params_w, mem_w, bps, _ = _whole(tmp_path_factory)
    part = _create(tmp_path / "part", compact_replay=True)
    part.train(epochs=1)
    part.logger.close()
    assert part.epoch == 1
    # the ring in state.pt: exactly size x bytes_per_sequence bytes
    state = th.load(tmp_path / "part" / "state.pt", map_location="cpu", weights_only=False)
    size = int(state["tensors"]["replay.state"][1])
    assert size == 8 and sum(v.numel() * v.element_size() for v in state["mem"].values()) == size * bps
    assert set(state["mem"]) == {"pos_ubs", "rate", "avg", "pos_gts", "h", "act", "rew", "done"}
    del part
    run = Run.resume(str(tmp_path / "part"))
    assert run.compact_replay and type(run.replay).__name__ == "CompactSequenceReplay" and run.epoch == 1
    run.train()
    run.logger.close()
    assert _without_time(tmp_path / "part") == _without_time(out_w)
    assert not _same(_final(tmp_path / "part"), _final(out_w))
    assert th.equal(run.learner.flat.flat, params_w)
    size = int(run.replay.state[1])
    bad = [k for k, v in run.replay.mem.items() if not th.equal(v[:size], mem_w[k])]
    assert not bad, f"the resumed run's ring differs in {bad}"


def test_exp1_refuses_the_compact_ring(tmp_path):
    from uav_bs_ctrl_amd.run import Run
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    with pytest.raises(ValueError, match="compact_replay"):
        Run.create("exp1", SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10), small_args("exp1"), str(tmp_path / "exp1"),
                   n_envs=E, n_test_envs=E_TEST, compact_replay=True)

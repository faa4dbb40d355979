"""No GPU: the host side of the compact replay ring - its byte formula, the constructor's refusals, ``compact_replay`` in ``config.json``
and on the command line."""
import json

import pytest

from tests.run_args import small_args
from uav_bs_ctrl_amd import run as R


def test_bytes_per_sequence_at_exp3_8ubs_sizes():
    from uav_bs_ctrl_amd.replay import compact_bytes_per_sequence
    n, M, T, H = 8, 50, 50, 256
    assert compact_bytes_per_sequence(n, M, T, H, rd=n) == 48712
    assert compact_bytes_per_sequence(n, M, T, H, rd=1) == 48712 - 4 * T * (n - 1)
    # the full ring's sequence at the same sizes (gt, ubs, agent, d_u2u, h of T+1 steps, no state, act / rew / done of T): DESIGN's 881 KB
    full = (T + 1) * 4 * (n * M * 5 + n * (n - 1) * 3 + 2 * n + n * n + n * H) + T * (8 * n + 4 * n + 4)
    assert 880_000 < full < 882_000 and full / 48712 > 18


def test_the_constructor_refuses_the_host_path_and_a_cpu_device():
    from uav_bs_ctrl_amd.replay import CompactSequenceReplay
    from uav_bs_ctrl_amd.sim import MAPS, BatchedUbsCoverageEnv
    env = BatchedUbsCoverageEnv(MAPS["debug"].params, 2, device="cpu")
    with pytest.raises(ValueError, match="device_state=True only"):
        CompactSequenceReplay(env, 4, 5, 8, device_state=False)
    with pytest.raises(ValueError, match="GPU"):
        CompactSequenceReplay.for_env(env, 4, 5, 8)
    with pytest.raises(ValueError, match="GPU"):
        CompactSequenceReplay(env, 4, 5, 8, seed=1)
    s = env.replay_state()
    assert set(s) == {"pos_ubs", "rate", "avg", "pos_gts"}
    assert s["pos_ubs"] is env.pos_ubs and s["rate"] is env.out["rate_per_gt"] and s["avg"] is env.avg_rate and s["pos_gts"] is env.pos_gts


def test_compact_replay_round_trips_through_config_json():
    ns = R.check_args("exp3", small_args("exp3"))
    assert not hasattr(ns, "compact_replay"), "the flag is the driver's, not an argument of the learner"
    for flag in (False, True):
        ours = R.run_config("exp3", "debug", ns, seed=3, n_envs=4, n_test_envs=2, compact_replay=flag)
        assert ours["compact_replay"] is flag
        text = R.config_text(dict(env_fn="MultiUbsCoverageEnv", env_kwargs={}, seed=3, args=ns, uav_bs_ctrl_amd=ours), "x")
        back = json.loads(text)
        assert back["uav_bs_ctrl_amd"] == json.loads(json.dumps(ours)) and back["uav_bs_ctrl_amd"]["compact_replay"] is flag
        again = R.check_args(back["uav_bs_ctrl_amd"]["exp"], next(iter(back["args"].values())))
        assert vars(again) == vars(ns)
    assert R.run_config("exp3", "debug", ns)["compact_replay"] is False, "the default ring changed"


def test_exp1_refuses_the_flag_on_the_host():
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    ns = R.check_args("exp1", small_args("exp1"))
    with pytest.raises(ValueError, match="compact_replay"):
        R.run_config("exp1", SingleUbsParams(), ns, compact_replay=True)
    assert R.run_config("exp1", SingleUbsParams(), ns)["compact_replay"] is False


def test_the_command_line_flag_parses():
    ap = R._parser()
    a = ap.parse_args(["--out", "d", "--exp", "exp3", "--env", "8ubs", "--args-json", "a.json", "--compact-replay"])
    assert a.compact_replay is True
    assert ap.parse_args(["--out", "d", "--resume"]).compact_replay is False

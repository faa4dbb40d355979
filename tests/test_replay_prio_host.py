"""No GPU: the rules of the prioritised replay on their NumPy restatement (tests/replay_prio_ref.py) - exactness at alpha = 0, the
strata, a dominant slot, the distribution of 32 000 draws - and the host side of the option: ``prioritized`` in ``config.json``, the
command line, the constructors' refusals."""
import json

import numpy as np
import pytest
import torch as th

from tests import replay_prio_ref as P
from tests.run_args import small_args
from uav_bs_ctrl_amd import run as R

CHI2_95_1E6 = 175.4          # the 1 - 1e-6 quantile of chi-square at 95 degrees of freedom (the project's quantile convention)


def test_alpha_zero_gives_unit_priorities_and_unit_weights():
    td = np.random.default_rng(1).standard_normal((7, 5, 3)).astype(np.float32) * 100.0
    q, finite = P.priority(td, 0.0, 0.9, 1e-3)
    assert finite.all() and (q == P.PRIO_ONE).all()
    for beta in (0.0, 0.4, 1.0):
        idx, w32, w64, bit = P.sample(5, 0, q.repeat(4), 17, 8, beta)
        assert bit == 0 and w32.dtype == np.float32 and (w32 == np.float32(1.0)).all() and (w64 == 1.0).all()


def test_alpha_one_is_the_fixed_point_value_itself():
    td = np.full((2, 3, 2), 0.75, dtype=np.float32)
    q, _ = P.priority(td, 1.0, 0.9, 0.25)
    assert (q == P.PRIO_ONE).all()
    assert P.priority(np.zeros((1, 1, 1), np.float32), 1.0, 0.9, 0.0)[0][0] == 1, "the lower clamp"
    assert P.priority(np.full((1, 1, 1), 1e30, np.float32), 1.0, 0.9, 0.0)[0][0] == P.PRIO_TOP, "the upper clamp"


def test_idx_ascends_and_every_target_lies_in_its_stratum():
    q = P.slots96()
    S = int(q.sum())
    for B in (1, 7, 8, 96, 257):
        st = P.strata(S, B)
        assert st[0][0] == 0 and st[-1][1] == S and all(a[1] == b[0] for a, b in zip(st[:-1], st[1:]))
        assert max(hi - lo for lo, hi in st) - min(hi - lo for lo, hi in st) <= 1
        for draws in (0, (1 << 32) - 1):
            tg = P.targets(12345, draws, S, B)
            assert all(lo <= t < hi for (lo, hi), t in zip(st, tg))
            idx, w32, _, bit = P.sample(12345, draws, q, 96, B, 0.4)
            assert bit == 0 and (np.diff(idx) >= 0).all() and idx.min() >= 0 and idx.max() < 96
            assert w32.max() == np.float32(1.0) and (w32 > 0).all()


def test_empty_strata_put_their_target_at_the_lower_end():
    st = P.strata(3, 8)
    assert [lo for lo, _ in st] == [0, 0, 0, 1, 1, 1, 2, 2] and st[-1][1] == 3
    idx, w32, _, bit = P.sample(3, 9, [1, 1, 1, 7, 7], 3, 8, 0.5)
    assert idx.tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and bit == 0 and (w32 == 1.0).all()


def test_a_dominant_slot_takes_the_whole_batch():
    prio = np.full(5, P.PRIO_ONE, dtype=np.uint64)
    prio[2] = P.PRIO_TOP
    idx, w32, _, _ = P.sample(12345, 0, prio, 5, 8, 0.4)
    assert idx.tolist() == [2] * 8 and (w32 == 1.0).all()


def test_an_empty_ring_and_what_lies_beyond_size():
    idx, w32, _, bit = P.sample(1, 0, [P.PRIO_TOP] * 4, 0, 4, 0.4)
    assert bit == 1 and idx.tolist() == [0] * 4 and (w32 == 1.0).all()
    a = P.sample(1, 3, [5, 6, 7, P.PRIO_TOP, P.PRIO_TOP], 3, 8, 0.4)
    b = P.sample(1, 3, [5, 6, 7, 0, 1], 3, 8, 0.4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].max() < 3


def test_draw_frequencies_are_proportional_to_priority():
    q = P.slots96()
    S, B, n_draws = int(q.sum()), 8, 4000
    counts = np.zeros(96, dtype=np.int64)
    inc = np.cumsum(q, dtype=np.uint64)
    for d in range(n_draws):
        tg = P.targets(12345, d, S, B)
        counts += np.bincount(np.searchsorted(inc, np.array(tg, dtype=np.uint64), side="right"), minlength=96)
    expected = n_draws * B * q.astype(np.float64) / S
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print(f"smallest expected count {expected.min():.2f}, chi-square {chi2:.1f} at 95 degrees of freedom")
    assert expected.min() >= 5.0, "the chi-square approximation needs expected counts of at least 5"
    assert chi2 < CHI2_95_1E6                            # stratification only lowers the statistic: no lower bound
    # and the searchsorted shortcut above is the sampler
    idx = P.sample(12345, 17, q, 96, B, 0.4)[0]
    assert np.array_equal(idx, np.searchsorted(inc, np.array(P.targets(12345, 17, S, B), dtype=np.uint64), side="right"))


def test_update_rule_repeats_skips_and_the_maximum():
    td = np.random.default_rng(2).standard_normal((3, 6, 2)).astype(np.float32)
    td[1, 4, 0] = np.nan
    idx = [1, 3, 3, 3, 5, 9]
    q, finite = P.priority(td, 0.6, 0.9, 1e-3)
    assert finite.tolist() == [True, True, True, True, False, True]
    prio, top, bit = P.update(td, idx, 9, 0.6, 0.9, 1e-3, [7] * 9, P.PRIO_ONE)
    assert bit == 2 and prio[1] == q[0] and prio[3] == q[3] and prio[5] == 7 and (prio[[0, 2, 4, 6, 7, 8]] == 7).all()
    assert top == max(P.PRIO_ONE, *(int(q[b]) for b in range(4)))
    assert P.commit([7] * 5, 3, 4, 5, 99).tolist() == [99, 99, 7, 99, 99]


# ---- the option on the host ----------------------------------------------------------------------------------------------------------
def test_the_key_enters_config_json_only_when_set():
    ns = R.check_args("exp3", small_args("exp3"))
    off = R.run_config("exp3", "debug", ns, seed=3, n_envs=4, n_test_envs=2)
    assert "prioritized" not in off, "an absent key means off: existing run directories resume unchanged"
    on = R.run_config("exp3", "debug", ns, seed=3, n_envs=4, n_test_envs=2, prioritized=(0.6, 0.4, 0.9, 1e-3))
    assert on["prioritized"] == [0.6, 0.4, 0.9, 1e-3] and {k: v for k, v in on.items() if k != "prioritized"} == off
    back = json.loads(R.config_text(dict(seed=3, args=ns, uav_bs_ctrl_amd=on)))
    assert back["uav_bs_ctrl_amd"]["prioritized"] == [0.6, 0.4, 0.9, 1e-3]
    with pytest.raises(ValueError, match="prioritized"):
        R.run_config("exp3", "debug", ns, prioritized=(0.6, 0.4, 0.9))
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    exp1 = R.run_config("exp1", SingleUbsParams(), R.check_args("exp1", small_args("exp1")), prioritized=(0.6, 0.4, 0.9, 1e-3),
                        compact_replay=False)
    assert exp1["prioritized"] == [0.6, 0.4, 0.9, 1e-3], "--prioritized works with exp1"


def test_the_command_line_flag_takes_four_numbers():
    ap = R._parser()
    a = ap.parse_args(["--out", "d", "--exp", "exp3", "--env", "debug", "--args-json", "a.json", "--compact-replay",
                       "--prioritized", "0.6", "0.4", "0.9", "1e-3"])
    assert a.prioritized == [0.6, 0.4, 0.9, 1e-3] and a.compact_replay is True
    assert ap.parse_args(["--out", "d", "--resume"]).prioritized is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--out", "d", "--prioritized", "0.6", "0.4"])


def test_a_host_state_ring_refuses_priorities():
    from uav_bs_ctrl_amd.replay import SequenceReplay, SingleUbsSequenceReplay
    pr = (0.6, 0.4, 0.9, 1e-3)
    with pytest.raises(ValueError, match="device_state=True"):
        SequenceReplay(4, 2, 2, 3, 8, device="cpu", prioritized=pr)
    with pytest.raises(ValueError, match="device_state=True"):
        SingleUbsSequenceReplay(4, 2, 3, 8, device="cpu", device_state=False, prioritized=pr)
    with pytest.raises(ValueError, match="four numbers"):
        SingleUbsSequenceReplay(4, 2, 3, 8, device="cpu", device_state=True, prioritized=(0.6, 0.4))
    with pytest.raises(ValueError, match="eta in"):
        SingleUbsSequenceReplay(4, 2, 3, 8, device="cpu", device_state=True, prioritized=(0.6, 0.4, 1.5, 1e-3))
    with pytest.raises(ValueError, match=r"beta in \[0, 16\]"):
        SingleUbsSequenceReplay(4, 2, 3, 8, device="cpu", device_state=True, prioritized=(0.6, 16.5, 0.9, 1e-3))
    rb = SingleUbsSequenceReplay(4, 2, 3, 8, device="cpu")          # the default: no priority tensors, no new attribute in use
    assert rb.prioritized is None and not hasattr(rb, "prio") and not hasattr(rb, "is_weights")
    with pytest.raises(ValueError, match="prioritized"):
        rb.update_priorities(th.zeros(2, dtype=th.int64), th.zeros(2, 2, 1))

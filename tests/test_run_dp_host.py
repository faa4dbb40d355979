"""`-m "not gpu"`: the host arithmetic of a data-parallel ``uav_bs_ctrl_amd.run.Run`` - ``stats.merge_acc``, ``plan(..., world)`` and
``derive_seeds(seed, rank)``.

``merge_acc`` against the accumulator of the concatenation: count, min, max and non-finite count exactly, mean and M2 within 1e-11
relative (a float64 prototype of the same recurrence gave 2.8e-14 at worst over 200 such cases; the bound leaves ~300x over that)."""
import math

import numpy as np
import pytest

from tests import eval_ref as R
from tests.run_args import small_args

REL = 1e-11


def _acc(values):
    """The [1, 6] accumulator of one push of ``values`` (tests/eval_ref.py: the restatement of uavgnn_stats_push)."""
    acc = R.stats_empty(1)
    if len(values):
        R.stats_push(acc, np.asarray(values, dtype=np.float64)[None])
    return acc


def _assert_merge_equals_concatenation(parts):
    from uav_bs_ctrl_amd.stats import merge_acc
    got = np.asarray(merge_acc([_acc(p) for p in parts]), dtype=np.float64)[0]
    want = _acc(np.concatenate(parts))[0]
    assert got[0] == want[0] and got[3] == want[3] and got[4] == want[4] and got[5] == want[5], (got, want)
    if want[0] > 0:
        err_mean = abs(got[1] - want[1]) / abs(want[1])
        err_m2 = abs(got[2] - want[2]) / want[2] if want[2] > 0 else abs(got[2])
        assert err_mean <= REL and err_m2 <= REL, (err_mean, err_m2)
        return err_mean, err_m2
    assert got[1] == 0.0 and got[2] == 0.0
    return 0.0, 0.0


def test_merge_acc_equals_the_accumulator_of_the_concatenation():
    rs = np.random.RandomState(11)
    worst = [0.0, 0.0]
    for case in range(200):
        parts = [rs.uniform(-100, 100) + rs.uniform(0.1, 50) * rs.standard_normal(rs.randint(0, 401)) for _ in range(rs.randint(2, 9))]
        if case % 10 == 0:
            parts[len(parts) // 2] = np.zeros(0)                       # an empty part in the middle
        if case % 25 == 0:                                             # non-finite values count and stay out of the moments
            parts[0] = np.concatenate([parts[0], [np.nan, np.inf]])
            parts[-1] = np.concatenate([[-np.inf], parts[-1]])
        errs = _assert_merge_equals_concatenation(parts)
        worst = [max(w, e) for w, e in zip(worst, errs)]
    print(f"merge_acc: worst relative error of the mean {worst[0]:.3e}, of M2 {worst[1]:.3e} (bound {REL:g})")


def test_merge_acc_empty_parts_are_the_identity():
    from uav_bs_ctrl_amd.stats import EMPTY, merge_acc
    empty = R.stats_empty(2)
    assert merge_acc([empty, empty, empty]) == [list(EMPTY), list(EMPTY)], "all-empty parts"
    rs = np.random.RandomState(3)
    acc = R.stats_empty(2)
    R.stats_push(acc, rs.standard_normal((2, 37)) * 7 + 3)
    for parts in ([acc], [empty, acc], [acc, empty], [empty, acc, empty, empty]):
        assert np.array_equal(np.asarray(merge_acc(parts)), acc), "bit for bit"
    other = R.stats_empty(2)
    R.stats_push(other, rs.standard_normal((2, 5)))
    assert merge_acc([acc, empty, other]) == merge_acc([acc, other]), "an empty part in the middle"
    only_bad = R.stats_empty(2)
    R.stats_push(only_bad, np.full((2, 3), np.nan))
    got = np.asarray(merge_acc([only_bad, acc]))
    assert np.array_equal(got[:, :5], acc[:, :5]) and got[:, 5].tolist() == [3.0, 3.0]
    with pytest.raises(ValueError):
        merge_acc([])
    with pytest.raises(ValueError):
        merge_acc([R.stats_empty(2), R.stats_empty(3)])


def test_merge_acc_takes_tensors_and_list_order():
    import torch as th
    from uav_bs_ctrl_amd.stats import merge_acc
    a, b = _acc([1.0, 2.0, 3.0]), _acc([10.0, 20.0])
    got = merge_acc([th.as_tensor(a), th.as_tensor(b)])
    assert got == merge_acc([a, b]) == merge_acc([a.tolist(), b.tolist()])
    assert got[0][0] == 5.0 and got[0][3] == 1.0 and got[0][4] == 20.0 and math.isclose(got[0][1], 7.2, rel_tol=1e-15)
    assert math.isclose(got[0][2], sum((v - 7.2) ** 2 for v in (1, 2, 3, 10, 20)), rel_tol=1e-14)


def test_summary_without_a_group_is_the_local_accumulator():
    from uav_bs_ctrl_amd.stats import EpochStats
    st = EpochStats(["a"], "cpu")
    st.acc.copy_(st.acc.new_tensor(_acc([1.0, 2.0, 6.0])))
    row = st.summary()
    assert row == st.summary(None) and row["Na"] == 3 and row["Averagea"] == 3.0 and row["Maxa"] == 6.0


# ---- plan -------------------------------------------------------------------------------------------------------------------------------
def test_plan_counts_all_ranks():
    from uav_bs_ctrl_amd.run import Plan, plan
    args = small_args("exp3")
    one = plan(args, 4, 10, 10)
    assert one == plan(args, 4, 10, 10, world=1) == plan(args, 4, 10, 10, 1)
    assert one == Plan(total_steps=240, update_after_eff=40, update_every=10, steps_per_episode=40, episodes_per_epoch=2,
                       interacts_per_epoch=80, epochs=3), "today's tuple"
    two = plan(args, 4, 10, 10, world=2)
    assert two.steps_per_episode == 2 * one.steps_per_episode == 80
    assert two.update_after_eff == max(args["update_after"], 2 * args["batch_size"] * 10) == 80
    assert two.episodes_per_epoch == 1 and two.interacts_per_epoch == 80 and two.total_steps == one.total_steps
    assert plan(small_args("exp3", update_after=500), 4, 10, 10, world=2).update_after_eff == 500
    assert two.collect_only(79) and not two.collect_only(80)
    with pytest.raises(ValueError):
        plan(args, 4, 10, 10, world=0)


# ---- seeds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 3, 12345])
def test_derive_seeds_by_rank(seed):
    from uav_bs_ctrl_amd.run import derive_seeds
    base = 1000003 * seed
    today = dict(torch=seed, train_env=base + 1, test_env=base + 2, replay=base + 3, explore=base + 4, evaluation=base + 5, comm=base + 16)
    zero = derive_seeds(seed)
    assert zero == derive_seeds(seed, 0) == today and list(zero) == list(today)
    one = derive_seeds(seed, 1)
    shifted = ("train_env", "replay", "explore", "comm")
    assert one["torch"] == zero["torch"]
    assert all(one[k] == zero[k] + 4096 for k in shifted)
    assert all(one[k] == zero[k] for k in one if k not in shifted)
    both = [zero[k] for k in shifted] + [one[k] for k in shifted]
    assert len(set(both)) == 8, "the shifted seeds of rank 1 are distinct from rank 0's and from each other"
    assert derive_seeds(seed, 3)["replay"] == zero["replay"] + 3 * 4096


def test_state_file_names():
    from uav_bs_ctrl_amd.run import state_file
    assert [state_file(r) for r in range(3)] == ["state.pt", "state.rank1.pt", "state.rank2.pt"]

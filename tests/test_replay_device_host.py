"""The device-resident replay state on the CPU: the sampler and the exploration schedule are checked here through their NumPy
restatement (tests/replay_sampler_ref.py, written from the header of csrc/replay.hip); tests/test_replay_device_gpu.py checks the
kernels bit for bit against that restatement.

  * the restatement's batches are distinct, in range and ascending, and depend on (seed, draws, size, B) as the rule says;
  * per-slot inclusion counts and pair co-inclusion counts of 20 000 draws at size 40, B = 8 against the counts of the reference's own
    ``ReplayBuffer.sample`` (tests/golden/replay_sample_stats.npz): two-sample chi-square below the quantile at 1 - 1e-6, the rule of
    tests/test_maps_registry.py - after the reference's own two halves were shown to pass that rule against each other;
  * the schedule against run.py:61's recorded values;
  * the new entries are in the signature table, and ``device_state=True`` on a CPU device raises."""
import numpy as np
import pytest

from tests import replay_sampler_ref as R
from tests.test_maps_registry import chi2_quantile, chi2_two_sample
from tests.util import GOLDEN

SEED = 77


def _stats():
    return np.load(f"{GOLDEN}/replay_sample_stats.npz")


@pytest.mark.parametrize("size,B", [(8, 8), (9, 8), (40, 8), (5000, 32)])
def test_restated_batches_are_distinct_in_range_and_ascending(size, B):
    got = R.sample_many(SEED, list(range(6)), size, B)
    assert got.shape == (6, B) and got.dtype == np.int64
    assert (got >= 0).all() and (got < size).all()
    assert (np.diff(got, axis=1) > 0).all(), "not strictly ascending: a repeat or a wrong order"
    if size > B:
        assert len({tuple(r) for r in got}) > 1, "the draw counter does not enter the keys"
        assert not np.array_equal(got, R.sample_many(SEED + 1, list(range(6)), size, B)), "the seed does not enter the keys"
    else:
        assert np.array_equal(got, np.broadcast_to(np.arange(size), got.shape))
    # the rule, once more in its plainest form: sort all (key, slot) pairs of one draw
    k = R.keys(SEED, [3], size)[0]
    pairs = sorted((int(k[s]), s) for s in range(size))[:B]
    assert np.array_equal(got[3], sorted(s for _, s in pairs))


def test_a_batch_larger_than_the_ring_wraps():
    assert np.array_equal(R.sample(SEED, 0, 3, 8), [0, 1, 2, 0, 1, 2, 0, 1])
    assert np.array_equal(R.sample(SEED, 0, 0, 4), [0, 0, 0, 0])


def test_the_references_own_halves_pass_the_rule_against_each_other():
    z = _stats()
    for name in ("incl", "pair"):
        stat, df = chi2_two_sample(z[name + "_a"], z[name + "_b"])
        print(f"reference halves: {name}: chi2 = {stat:.2f}, bound {chi2_quantile(df):.2f} (df {df})")
        assert stat < chi2_quantile(df), name


def test_inclusion_and_co_inclusion_counts_against_the_references_sampler():
    """Measured chi-square statistic / bound (degrees of freedom) at the committed seeds: incl 33.40 / 96.62 (39),
    pair 731.41 / 981.31 (779); the reference's own halves against each other: incl 33.87, pair 756.17.  The pair counts are what
    catches a sampler that prefers some subsets (next test)."""
    z = _stats()
    size, B, N = int(z["size"]), int(z["batch"]), int(z["n_draws"])
    assert (size, B, N) == (40, 8, 20000)
    incl, pair = R.inclusion_counts(R.sample_many(SEED, list(range(N)), size, B), size)
    bad = []
    for name, got in (("incl", incl), ("pair", pair)):
        ref = z[name + "_a"] + z[name + "_b"]
        stat, df = chi2_two_sample(ref, got)
        bound = chi2_quantile(df)
        print(f"{name}: chi2 = {stat:.2f}, bound {bound:.2f} (df {df})")
        if not stat < bound:
            bad.append((name, stat, bound, df))
    assert not bad, bad


def test_a_sampler_that_prefers_neighbouring_slots_is_caught():
    """The pair counts have the power the test relies on: contiguous windows have uniform inclusion counts and fail on the pairs."""
    z = _stats()
    size, B, N = int(z["size"]), int(z["batch"]), int(z["n_draws"])
    start = np.random.RandomState(0).randint(0, size, N)
    windows = (start[:, None] + np.arange(B)[None]) % size
    incl, pair = R.inclusion_counts(windows, size)
    stat, df = chi2_two_sample(z["pair_a"] + z["pair_b"], pair)
    assert stat > chi2_quantile(df)


def test_eps_schedule_against_the_references_values():
    z = _stats()
    s, e = float(z["eps_start"]), float(z["eps_end"])
    assert (s, e) == (1.0, 0.05)
    for decay, t, val in zip(z["eps_decay"], z["eps_t"], z["eps_val"]):
        assert list(t) == [0, 1, decay // 2, decay - 1, decay, decay + 10, 3 * 10 ** 6]
        got = R.eps_schedule64(t, s, e, int(decay))
        assert np.array_equal(got, val), (decay, got, val)
        assert R.eps_schedule(t, s, e, int(decay)).dtype == np.float32
        assert got[0] == 1.0 and (got[4:] >= e).all() and got[-1] == e


def test_signatures_and_the_cpu_guard():
    import torch as th

    from uav_bs_ctrl_amd import _lib
    from uav_bs_ctrl_amd.replay import SequenceReplay, SingleUbsSequenceReplay
    for name in ("uavgnn_replay_commit", "uavgnn_replay_sample", "uavgnn_replay_gather", "uavgnn_eps_schedule"):
        assert name in _lib.SIGNATURES, name
    with pytest.raises(ValueError, match="device_state"):
        SequenceReplay(4, 2, 2, 3, 8, n_envs=2, device="cpu", device_state=True)
    with pytest.raises(ValueError, match="device_state"):
        SingleUbsSequenceReplay(4, 2, 3, 8, n_envs=2, device="cpu", device_state=True)
    # the default stays the host path: Python counters, torch.randperm
    rb = SingleUbsSequenceReplay(4, 1, 3, 8, n_envs=2, device="cpu")
    assert rb.device_state is False and (rb.head, rb.size, rb.ptr) == (0, 0, 0)
    rb.push(dict(gt=th.ones(2, 3, 4), agent=th.ones(2, 2), h=th.ones(2, 8), act=th.ones(2, 1), rew=th.ones(2, 1), done=th.zeros(2, 1),
                 next_gt=th.ones(2, 3, 4), next_agent=th.ones(2, 2), next_h=th.ones(2, 8)))
    assert (rb.head, rb.size, len(rb)) == (2, 2, 2)
    g = th.Generator().manual_seed(3)
    assert sorted(rb.sample_indices(2, g).tolist()) == [0, 1]
    with pytest.raises(ValueError, match="gather_into"):
        rb.gather_into(th.zeros(1, dtype=th.int64), None)

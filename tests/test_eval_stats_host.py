"""Evaluation draws and epoch statistics on the CPU, through their NumPy restatement (tests/eval_ref.py, written from include/uavgnn.h);
tests/test_eval_device_gpu.py checks the kernels against that restatement.

  * Philox4x32-10 against the Random123 known answer;
  * the restated draws over 20 000 steps at eps = 0.05, A = 5, 3 teams of 3 agents: exploration frequency, action histogram and the
    independence of a step's team draw from its agent draws, each a chi-square test below the quantile at 1 - 1e-6 (the rule of
    tests/test_maps_registry.py);
  * the restated merge over pushes of sizes 1, 2, 63, 64, 65, 257, 4099, 1, 3 against a two-pass evaluation in np.longdouble, against the
    logger's float32 formula, and with the values shifted by 1e6;
  * non-finite values; the argument errors of the two entries (no GPU needed) and their rows in the signature table."""
import numpy as np
import pytest

from tests import eval_ref as R
from tests.map_sampler_ref import philox4x32_10
from tests.test_maps_registry import chi2_quantile

SEED = 2 ** 40 + 12345
SIZES = (1, 2, 63, 64, 65, 257, 4099, 1, 3)


def test_philox_known_answer():
    out = philox4x32_10(np.uint64(0), np.uint64(0), np.uint64(0), np.uint64(0), 0, 0)
    assert [int(w) for w in out] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def _chi2_one_sample(obs, expected):
    obs, expected = np.asarray(obs, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    assert abs(obs.sum() - expected.sum()) < 1e-6 * obs.sum()
    return float(((obs - expected) ** 2 / expected).sum()), obs.size - 1


def _chi2_independence(table):
    table = np.asarray(table, dtype=np.float64)
    exp = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / table.sum()
    return float(((table - exp) ** 2 / exp).sum()), (table.shape[0] - 1) * (table.shape[1] - 1)


@pytest.fixture(scope="module")
def drawn():
    steps, A, teams, n = 20000, 5, 3, 3
    st = np.arange(steps)[:, None]
    u_team = R.uniforms(SEED, st, np.arange(teams)[None], 0)                  # [steps, 3]
    u_agent = R.uniforms(SEED, st, np.arange(teams * n)[None], 1)             # [steps, 9]
    assert u_team.dtype == np.float32 and (u_team >= 0).all() and (u_team < 1).all() and (u_agent < 1).all()
    act = np.minimum((u_agent * np.float32(A)).astype(np.int64), A - 1)
    return u_team, u_agent, act, A


def test_exploration_frequency_and_action_histogram(drawn):
    u_team, _, act, A = drawn
    eps = np.float32(0.05)
    n_exp = int((u_team <= eps).sum())
    stat, df = _chi2_one_sample([n_exp, u_team.size - n_exp], [u_team.size * 0.05, u_team.size * 0.95])
    print(f"explore: {n_exp} of {u_team.size}: chi2 = {stat:.2f}, bound {chi2_quantile(df):.2f}")
    assert stat < chi2_quantile(df)
    hist = np.bincount(act.ravel(), minlength=A)
    stat, df = _chi2_one_sample(hist, np.full(A, act.size / A))
    print(f"actions: {hist}: chi2 = {stat:.2f}, bound {chi2_quantile(df):.2f}")
    assert stat < chi2_quantile(df)


def test_team_and_agent_draws_of_a_step_are_uncorrelated(drawn):
    """Row t and team t share the counter's index word and differ in the lane word only: the pairing a keying mistake would couple.  Also
    team t against the first row of its own team."""
    u_team, _, act, A = drawn
    tb = np.minimum((u_team * np.float32(4)).astype(np.int64), 3)            # the team draw in four bins
    for name, rows in (("same index", [0, 1, 2]), ("own team", [0, 3, 6])):
        table = np.zeros((4, A))
        np.add.at(table, (tb.ravel(), act[:, rows].ravel()), 1)
        stat, df = _chi2_independence(table)
        print(f"{name}: chi2 = {stat:.2f}, bound {chi2_quantile(df):.2f} (df {df})")
        assert stat < chi2_quantile(df), name
    # and the exploration event itself (5 % of the steps) against the actions
    table = np.zeros((2, A))
    np.add.at(table, ((u_team <= np.float32(0.05)).astype(np.int64).ravel(), act[:, [0, 1, 2]].ravel()), 1)
    stat, df = _chi2_independence(table)
    assert stat < chi2_quantile(df)


def test_selection_rule():
    q = np.array([[0.0, 2.0, 2.0, 1.0, -1.0, 9.0], [3.0, 3.0, 3.0, 3.0, 3.0, 9.0], [-1.0, -2.0, -0.5, -0.5, -3.0, 9.0]], dtype=np.float32)
    assert R.eps_greedy_philox(q, 5, 3, SEED, 0, 0.0).tolist() == [1, 0, 2], "first maximum; the padding column is not read"
    a1 = R.eps_greedy_philox(q, 5, 3, SEED, 0, 1.0)
    _, u_agent = R.draws(SEED, 0, 3, 3)
    assert a1.tolist() == np.minimum((u_agent * np.float32(5)).astype(np.int64), 4).tolist()
    assert not np.array_equal(R.draws(SEED, 0, 3, 3)[1], R.draws(SEED, 1, 3, 3)[1]), "the step does not enter the counter"
    assert not np.array_equal(R.draws(SEED, 0, 3, 3)[1], R.draws(SEED + 2 ** 32, 0, 3, 3)[1]), "the seed's high word does not enter the key"
    assert R.eps_greedy_philox(np.zeros((0, 5)), 5, 3, SEED, 0, 0.5).shape == (0,)


def _pushes(shift=0.0):
    rs = np.random.RandomState(5)
    return [rs.standard_normal(n) + shift for n in SIZES]


def _merged(chunks):
    acc = R.stats_empty(1)
    for c in chunks:
        R.stats_push(acc, c[None])
    return acc[0]


def test_merge_against_two_pass_longdouble():
    chunks = _pushes()
    allv = np.concatenate(chunks)
    assert allv.size == sum(SIZES) == 4555
    acc = _merged(chunks)
    mean, m2 = R.two_pass(allv)
    # the bound was set as 4 n 2^-53 with n quoted as 4455; the sizes add up to 4555 - the smaller n is kept in the bound
    tol_mean, tol_m2 = (t * 4455 / 4555 for t in R.moment_tolerances(allv))
    print(f"mean err {abs(acc[1] - mean):.3e} (tol {tol_mean:.3e}), M2 err {abs(acc[2] - m2):.3e} (tol {tol_m2:.3e})")
    assert acc[0] == 4555 and acc[5] == 0 and acc[3] == allv.min() and acc[4] == allv.max()
    assert abs(acc[1] - mean) <= tol_mean and abs(acc[2] - m2) <= tol_m2
    lm, ls = R.logger_mean_std(allv)
    assert abs(acc[1] - lm) <= 1e-5 and abs(np.sqrt(acc[2] / acc[0]) - ls) <= 1e-5


def test_merge_of_shifted_values():
    chunks = _pushes(1e6)
    allv = np.concatenate(chunks)
    acc = _merged(chunks)
    _, m2 = R.two_pass(allv)
    rel = abs(acc[2] - m2) / m2
    print(f"shifted: M2 relative error {float(rel):.3e}")
    assert rel <= 1e-9
    # the shortcut a kernel must not take: sum of squares minus n mean^2
    short = (allv ** 2).sum() - allv.size * allv.mean() ** 2
    assert abs(short - m2) / m2 > 1e-9


def test_non_finite_values_are_counted_and_left_out():
    acc = R.stats_empty(2)
    R.stats_push(acc, np.array([[1.0, np.nan, 3.0, np.inf], [-np.inf, 2.0, 2.0, 2.0]]))
    assert acc[0].tolist() == [2.0, 2.0, 2.0, 1.0, 3.0, 2.0] and acc[1].tolist() == [3.0, 2.0, 0.0, 2.0, 2.0, 1.0]
    before = acc.copy()
    R.stats_push(acc, np.full((2, 3), np.nan))
    assert np.array_equal(acc[:, :5], before[:, :5]) and acc[:, 5].tolist() == [5.0, 4.0]
    empty = R.stats_empty(1)
    R.stats_push(empty, np.array([[np.inf, np.nan]]))
    assert empty[0, :5].tolist() == [0.0, 0.0, 0.0, np.inf, -np.inf] and empty[0, 5] == 2


def test_signatures_and_argument_errors_without_a_gpu():
    from uav_bs_ctrl_amd import _lib
    for name in ("uavgnn_eps_greedy_philox", "uavgnn_stats_push"):
        assert name in _lib.SIGNATURES, name
    lib = _lib.lib()
    assert lib.uavgnn_stats_push(None, 4, 4, 1, None, None) == -1000
    assert lib.uavgnn_eps_greedy_philox(None, 5, 4, 5, 1, None, None, 0.05, None, None) == -1000
    # argument errors that are decided before any pointer is read
    assert lib.uavgnn_stats_push(8, 4, -1, 1, 8, None) == -1000
    assert lib.uavgnn_stats_push(8, 4, 4, 0, 8, None) == -1000 and lib.uavgnn_stats_push(8, 4, 4, 17, 8, None) == -1000
    assert lib.uavgnn_stats_push(8, 3, 4, 1, 8, None) == -1000
    assert lib.uavgnn_eps_greedy_philox(8, 4, 4, 5, 1, 8, None, 0.05, 8, None) == -1000      # ld_q < A
    assert lib.uavgnn_eps_greedy_philox(8, 5, 4, 5, 0, 8, None, 0.05, 8, None) == -1000      # n_agents < 1


def test_epoch_stats_argument_errors_need_no_launch():
    from uav_bs_ctrl_amd.stats import EpochStats
    with pytest.raises(ValueError, match="distinct"):
        EpochStats(["a", "a"], "cpu")
    st = EpochStats(["a", "b"], "cpu")
    import torch as th
    with pytest.raises(ValueError, match="unknown"):
        st.push(c=th.zeros(2))
    with pytest.raises(ValueError, match="equal"):
        st.push(a=th.zeros(2), b=th.zeros(3))
    row = st.summary()
    assert row["Na"] == 0 and np.isnan(row["Averagea"]) and row["Mina"] == np.inf and row["Maxa"] == -np.inf

"""`-m gpu`: uavgnn_replay_rebuild_obs (csrc/replay_rebuild.hip) alone, through the C ABI - the padded observations, d_u2u and the global
state of sampled sequences rebuilt from pos_ubs / rate / avg / pos_gts, bit for bit what uavgnn_env_step wrote when it simulated them.

Per case: a ``BatchedUbsCoverageEnv`` of 5 environments is reset and stepped 6 times; ``replay_state()`` and ``observations()`` are recorded
after the reset and after every step, environment e's 7 steps become sequence e of a hand-filled ring of capacity 7 (slots 5 and 6 stay
NaN), and the rebuild runs with an idx that repeats a slot, is out of order and holds one index beyond the 5 sequences (clamped to the
last).  Destinations are filled with NaN first.  Every comparison is ``torch.equal``: the rebuilt data is DEFINED as what the simulator
wrote, no tolerance is involved."""
import math

import pytest
import torch as th

pytestmark = pytest.mark.gpu

E, STEPS, CAP = 5, 6, 7
IDX = (3, 0, 3, 4, 9, 1)                # a repeat, out of order, 9 >= 5 sequences: clamped to 4


def _params(**kw):
    from uav_bs_ctrl_amd.sim import MapParams
    return MapParams(**kw)


def _record(env, actions=None, seed=0):
    """Steps ``env`` (already reset) STEPS times; returns (ring fields with sequence e = environment e, recorded observations
    [STEPS+1, E, ...])."""
    gen = th.Generator(device="cuda").manual_seed(seed)
    n, M = env.n_agents, env.n_gts
    ring = dict(pos_ubs=th.full((CAP, STEPS + 1, n, 2), float("nan"), dtype=th.float64, device="cuda"),
                rate=th.full((CAP, STEPS + 1, M), float("nan"), device="cuda"), avg=th.full((CAP, STEPS + 1, M), float("nan"), device="cuda"),
                pos_gts=th.full((CAP, M, 2), float("nan"), device="cuda"))
    rec = {k: [] for k in ("gt", "ubs", "agent", "d_u2u", "state")}
    for t in range(STEPS + 1):
        if t > 0:
            a = th.randint(env.n_actions, (E, n), device="cuda", generator=gen) if actions is None else actions(t - 1)
            env.step(a)
        s = env.replay_state()
        for k in ("pos_ubs", "rate", "avg"):
            assert s[k].data_ptr() == dict(pos_ubs=env.pos_ubs, rate=env.out["rate_per_gt"], avg=env.avg_rate)[k].data_ptr(), "not a view"
            ring[k][:E, t] = s[k]
        if t == 0:
            ring["pos_gts"][:E] = s["pos_gts"]
        for k, v in env.observations().items():
            rec[k].append(v.clone())
    return ring, {k: th.stack(v) for k, v in rec.items()}


def _rebuild(env, ring, Sg=None, with_duu=True, with_state=True, n_seq=E, idx=IDX):
    """(return code, rebuilt buffers) of one uavgnn_replay_rebuild_obs call into NaN-filled destinations."""
    from uav_bs_ctrl_amd import _lib as L
    n, M, B, T1 = env.n_agents, env.n_gts, len(idx), STEPS + 1
    Sg = env.out["obs_gt"].shape[-1] if Sg is None else Sg
    nan = lambda *shape: th.full(shape, float("nan"), device="cuda")  # noqa: E731
    out = dict(gt=nan(T1, B, n, M, Sg), ubs=nan(T1, B, n, max(n - 1, 0), 3), agent=nan(T1, B, n, 2),
               d_u2u=nan(T1, B, n, n) if with_duu else None, state=nan(T1, B, env.state_dim) if with_state else None)
    ix = th.tensor(idx, dtype=th.int64, device="cuda")
    code = L.lib().uavgnn_replay_rebuild_obs(env._ic, env._fc, ring["pos_ubs"].data_ptr(), ring["rate"].data_ptr(), ring["avg"].data_ptr(),
                                             ring["pos_gts"].data_ptr(), n_seq, T1, ix.data_ptr(), B, out["gt"].data_ptr(), Sg,
                                             L.ptr(out["ubs"]) or None, out["agent"].data_ptr(), L.ptr(out["d_u2u"]), L.ptr(out["state"]),
                                             L.stream())
    th.cuda.synchronize()
    return code, out


def _compare(env, ring, rec, **kw):
    code, got = _rebuild(env, ring, **kw)
    assert code == 0, code
    rows = th.tensor([min(i, E - 1) for i in IDX], device="cuda")
    for k, v in got.items():
        if v is None:
            continue
        want = rec[k].index_select(1, rows)
        assert v.shape == want.shape, (k, v.shape, want.shape)
        assert not th.isnan(v).any(), f"{k}: an element of the destination was not written"
        assert th.equal(v, want), f"{k}: {int((v != want).sum())} of {v.numel()} elements differ from what the simulator wrote"
    return got


def _uniform_env(p, seed, pos_ubs=None):
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    env = BatchedUbsCoverageEnv(p, E)
    gen = th.Generator(device="cuda").manual_seed(seed)
    env.reset(pos_ubs=pos_ubs, generator=gen)
    return env


def _both(x):
    return bool((x == 0).any()) and bool((x == 1).any())


def test_debug_map_both_sensing_outcomes():
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    env = BatchedUbsCoverageEnv.from_map("debug", E, seed=5)              # n = 3, M = 4, r_sns = 300 on a 1000 m square
    env.reset_from_map()
    ring, rec = _record(env, seed=1)
    assert _both(rec["gt"][..., 0]), "the case is vacuous: every GT is seen, or none"
    _compare(env, ring, rec)


def test_finite_comm_range_both_outcomes_in_obs_ubs():
    # 'r400' shrunk to n = 4, M = 10: r_comm = 400 on a 2000 m square; UBS 1 starts 112 m from UBS 0, the others wherever they fall
    p = _params(n_ubs=4, n_gts=10, n_rbs=1, range_pos=2000.0, episode_limit=40, dt=20.0, r_sns=200.0, r_comm=400.0, vels=(5.0, 10.0),
                reward_scale_rate=10.0)
    gen = th.Generator(device="cuda").manual_seed(8)
    pos = th.rand(E, 4, 2, device="cuda", generator=gen, dtype=th.float64) * 2000.0
    pos[:, 1] = (pos[:, 0] + th.tensor([100.0, 50.0], dtype=th.float64, device="cuda")).clamp(0.0, 2000.0)
    pos[:, 3] = (pos[:, 0] + 1000.0) % 2000.0                             # at least 1000 m from UBS 0 on both axes
    env = _uniform_env(p, 9, pos_ubs=pos)
    ring, rec = _record(env, seed=2)
    assert _both(rec["ubs"][..., 0]), "the case is vacuous: every UBS pair is in range, or none"
    _compare(env, ring, rec)


def test_one_ubs_one_gt_zero_row_ubs_buffer():
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    env = BatchedUbsCoverageEnv.from_map("test", E, seed=6)               # n = 1, M = 1
    env.reset_from_map()
    ring, rec = _record(env, seed=3)
    got = _compare(env, ring, rec)
    assert got["ubs"].numel() == 0


@pytest.mark.parametrize("n,M,R", [(8, 80, 5), (3, 7, 2), (16, 70, 4)], ids=["8x80-lane-loop", "3x7-odd-M", "16x70"])
def test_shapes(n, M, R):
    p = _params(n_ubs=n, n_gts=M, n_rbs=R, range_pos=1500.0, episode_limit=30, r_sns=500.0, r_comm=700.0, vels=(5.0, 10.0))
    env = _uniform_env(p, 10 + n)
    ring, rec = _record(env, seed=4)
    assert _both(rec["gt"][..., 0]), "the case is vacuous: every GT is seen, or none"
    _compare(env, ring, rec)


def test_without_fair_service_and_a_destination_of_the_wrong_width():
    from uav_bs_ctrl_amd import _lib as L
    p = _params(n_ubs=3, n_gts=6, n_rbs=2, range_pos=800.0, r_sns=400.0, fair_service=False)
    env = _uniform_env(p, 21)
    assert env.out["obs_gt"].shape[-1] == 4 and env.state_dim == 2 * 3 + 6 * 3
    ring, rec = _record(env, seed=5)
    _compare(env, ring, rec)
    code, got = _rebuild(env, ring, Sg=5)
    assert code == L.UAVGNN_EINVAL and bool(th.isnan(got["gt"]).all()), "the refused call launched"
    p5 = _params(n_ubs=3, n_gts=6, n_rbs=2, range_pos=800.0, r_sns=400.0)
    env5 = _uniform_env(p5, 21)
    assert _rebuild(env5, ring, Sg=4)[0] == L.UAVGNN_EINVAL


def test_null_d_u2u_and_state():
    p = _params(n_ubs=4, n_gts=8, n_rbs=2, range_pos=900.0, r_sns=350.0, r_comm=500.0)
    env = _uniform_env(p, 22)
    ring, rec = _record(env, seed=6)
    got = _compare(env, ring, rec, with_duu=False, with_state=False)
    assert got["d_u2u"] is None and got["state"] is None


def test_two_ubs_clipped_into_one_corner():
    # vels = (10,), dt = 10: actions 3 / 4 move 100 m towards x = 0 / y = 0; UBSs 0 and 1 start inside (100, 100) and reach (0, 0) both
    p = _params(n_ubs=3, n_gts=5, n_rbs=2, range_pos=600.0, r_sns=300.0, r_comm=250.0)
    gen = th.Generator(device="cuda").manual_seed(12)
    pos = th.rand(E, 3, 2, device="cuda", generator=gen, dtype=th.float64) * 600.0
    pos[:, 0] = th.tensor([55.0, 35.0], dtype=th.float64, device="cuda")
    pos[:, 1] = th.tensor([80.0, 30.0], dtype=th.float64, device="cuda")
    env = _uniform_env(p, 23, pos_ubs=pos)
    assert math.isclose(float(env.moves[3, 0]), -100.0, abs_tol=1e-9) and math.isclose(float(env.moves[4, 1]), -100.0, abs_tol=1e-9)

    def actions(t):
        a = th.randint(env.n_actions, (E, 3), device="cuda", generator=gen)
        a[:, :2] = 3 if t % 2 == 0 else 4
        return a
    ring, rec = _record(env, actions=actions)
    assert bool((rec["d_u2u"][2:, :, 0, 1] == 0).all()), "the two UBSs did not meet in the corner"
    assert bool((ring["pos_ubs"][:E, 2:, 0] == ring["pos_ubs"][:E, 2:, 1]).all())
    _compare(env, ring, rec)


def test_bounds_and_null_arguments_are_codes():
    from uav_bs_ctrl_amd import _lib as L
    p = _params(n_ubs=3, n_gts=5, n_rbs=2)
    env = _uniform_env(p, 24)
    ring, _ = _record(env, seed=7)
    ic17 = type(env._ic)(*env._ic)
    ic17[0] = 17
    saved, env._ic = env._ic, ic17
    code, got = _rebuild(env, ring)
    env._ic = saved
    assert code == L.UAVGNN_EUNSUPPORTED and bool(th.isnan(got["gt"]).all())
    x = ring["rate"].data_ptr()
    ix = th.zeros(2, dtype=th.int64, device="cuda")
    call = lambda *a: L.lib().uavgnn_replay_rebuild_obs(*a, L.stream())  # noqa: E731
    assert call(None, env._fc, x, x, x, x, 5, 7, ix.data_ptr(), 2, x, 5, x, x, None, None) == L.UAVGNN_EINVAL
    assert call(env._ic, env._fc, None, x, x, x, 5, 7, ix.data_ptr(), 2, x, 5, x, x, None, None) == L.UAVGNN_EINVAL
    assert call(env._ic, env._fc, x, x, x, x, 5, 7, None, 2, x, 5, x, x, None, None) == L.UAVGNN_EINVAL
    assert call(env._ic, env._fc, x, x, x, x, 5, 7, ix.data_ptr(), 2, None, 5, x, x, None, None) == L.UAVGNN_EINVAL
    assert call(env._ic, env._fc, x, x, x, x, 5, 7, ix.data_ptr(), 2, x, 5, None, x, None, None) == L.UAVGNN_EINVAL     # n > 1 needs obs_ubs
    assert call(env._ic, env._fc, x, x, x, x, 0, 7, ix.data_ptr(), 2, x, 5, x, x, None, None) == L.UAVGNN_EINVAL

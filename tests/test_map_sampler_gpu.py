"""The reset-time placement sampler on the device (csrc/map_sample.hip, BatchedUbsCoverageEnv.from_map / sample_positions /
reset_from_map) against its NumPy restatement (tests/map_sampler_ref.py) - BIT-EXACT: positions and permutations are integer
work and exact double arithmetic - and through the simulator: reset, counter, graph capture.  What the sampled distribution is
worth against the reference's own draws is checked on the restatement (tests/test_maps_registry.py)."""
import ctypes

import numpy as np
import pytest
import torch as th

from tests import map_sampler_ref as R
from tests.test_maps_registry import check_structure

pytestmark = pytest.mark.gpu
SEED = 0x1234ABCD5678


def _spec(name):
    from uav_bs_ctrl_amd import sim
    return sim.dense_hotspot_v2() if name == "dense_hotspot_v2" else sim.MAPS[name]


def _env(name, B, seed=SEED, resets=0):
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    env = BatchedUbsCoverageEnv.from_map(_spec(name), B, seed=seed)
    env.map_rng[1] = resets
    return env


def _ref(name, B, resets, seed=SEED):
    spec = _spec(name)
    ic, fc = spec.sampler_consts()
    return R.sample(ic, fc, B, seed, resets, spec.fixed_ubs, spec.fixed_gts)


def _same(got, ref, what):
    for g, r, k in zip(got, ref, ("pos_ubs", "pos_gts", "prior")):
        g = g.cpu().numpy()
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, g.shape)
        assert np.array_equal(g, r), f"{what}: {k} differs in {int((g != r).sum())} of {r.size} entries"


@pytest.mark.parametrize("resets", [0, 1, 2 ** 32 + 3])
@pytest.mark.parametrize("name", ["test", "debug", "inf", "8ubs", "dense_hotspot_v2"])
def test_bit_exact_against_the_restatement(name, resets):
    env = _env(name, 5, resets=resets)                       # 5: not a multiple of the wavefronts per workgroup
    _same(env.sample_positions(), _ref(name, 5, resets), f"{name} @ {resets}")
    assert env.map_rng.tolist() == [SEED, resets + 1]


def test_sparse_table_with_many_picks_from_a_small_lattice():
    """16 UBSs and 40 GTs from 49 lattice points: almost every pick reads or rewrites a displaced entry."""
    from uav_bs_ctrl_amd import sim
    spec = sim.MapSpec(sim.MapParams(n_ubs=16, n_gts=40, range_pos=7.0), "uniform_lattice")
    env = sim.BatchedUbsCoverageEnv.from_map(spec, 9, seed=SEED)
    ic, fc = spec.sampler_consts()
    got = env.sample_positions()
    _same(got, R.sample(ic, fc, 9, SEED, 0), "lattice 16 x 40 of 49")
    check_structure(spec, *(t.cpu().numpy() for t in got))


@pytest.mark.parametrize("name", ["8ubs", "dense_hotspot_v2"])
def test_environment_b_does_not_depend_on_the_launch_geometry(name):
    a, b = _env(name, 7).sample_positions(), _env(name, 3).sample_positions()
    for x, y in zip(a, b):
        assert th.equal(x[:3], y)


@pytest.mark.parametrize("name", ["8ubs", "inf"])
def test_large_batch_passes_the_structural_invariants(name):
    got = [t.cpu().numpy() for t in _env(name, 4096).sample_positions()]
    check_structure(_spec(name), *got)
    tail = slice(4090, 4096)
    _same([th.as_tensor(g[tail]) for g in got],
          R.sample(*_spec(name).sampler_consts(), 6, SEED, 0, envs=np.arange(4090, 4096)), f"{name} tail of 4096")


def test_reset_from_map_is_reset_on_the_sampled_arrays():
    env, twin, feed = _env("8ubs", 4), _env("8ubs", 4), _env("8ubs", 4)
    act = th.randint(0, env.n_actions, (4, env.n_agents), device="cuda", generator=th.Generator("cuda").manual_seed(1))
    env.reset_from_map(), env.step(act), env.step(act)                       # dirty running state, counter at 1
    for k in (1, 2):
        obs = {n: v.clone() for n, v in env.reset_from_map().items()}
        feed.map_rng[1] = k
        ubs, gts, prior = feed.sample_positions()
        _same((ubs, gts, prior), _ref("8ubs", 4, k), f"reset {k}")
        assert th.equal(env.pos_ubs, ubs) and th.equal(env.pos_gts, gts)
        ref_obs = twin.reset(ubs, gts, prior)
        for n in obs:
            assert th.equal(obs[n], ref_obs[n]), n
        for n in ("t", "avg_rate", "run_f32", "n_colls", "ep_ret", "prior"):
            assert th.equal(getattr(env, n), getattr(twin, n)), n
        assert int(env.t.abs().sum()) == 0 and float(env.n_colls.abs().sum()) == 0.0 and float(env.ep_ret.abs().sum()) == 0.0
        if k == 1:
            first = ubs.clone()
            env.step(act)
    assert not th.equal(first, env.pos_ubs)
    assert env.map_rng.tolist() == [SEED, 3]


def test_running_state_is_cleared_before_the_transmission():
    """After a reset t = 0 and the running averages hold the reset-time transmission alone, as after ``reset`` (mubs_cov.py:86-97)."""
    env = _env("8ubs", 4)
    act = th.zeros(4, env.n_agents, dtype=th.int64, device="cuda")
    env.reset_from_map()
    for _ in range(3):
        env.step(act)
    assert int(env.t.sum()) == 12
    for t_ in (env.avg_rate, env.run_f32, env.n_colls, env.ep_ret):          # hovering away from the hotspot may earn nothing:
        t_.fill_(3.0)                                                        # every running buffer is made dirty by hand
    env.reset_from_map()
    assert int(env.t.abs().sum()) == 0 and float(env.ep_ret.abs().sum()) == 0.0
    assert th.equal(env.avg_rate, env.out["rate_per_gt"])                    # (0 x old average + rate) / 1
    assert th.equal(env.run_f32[:, 1], env.run_f32[:, 3])                    # average utility = this transmission's utility
    assert th.equal(env.n_colls, env.out["mask_collision"].sum(1).double() / 2)


def test_captured_reset_and_step_replay_with_the_current_counter():
    env, eager = _env("8ubs", 4), _env("8ubs", 4)
    act = th.randint(0, env.n_actions, (4, env.n_agents), device="cuda", generator=th.Generator("cuda").manual_seed(2))
    s = th.cuda.Stream()
    s.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(s):                                   # warm-up on the side stream, as torch's capture protocol asks
        env.reset_from_map(), env.step(act)
    th.cuda.current_stream().wait_stream(s)
    env.map_rng[1] = 0
    g = th.cuda.CUDAGraph()
    with th.cuda.graph(g):
        env.reset_from_map()
        env.step(act)
    env.map_rng[1] = 5                                        # capture launched nothing; the replays start here
    for k in (5, 6):
        g.replay()
        th.cuda.synchronize()
        eager.map_rng[1] = k
        eager.reset_from_map()
        ref = _ref("8ubs", 4, k)
        assert np.array_equal(eager.pos_gts.cpu().numpy(), ref[1]) and np.array_equal(env.pos_gts.cpu().numpy(), ref[1])
        obs, rew, done, _ = eager.step(act)
        assert th.equal(env.pos_ubs, eager.pos_ubs) and th.equal(env.t, eager.t) and th.equal(env.prior, eager.prior)
        for n, v in env.out.items():
            assert th.equal(v, eager.out[n]), n
        assert th.equal(env.ep_ret, eager.ep_ret)
    assert env.map_rng.tolist() == [SEED, 7]


def test_argument_errors_are_codes():
    from uav_bs_ctrl_amd import _lib as L
    fc = (ctypes.c_double * 5)(6000.0, 200.0, 800.0, 200.0, 100.0)
    rng = th.tensor([1, 0], dtype=th.int64, device="cuda")
    ubs, gts = th.zeros(1, 17, 2, dtype=th.float64, device="cuda"), th.zeros(1, 1025, 2, device="cuda")
    prior = th.zeros(1, 1025, dtype=th.int32, device="cuda")

    def call(n, M, rng_=rng, n_picks=10, gpg=5):
        ic = (ctypes.c_int32 * 9)(3, n, M, 30, 7, 4, n_picks, gpg, 0)
        return L.lib().uavgnn_map_sample(ic, fc, 1, L.ptr(rng_), None, None, ubs.data_ptr(), gts.data_ptr(), prior.data_ptr(), L.stream())
    assert call(17, 50) == L.UAVGNN_EUNSUPPORTED
    assert call(8, 1025, n_picks=205) == L.UAVGNN_EUNSUPPORTED
    assert call(0, 50) == L.UAVGNN_EUNSUPPORTED
    assert call(8, 50, rng_=None) == L.UAVGNN_EINVAL
    assert call(8, 50, n_picks=17, gpg=3) == L.UAVGNN_EINVAL            # 17 groups do not fit the 4 x 4 block
    ic = (ctypes.c_int32 * 9)(1, 3, 4, 1000, 1, 1, 0, 1, 0)              # `fixed` without its arrays
    assert L.lib().uavgnn_map_sample(ic, fc, 1, rng.data_ptr(), None, None, ubs.data_ptr(), gts.data_ptr(), prior.data_ptr(),
                                     L.stream()) == L.UAVGNN_EINVAL
    th.cuda.synchronize()
    with pytest.raises(L.UavGnnError):
        from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv, MapParams
        BatchedUbsCoverageEnv(MapParams(n_ubs=2, n_gts=3), 1).reset_from_map()

"""Experiment 1 on the device: the single-UBS simulator and its placement sampler (csrc/subs_env.hip,
uav_bs_ctrl_amd/sim.py ``BatchedSingleUbsCoverageEnv``) against the REFERENCE simulator's own output
(tests/golden/env_subs_cov.npz: envs/subs_cov/subs_cov.py imported unchanged and stepped by a seeded policy,
tests/golden/make_golden_exp1.py) and against the NumPy restatement of the sampler (tests/subs_sampler_ref.py).

Decisions - the schedule, termination, the step counter - are BIT-EXACT; floating point holds at the project's standing 1e-5
relative rule (``_close``, copied from tests/test_env_sim.py); the UBS position at 1e-12.  Priorities: as in
tests/test_env_sim.py, every transition is replayed with the reference's own priority vector, and the kernel's next priorities
must be a stable argsort of the averages that equals the reference's wherever the reference's keys are distinct."""
import types

import numpy as np
import pytest
import torch as th

from oracle import restatement as R
from oracle.closed_form import fill_closed_form
from tests import subs_sampler_ref as S
from tests.test_subs_env_host import ENV_CASES, assert_same_graph, env_case, wrapper_graphs
from tests.util import assert_close

pytestmark = pytest.mark.gpu


def _close(got, ref, what, rel=1e-5):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = rel * max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-30) + rel * np.abs(ref)
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{ref.size} off; worst {np.abs(got - ref).max():.3e} (max|ref| {np.abs(ref).max():.3e})"


@pytest.mark.parametrize("case", ENV_CASES)
def test_every_transition_replayed_with_the_reference_priorities(case):
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv
    z, p, c, steps = env_case(case)
    f = lambda t, k: z[f"{case}:t{t}:{k}"]  # noqa: E731
    M = p.n_gts
    env = BatchedSingleUbsCoverageEnv(p, 1, seed=0)
    env.reset(pos_ubs=f(0, "pos_ubs")[None], pos_gts=z[f"{case}:pos_gts"][None], prior=f(0, "prior_used")[None])
    ep_ret, n_served, n_distinct = 0.0, 0, 0
    for t in range(steps + 1):
        if t > 0:
            env.prior.copy_(th.as_tensor(f(t, "prior_used")[None]).to(th.int32))     # the reference's tie resolution
            obs, rew, done, info = env.step(th.as_tensor(f(t, "actions")[None]).cuda())
            ep_ret += float(f(t, "reward"))
            assert float(info["BadMask"][0]) == float(f(t, "BadMask")) and int(info["EpLen"][0]) == t
            _close(info["EpRet"][0].cpu(), ep_ret, "EpRet")
            _close(rew[0].cpu(), f(t, "reward"), f"{case} t={t} reward")
            _close(info["TotalThroughput"][0].cpu(), f(t, "total_throughput"), "info TotalThroughput")
            _close(info["AvgGlobalUtility"][0].cpu(), f(t, "avg_global_util"), "info AvgGlobalUtility")
            _close(info["FairIdx"][0].cpu(), f(t, "fair_idx"), "info FairIdx")
        o = {k: v[0].cpu().numpy() for k, v in env.out.items()}
        # ---- decisions: bit-exact -----------------------------------------------------------------------------------------
        assert np.array_equal(o["sched"], f(t, "sched")), (case, t, "schedule")
        assert float(o["done"]) == float(f(t, "done")) and int(env.t[0]) == t
        n_served += int(f(t, "sched").sum())
        # ---- floating point --------------------------------------------------------------------------------------------------
        _close(env.pos_ubs[0].cpu(), f(t, "pos_ubs"), "pos_ubs", 1e-12)
        for k in ("d_u2g", "rate_per_gt", "obs_gt", "obs_agent"):
            _close(o[k], f(t, k), f"{case} t={t} {k}")
        _close(env.avg_rate[0].cpu(), f(t, "avg_rate"), "avg_rate")
        _close(env.run_f64[0].cpu(), [f(t, "total_throughput"), f(t, "avg_global_util"), f(t, "fair_idx"), f(t, "global_util")],
               "running scalars")
        flat = np.concatenate((o["obs_agent"], o["obs_gt"].reshape(-1)))
        assert o["obs_flat"].tobytes() == flat.tobytes(), "obs_flat is not agent || gt, bit for bit"
        obs_now = env.observations()
        assert obs_now["flat"].data_ptr() == env.out["obs_flat"].data_ptr() and obs_now["gt"].shape == (1, M, 4)
        # ---- next priorities: a stable argsort of the stored averages; the reference's when its keys are distinct -----------------
        pr, avg = env.prior[0].cpu().numpy(), env.avg_rate[0].cpu().numpy()
        assert sorted(pr.tolist()) == list(range(M))
        keys = avg[pr]
        assert (np.diff(keys) >= 0).all()
        assert (np.diff(pr)[np.diff(keys) == 0] > 0).all(), "ties must keep GT index order (stable)"
        ref_avg = f(t, "avg_rate")
        vals, counts = np.unique(ref_avg, return_counts=True)
        single = np.isin(ref_avg, vals[counts == 1])           # GTs whose reference key no other GT shares (the unserved tie at 0)
        assert [m for m in pr if single[m]] == [m for m in f(t, "prior_next") if single[m]], (case, t, "order of the untied GTs")
        if len(vals) == M:
            n_distinct += 1
            assert np.array_equal(pr, f(t, "prior_next")), (case, t)
        else:                                   # the reference's order is also a valid argsort of (its) averages
            assert (np.diff(ref_avg[f(t, "prior_next")]) >= 0).all()
    assert n_served > 0 and float(o["done"]) == 1.0
    print(f"{case}: {steps + 1} transitions, {n_served} served GT-steps, {n_distinct} transitions with distinct priority keys")


def test_argument_errors_are_codes_not_crashes():
    import ctypes

    from uav_bs_ctrl_amd import _lib
    L = _lib.lib()
    ic = (ctypes.c_int32 * 5)(1025, 2, 5, 10, 2)
    fc = (ctypes.c_double * 14)(*([1.0] * 14))
    one = th.zeros(1 << 14, dtype=th.float64, device="cuda").data_ptr()
    ptrs = [None, one] + [one] * 14
    assert L.uavgnn_subs_env_step(ic, fc, 1, *ptrs, None) == _lib.UAVGNN_EUNSUPPORTED          # M > 1024
    ic[0] = 10
    assert L.uavgnn_subs_env_step(ic, fc, 1, *([None] * 16), None) == _lib.UAVGNN_EINVAL
    assert L.uavgnn_subs_env_step(None, fc, 1, *ptrs, None) == _lib.UAVGNN_EINVAL
    assert L.uavgnn_subs_env_step(ic, fc, -1, *ptrs, None) == _lib.UAVGNN_EINVAL
    assert L.uavgnn_subs_env_step(ic, fc, 0, *ptrs, None) == 0
    sc, sf = (ctypes.c_int32 * 2)(33, 32), (ctypes.c_double * 2)(1000.0, 100.0)
    assert L.uavgnn_subs_env_sample(sc, sf, 1, one, one, one, one, None) == _lib.UAVGNN_EUNSUPPORTED   # 33 x 32 > 1024
    sc[0] = 0
    assert L.uavgnn_subs_env_sample(sc, sf, 1, one, one, one, one, None) == _lib.UAVGNN_EINVAL
    sc[0] = 2
    assert L.uavgnn_subs_env_sample(sc, sf, 1, None, one, one, one, None) == _lib.UAVGNN_EINVAL


@pytest.mark.parametrize("case", ["m65", "short_rb"])
def test_batched_environments_are_independent(case):
    """B = 70 environments (not a multiple of the 64 lanes, nor of the wavefronts of a workgroup) from shifted copies of the
    fixture's state, with different priorities and actions, in ONE launch == the same environments stepped one by one, bit for bit."""
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv
    z, p, c, steps = env_case(case)
    B, M = 70, p.n_gts
    gen = th.Generator(device="cuda").manual_seed(0)
    t0 = steps // 2                                            # a state in which the UBS sits among the GTs
    shift = th.rand(B, 2, device="cuda", generator=gen, dtype=th.float64) * 60 - 30
    shift[0] = 0
    pos_u = th.as_tensor(z[f"{case}:t{t0}:pos_ubs"]).cuda()[None] + shift
    pos_g = th.as_tensor(z[f"{case}:pos_gts"]).cuda()[None].expand(B, -1, -1)
    prior = th.argsort(th.rand(B, M, device="cuda", generator=gen), dim=1).to(th.int32)
    env = BatchedSingleUbsCoverageEnv(p, B, seed=0)
    env.reset(pos_u, pos_g, prior)
    singles = []
    for b in range(B):
        e1 = BatchedSingleUbsCoverageEnv(p, 1, seed=0)
        e1.reset(pos_u[b:b + 1], pos_g[b:b + 1], prior[b:b + 1])
        singles.append(e1)

    def same(t):
        for b, e1 in enumerate(singles):
            for k in env.out:
                assert th.equal(env.out[k][b], e1.out[k][0]), (t, b, k)
            for k in ("prior", "avg_rate", "run_f64", "pos_ubs", "t"):
                assert th.equal(getattr(env, k)[b], getattr(e1, k)[0]), (t, b, k)
    same(0)
    for t in range(1, 4):
        a = th.randint(0, env.n_actions, (B,), device="cuda", generator=gen)
        env.step(a)
        for b, e1 in enumerate(singles):
            e1.step(a[b:b + 1])
        same(t)
    assert int(env.out["sched"].sum()) > 0
    assert len({tuple(r) for r in env.out["sched"].cpu().tolist()}) > 1, "every environment has the same schedule: nothing was told apart"


@pytest.mark.parametrize("n_grps,gpg", [(2, 5), (5, 13)])
def test_sampler_against_the_numpy_restatement(n_grps, gpg):
    """B = 70, resets 0 and 1: shuffle and priorities bit-exact; positions within ONE float32 ulp of the float64 restatement
    rounded to float32 (the kernel evaluates in double and rounds once; its double log / cos / sin may differ from NumPy's in the
    last double bits, which moves the float32 rounding by at most one ulp); a second launch at the same {seed, resets} is
    bitwise identical; the sampler-driven reset serves its observations through the same buffers."""
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    p = SingleUbsParams(n_grps=n_grps, gts_per_grp=gpg, r_cov=150.0)
    B, M, seed = 70, n_grps * gpg, 977
    env = BatchedSingleUbsCoverageEnv(p, B, seed=seed)
    for resets in (0, 1):
        assert env.rng.cpu().tolist() == [seed, resets]
        ubs, gts, prior = (x.cpu().numpy() for x in env.sample_positions())
        r_ubs, r_gts64, r_prior, _ = S.sample64(n_grps, gpg, p.range_pos, p.r_cov, B, seed, resets)
        r_gts = r_gts64.astype(np.float32)
        assert np.array_equal(prior, r_prior), "priority permutation"
        assert np.array_equal(ubs, r_ubs)
        err = np.abs(gts.astype(np.float64) - r_gts.astype(np.float64))
        assert (err <= np.spacing(np.abs(r_gts)).astype(np.float64)).all(), f"positions / shuffle: worst {err.max():.3e}"
        print(f"({n_grps},{gpg}) resets {resets}: {int((err > 0).sum())}/{err.size} coordinates differ by one ulp")
        env.rng[1] = resets                                    # the same {seed, resets} again
        again = env.sample_positions()
        assert np.array_equal(again[1].cpu().numpy(), gts) and np.array_equal(again[2].cpu().numpy(), prior)
    assert not np.array_equal(gts, env.sample_positions()[1].cpu().numpy()), "the reset counter does not reach the draws"
    # reset() without arguments: the sampler writes the state buffers, then the reset-time transmission runs
    env.rng[1] = 0
    obs = env.reset()
    r_ubs, r_gts64, r_prior, _ = S.sample64(n_grps, gpg, p.range_pos, p.r_cov, B, seed, 0)
    assert int(env.rng[1]) == 1 and int(env.t.abs().max()) == 0
    assert np.array_equal(env.prior.shape, r_prior.shape) and np.array_equal(env.pos_ubs.cpu().numpy(), r_ubs)
    want = (env.pos_gts.double() - env.pos_ubs[:, None, :]) / p.range_pos
    assert_close(obs["gt"][..., :2], want, 1e-6, "reset-time GT offsets")          # float32 operations at reset: 1e-6 of float64
    assert float(obs["agent"].min()) == float(obs["agent"].max()) == 0.5


@pytest.mark.parametrize("case", ["exp1_g2", "m65"])
def test_graph_of_the_simulator_and_the_drqn_agent_on_it(case):
    """``env.graph()`` == ``graph.batch`` of per-environment ``heterograph``s built as the reference's wrapper builds them, array for
    array, without copying the observations; ``DrqnGnnAgent`` on it == the float64 oracle at 1e-5."""
    from uav_bs_ctrl_amd.agents import REGISTRY
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv
    z, p, c, steps = env_case(case)
    B, H = 8, 32
    env = BatchedSingleUbsCoverageEnv(p, B, seed=5)
    env.reset()
    env.step(th.arange(B, device="cuda") % env.n_actions)
    g = env.graph()
    assert_same_graph(g, wrapper_graphs(env.out["obs_gt"].cpu(), env.out["obs_agent"].cpu()))
    x, off = g.relation_segments("seen-by")
    assert x.data_ptr() == env.out["obs_gt"].data_ptr() and g.agent_feat().data_ptr() == env.out["obs_agent"].data_ptr()
    info = env.get_env_info("gnn")
    assert info == dict(obs_shape=dict(agent=2, gt=4), n_actions=env.n_actions, episode_limit=p.episode_limit)
    assert env.get_env_info("rnn")["obs_shape"] == 2 + 4 * p.n_gts == env.out["obs_flat"].shape[1]
    net = REGISTRY["drqn_gnn"](info["obs_shape"], info["n_actions"], types.SimpleNamespace(hidden_size=H, n_heads=4))
    fill_closed_form(net)
    p64 = {k: v.detach().double().clone() for k, v in net.state_dict().items()}
    h = 0.5 * th.randn(B, H, generator=th.Generator().manual_seed(2))
    arrays = dict(x_a=env.out["obs_agent"].cpu().double(), x_gt=x.cpu().double(), seen_off=off.cpu())
    q64, h64 = R.drqn_gnn_agent_forward(arrays, h.double(), p64, 4)
    q, h2 = net.cuda()(g, h.cuda())
    assert_close(q, q64, 1e-5, f"{case}: q on env.graph()")
    assert_close(h2, h64, 1e-5, f"{case}: h' on env.graph()")

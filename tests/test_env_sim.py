"""Row f3: the batched device simulator (csrc/env_sim.hip, uav_bs_ctrl_amd/sim.py) against the REFERENCE simulator's own
output (tests/golden/env_mubs_cov*.npz: envs/mubs_cov/mubs_cov.py imported unchanged and stepped with seeded actions,
tests/golden/make_golden.py `env` and `env_edges`).

Index / decision work is BIT-EXACT: the greedy schedule (serving UBS and resource block per GT), collision masks,
visibility flags, termination.  Floating point (distances, rates, averages, Jain index, utilities, rewards, observation
and state features, the episode return and collision rate of ``info``) to 1e-5 relative.

Priorities.  ``np.argsort(avg_rate)`` (mubs_cov.py:209) is not a stable sort and its tie order depends on NumPy's SIMD
dispatch; most GTs tie at rate 0.  The kernel uses the STABLE order.  Therefore every transition is checked twice:
  * replayed with the reference's own priority vector as input (``prior_used``): pins the whole step;
  * the kernel's next priorities must be a valid argsort of the averages (non-decreasing keys, a permutation, stable
    among equal keys), must equal the reference's wherever the reference's keys are all distinct, and every GT whose
    reference average is separated from all others by more than 2e-5 of the largest (twice the floating-point rule, so
    the kernel's own averages order it the same way) must sit at the reference's position - a position that does not
    depend on how anybody's ties are broken;
and a free-running episode (the kernel's own priorities fed forward) is checked for the permutation-invariant
quantities that do not depend on tie order whenever no RB shortage occurred.

The first five cases (`env`) never let the nearest covering UBS be full, stay at M <= 50, n <= 8, R <= 5 and keep both
constructor switches on; the `env_edges` cases are there for the rest - ``edge_counts`` says what they reach, and
``test_edge_fixture_reaches_what_it_is_for`` holds the committed files to it without a GPU.  The GPU tests append what they
measured (worst relative error per quantity, rank checks made / skipped, the event counts) to
env_sim_edges.jsonl, next to the gradient log of tests/util.py; profiles/env_sim_edges.txt is the table of one such run."""
import functools
import json
import os

import numpy as np
import pytest
import torch as th

from tests.util import _GRAD_LOG, GOLDEN

gpu = pytest.mark.gpu
CASES = ["debug", "r800", "8ubs", "8ubs_parked", "8ubs_crowded"]
EDGE_CASES = ["m80_r2", "m80_r5", "v2_n16_m136", "v2_m65_r16", "m64_plain"]
FIXTURES = ("env_mubs_cov.npz", "env_mubs_cov_edges_a.npz", "env_mubs_cov_edges_b.npz")
EDGE_FIXTURE_MAX_BYTES = 427456          # the largest fixture the repository carried before the edge files
RANK_SEP = 2e-5                          # separation (of the largest average) above which a GT's priority position is pinned
_EDGE_LOG = os.path.join(os.path.dirname(_GRAD_LOG), "env_sim_edges.jsonl")          # next to grad_errors.jsonl
FLOAT_FIELDS = ("d_u2g", "d_u2u", "rate_per_gt", "rate_per_ubs", "obs_gt", "obs_ubs", "obs_agent", "state")


@functools.lru_cache(maxsize=None)
def _npz(name):
    return np.load(os.path.join(GOLDEN, name))


def _fixture_of(case):
    for name in FIXTURES:
        z = _npz(name)
        if f"{case}:steps" in z.files:
            return z
    raise KeyError(f"no fixture under tests/golden holds the case {case!r}")


def _case(case):
    from uav_bs_ctrl_amd.sim import MapParams
    z = _fixture_of(case)
    c = {k.split(":")[-1]: float(z[k]) for k in z.files if k.startswith(f"{case}:const:")}
    moves = z[f"{case}:avail_moves"]
    n_dirs = 4
    dt = c["dt"]
    vels = tuple(sorted({round(float(np.hypot(*mv)) / dt, 9) for mv in moves[1:]}))
    p = MapParams(n_ubs=int(c["n_ubs"]), n_gts=int(c["n_gts"]), n_rbs=int(c["n_rbs"]), range_pos=c["range_pos"],
                  episode_limit=int(c["episode_limit"]), dt=dt, r_cov=c["r_cov"], r_sns=c["r_sns"], r_comm=c["r_comm"],
                  vels=vels, n_dirs=n_dirs, reward_scale_rate=c["reward_scale_rate"],
                  fair_service=bool(c.get("fair_service", 1.0)), avoid_collision=bool(c.get("avoid_collision", 1.0)))
    assert np.allclose(p.avail_moves(), moves, atol=1e-9)
    assert abs(p.max_rate - c["max_rate"]) < 1e-12 * c["max_rate"]
    steps = int(z[f"{case}:steps"])
    return z, p, steps


def _close(got, ref, what, rel=1e-5, errs=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = rel * max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-30) + rel * np.abs(ref)
    bad = np.abs(got - ref) > tol
    if errs is not None and ref.size:      # recorded before the assertion: error / (max|ref| + |ref|), the rule's own measure
        key = what.split(" ")[-1]
        den = np.maximum(float(np.abs(ref).max()) + np.abs(ref), 1e-30)
        errs[key] = max(errs.get(key, 0.0), float((np.abs(got - ref) / den).max()))
    assert not bad.any(), f"{what}: {int(bad.sum())}/{ref.size} off; worst {np.abs(got - ref).max():.3e} (max|ref| {np.abs(ref).max():.3e})"


def _separated(avg):
    """Mask of the GTs whose average differs from EVERY other GT's by more than RANK_SEP of the largest average."""
    avg = np.asarray(avg, dtype=np.float64)
    order = np.argsort(avg, kind="stable")
    gap = np.diff(avg[order])
    thr = RANK_SEP * float(np.abs(avg).max())
    ok = (np.concatenate(([np.inf], gap)) > thr) & (np.concatenate((gap, [np.inf])) > thr)
    out = np.zeros(avg.size, dtype=bool)
    out[order] = ok
    return out


def edge_counts(z, case):
    """What a case of the fixture reaches, from its stored arrays alone (z: an npz or the dict it is saved from) - over all
    transitions: GT-steps served by a UBS strictly farther than the nearest one (the nearest covering UBS was full), GT-steps
    covered but unserved, collision flags, GT-steps covered by several UBSs, transitions with done = 1, GT-steps whose priority
    position is pinned (``_separated``), UBS moves clipped at a border, GT-steps with two covering UBSs at EXACTLY the same float32
    distance (``distance_ties``: must be 0, see check_edge_counts); and the maxima that select kernel paths."""
    steps, r_cov = int(z[f"{case}:steps"]), np.float32(float(z[f"{case}:const:r_cov"]))
    moves, range_pos = z[f"{case}:avail_moves"], float(z[f"{case}:const:range_pos"])
    f = lambda t, k: z[f"{case}:t{t}:{k}"]  # noqa: E731
    c = dict(non_nearest=0, covered_unserved=0, collision_flags=0, multiply_covered=0, done=0, rank_checkable=0,
             clipped_moves=0, served=0, distance_ties=0)
    for t in range(steps + 1):
        d, gu = f(t, "d_u2g"), f(t, "gt_ubs")
        cov, served = d <= r_cov, gu >= 0
        nearest = np.argsort(d, axis=0, kind="stable")[0]
        cols = np.arange(d.shape[1])
        c["non_nearest"] += int((served & (d[np.maximum(gu, 0), cols] > d[nearest, cols])).sum())
        c["distance_ties"] += sum(len(np.unique(d[cov[:, m], m])) != int(cov[:, m].sum()) for m in cols)
        c["covered_unserved"] += int((cov.any(0) & ~served).sum())
        c["collision_flags"] += int(f(t, "mask_collision").sum())
        c["multiply_covered"] += int((cov.sum(0) >= 2).sum())
        c["done"] += int(float(f(t, "done")) == 1.0)
        c["rank_checkable"] += int(_separated(f(t, "avg_rate")).sum())
        c["served"] += int(served.sum())
        if t > 0:
            want = f(t - 1, "pos_ubs") + moves[f(t, "actions")]
            c["clipped_moves"] += int(((want < 0) | (want > range_pos)).any(1).sum())
    c.update(n_ubs=int(z[f"{case}:const:n_ubs"]), n_gts=int(z[f"{case}:const:n_gts"]), n_rbs=int(z[f"{case}:const:n_rbs"]))
    return c


def check_edge_counts(counts):
    """The minimums the edge cases exist for (counts: {case: edge_counts}); tests/golden/make_golden.py `env_edges` asserts the same
    over what it writes."""
    assert set(counts) == set(EDGE_CASES), sorted(counts)
    total = lambda k: sum(c[k] for c in counts.values())  # noqa: E731
    assert total("non_nearest") >= 20, "GT-steps served by a UBS that is not the nearest covering one"
    assert total("covered_unserved") >= 100, "covered GT-steps left unserved because the RBs ran out"
    assert total("collision_flags") >= 4
    assert sum(c["done"] > 0 for c in counts.values()) >= 2, "cases that reach the episode limit"
    assert total("clipped_moves") >= 1, "a UBS move clipped at a border"
    for case, c in counts.items():
        assert c["rank_checkable"] >= 100, (case, "GT-steps whose priority position is pinned", c["rank_checkable"])
        # two covering UBSs at the same float32 distance of a GT (co-located UBSs: both clipped into the same corner): which one
        # ``np.argsort(d_u2g[:, m])`` (mubs_cov.py:177) puts first is NumPy's choice - the stable order with its insertion sort, another
        # with the AVX-512 sort it dispatches to where the CPU has one - so such a transition pins nothing; the kernel keeps the
        # stable order
        assert c["distance_ties"] == 0, (case, "exact distance ties among covering UBSs", c["distance_ties"])
    assert max(c["n_ubs"] for c in counts.values()) == 16 and max(c["n_rbs"] for c in counts.values()) == 16
    assert any(c["n_gts"] == 65 for c in counts.values()) and any(c["n_gts"] > 128 for c in counts.values())


def _log_row(**row):
    try:
        os.makedirs(os.path.dirname(_EDGE_LOG), exist_ok=True)
        with open(_EDGE_LOG, "a") as fh:
            fh.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], **row)) + "\n")
    except OSError:
        pass


def _positions(order):
    pos = np.empty(len(order), dtype=np.int64)
    pos[np.asarray(order, dtype=np.int64)] = np.arange(len(order))
    return pos


def _check_next_priorities(pr, avg, ref_avg, ref_next, M, where):
    """The kernel's next priorities `pr` (over its averages `avg`) against the reference's.  -> (GTs rank-checked, GTs skipped)."""
    assert sorted(pr.tolist()) == list(range(M))
    keys = avg[pr]
    assert (np.diff(keys) >= 0).all()
    same = np.diff(keys) == 0
    assert (np.diff(pr)[same] > 0).all(), "ties must keep GT index order (stable)"
    if len(np.unique(ref_avg)) == M:
        assert np.array_equal(pr, ref_next)
    else:                                   # the reference's order is also a valid argsort of (its) averages
        assert (np.diff(ref_avg[ref_next]) >= 0).all()
    sep = _separated(ref_avg)
    got, want = _positions(pr)[sep], _positions(ref_next)[sep]
    assert np.array_equal(got, want), (where, "priority position of the GTs with a separated average",
                                       np.flatnonzero(sep)[got != want].tolist())
    return int(sep.sum()), int((~sep).sum())


@gpu
@pytest.mark.parametrize("case", CASES + EDGE_CASES)
def test_every_transition_replayed_with_the_reference_priorities(case):
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    z, p, steps = _case(case)
    f = lambda t, k: z[f"{case}:t{t}:{k}"]  # noqa: E731
    env = BatchedUbsCoverageEnv(p, 1)
    env.reset(pos_ubs=f(0, "pos_ubs")[None], pos_gts=z[f"{case}:pos_gts"][None], prior=f(0, "prior_used")[None])
    n_dec, n_ranked, n_skipped, ep_ret, errs = 0, 0, 0, 0.0, {}
    for t in range(steps + 1):
        if t > 0:
            env.prior.copy_(th.as_tensor(f(t, "prior_used")[None]).to(th.int32))     # the reference's tie resolution
            obs, rew, done, info = env.step(th.as_tensor(f(t, "actions")[None]).cuda())
            # ---- info (mubs_cov.py:115-121): the return so far, collisions per step ----------------------------------
            ep_ret += float(f(t, "reward").mean())
            _close(info["EpRet"][0].cpu(), ep_ret, f"{case} t={t} EpRet", errs=errs)
            _close(info["ProbCollision"][0].cpu(), float(f(t, "n_colls")) / t, f"{case} t={t} ProbCollision", errs=errs)
            if f"{case}:t{t}:info:EpRet" in z.files:                                     # the reference's own info, where stored
                _close(info["EpRet"][0].cpu(), f(t, "info:EpRet"), f"{case} t={t} EpRet", errs=errs)
                _close(info["ProbCollision"][0].cpu(), f(t, "info:ProbCollision"), f"{case} t={t} ProbCollision", errs=errs)
            assert int(info["EpLen"][0]) == t and float(info["BadMask"][0]) == float(f(t, "done"))
        o = {k: v[0].cpu().numpy() for k, v in env.out.items()}
        # ---- decisions: bit-exact --------------------------------------------------------------------------------
        assert np.array_equal(o["gt_ubs"], f(t, "gt_ubs")), (case, t, "serving UBS per GT")
        assert np.array_equal(o["gt_rb"], f(t, "gt_rb")), (case, t, "resource block per GT")
        assert np.array_equal(o["mask_collision"].astype(bool), f(t, "mask_collision")), (case, t)
        assert np.array_equal(o["obs_gt"][..., 0], f(t, "obs_gt")[..., 0]) and np.array_equal(o["obs_ubs"][..., 0], f(t, "obs_ubs")[..., 0])
        assert float(o["done"]) == float(f(t, "done")) and int(env.t[0]) == t
        n_dec += int((f(t, "gt_ubs") >= 0).sum())
        # ---- floating point: 1e-5 --------------------------------------------------------------------------------
        _close(env.pos_ubs[0].cpu(), f(t, "pos_ubs"), "pos_ubs", 1e-12)
        for k in FLOAT_FIELDS:
            _close(o[k], f(t, k), f"{case} t={t} {k}", errs=errs)
        _close(env.avg_rate[0].cpu(), f(t, "avg_rate"), "avg_rate", errs=errs)
        rf = env.run_f32[0].cpu().numpy()
        _close(rf, [f(t, "total_throughput"), f(t, "avg_global_util"), f(t, "fair_idx"), f(t, "global_util")], "running scalars",
               errs=errs)
        _close(env.n_colls[0].cpu(), f(t, "n_colls"), "n_colls", 1e-12)
        if t > 0:
            _close(o["reward"], f(t, "reward"), "reward", errs=errs)
        # ---- next priorities: a valid (stable) argsort; equal to the reference's when its keys are distinct; the GTs with a
        # separated average at the reference's position ------------------------------------------------------------
        made, skipped = _check_next_priorities(env.prior[0].cpu().numpy(), env.avg_rate[0].cpu().numpy(), f(t, "avg_rate"),
                                               f(t, "prior_next"), p.n_gts, (case, t))
        n_ranked, n_skipped = n_ranked + made, n_skipped + skipped
    counts = edge_counts(z, case)
    print(f"{case}: rank checks made {n_ranked}, skipped {n_skipped}; errors {errs}; {counts}")
    _log_row(case=case, launch="one per transition", errors=errs, rank_checked=n_ranked, rank_skipped=n_skipped, counts=counts)
    assert case in ("8ubs",) or n_dec > 0
    assert n_ranked == counts["rank_checkable"]
    if case in EDGE_CASES:
        assert n_ranked >= 100, (case, n_ranked, n_skipped)


@gpu
@pytest.mark.parametrize("case", ["m80_r5", "v2_n16_m136"])
def test_all_transitions_of_a_case_in_one_launch(case):
    """B = steps environments, environment b loaded with the REFERENCE's state before its transition b + 1 (positions, the
    priorities it used, averages, t, the running scalars, the collision count), one step with the recorded actions: environment b
    must be transition b + 1 of the fixture.  Per-environment t and done, and the independence of the environments of a launch,
    against the reference itself."""
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    z, p, steps = _case(case)
    f = lambda t, k: z[f"{case}:t{t}:{k}"]  # noqa: E731
    B = steps
    before = lambda k: np.stack([np.asarray(f(t, k)) for t in range(0, steps)])           # noqa: E731
    after = lambda k: np.stack([np.asarray(f(t, k)) for t in range(1, steps + 1)])        # noqa: E731
    env = BatchedUbsCoverageEnv(p, B)
    env.pos_ubs.copy_(th.as_tensor(before("pos_ubs")))
    env.pos_gts.copy_(th.as_tensor(z[f"{case}:pos_gts"]).to(th.float32)[None].expand(B, -1, -1))
    env.prior.copy_(th.as_tensor(after("prior_used")).to(th.int32))
    env.avg_rate.copy_(th.as_tensor(before("avg_rate")))
    env.t.copy_(th.arange(steps, dtype=th.int32))
    env.run_f32.copy_(th.as_tensor(np.stack([before(k) for k in ("total_throughput", "avg_global_util", "fair_idx", "global_util")],
                                            axis=1)).to(th.float32))
    env.n_colls.copy_(th.as_tensor(before("n_colls")))
    ret_before = np.concatenate(([0.0], np.cumsum(after("reward").mean(1))))[:-1]
    env.ep_ret.copy_(th.as_tensor(ret_before))
    obs, rew, done, info = env.step(th.as_tensor(after("actions")).cuda())
    o = {k: v.cpu().numpy() for k, v in env.out.items()}
    errs, n_ranked, n_skipped = {}, 0, 0
    assert np.array_equal(env.t.cpu().numpy(), np.arange(1, steps + 1))
    assert np.array_equal(o["done"], after("done").astype(np.float32)), "per-environment done"
    for k in ("gt_ubs", "gt_rb"):
        assert np.array_equal(o[k], after(k)), (case, k)
    assert np.array_equal(o["mask_collision"].astype(bool), after("mask_collision"))
    assert np.array_equal(o["obs_gt"][..., 0], after("obs_gt")[..., 0]) and np.array_equal(o["obs_ubs"][..., 0], after("obs_ubs")[..., 0])
    for b in range(B):                      # per environment: the rule's max|ref| is that of its own transition, as in the replay
        t = b + 1
        _close(env.pos_ubs[b].cpu(), f(t, "pos_ubs"), "pos_ubs", 1e-12)
        for k in FLOAT_FIELDS:
            _close(o[k][b], f(t, k), f"{case} env {b} {k}", errs=errs)
        _close(env.avg_rate[b].cpu(), f(t, "avg_rate"), "avg_rate", errs=errs)
        _close(env.run_f32[b].cpu(), [f(t, "total_throughput"), f(t, "avg_global_util"), f(t, "fair_idx"), f(t, "global_util")],
               "running scalars", errs=errs)
        _close(env.n_colls[b].cpu(), f(t, "n_colls"), "n_colls", 1e-12)
        _close(o["reward"][b], f(t, "reward"), "reward", errs=errs)
        _close(info["EpRet"][b].cpu(), f(t, "info:EpRet"), f"{case} env {b} EpRet", errs=errs)
        _close(info["ProbCollision"][b].cpu(), f(t, "info:ProbCollision"), f"{case} env {b} ProbCollision", errs=errs)
        made, skipped = _check_next_priorities(env.prior[b].cpu().numpy(), env.avg_rate[b].cpu().numpy(), f(t, "avg_rate"),
                                               f(t, "prior_next"), p.n_gts, (case, t))
        n_ranked, n_skipped = n_ranked + made, n_skipped + skipped
    print(f"{case} in one launch: rank checks made {n_ranked}, skipped {n_skipped}; errors {errs}")
    _log_row(case=case, launch=f"one for all {B}", errors=errs, rank_checked=n_ranked, rank_skipped=n_skipped,
             counts=edge_counts(z, case))
    assert n_ranked >= 100


@gpu
def test_plain_case_has_no_fairness_column_no_penalty_and_no_graph():
    """fair_service = avoid_collision = False (m64_plain): 4-column GT observations, 3 state features per GT, the reward is
    the scaled mean rate for every serving UBS - colliding ones included -, and the device graph builder, which compacts 4 GT
    features only, refuses the 3 this leaves with the library's error instead of returning a graph."""
    from uav_bs_ctrl_amd._lib import UavGnnError
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    z, p, steps = _case("m64_plain")
    f = lambda t, k: z[f"m64_plain:t{t}:{k}"]  # noqa: E731
    assert not p.fair_service and not p.avoid_collision
    n, M = p.n_ubs, p.n_gts
    env = BatchedUbsCoverageEnv(p, 1)
    env.reset(pos_ubs=f(0, "pos_ubs")[None], pos_gts=z["m64_plain:pos_gts"][None], prior=f(0, "prior_used")[None])
    assert env.out["obs_gt"].shape == (1, n, M, 4) and env.out["state"].shape == (1, 2 * n + 3 * M) == (1, env.state_dim)
    collided = 0
    for t in range(1, steps + 1):
        env.prior.copy_(th.as_tensor(f(t, "prior_used")[None]).to(th.int32))
        obs, rew, done, info = env.step(th.as_tensor(f(t, "actions")[None]).cuda())
        assert obs["gt"].shape == (1, n, M, 4) and f(t, "obs_gt").shape == (n, M, 4) and f(t, "state").shape == (2 * n + 3 * M,)
        # mubs_cov.py:329-335 from the fixture's rates: float32 mean, scaled in float32, divided in float64, idle UBSs get 0
        base = np.float32(p.reward_scale_rate) * f(t, "rate_per_gt").mean(dtype=np.float32)
        want = np.float64(base) / p.max_rate * (f(t, "rate_per_ubs") != 0)
        _close(want, f(t, "reward"), "the fixture's own reward is the non-fair base without penalties", 1e-6)
        _close(rew[0].cpu(), want, f"m64_plain t={t} reward")
        assert (rew[0].cpu().numpy() >= 0).all()
        collided += int(f(t, "mask_collision").sum())
    assert collided > 0, "the case must hold collisions for 'no penalty' to mean anything"
    assert float(done[0]) == 1.0
    with pytest.raises(UavGnnError, match="uavgnn_obs_compact"):
        env.graph()


def test_env_step_argument_errors_are_codes_never_a_launch():
    """No GPU needed: every call returns before it would launch (the addresses are made up and never dereferenced)."""
    import ctypes

    from uav_bs_ctrl_amd import _lib
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = _lib.UAVGNN_EINVAL, _lib.UAVGNN_EUNSUPPORTED
    fc = (ctypes.c_double * 18)(*([1.0] * 18))
    names = ("actions", "avail_moves", "pos_ubs", "pos_gts", "prior", "avg_rate", "t", "run_f32", "n_colls", "d_u2g", "d_u2u", "gt_ubs",
             "gt_rb", "rate_per_gt", "rate_per_ubs", "mask_collision", "reward", "done", "obs_gt", "obs_ubs", "obs_agent", "state")
    addr = {k: 0x100000 * (i + 1) for i, k in enumerate(names)}

    def step(n=8, M=80, R=5, A=9, B=1, ic="given", fc=fc, **ptrs):
        ic = (ctypes.c_int32 * 7)(n, M, R, A, 50, 1, 1) if ic == "given" else ic
        return lib.uavgnn_env_step(ic, fc, B, *[ptrs.get(k, addr[k]) for k in names], None)
    assert step(ic=None) == EINVAL and step(fc=None) == EINVAL
    for k in names[2:-1]:                                   # every required pointer; `state` is optional, actions mean "a step"
        assert step(**{k: None}) == EINVAL, k
    assert step(B=-1) == EINVAL
    assert step(avail_moves=None) == EINVAL, "actions without moves"
    for kw in (dict(n=0), dict(n=17), dict(M=0), dict(M=1025), dict(R=17), dict(R=0), dict(A=0), dict(n=16, M=1024)):
        assert step(**kw) == EUNSUPPORTED, kw
    assert step(B=0) == 0 and step(B=0, n=16, M=136, R=16) == 0
    assert step(B=0, n=16, M=1024) == EUNSUPPORTED, "the LDS limit is a property of the shape, not of the batch"


def test_edge_fixture_reaches_what_it_is_for():
    """The committed edge files, without a GPU: the counts `make_golden.py env_edges` printed are recomputed and held to the same
    minimums, so a regenerated fixture that reaches less fails here."""
    counts = {case: edge_counts(_fixture_of(case), case) for case in EDGE_CASES}
    for case, c in counts.items():
        print(case, c)
    check_edge_counts(counts)
    for name in FIXTURES[1:]:
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= EDGE_FIXTURE_MAX_BYTES, name
    z = _fixture_of("m64_plain")
    assert float(z["m64_plain:const:fair_service"]) == 0.0 and float(z["m64_plain:const:avoid_collision"]) == 0.0
    assert z["m64_plain:t1:obs_gt"].shape[-1] == 4
    assert sum(int(z[f"m64_plain:t{t}:mask_collision"].sum()) for t in range(1, int(z["m64_plain:steps"]) + 1)) > 0
    for case in EDGE_CASES[:-1]:
        assert float(_fixture_of(case)[f"{case}:const:fair_service"]) == 1.0, case
    # what the first five cases reach of the same events - why the edge cases exist
    old = {case: edge_counts(_fixture_of(case), case) for case in CASES}
    assert sum(c["non_nearest"] for c in old.values()) == 0 and max(c["n_gts"] for c in old.values()) <= 64


@gpu
def test_batched_environments_are_independent_and_feed_the_graph_builder():
    """B copies with different inputs in one launch == the same environments stepped one by one; the emitted padded
    observations go straight into the device graph builder (f3 -> f1) and the agent."""
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    z, p, steps = _case("8ubs_crowded")
    f = lambda t, k: z[f"8ubs_crowded:t{t}:{k}"]  # noqa: E731
    B = 5
    gen = th.Generator(device="cuda").manual_seed(0)
    shift = th.rand(B, 1, 2, device="cuda", generator=gen, dtype=th.float64) * 40
    shift[0] = 0
    pos_u = th.as_tensor(f(0, "pos_ubs")).cuda()[None] + shift
    pos_g = th.as_tensor(z["8ubs_crowded:pos_gts"]).cuda()[None].expand(B, -1, -1)
    prior = th.as_tensor(f(0, "prior_used")).cuda()[None].expand(B, -1)
    env = BatchedUbsCoverageEnv(p, B)
    env.reset(pos_u, pos_g, prior)
    singles = []
    for b in range(B):
        e1 = BatchedUbsCoverageEnv(p, 1)
        e1.reset(pos_u[b:b + 1], pos_g[b:b + 1], prior[b:b + 1])
        singles.append(e1)
    for t in range(1, 4):
        a = th.randint(0, env.n_actions, (B, p.n_ubs), device="cuda", generator=gen)
        env.step(a)
        for b, e1 in enumerate(singles):
            e1.step(a[b:b + 1])
            for k in ("gt_ubs", "gt_rb", "rate_per_gt", "reward", "obs_gt", "state"):
                assert th.equal(env.out[k][b], e1.out[k][0]), (t, b, k)
            assert th.equal(env.prior[b], e1.prior[0])
    # environment 0 follows the fixture while its priorities do (free-running: the kernel's own stable priorities)
    g = env.graph()
    assert g.num_nodes("agent") == B * p.n_ubs and g.graph_off.cpu().tolist() == list(range(0, B * p.n_ubs + 1, p.n_ubs))
    xs, off = g.relation_segments("seen")
    vis = env.out["obs_gt"][..., 0].sum(-1).reshape(-1).to(th.int32)
    assert th.equal(off[1:] - off[:-1], vis)


def edge_log_table(path=_EDGE_LOG):
    """env_sim_edges.jsonl (``_EDGE_LOG``) -> the text of profiles/env_sim_edges.txt (`python -m tests.test_env_sim [path]`)."""
    rows = [json.loads(line) for line in open(path)]
    quantities = sorted({k for r in rows for k in r["errors"]})
    events = ("non_nearest", "covered_unserved", "collision_flags", "multiply_covered", "done", "clipped_moves", "served")
    out = ["worst error / (max|ref| + |ref|) per quantity (bound 1e-5), rank checks made / skipped, event counts of the case", ""]
    for r in rows:
        c = r["counts"]
        out.append(f"{r['case']}  [{c['n_ubs']} x {c['n_gts']}, {c['n_rbs']} RBs; launches: {r['launch']}]")
        out.append("  errors  " + "  ".join(f"{k} {r['errors'][k]:.1e}" for k in quantities if k in r["errors"]))
        out.append(f"  ranks   checked {r['rank_checked']}  skipped {r['rank_skipped']}")
        out.append("  events  " + "  ".join(f"{k} {c[k]}" for k in events))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    import sys
    print(edge_log_table(*sys.argv[1:2]), end="")

"""`-m gpu`: trajectory films on the device (csrc/film.hip, uav_bs_ctrl_amd/film.py).

  1. a film slot is a COPY of the simulator's tensors at that step - bit-identical - for both simulators, B = 1 and B = 5 (episode
     base 5 of a 10-episode film), odd widths; unwritten slots keep the fill value; at the end of an episode the film agrees with
     ``info`` (cumulative reward = EpRet to 1e-12, last fair_idx = FairIdx exactly);
  2. the device films of the two cases of tests/golden/film_files.npz against the REFERENCE's recorder (pos_ubs at 1e-12, the rest at
     the 1e-5 rule of tests/test_env_sim.py), velocity = |avail_moves[a]| / dt to 1e-12;
  3. bounds: a click beyond the limit or beyond the film's episodes writes nothing and raises in ``check``; argument errors are codes;
  4. ``Evaluation(film=...)`` / ``GraphedEvaluation(film=...)``: the table and the training run are what they are without a film, the
     graphed film is the eager film over two calls;
  5. ``load_and_run_policy``."""
import os

import numpy as np
import pytest
import torch as th

import tests.test_eval_device_gpu as E
from tests.test_env_sim import _case, _close
from tests.test_film_host import CSV_FILES, film_arrays, film_npz
from tests.test_subs_env_host import ENV_CASES, env_case

pytestmark = pytest.mark.gpu

MUBS_CASES = ["debug", "v2_n16_m136", "v2_m65_r16"]        # 3 x 4; 16 UBSs x 136 GTs; 5 UBSs x 65 GTs: odd widths
SEED = E.SEED


def _film_bytes(film):
    return film.buf.clone()


def _mean_in_order(r):
    """[B, n] float64 -> the n values of a row added in agent order, divided by n."""
    s = np.zeros(r.shape[0], dtype=np.float64)
    for a in range(r.shape[1]):
        s = s + r[:, a]
    return s / np.float64(r.shape[1])


def _simulator(kind, case, B):
    """(env of B copies of the fixture's initial state, actions [steps, B, ...] int64: row 0 the fixture's, the others seeded)."""
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
    if kind == "mubs":
        z, p, steps = _case(case)
        env = BatchedUbsCoverageEnv(p, B)
    else:
        z, p, _, steps = env_case(case)
        env = BatchedSingleUbsCoverageEnv(p, B, seed=0)
    f = lambda t, k: z[f"{case}:t{t}:{k}"]  # noqa: E731
    rep = lambda a: np.repeat(np.asarray(a)[None], B, axis=0)  # noqa: E731
    env.reset(pos_ubs=rep(f(0, "pos_ubs")), pos_gts=rep(z[f"{case}:pos_gts"]), prior=rep(f(0, "prior_used")))
    acts = np.stack([rep(f(t, "actions")) for t in range(1, steps + 1)]).astype(np.int64)
    rs = np.random.RandomState(B)
    acts[:, 1:] = rs.randint(0, env.n_actions, acts[:, 1:].shape)
    return env, acts, steps


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("kind,case", [("mubs", c) for c in MUBS_CASES] + [("subs", c) for c in ENV_CASES])
def test_a_slot_is_a_copy_of_the_simulator(kind, case, B):
    from uav_bs_ctrl_amd.film import Film
    env, acts, steps = _simulator(kind, case, B)
    single, T, M = kind == "subs", env.episode_limit, env.n_gts
    episodes, base = 2 * B, (5 if B == 5 else 1)
    film = Film(env, episodes)
    mine = slice(base, base + B)
    film.reload(env, base)
    h = film.numpy()
    assert np.array_equal(h["pos_ubs"][mine, 0], env.pos_ubs.cpu().numpy()) and np.array_equal(h["pos_gts"][mine], env.pos_gts.cpu().numpy())
    assert np.isnan(h["pos_ubs"][mine, 1:]).all() and np.isnan(h["reward"]).all()
    series = [k for k in h if k not in ("pos_ubs", "pos_gts", "status")]
    moves = env.moves.cpu().numpy()
    info = None
    for t in range(1, steps + 1):
        a = th.as_tensor(acts[t - 1]).cuda()
        _, _, _, info = env.step(a)
        film.click(env, a, base)
        h = film.numpy()
        assert int(env.t[0]) == t
        assert np.array_equal(h["pos_ubs"][mine, t], env.pos_ubs.cpu().numpy()), (case, t, "pos_ubs")
        rew = env.out["reward"].cpu().numpy()
        if single:
            run = env.run_f64.cpu().numpy()
            assert np.array_equal(h["total_throughput"][mine, t - 1], run[:, 0]) and np.array_equal(h["fair_idx"][mine, t - 1], run[:, 2])
            assert np.array_equal(h["global_utility"][mine, t - 1], run[:, 3]) and np.array_equal(h["reward"][mine, t - 1], rew)
            assert np.array_equal(h["rate_per_gt"][mine, t - 1], env.out["rate_per_gt"].cpu().numpy())
            vel = np.hypot(*moves[acts[t - 1]].T) / env.p.dt
            assert np.all(np.abs(h["velocity"][mine, t - 1] - vel) <= 1e-12 * np.abs(vel)), (case, t, "velocity")
        else:
            assert np.array_equal(h["fair_idx"][mine, t - 1], env.run_f32[:, 2].cpu().numpy().astype(np.float64))
            assert np.array_equal(h["reward"][mine, t - 1], _mean_in_order(rew)), (case, t, "reward")
        # slots not yet written, and the episodes of other rounds, still hold the fill value
        assert np.isnan(h["pos_ubs"][mine, t + 1:]).all() and all(np.isnan(h[k][mine, t:]).all() for k in series)
        other = np.ones(episodes, dtype=bool)
        other[mine] = False
        assert all(np.isnan(h[k][other]).all() for k in h if k != "status")
    film.check()
    assert not np.isnan(h["pos_ubs"][mine, :steps + 1]).any() and np.array_equal(h["pos_gts"][mine], env.pos_gts.cpu().numpy())
    if B > 1:
        assert len({h["pos_ubs"][base + b].tobytes() for b in range(B)}) > 1, "the environments did not diverge"
    # ---- consistency with the metrics at the end of the episode ----------------------------------------------------------------------
    if steps == T:
        ep_ret = info["EpRet"].cpu().numpy()
        cum = np.zeros(B)
        for t in range(T):
            cum = cum + h["reward"][mine, t]
        assert np.all(np.abs(cum - ep_ret) <= 1e-12 * np.abs(ep_ret)), (cum, ep_ret)
        assert np.array_equal(h["fair_idx"][mine, T - 1], info["FairIdx"].cpu().numpy().astype(np.float64))
    else:
        assert case == "v2_m65_r16", "every other case runs to its limit"
    assert M > 0


def test_the_cases_cover_whole_episodes_of_both_simulators():
    assert _case("debug")[2] == _case("debug")[1].episode_limit and _case("v2_n16_m136")[2] == _case("v2_n16_m136")[1].episode_limit
    assert all(env_case(c)[3] == env_case(c)[1].episode_limit for c in ENV_CASES)
    assert (_case("v2_n16_m136")[1].n_ubs, _case("v2_m65_r16")[1].n_gts) == (16, 65)


# ---- 2. against the reference's recorder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mubs", "subs"])
def test_device_film_against_the_reference_recorder(case):
    from uav_bs_ctrl_amd.film import Film
    from uav_bs_ctrl_amd.sim import MAPS, BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv, SingleUbsParams
    z, ref = film_npz(), film_arrays(case)
    steps = int(z[f"{case}:steps"])
    if case == "mubs":
        env = BatchedUbsCoverageEnv(MAPS["debug"].params, 1)
    else:
        env = BatchedSingleUbsCoverageEnv(SingleUbsParams(n_grps=2, gts_per_grp=2), 1, seed=0)
    assert np.allclose(env.moves.cpu().numpy(), z[f"{case}:avail_moves"], atol=1e-9) and env.p.dt == float(z[f"{case}:dt"])
    film = Film(env, 1)
    env.reset(pos_ubs=z[f"{case}:pos_ubs0"][None], pos_gts=z[f"{case}:pos_gts"][None], prior=z[f"{case}:prior0"][None])
    film.reload(env, 0)
    for t in range(steps):
        env.prior.copy_(th.as_tensor(z[f"{case}:prior_used"][t][None]).to(th.int32))          # the reference's tie resolution
        a = th.as_tensor(z[f"{case}:actions"][t][None]).cuda()
        env.step(a)
        film.click(env, a, 0)
    film.check()
    ep = film.episode(0)
    assert set(ep) == set(ref) | {"pos_gts"}
    _close(ep["pos_ubs"][:steps + 1], ref["pos_ubs"], "pos_ubs", 1e-12)
    assert np.array_equal(ep["pos_gts"], z[f"{case}:pos_gts"].astype(np.float32))
    for k in ref:
        if k != "pos_ubs":
            _close(ep[k][:steps], ref[k], f"{case} {k}")
            print(f"{case} {k}: worst |got - ref| = {np.abs(ep[k][:steps] - ref[k]).max():.3e}")
            assert np.isnan(ep[k][steps:]).all()
    if case == "subs":
        moves, acts = z["subs:avail_moves"], z["subs:actions"]
        vel = np.linalg.norm(moves[acts], axis=1) / float(z["subs:dt"])
        assert np.all(np.abs(ep["velocity"][:steps] - vel) <= 1e-12 * np.abs(vel)) and (vel > 0).any() and (vel == 0).any()


# ---- 3. bounds and arguments ------------------------------------------------------------------------------------------------------------
def _bounds_setup(kind):
    from uav_bs_ctrl_amd.film import Film
    env, acts, _ = _simulator(kind, "debug" if kind == "mubs" else "short_rb", 2)
    film = Film(env, 2)
    film.reload(env, 0)
    a = th.as_tensor(acts[0]).cuda()
    env.step(a)
    film.click(env, a, 0)
    film.check()
    return env, film, a


@pytest.mark.parametrize("kind", ["mubs", "subs"])
def test_a_click_outside_the_film_writes_nothing_and_is_reported(kind):
    from uav_bs_ctrl_amd._lib import UavGnnError
    for what in ("beyond the limit", "negative step", "episode past the film", "second environment past the film"):
        env, film, a = _bounds_setup(kind)
        before = _film_bytes(film)
        T = env.episode_limit
        if what == "beyond the limit":            # the simulator is NOT stepped: only its counter is moved, on the device
            env.t.fill_(T + 1)
            film.click(env, a, 0)
        elif what == "negative step":
            env.t.fill_(-1)
            film.click(env, a, 0)
        elif what == "episode past the film":
            film.click(env, a, 2)
        else:                                      # episode 1 is inside (environment 0 records), episode 2 is not
            env.t.fill_(2)
            film.click(env, a, 1)
        after = _film_bytes(film)
        assert int(film.status) == 1, what
        if what == "second environment past the film":
            h = film.numpy()
            assert np.array_equal(h["pos_ubs"][1, 2], env.pos_ubs[0].cpu().numpy()) and not np.isnan(h["reward"][1, 1])
            film.fields["pos_ubs"][1, 2] = float("nan")             # undo environment 0's legitimate slot: the rest is untouched
            for k, v in film.fields.items():
                if k not in ("pos_ubs", "pos_gts"):
                    v[1, 1] = float("nan")
            after = _film_bytes(film)
        assert th.equal(after[8:], before[8:]), f"{what}: the film changed"
        with pytest.raises(UavGnnError, match="outside the film"):
            film.check()
    if kind == "subs":
        env, film, a = _bounds_setup(kind)
        before = _film_bytes(film)
        film.click(env, th.full_like(a, env.n_actions), 0)          # an action the move table does not hold
        assert int(film.status) == 1 and th.equal(_film_bytes(film)[8:], before[8:])
        film.status.zero_()
        film.click(env, th.full_like(a, -1), 0)
        assert int(film.status) == 1 and th.equal(_film_bytes(film)[8:], before[8:])
        film.status.zero_()
        film._launch(env, None, 0)                                  # a step slot without actions
        assert int(film.status) == 1 and th.equal(_film_bytes(film)[8:], before[8:])


def test_film_argument_errors_are_codes_never_a_launch():
    from uav_bs_ctrl_amd import _lib
    L = _lib.lib()
    buf = th.full((4096,), 7.0, dtype=th.float64, device="cuda")
    one = buf.data_ptr()
    EINVAL = _lib.UAVGNN_EINVAL
    good = [1, 3, 4, 10, 2, 0] + [one] * 10                         # B, n, M, T, episodes, episode_base, 10 pointers
    for i, bad in ((0, -1), (1, 0), (2, -1), (3, 0), (4, -1), (5, -1)):
        args = list(good)
        args[i] = bad
        assert L.uavgnn_film_click_mubs(*args, None) == EINVAL, (i, bad)
    for i in range(6, 16):
        args = list(good)
        args[i] = None
        assert L.uavgnn_film_click_mubs(*args, None) == EINVAL, i
    assert L.uavgnn_film_click_mubs(0, *good[1:], None) == 0          # B = 0: nothing to do
    good = [1, 4, 10, 5, 10.0, 2, 0] + [one] * 17                   # B, M, T, A, dt, episodes, episode_base, 17 pointers
    for i, bad in ((0, -1), (1, -1), (2, 0), (3, 0), (4, 0.0), (4, -1.0), (5, -1), (6, -1)):
        args = list(good)
        args[i] = bad
        assert L.uavgnn_film_click_subs(*args, None) == EINVAL, (i, bad)
    for i in range(7, 24):
        if i == 8:                                                  # actions may be NULL: the call after a reset
            continue
        args = list(good)
        args[i] = None
        assert L.uavgnn_film_click_subs(*args, None) == EINVAL, i
    assert L.uavgnn_film_click_subs(0, *good[1:], None) == 0
    th.cuda.synchronize()
    assert bool((buf == 7.0).all()), "a rejected call launched"


# ---- 4. the evaluation ------------------------------------------------------------------------------------------------------------------
def _host_side(learner):
    out = dict(params=learner.flat.flat.clone(), gen=learner._gen.get_state(), host=th.get_rng_state())
    for mn, m in learner.policy_net.named_modules():
        if isinstance(getattr(m, "rng_state", None), th.Tensor):
            out["comm." + mn] = m.rng_state.clone()
    return out


def _check_film_against_table(film, table, keys, T):
    h = film.numpy()
    film.check(h)
    assert not any(np.isnan(v).any() for v in h.values()), "an evaluation left a slot unwritten"
    t = {k: table[i].cpu().numpy() for i, k in enumerate(keys)}
    cum = np.zeros(film.episodes)
    for s in range(T):
        cum = cum + h["reward"][:, s]
    assert np.all(np.abs(cum - t["EpRet"]) <= 1e-12 * np.abs(t["EpRet"])) and np.array_equal(h["fair_idx"][:, T - 1], t["FairIdx"])
    assert (t["EpLen"] == T).all()


@pytest.mark.parametrize("name", list(E.SETUPS))
def test_evaluation_with_a_film_is_the_evaluation_without(name):
    from uav_bs_ctrl_amd.film import Film
    from uav_bs_ctrl_amd.graphs import Evaluation
    learner, _, _, kw, test_env = E.SETUPS[name]()
    env_a, env_b = test_env(), test_env()
    plain = Evaluation(learner, env_a, 8, eps=0.3, seed=SEED, enc=kw["enc"])
    film = Film(env_b, 8)
    filmed = Evaluation(learner, env_b, 8, eps=0.3, seed=SEED, enc=kw["enc"], film=film)
    for call in range(2):
        plain()
        side_a = _host_side(learner)
        filmed()
        side_b = _host_side(learner)
        assert th.equal(plain.table, filmed.table), f"call {call}: the film changed the table"
        assert side_a.keys() == side_b.keys() and all(th.equal(side_a[k], side_b[k]) for k in side_a)
        assert th.equal(plain.rng, filmed.rng) and not E._differences(E._sim_state(env_a), E._sim_state(env_b))
        _check_film_against_table(film, filmed.table, filmed.keys, env_b.episode_limit)
    with pytest.raises(ValueError, match="episodes"):
        Evaluation(learner, env_b, 4, enc=kw["enc"], film=film)


@pytest.mark.parametrize("name", list(E.SETUPS))
def test_graphed_evaluation_records_the_eager_film(name):
    from uav_bs_ctrl_amd.film import Film
    from uav_bs_ctrl_amd.graphs import Evaluation, GraphedEvaluation
    learner, _, _, kw, test_env = E.SETUPS[name]()
    env_e, env_g = test_env(), test_env()
    film_e, film_g = Film(env_e, 8), Film(env_g, 8)
    eager = Evaluation(learner, env_e, 8, eps=0.3, seed=SEED, enc=kw["enc"], film=film_e)
    graphed = GraphedEvaluation(learner, env_g, 8, eps=0.3, seed=SEED, enc=kw["enc"], film=film_g)
    assert int(film_g.status) == 0 and graphed.rng.tolist() == [SEED, 0]
    films = []
    for call in range(2):
        eager(), graphed()
        assert th.equal(eager.table, graphed.table), f"call {call}: the tables differ"
        assert th.equal(film_e.buf, film_g.buf), f"call {call}: the films differ"
        _check_film_against_table(film_g, graphed.table, graphed.keys, env_g.episode_limit)
        films.append(film_g.buf.clone())
    assert not th.equal(films[0], films[1]), "both replays recorded the same film: the counters are baked in"


@pytest.mark.parametrize("name", list(E.SETUPS))
def test_recording_evaluations_leave_the_training_run_untouched(name):
    from uav_bs_ctrl_amd.film import Film
    from uav_bs_ctrl_amd.graphs import Episode, Evaluation, GraphedEvaluation
    learner, env, rb, kw, _ = E.SETUPS[name]()
    plain = Episode(learner, env, rb, **kw)
    for _ in range(3):
        plain()
    want = E._train_state(learner, rb)
    learner, env, rb, kw, test_env = E.SETUPS[name]()       # seeded again: the same run, now with recording evaluations in between
    mixed = Episode(learner, env, rb, **kw)
    mixed()
    te = test_env()
    film = Film(te, 8)
    Evaluation(learner, te, 8, seed=5, enc=kw["enc"], film=film)()
    film.check()
    mixed()
    tg = test_env()
    film_g = Film(tg, 8)
    gev = GraphedEvaluation(learner, tg, 8, seed=5, enc=kw["enc"], film=film_g)
    gev(), gev()
    film_g.check()
    mixed()
    bad = E._differences(want, E._train_state(learner, rb))
    assert not bad, bad


# ---- 5. load_and_run_policy --------------------------------------------------------------------------------------------------------------
def _two_env_setup(name, seed):
    """The setups of tests/test_eval_device_gpu.py with a 2-environment evaluation simulator."""
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
    learner, env, _, kw, _ = (E._multi(seed=seed) if name == "multi-tarmac" else E._exp1(seed=seed))
    if name == "multi-tarmac":
        test_env = lambda: BatchedUbsCoverageEnv.from_map("debug", 2, seed=31)          # noqa: E731
    else:
        test_env = lambda: BatchedSingleUbsCoverageEnv(env.p, 2, seed=32)               # noqa: E731
    return learner, kw["enc"], test_env


def _same_policy(a, b):
    """The parameters a checkpoint carries (the flat buffer's alignment padding is not part of it)."""
    sa, sb = a.policy_net.state_dict(), b.policy_net.state_dict()
    return sa.keys() == sb.keys() and all(th.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("name", list(E.SETUPS))
def test_load_and_run_policy(name, tmp_path):
    from uav_bs_ctrl_amd.film import load_and_run_policy
    from uav_bs_ctrl_amd.graphs import Evaluation
    trained, enc, test_env = _two_env_setup(name, 3)
    gen = th.Generator(device="cuda").manual_seed(1)
    trained.flat.flat.add_(0.2 * th.randn(trained.flat.flat.shape, device="cuda", generator=gen))      # "trained": perturbed weights
    trained.invalidate_weight_cache()
    ckpt = str(tmp_path / "model.pt")
    trained.save_checkpoint(ckpt, dict(epoch=1))
    want = Evaluation(trained, test_env(), 4, eps=0.05, seed=9, enc=enc)()
    want = {k: v.cpu().numpy()[:3] for k, v in want.items()}
    got = {}
    for graphed in (False, True):
        fresh, _, _ = _two_env_setup(name, 77)                      # other initial weights: the result can only come from the checkpoint
        assert not _same_policy(fresh, trained)
        out_dir = tmp_path / ("graphed" if graphed else "eager")
        env = test_env()
        rsts = load_and_run_policy(ckpt, fresh, env, 3, output_dir=str(out_dir), eps=0.05, seed=9, enc=enc, graphed=graphed)
        assert _same_policy(fresh, trained), "the checkpoint was not loaded"
        assert list(rsts) == list(want)
        for k in want:
            assert rsts[k].dtype == np.float64 and rsts[k].shape == (3,) and np.array_equal(rsts[k], want[k]), (graphed, k)
        assert sorted(os.listdir(out_dir)) == ["episode0", "episode1", "episode2"]
        for k in range(3):
            d = out_dir / f"episode{k}"
            assert sorted(os.listdir(d)) == sorted(CSV_FILES)
            with open(d / "path_ubs.csv") as f:
                lines = f.read().splitlines()
            assert len(lines) == 3 + env.episode_limit + 1 and all(c != "" for c in lines[-1].split(","))
        got[graphed] = {k: {n: open(out_dir / f"episode{k}" / n, "rb").read() for n in CSV_FILES} for k in range(3)}
    assert got[False] == got[True], "the graphed and the eager run wrote other files"
    if name != "multi-tarmac":                                      # the debug map starts every episode from the same placement
        assert got[True][0]["pos_gts.csv"] != got[True][2]["pos_gts.csv"], "two rounds wrote the same placement"

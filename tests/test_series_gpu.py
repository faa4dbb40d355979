"""uav_bs_ctrl_amd/series.py on the GPU: a series of run directories evaluated through reused captured evaluations against the same
evaluations written by hand, one ``film.load_and_run_policy`` with fresh objects per run.  Every comparison is bit for bit: the same
kernels, the same seeds, no tolerance.

Sizes: the ``debug`` map (3 UBS x 4 GT, limit 10) and ``SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10)``, H = 32 with the
arguments of tests/run_args.py, 4 episodes on 2 evaluation environments (two rounds: the reset counter and the film's episode base
move).  The run directories are built once per module: two by real one-epoch ``Run``s (multi-UBS TarMAC, exp1 rnn), the others from a
freshly initialised learner's ``save_checkpoint`` (its weights perturbed, so that the policy depends on what it observes and hears) and a
written ``config.json`` - trained weights are not needed to compare evaluations.
One DiscreteComm checkpoint (disc/s1) carries a ``comm_rng_state`` as a trained one does, and one no-comm checkpoint (none_qmix) is saved
by a learner WITH a mixer, as the reference's QMIX arm saves it.

  1. ``test_series`` over two arms x two seeds + one reference-style directory against the hand-written evaluations
  2. one runner, several checkpoints: A, B, A again
  3. graphed against eager
  4. exp1 with both agents: no ProbCollision column
  5. the command line writes the function's files
  6. a ``none_qmix`` directory of the reference next to the plain arm: one capture, the mixer learner's own evaluation"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from tests.run_args import small_args
from tests.series_util import reference_text as _reference_text, run_text as _run_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT, EPISODES, ENVS = "checkpoint_epoch1.pt", 4, 2
FILM_FILES = ("others.csv", "path_ubs.csv", "pos_gts.csv")
KEYS = ("EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx", "ProbCollision")
DEBUG_KW = dict(map_id="debug", fair_service=True, avoid_collision=True)


def _p1():
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    return SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10)


def _args(arm):
    """Complete arguments of an arm: 'tarmac' / 'disc' / 'none' / 'none_qmix' (exp3 on the debug map), 'rnn' / 'gnn' (exp1)."""
    over = dict(epochs=1, save_freq=1)
    if arm in ("rnn", "gnn"):
        return "exp1", small_args("exp1", agent=arm, **over)
    if arm == "none_qmix":
        over.update(mixer=True, embed_dim=32, share_reward=True)
    return "exp3", small_args("exp3", c=None if arm.startswith("none") else arm, **over)


def _fresh(arm, torch_seed):
    """(learner with freshly initialised weights, enc, make_env(B, seed)) - nothing of uav_bs_ctrl_amd.series is used here."""
    from uav_bs_ctrl_amd import run as R
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner, QLearner
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv
    exp, args = _args(arm)
    ns = R.check_args(exp, args)
    th.manual_seed(torch_seed)
    if exp == "exp1":
        make = lambda B, seed: BatchedSingleUbsCoverageEnv(_p1(), B, seed=seed)             # noqa: E731
        return QLearner(make(ENVS, 0).get_env_info(arm), ns), arm, make
    make = lambda B, seed: BatchedUbsCoverageEnv.from_map("debug", B, seed=seed)             # noqa: E731
    return MultiAgentQLearner(make(ENVS, 0).get_env_info("gnn"), ns), "gnn", make


def _crafted(path, arm, seed, exp_name, kind="crafted"):
    """A run directory without a run: the checkpoint of a fresh learner with perturbed weights and the ``config.json`` ``Run.create``
    would write.
    kind 'noise': the checkpoint carries a ``comm_rng_state`` some way into its stream, as a trained DiscreteComm checkpoint does.
    kind 'qmix': the learner has a mixer and the ``config.json`` is the reference's (``Run`` trains no mixer)."""
    from uav_bs_ctrl_amd.run import comm_modules, seed_comm_modules
    exp, args = _args(arm)
    os.makedirs(path)
    learner = _fresh(arm, 100 + seed)[0]
    # away from the initialisation, where the greedy action hardly depends on the observation or on the messages (tests/test_film_gpu.py)
    gen = th.Generator(device="cuda").manual_seed(100 + seed)
    learner.flat.flat.add_(0.2 * th.randn(learner.flat.flat.shape, device="cuda", generator=gen))
    learner.invalidate_weight_cache()
    if kind == "noise":
        seed_comm_modules(learner, 4242)
        for _, m in comm_modules(learner):
            m.rng_state[1:].fill_(17)
    learner.save_checkpoint(os.path.join(path, CKPT), dict(epoch=1, t=0))
    ck = th.load(os.path.join(path, CKPT), map_location="cpu")
    assert ("comm_rng_state" in ck) == (kind == "noise") and ("mixer_state_dict" in ck) == (kind == "qmix")
    with open(os.path.join(path, "config.json"), "w") as f:
        if kind == "qmix":
            f.write(_reference_text("MultiUbsCoverageEnv", DEBUG_KW, dict(args, device="cuda:0"), seed=seed, exp_name=exp_name))
        else:
            f.write(_run_text(exp, _p1() if exp == "exp1" else "debug", args, seed, exp_name))


def _trained(path, arm, seed, exp_name):
    """A run directory of a real one-epoch ``Run``."""
    from uav_bs_ctrl_amd.run import Run
    exp, args = _args(arm)
    Run.create(exp, _p1() if exp == "exp1" else "debug", args, path, exp_name=exp_name, seed=seed, n_envs=4, n_test_envs=ENVS).train()
    assert os.path.exists(os.path.join(path, CKPT))


def _by_hand(arm, ckpt, seed, out_dir, graphed=True, reseed_after_load=False):
    """The evaluation of one run as a user writes it today: fresh simulator, fresh learner (for none_qmix: one WITH a mixer, which
    alone loads that checkpoint), ``load_and_run_policy``.  reseed_after_load: ``load_and_run_policy`` written out, with the comm pairs
    seeded AFTER ``load_checkpoint`` - the expectation for a checkpoint that carries a ``comm_rng_state``."""
    from uav_bs_ctrl_amd.film import Film, load_and_run_policy
    from uav_bs_ctrl_amd.graphs import GraphedEvaluation
    from uav_bs_ctrl_amd.run import derive_seeds, seed_comm_modules
    seeds = derive_seeds(seed)
    learner, enc, make = _fresh(arm, 999)
    env = make(ENVS, seeds["test_env"])
    if not reseed_after_load:
        if arm == "disc":
            seed_comm_modules(learner, seeds["comm"])
        return load_and_run_policy(ckpt, learner, env, EPISODES, output_dir=out_dir, eps=0.05, seed=seeds["evaluation"], enc=enc,
                                   graphed=graphed)
    learner.load_checkpoint(ckpt)
    seed_comm_modules(learner, seeds["comm"])
    film = Film(env, EPISODES)
    ev = GraphedEvaluation(learner, env, EPISODES, eps=0.05, seed=seeds["evaluation"], enc=enc, film=film)
    ev()
    table, host = ev.table.cpu().numpy(), film.numpy()
    film.check(host)
    for k in range(EPISODES):
        film.write(os.path.join(out_dir, f"episode{k}"), k, host=host)
    return {key: np.array(table[i], dtype=np.float64) for i, key in enumerate(ev.keys)}


def _films(d):
    return {(k, n): open(os.path.join(d, f"episode{k}", n), "rb").read() for k in range(EPISODES) for n in FILM_FILES}


def _same(a, b):
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


# (arm, exp_name, seed, directory under the log root, kind)
RUNS = (("tarmac", "tarmac", 0, "exp3_tarmac/s0", "trained"), ("tarmac", "tarmac", 1, "exp3_tarmac/s1", "crafted"),
        ("disc", "disc", 0, "exp3_disc/s0", "crafted"), ("disc", "disc", 1, "exp3_disc/s1", "noise"),
        ("tarmac", "tarmac", 7, "reference/exp3_tarmac_s7", "reference"),
        ("rnn", "exp1_rnn", 2, "exp1_rnn/s2", "trained"), ("gnn", "exp1_gnn", 3, "exp1_gnn/s3", "crafted"),
        ("none", "none", 0, "exp3_none/s0", "crafted"), ("none_qmix", "none_qmix", 4, "exp3_none_qmix/s4", "qmix"))
MULTI_LOGDIRS, EXP1_LOGDIRS, QMIX_LOGDIRS = ("exp3_tarmac", "exp3_disc", "reference"), ("exp1_rnn", "exp1_gnn"), ("exp3_none", "exp3_none_qmix")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """{root, want: {directory: (table, films) of the hand-written evaluation}} - built once, read by every test."""
    root = str(tmp_path_factory.mktemp("series"))
    want = {}
    for arm, exp_name, seed, rel, kind in RUNS:
        path = os.path.join(root, "logs", rel)
        if kind == "trained":
            _trained(path, arm, seed, exp_name)
        elif kind in ("crafted", "noise", "qmix"):
            _crafted(path, arm, seed, exp_name, kind)
        else:                       # the reference's logger: no uav_bs_ctrl_amd key, the device it trained on; the trained run's checkpoint
            os.makedirs(path)
            shutil.copy(os.path.join(root, "logs", "exp3_tarmac/s0", CKPT), os.path.join(path, CKPT))
            with open(os.path.join(path, "config.json"), "w") as f:
                f.write(_reference_text("MultiUbsCoverageEnv", DEBUG_KW, dict(_args(arm)[1], device="cpu"), seed=seed, exp_name=exp_name))
        out = os.path.join(root, "by_hand", rel)
        want[rel] = (_by_hand(arm, os.path.join(path, CKPT), seed, out, reseed_after_load=kind == "noise"), _films(out))
    return dict(root=root, want=want)


def _logdirs(world, names):
    return [os.path.join(world["root"], "logs", n) for n in names]


@pytest.fixture(scope="module")
def multi_series(world):
    from uav_bs_ctrl_amd import series as S
    out = os.path.join(world["root"], "out_multi")
    return S.test_series(list(KEYS), _logdirs(world, MULTI_LOGDIRS), CKPT, EPISODES, out, n_envs=ENVS), out


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_hand_written_evaluations_tell_the_runs_apart(world):
    """What the comparisons below can see: seeds, arms and checkpoints all move the result."""
    w = world["want"]
    assert not _same(w["exp3_tarmac/s0"][0], w["exp3_tarmac/s1"][0]) and not _same(w["exp3_disc/s0"][0], w["exp3_disc/s1"][0])
    assert not _same(w["exp3_tarmac/s0"][0], w["reference/exp3_tarmac_s7"][0]), "one checkpoint, two seeds"
    assert all(np.isfinite(t[k]).all() and t[k].shape == (EPISODES,) for t, _ in w.values() for k in t)
    assert not _same(w["exp3_none/s0"][0], w["exp3_none_qmix/s4"][0])


def test_a_checkpoints_own_noise_state_is_not_the_seeded_one(world, tmp_path):
    """disc/s1 carries a ``comm_rng_state``: ``load_and_run_policy`` continues from it, the series seeds the noise from the run's seed
    (the expectation held in ``world``) - the two differ, so the comparisons below see which of them the runner does."""
    ckpt = os.path.join(world["root"], "logs", "exp3_disc/s1", CKPT)
    continued = _by_hand("disc", ckpt, 1, str(tmp_path / "continued"))
    assert not _same(continued, world["want"]["exp3_disc/s1"][0]) or _films(str(tmp_path / "continued")) != world["want"]["exp3_disc/s1"][1]


def test_series_against_hand_written_evaluations(world, multi_series):
    rsts, out = multi_series
    assert rsts["runs"] == 5 and rsts["captures"] == 2, (rsts["runs"], rsts["captures"])
    visit = [r for r in RUNS if r[3].split("/")[0] in MULTI_LOGDIRS]
    assert [os.path.relpath(d, os.path.join(world["root"], "logs")) for d in rsts["run_dirs"]] == [r[3] for r in visit]
    assert list(rsts["dataset"]) == ["tarmac", "disc"]
    for exp_name, table in rsts["dataset"].items():
        parts = [world["want"][rel][0] for _, name, _, rel, _ in visit if name == exp_name]
        assert list(table) == list(KEYS)
        for k in KEYS:
            want = np.concatenate([p[k] for p in parts])
            assert table[k].dtype == np.float64 and np.array_equal(table[k], want), (exp_name, k, table[k], want)
    for _, exp_name, seed, rel, _ in visit:
        assert _films(os.path.join(out, f"{exp_name}_seed{seed}")) == world["want"][rel][1], f"{rel}: the films differ"
    with open(rsts["summary"]) as f:
        lines = f.read().splitlines()
    assert lines[0].split(",")[:3] == ["metric", "AvgGlobalUtility", "AvgGlobalUtility"] and lines[1].split(",")[:3] == ["exp_name", "disc", "tarmac"]
    assert len(lines) == 2 + 3 * EPISODES and lines[2 + 2 * EPISODES].split(",")[1] == "", "disc has two seeds, tarmac three"
    assert lines[2].split(",")[2] == repr(float(rsts["dataset"]["tarmac"]["AvgGlobalUtility"][0]))
    assert os.path.getsize(rsts["summary_t"]) > 0
    try:
        import matplotlib  # noqa: F401
        assert os.path.getsize(rsts["figure"]) > 0
    except ImportError:
        assert rsts["figure"] is None and "matplotlib" in rsts["figure_skipped"]


# ---- 2, 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["tarmac", "disc"])
def test_one_runner_several_checkpoints(world, arm, tmp_path):
    """A, B, A again: the second A is the first A and what a fresh runner - and the hand-written evaluation - gives for A."""
    from uav_bs_ctrl_amd import series as S
    from uav_bs_ctrl_amd.run import comm_modules
    a, b = (r for r in RUNS if r[0] == arm and r[4] != "reference")
    dirs = [os.path.join(world["root"], "logs", r[3]) for r in (a, b)]
    runner = S.PolicyRunner(S.describe(dirs[0]), EPISODES, n_envs=ENVS)
    held = [m.rng_state.data_ptr() for _, m in comm_modules(runner.learner)]
    assert (len(held) > 0) == (arm == "disc")
    got = [runner(os.path.join(d, CKPT), r[2], str(tmp_path / f"call{i}")) for i, (d, r) in enumerate(((dirs[0], a), (dirs[1], b), (dirs[0], a)))]
    assert runner.calls == 3
    assert _same(got[0], world["want"][a[3]][0]) and _same(got[1], world["want"][b[3]][0]), "a reused runner is not the hand-written evaluation"
    assert _same(got[2], got[0]), "what the runner evaluated before changed its result"
    assert _films(str(tmp_path / "call2")) == world["want"][a[3]][1] and _films(str(tmp_path / "call1")) == world["want"][b[3]][1]
    fresh = S.PolicyRunner(S.describe(dirs[0]), EPISODES, n_envs=ENVS)(os.path.join(dirs[0], CKPT), a[2])
    assert _same(fresh, got[2])
    assert [m.rng_state.data_ptr() for _, m in comm_modules(runner.learner)] == held, "a comm rng_state was replaced, not copied into"


@pytest.mark.parametrize("arm", ["tarmac", "disc", "rnn"])
def test_the_eager_runner_is_the_graphed_runner(world, arm, tmp_path):
    from uav_bs_ctrl_amd import series as S
    from uav_bs_ctrl_amd.graphs import Evaluation, GraphedEvaluation
    a, b = [r for r in RUNS if r[0] == arm and r[4] != "reference"][0], [r for r in RUNS if r[0] == arm][-1]
    d = os.path.join(world["root"], "logs", a[3])
    eager, graphed = (S.PolicyRunner(S.describe(d), EPISODES, n_envs=ENVS, graphed=g) for g in (False, True))
    assert type(eager.evaluation) is Evaluation and type(graphed.evaluation) is GraphedEvaluation
    for i, r in enumerate((a, b, a)):
        ckpt = os.path.join(world["root"], "logs", r[3], CKPT)
        e, g = eager(ckpt, r[2], str(tmp_path / f"e{i}")), graphed(ckpt, r[2], str(tmp_path / f"g{i}"))
        assert _same(e, g) and _same(e, world["want"][r[3]][0]), (arm, i)
        assert _films(str(tmp_path / f"e{i}")) == _films(str(tmp_path / f"g{i}")) == world["want"][r[3]][1]


def test_a_runner_refuses_environments_that_do_not_divide_the_episodes(world):
    from uav_bs_ctrl_amd import series as S
    with pytest.raises(ValueError, match="must divide"):
        S.PolicyRunner(S.describe(os.path.join(world["root"], "logs", "exp3_tarmac/s0")), 4, n_envs=3)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
def test_an_exp1_series_has_no_collision_column(world, tmp_path):
    from uav_bs_ctrl_amd import series as S
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="ProbCollision"):
        S.test_series(["EpRet", "ProbCollision"], _logdirs(world, EXP1_LOGDIRS), CKPT, EPISODES, out, n_envs=ENVS)
    assert not os.path.exists(out)
    metrics = ["EpRet", "AvgGlobalUtility", "TotalThroughput", "FairIdx"]          # test_policies.py:113
    rsts = S.test_series(metrics, _logdirs(world, EXP1_LOGDIRS), CKPT, EPISODES, out, n_envs=ENVS)
    assert rsts["runs"] == 2 and rsts["captures"] == 2 and list(rsts["dataset"]) == ["exp1_rnn", "exp1_gnn"]
    for exp_name, rel in (("exp1_rnn", "exp1_rnn/s2"), ("exp1_gnn", "exp1_gnn/s3")):
        assert list(rsts["dataset"][exp_name]) == list(KEYS[:-1])
        assert _same(rsts["dataset"][exp_name], world["want"][rel][0]), exp_name
        assert _films(os.path.join(out, f"{exp_name}_seed{rel[-1]}")) == world["want"][rel][1]
    for name in ("test_summary.csv", "test_summary_t.csv"):
        with open(os.path.join(out, name)) as f:
            text = f.read()
        assert "ProbCollision" not in text and "exp1_gnn" in text
    with open(rsts["summary"]) as f:
        assert f.readline().rstrip("\n").split(",") == ["metric"] + [m for m in sorted(metrics) for _ in range(2)]


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_command_line_writes_the_functions_files(world, multi_series, tmp_path):
    rsts, _ = multi_series
    out = str(tmp_path / "cli")
    cmd = [sys.executable, "-m", "uav_bs_ctrl_amd.series", "--logdirs", *_logdirs(world, MULTI_LOGDIRS), "--checkpoint", CKPT, "--episodes",
           str(EPISODES), "--envs", str(ENVS), "--metrics", *KEYS, "--out", out]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "5 runs of 2 experiments, 2 evaluations built" in done.stdout
    for key, name in (("summary", "test_summary.csv"), ("summary_t", "test_summary_t.csv")):
        with open(rsts[key], "rb") as f, open(os.path.join(out, name), "rb") as g:
            assert f.read() == g.read(), name


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_none_qmix_directory_is_evaluated_on_the_plain_arms_capture(world, tmp_path):
    """The reference's QMIX arm: a checkpoint whose optimiser state and ``mixer_state_dict`` belong to a learner with a mixer, a
    ``config.json`` with ``mixer: true`` - evaluated without a mixer, on the capture the plain no-comm arm built, to what a learner
    WITH the mixer gives by hand."""
    from uav_bs_ctrl_amd import series as S
    out = str(tmp_path / "out")
    rsts = S.test_series(list(KEYS), _logdirs(world, QMIX_LOGDIRS), CKPT, EPISODES, out, n_envs=ENVS)
    assert rsts["runs"] == 2 and rsts["captures"] == 1 and list(rsts["dataset"]) == ["none", "none_qmix"]
    for exp_name, seed, rel in (("none", 0, "exp3_none/s0"), ("none_qmix", 4, "exp3_none_qmix/s4")):
        assert _same(rsts["dataset"][exp_name], world["want"][rel][0]), exp_name
        assert _films(os.path.join(out, f"{exp_name}_seed{seed}")) == world["want"][rel][1], exp_name

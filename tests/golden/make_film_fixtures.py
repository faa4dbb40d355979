#!/usr/bin/env python
"""Generates tests/golden/film_files.npz: what the REFERENCE's trajectory recorders hold and write for one episode of each
simulator (envs/mubs_cov/recorder.py, envs/subs_cov/recorder.py, envs/common.py:80-100 ``write_to_disk``), by running the reference's
own modules, imported unchanged from /root/reference over oracle/gym_standin, on the CPU with matplotlib's Agg backend.  Skips when
the reference is not on this machine.  The fixture is data only, a few KB.

    python tests/golden/make_film_fixtures.py

Cases (both stepped with seeded random actions):
  mubs   ``MultiUbsCoverageEnv('debug', record=True)``: 3 UBSs x 4 GTs, a whole episode of 10 steps
  subs   ``SingleUbsCoverageEnv(n_grps=2, gts_per_grp=2, record=True)``: 12 steps

Per case:  <case>:pos_ubs0 / pos_gts / prior0   the initial state (prior0: the permutation ``reset`` drew, recovered by replaying the
                                                RNG stream as tests/golden/make_golden.py does - the transmission overwrites it)
           <case>:actions                       [steps, n] / [steps] int64
           <case>:prior_used                    [steps, M]: the GT priorities each step used (``np.argsort`` is not a stable sort: a
                                                replay feeds the reference's own tie resolution, as tests/test_env_sim.py does)
           <case>:avail_moves, <case>:dt, <case>:steps
           <case>:film:<key>                    every array the recorder held, stacked (pos_ubs [steps+1, ...])
           <case>:csv:<file>                    the bytes of path_ubs.csv, pos_gts.csv, others.csv that ``replay(save_dir=...)`` wrote
The PNG the recorder also writes is not stored."""
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
CSV_FILES = ("path_ubs.csv", "pos_gts.csv", "others.csv")
MUBS_SEED, SUBS_SEED, SUBS_STEPS = 1, 7, 12


def _store(out, case, env, pos_ubs0, prior0, actions, prior_used):
    out[f"{case}:pos_ubs0"] = np.asarray(pos_ubs0, dtype=np.float64)
    out[f"{case}:pos_gts"] = np.asarray(env.pos_gts)
    out[f"{case}:prior0"] = np.asarray(prior0, dtype=np.int32)
    out[f"{case}:actions"] = np.asarray(actions, dtype=np.int64)
    out[f"{case}:prior_used"] = np.asarray(prior_used, dtype=np.int32)
    out[f"{case}:avail_moves"] = np.asarray(env.avail_moves, dtype=np.float64)
    out[f"{case}:dt"] = np.array(env.dt, dtype=np.float64)
    out[f"{case}:steps"] = np.array(len(actions))
    film = env.recorder.film
    for k, v in film.items():
        out[f"{case}:film:{k}"] = np.stack(v) if k in ("pos_ubs", "rate_per_gt") else np.asarray(v)
    with tempfile.TemporaryDirectory() as tmp:
        env.recorder.replay(save_dir=tmp)
        assert os.path.getsize(os.path.join(tmp, "trajectories.png")) > 0
        for name in CSV_FILES:
            with open(os.path.join(tmp, name), "rb") as f:
                out[f"{case}:csv:{name}"] = np.frombuffer(f.read(), dtype=np.uint8)
    print(f"{case}: steps={len(actions)} film keys={sorted(film)} csv bytes=" + str([int(out[f'{case}:csv:{n}'].size) for n in CSV_FILES]))


def make_mubs(out):
    from envs.mubs_cov.maps import MAPS
    from envs.mubs_cov.mubs_cov import MultiUbsCoverageEnv
    np.random.seed(MUBS_SEED), random.seed(MUBS_SEED)
    env = MultiUbsCoverageEnv("debug", record=True)
    env.reset()
    pos_ubs0 = np.asarray(env.pos_ubs, dtype=np.float64).copy()
    np.random.seed(MUBS_SEED), random.seed(MUBS_SEED)
    twin = MultiUbsCoverageEnv("debug", record=False)
    positions = MAPS["debug"].set_positions()
    prior0 = np.random.permutation(twin.n_gts)
    assert np.array_equal(np.asarray(positions["gt"]), np.asarray(env.pos_gts))
    rng = np.random.default_rng(100 + MUBS_SEED)
    actions, prior_used = [], []
    for _ in range(env.episode_limit):
        prior_used.append(env.prior_gts.copy())
        a = rng.integers(0, env.n_actions, env.n_ubs)
        _, _, _, done, _ = env.step(list(a))
        actions.append(a)
    assert done, "the episode did not end at its limit"
    _store(out, "mubs", env, pos_ubs0, prior0, actions, prior_used)


def make_subs(out):
    from envs.subs_cov.subs_cov import SingleUbsCoverageEnv
    kw = dict(n_grps=2, gts_per_grp=2)
    np.random.seed(SUBS_SEED), random.seed(SUBS_SEED)
    env = SingleUbsCoverageEnv(record=True, **kw)
    env.reset()
    pos_ubs0 = np.asarray(env.pos_ubs, dtype=np.float64).copy()
    np.random.seed(SUBS_SEED), random.seed(SUBS_SEED)
    twin = SingleUbsCoverageEnv(record=False, **kw)
    twin._set_position()
    prior0 = np.random.permutation(twin.n_gts)
    assert np.array_equal(twin.pos_gts, env.pos_gts)
    rng = np.random.default_rng(100 + SUBS_SEED)
    actions, prior_used = [], []
    for _ in range(SUBS_STEPS):
        prior_used.append(env.prior_gts.copy())
        a = int(rng.integers(0, env.n_actions))
        env.step(a)
        actions.append(a)
    assert len(set(actions)) > 2 and 0 in actions, "the actions should hover at least once and move in several directions"
    _store(out, "subs", env, pos_ubs0, prior0, actions, prior_used)


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "envs", "subs_cov")):
        print("[make_film_fixtures] reference not found: skipped")
        sys.exit(0)
    import matplotlib
    matplotlib.use("Agg")
    sys.path[:0] = [os.path.join(ROOT, "oracle", "gym_standin"), REF, ROOT]
    out = {}
    make_mubs(out)
    make_subs(out)
    path = os.path.join(HERE, "film_files.npz")
    np.savez_compressed(path, **out)
    print(f"film_files -> {os.path.getsize(path)} B")

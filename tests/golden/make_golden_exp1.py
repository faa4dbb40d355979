#!/usr/bin/env python
"""Generates the fixtures of experiment 1 (single-UBS environment + DRQN) by running the REFERENCE's own modules, imported
unchanged from /root/reference over oracle/dgl_standin + oracle/gym_standin, on the CPU.  Skips when the reference is not on this
machine.  Fixtures are data only.

    python tests/golden/make_golden_exp1.py [env] [learner] [sampler]        (no argument: all three)

env_subs_cov.npz            envs/subs_cov/subs_cov.py stepped by a seeded policy, five cases; per case the constants, avail_moves,
                            pos_gts and, for every transition t = 0 (reset) ... T: actions, pos_ubs, prior_used, prior_next, d_u2g,
                            sched, rate_per_gt, avg_rate, the four running scalars, reward, done, BadMask, obs_gt, obs_agent.
learner_update_drqn.npz     algos/drqn/learner.py QLearner (agent 'gnn', H = 32, 4 heads, float64) on `exp1_g2`: the raw arguments
                            of every ``cache`` call of a 36-step rollout, the sequences its buffer stored, and one ``update`` on
                            B = 4 sequences of T = 6 (indices, loss, QVals, gradients, parameters and target parameters after it).
subs_sampler_stats.npz      histograms (tests/subs_sampler_ref.py ``histograms``) of 20 000 seeded draws of what ``reset`` draws -
                            ``_set_position`` then ``np.random.permutation``, in reset's order - for (n_grps, gts_per_grp) =
                            (2, 5) and (4, 5).
"""
import os
import random
import sys
import types

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

ENV_CASES = [  # case, environment arguments, T
    ("exp1_g2", dict(n_grps=2, gts_per_grp=5, episode_limit=24), 24),
    ("exp1_g4", dict(n_grps=4, gts_per_grp=5, episode_limit=24), 24),
    ("short_rb", dict(n_grps=2, gts_per_grp=5, n_rbs=2, episode_limit=16), 16),
    ("two_speeds", dict(n_grps=3, gts_per_grp=4, n_rbs=3, vels=[5, 10], r_cov=150, episode_limit=20), 20),
    ("m65", dict(n_grps=5, gts_per_grp=13, n_rbs=4, r_cov=300, episode_limit=8), 8),
]
SHORTAGE_CASES = ("short_rb", "two_speeds", "m65")
ENV_SEED = 7


def policy(env, rng):
    """Head for GT 0 with the best-aligned move, hover within 40 m of it; with probability 0.3 a seeded random action."""
    if rng.uniform() < 0.3:
        return int(rng.integers(0, env.n_actions))
    to = env.pos_gts[0].astype(np.float64) - np.asarray(env.pos_ubs, dtype=np.float64)
    if np.hypot(*to) <= 40.0:
        return 0
    return 1 + int(np.argmax(env.avail_moves[1:] @ to))


def make_env_golden():
    from envs.subs_cov.subs_cov import SingleUbsCoverageEnv
    out = {}
    for case, kw, T in ENV_CASES:
        np.random.seed(ENV_SEED), random.seed(ENV_SEED)
        env = SingleUbsCoverageEnv(record=False, **kw)
        env.reset()
        # the permutation reset() drew is overwritten by the reset-time transmission: recover it from the same stream
        np.random.seed(ENV_SEED), random.seed(ENV_SEED)
        twin = SingleUbsCoverageEnv(record=False, **kw)
        twin._set_position()
        perm0 = np.random.permutation(twin.n_gts)
        assert np.array_equal(twin.pos_gts, env.pos_gts)
        consts = dict(n_gts=env.n_gts, n_grps=env.n_grps, gts_per_grp=env.gts_per_grp, n_rbs=env.n_rbs, n_dirs=4,
                      range_pos=float(env.range_pos), r_cov=float(env.r_cov), dt=float(env.dt), episode_limit=int(env.episode_limit),
                      reward_scale_rate=float(env.reward_scale_rate), max_rate=float(env.max_rate), p_tx=float(env.p_tx),
                      n0=float(env.n0), bw=float(env.bw), fc=float(env.fc), h_ubs=float(env.h_ubs), a=float(env.chan.a),
                      b=float(env.chan.b), eta_los=float(env.chan.eta_los), eta_nlos=float(env.chan.eta_nlos))
        for k, v in consts.items():
            out[f"{case}:const:{k}"] = np.array(v, dtype=np.float64)
        out[f"{case}:vels"] = np.atleast_1d(np.asarray(kw.get("vels", 10), dtype=np.float64))
        out[f"{case}:avail_moves"] = np.asarray(env.avail_moves, dtype=np.float64)
        out[f"{case}:pos_gts"] = np.asarray(env.pos_gts, dtype=np.float32)

        def snap(t, action, prior_used, reward, done, bad):
            obs = env.get_obs()
            rec = dict(actions=np.int64(action), prior_used=np.asarray(prior_used, dtype=np.int32),
                       pos_ubs=np.asarray(env.pos_ubs, dtype=np.float64), d_u2g=np.asarray(env.d_u2g),
                       sched=np.asarray(env.sched, dtype=np.int32), rate_per_gt=np.asarray(env.rate_per_gt, dtype=np.float64),
                       avg_rate=np.asarray(env.aver_rate_per_gt, dtype=np.float64), total_throughput=np.float64(env.total_throughput),
                       avg_global_util=np.float64(env.avg_global_util), fair_idx=np.float64(env.fair_idx),
                       global_util=np.float64(env.global_util), prior_next=np.asarray(env.prior_gts, dtype=np.int32),
                       reward=np.float64(reward), done=np.float64(done), BadMask=np.float64(bad), obs_gt=obs["gt"],
                       obs_agent=obs["agent"])
            for k, v in rec.items():
                out[f"{case}:t{t}:{k}"] = np.asarray(v)
        snap(0, 0, perm0, 0.0, 0.0, 0.0)
        rng = np.random.default_rng(100 + ENV_SEED)
        served = shortage = unserved = 0
        for t in range(1, T + 1):
            prior_used = env.prior_gts.copy()
            a = policy(env, rng)
            _, r, d, info = env.step(a)
            snap(t, a, prior_used, r, d, info["BadMask"])
            covered = int((env.d_u2g <= env.r_cov).sum())
            served += int(env.sched.sum())
            shortage += covered > env.n_rbs
            unserved += covered - int(env.sched.sum())
        out[f"{case}:steps"] = np.array(T)
        # what makes the case worth having
        assert served >= 1, f"{case}: no GT was ever served"
        assert d and info["BadMask"], f"{case}: the episode did not end at its limit"
        assert case not in SHORTAGE_CASES or shortage >= 5, f"{case}: only {shortage} steps with more covered GTs than RBs"
        print(f"env[{case}]: M={env.n_gts} rbs={env.n_rbs} transitions={T + 1} served GT-steps={served} shortage steps={shortage} "
              f"covered-but-unserved GT-steps={unserved}")
    path = os.path.join(HERE, "env_subs_cov.npz")
    np.savez_compressed(path, **out)
    print(f"env_subs_cov -> {os.path.getsize(path)} B")


def make_learner_golden():
    from algos.drqn.learner import QLearner
    from algos.drqn.utils.env_wrappers import Wrapper
    from envs.subs_cov.subs_cov import SingleUbsCoverageEnv
    from oracle.closed_form import fill_closed_form
    th.set_default_dtype(th.float64)
    T, B, STEPS = 6, 4, 36
    args = types.SimpleNamespace(device="cpu", agent="gnn", hidden_size=32, n_heads=4, n_layers=2, max_seq_len=T, gamma=0.99,
                                 polyak=0.995, batch_size=B, replay_size=100, lr=5e-4, anneal_lr=False)
    np.random.seed(41), random.seed(41), th.manual_seed(41)
    assert ENV_CASES[0][0] == "exp1_g2"
    env = Wrapper(SingleUbsCoverageEnv(record=False, **ENV_CASES[0][1]), args)

    def to_double(g):
        for fr in g._nframes.values():
            for k in list(fr):
                fr[k] = fr[k].double()
        return g
    learner = QLearner(env.get_env_info(), args)
    fill_closed_form(learner.policy_net)
    learner.target_net.load_state_dict(learner.policy_net.state_dict())
    calls = {k: [] for k in ("gt", "agent", "h", "act", "rew", "next_gt", "next_agent", "next_h", "done", "bad_mask")}

    def feats(g):
        f = g.ndata["feat"]
        return f["gt"].numpy().copy(), f["agent"].numpy().copy()
    random.seed(42), th.manual_seed(42)
    o, h = to_double(env.reset()), learner.init_hidden()
    for _ in range(STEPS):
        a, h2 = learner.act(o, h, 0.5)
        o2, r, d, info = env.step(a)
        o2 = to_double(o2)
        learner.cache(o, h, a, r, o2, h2, d, info.get("BadMask"))
        (gt, ag), (gt2, ag2) = feats(o), feats(o2)
        for k, v in (("gt", gt), ("agent", ag[0]), ("h", h.numpy()[0].copy()), ("act", a), ("rew", r), ("next_gt", gt2),
                     ("next_agent", ag2[0]), ("next_h", h2.numpy()[0].copy()), ("done", float(d)),
                     ("bad_mask", float(info.get("BadMask")))):
            calls[k].append(v)
        o, h = o2, h2
        if d:
            o, h = to_double(env.reset()), learner.init_hidden()
    out = {"cache:" + k: np.asarray(v) for k, v in calls.items()}
    assert out["cache:done"].sum() >= 1, "the rollout crossed no episode end"
    mem = list(learner.buffer.memory)
    assert len(mem) == STEPS // T
    out["seq:gt"] = np.stack([np.stack([s["obs"][t].ndata["feat"]["gt"].numpy() for t in range(T + 1)]) for s in mem])
    out["seq:agent"] = np.stack([np.stack([s["obs"][t].ndata["feat"]["agent"].numpy()[0] for t in range(T + 1)]) for s in mem])
    out["seq:h"] = np.stack([np.stack([s["h"][t].numpy()[0] for t in range(T + 1)]) for s in mem])
    for k in ("act", "rew", "done"):
        out["seq:" + k] = np.stack([np.stack([s[k][t].numpy().reshape(1) for t in range(T)]) for s in mem])
    idx = [4, 1, 3, 0]                 # sequence 3 ends with the episode: its stored h[T] is the zeroed next_h
    learner.buffer.sample = lambda n: [mem[i] for i in idx]
    out["indices"] = np.asarray(idx, dtype=np.int64)
    res = learner.update()
    out["loss"] = np.array(res["LossQ"])
    out["qvals"] = res["QVals"]
    for k, p in learner.policy_net.named_parameters():
        out[f"grad:{k}"] = p.grad.detach().numpy()
        out[f"after:{k}"] = p.detach().numpy()
    for k, p in learner.target_net.named_parameters():
        out[f"target_after:{k}"] = p.detach().numpy()
    out["param_names"] = np.array([k for k, _ in learner.policy_net.named_parameters()])
    out["param_shapes"] = np.array([repr(tuple(p.shape)) for p in learner.policy_net.parameters()])
    out["cfg"] = np.array(repr(dict(agent="gnn", hidden_size=32, n_heads=4, n_actions=int(env.n_actions), n_gts=int(env.n_gts), T=T,
                                    B=B, gamma=0.99, polyak=0.995, lr=5e-4, episode_limit=int(env.episode_limit))))
    path = os.path.join(HERE, "learner_update_drqn.npz")
    np.savez_compressed(path, **out)
    print(f"learner_update_drqn: loss={float(out['loss']):.6f} qvals={out['qvals'].shape} episode ends={int(out['cache:done'].sum())} "
          f"-> {os.path.getsize(path)} B")
    th.set_default_dtype(th.float32)


def make_sampler_stats():
    from envs.subs_cov.subs_cov import SingleUbsCoverageEnv
    from tests.subs_sampler_ref import histograms
    N = 20000
    out = {}
    for n_grps, gpg in ((2, 5), (4, 5)):
        np.random.seed(1000 + n_grps), random.seed(1000 + n_grps)
        env = SingleUbsCoverageEnv(n_grps=n_grps, gts_per_grp=gpg, record=False)
        M = env.n_gts
        ubs, gts, prior = np.zeros((N, 2)), np.zeros((N, M, 2), dtype=np.float32), np.zeros((N, M), dtype=np.int64)
        for i in range(N):                     # what reset() draws, in its order (subs_cov.py:82-84)
            env._set_position()
            ubs[i], gts[i], prior[i] = env.pos_ubs, env.pos_gts, np.random.permutation(M)
        for k, v in histograms(ubs, gts, prior, float(env.range_pos)).items():
            out[f"g{n_grps}x{gpg}:{k}"] = v
        out[f"g{n_grps}x{gpg}:const"] = np.array([n_grps, gpg, env.range_pos, env.r_cov], dtype=np.float64)
    out["draws"] = np.array(N)
    path = os.path.join(HERE, "subs_sampler_stats.npz")
    np.savez_compressed(path, **out)
    print(f"subs_sampler_stats -> {os.path.getsize(path)} B")


PARTS = dict(env=make_env_golden, learner=make_learner_golden, sampler=make_sampler_stats)

if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "envs", "subs_cov")):
        print("[make_golden_exp1] reference not found: skipped")
        sys.exit(0)
    sys.path[:0] = [os.path.join(ROOT, "oracle", "dgl_standin"), os.path.join(ROOT, "oracle", "gym_standin"), REF, ROOT]
    for part in (sys.argv[1:] or ["env", "learner", "sampler"]):
        PARTS[part]()

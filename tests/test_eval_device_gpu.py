"""`-m gpu`: evaluation episodes and epoch statistics on the device loop.

  1. uavgnn_eps_greedy_philox bit for bit against the NumPy restatement (tests/eval_ref.py, written from include/uavgnn.h);
  2. uavgnn_stats_push against a two-pass evaluation in np.longdouble at the restatement's bound, and bit-reproducible;
  3. ``graphs.Evaluation`` against a loop written out here from public pieces (reset, policy_net, the restated draws fed to
     uavgnn_eps_greedy, env.step): every step's actions and the returned table are identical;
  4. ``GraphedEvaluation`` equals ``Evaluation`` over two calls;
  5. an evaluation between training episodes leaves the training run bit-identical (TarMAC and c = 'disc');
  6. ``Episode(stats=...)`` / ``GraphedEpisode(stats=...)``;
  7. argument errors."""
import types

import numpy as np
import pytest
import torch as th

from tests import eval_ref as R

pytestmark = pytest.mark.gpu

INFO = ("EpRet", "EpLen", "AvgGlobalUtility", "TotalThroughput", "FairIdx", "ProbCollision")
SEED = 2 ** 33 + 17          # a seed whose high word is not zero


# ---- 1. the selection kernel --------------------------------------------------------------------------------------------------------
def _select(q, N, A, n_agents, rng, eps, eps_on_device):
    """acts [N] int64 (CPU) of one call, written between two guard regions that are checked."""
    from uav_bs_ctrl_amd import _lib as L
    G = 8
    buf = th.full((N + 2 * G,), -7, dtype=th.int64, device="cuda")
    eps_dev = th.tensor([eps], dtype=th.float32, device="cuda") if eps_on_device else None
    code = L.lib().uavgnn_eps_greedy_philox(L.ptr(q), q.stride(0) if q is not None else A, N, A, n_agents, rng.data_ptr(), L.ptr(eps_dev),
                                            0.5 if eps_on_device else float(eps), buf.data_ptr() + 8 * G, L.stream())
    assert code == 0, code
    out = buf.cpu()
    assert (out[:G] == -7).all() and (out[G + N:] == -7).all(), "a guard word was written"
    return out[G:G + N].numpy()


@pytest.mark.parametrize("N,A,n_agents,ld", [(1, 1, 1, 1), (12, 5, 3, 8), (524291, 5, 1, 5)])
def test_eps_greedy_philox_matches_the_restatement(N, A, n_agents, ld):
    gen = th.Generator().manual_seed(N)
    q = th.randint(0, 3, (N, ld), generator=gen).float().cuda()      # three levels: most rows have tied maxima
    q_np = q.cpu().numpy()
    step0 = 2 ** 32 + 5 if N == 12 else 5                            # the step's high word enters the counter
    rng = th.tensor([SEED, step0], dtype=th.int64, device="cuda")
    step = step0
    for eps in (0.0, 0.05, 1.0):
        for on_device in (False, True):
            got = _select(q, N, A, n_agents, rng, eps, on_device)
            want = R.eps_greedy_philox(q_np, A, n_agents, SEED, step, eps)
            assert np.array_equal(got, want), f"eps = {eps}, device eps = {on_device}: {int((got != want).sum())} of {N} rows differ"
            step += 1
            assert rng.tolist() == [SEED, step], "the step did not advance by one"
            if eps == 0.0:
                assert np.array_equal(got, np.argmax(q_np[:, :A], axis=1)), "eps = 0 is the first maximum everywhere"
    # resetting {seed, step} reproduces a call
    rng.copy_(th.tensor([SEED, step0 + 2], dtype=th.int64))
    again = _select(q, N, A, n_agents, rng, 0.05, False)
    assert np.array_equal(again, R.eps_greedy_philox(q_np, A, n_agents, SEED, step0 + 2, 0.05))
    if N > 1000:
        explored = again != np.argmax(q_np[:, :A], axis=1)
        assert 0.02 < explored.mean() < 0.06, "about 5 % x 4 / 5 of the rows explore away from the maximum"


def test_eps_greedy_philox_arguments():
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    rng = th.tensor([1, 41], dtype=th.int64, device="cuda")
    q, acts = th.zeros(4, 5, device="cuda"), th.zeros(4, dtype=th.int64, device="cuda")
    assert lib.uavgnn_eps_greedy_philox(None, 5, 0, 5, 1, rng.data_ptr(), None, 0.1, None, L.stream()) == 0
    assert rng.tolist() == [1, 42], "N = 0 still advances the step"
    for args in ((q.data_ptr(), 5, 4, 5, 1, None, None, 0.1, acts.data_ptr()),            # rng NULL
                 (q.data_ptr(), 4, 4, 5, 1, rng.data_ptr(), None, 0.1, acts.data_ptr()),  # ld_q < A
                 (q.data_ptr(), 5, -1, 5, 1, rng.data_ptr(), None, 0.1, acts.data_ptr()),
                 (q.data_ptr(), 5, 4, 0, 1, rng.data_ptr(), None, 0.1, acts.data_ptr()),
                 (q.data_ptr(), 5, 4, 5, 0, rng.data_ptr(), None, 0.1, acts.data_ptr()),
                 (None, 5, 4, 5, 1, rng.data_ptr(), None, 0.1, acts.data_ptr()),
                 (q.data_ptr(), 5, 4, 5, 1, rng.data_ptr(), None, 0.1, None)):
        assert lib.uavgnn_eps_greedy_philox(*args, L.stream()) == -1000, args
    assert rng.tolist() == [1, 42], "a rejected call advanced the step"


# ---- 2. the statistics kernel ----------------------------------------------------------------------------------------------------------
PUSH_SIZES = (1, 2, 63, 64, 65, 257, 4099)


def _push_all(chunks, n_keys):
    """The accumulator [n_keys, 6] (CPU float64 numpy) after pushing chunks (each [n_keys, n]) from rows of stride ld = n + 3."""
    from uav_bs_ctrl_amd import _lib as L
    acc = th.tensor(R.stats_empty(n_keys), dtype=th.float64, device="cuda")
    for c in chunks:
        n = c.shape[1]
        vals = th.full((n_keys, n + 3), 1e300, dtype=th.float64, device="cuda")     # the padding must not be read
        vals[:, :n] = th.as_tensor(c, dtype=th.float64)
        assert L.lib().uavgnn_stats_push(vals.data_ptr(), n + 3, n, n_keys, acc.data_ptr(), L.stream()) == 0
    return acc.cpu().numpy()


@pytest.mark.parametrize("n_keys", [1, 6])
@pytest.mark.parametrize("shift", [0.0, 1e6])
def test_stats_push_against_two_pass_longdouble(n_keys, shift):
    rs = np.random.RandomState(9 + n_keys)
    chunks = [rs.standard_normal((n_keys, n)) * (1.0 + np.arange(n_keys))[:, None] + shift for n in PUSH_SIZES]
    acc = _push_all(chunks, n_keys)
    ref = R.stats_empty(n_keys)
    for c in chunks:
        R.stats_push(ref, c)
    for k in range(n_keys):
        allv = np.concatenate([c[k] for c in chunks])
        mean, m2 = R.two_pass(allv)
        tol_mean, tol_m2 = R.moment_tolerances(allv)
        err_mean, err_m2 = abs(acc[k, 1] - mean), abs(acc[k, 2] - m2)
        print(f"keys {n_keys} shift {shift:g} key {k}: mean err {float(err_mean):.3e} (tol {tol_mean:.3e}), "
              f"M2 err {float(err_m2):.3e} = {float(err_m2 / m2):.3e} relative (tol {tol_m2:.3e})")
        assert acc[k, 0] == allv.size == ref[k, 0] and acc[k, 5] == 0
        assert acc[k, 3] == allv.min() and acc[k, 4] == allv.max()
        if shift == 0.0:
            assert err_mean <= tol_mean and err_m2 <= tol_m2
        else:
            assert err_m2 / m2 <= 1e-9 and err_mean <= tol_mean
    assert np.array_equal(acc, _push_all(chunks, n_keys)), "the same pushes gave other bits"


def test_stats_push_non_finite_and_arguments():
    from uav_bs_ctrl_amd import _lib as L
    first = np.array([[1.0, np.nan, 3.0, np.inf], [-np.inf, 2.0, 2.0, 2.0]])
    acc = _push_all([first], 2)
    assert acc.tolist() == R.stats_push(R.stats_empty(2), first).tolist()
    both = _push_all([first, np.full((2, 5), np.nan)], 2)
    assert np.array_equal(both[:, :5], acc[:, :5]) and both[:, 5].tolist() == [7.0, 6.0]
    a = th.tensor(R.stats_empty(1), dtype=th.float64, device="cuda")
    v = th.zeros(1, 4, dtype=th.float64, device="cuda")
    lib = L.lib()
    assert lib.uavgnn_stats_push(v.data_ptr(), 4, 0, 1, a.data_ptr(), L.stream()) == 0
    assert a.cpu().numpy().tolist() == R.stats_empty(1).tolist(), "n = 0 is a no-op"
    for args in ((v.data_ptr(), 4, -1, 1, a.data_ptr()), (v.data_ptr(), 4, 4, 0, a.data_ptr()), (v.data_ptr(), 4, 4, 17, a.data_ptr()),
                 (v.data_ptr(), 3, 4, 1, a.data_ptr()), (None, 4, 4, 1, a.data_ptr()), (v.data_ptr(), 4, 4, 1, None)):
        assert lib.uavgnn_stats_push(*args, L.stream()) == -1000, args


# ---- the two setups of tests/test_graphed_episode_gpu.py ---------------------------------------------------------------------------------
def _multi(c="tarmac", seed=3):
    """'debug' map (3 UBSs x 4 GTs, episode limit 10), H = 32, 4 training environments and 4 evaluation environments."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(seed)
    E, Hs = 4, 32
    env = BatchedUbsCoverageEnv.from_map("debug", E, seed=11)
    args = types.SimpleNamespace(device="cuda", hidden_size=Hs, c=c, n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                                 dueling=False, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9, max_seq_len=None,
                                 batch_size=4, seed=seed)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    learner = MultiAgentQLearner(info, args)
    rb = SequenceReplay(8, env.episode_limit, env.n_agents, env.n_gts, Hs, n_envs=E, state_dim=env.state_dim, r_comm=env.p.r_comm,
                        device_state=True, seed=21)
    test_env = lambda: BatchedUbsCoverageEnv.from_map("debug", E, seed=31)      # noqa: E731
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 200.0), enc="gnn"), test_env


def _exp1(agent="rnn", seed=4):
    """exp1 'rnn': n_grps = 2, gts_per_grp = 3, T = 5, episode limit 10, 4 + 4 environments."""
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, SingleUbsParams
    th.manual_seed(seed)
    E, Hs, T = 4, 32, 5
    p = SingleUbsParams(n_grps=2, gts_per_grp=3, episode_limit=10)
    env = BatchedSingleUbsCoverageEnv(p, E, seed=12)
    args = types.SimpleNamespace(device="cuda", agent=agent, hidden_size=Hs, n_heads=4, n_layers=2, max_seq_len=T, gamma=0.99,
                                 polyak=0.9, batch_size=4, lr=1e-3, anneal_lr=False, seed=seed)
    learner = QLearner(env.get_env_info(agent), args)
    rb = SingleUbsSequenceReplay(20, T, p.n_gts, Hs, n_envs=E, device_state=True, seed=22)
    test_env = lambda: BatchedSingleUbsCoverageEnv(p, E, seed=32)               # noqa: E731
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 300.0), enc=agent), test_env


SETUPS = {"multi-tarmac": _multi, "exp1-rnn": _exp1}


def _keys(env):
    return tuple(k for k in INFO if k != "ProbCollision" or hasattr(env, "n_colls"))


def _sim_state(env):
    out = dict(pos_ubs=env.pos_ubs, pos_gts=env.pos_gts, prior=env.prior, avg_rate=env.avg_rate, t=env.t, ep_ret=env.ep_ret,
               rng=env.map_rng if hasattr(env, "map_rng") else env.rng)
    out.update({"out." + k: v for k, v in env.out.items()})
    return {k: v.clone() for k, v in out.items()}


def _train_state(learner, rb):
    opt = learner.optimizer
    out = dict(params=learner.flat.flat, target=learner.flat_target, adam_m=opt.m, adam_v=opt.v, hyper=opt.hyper, state=rb.state,
               rng=rb.rng, status=rb.status, gen=learner._gen.get_state())
    out.update({"mem." + k: v for k, v in rb.mem.items()})
    for name, net in (("policy", learner.policy_net), ("target", learner.target_net)):
        for mn, m in net.named_modules():
            if isinstance(getattr(m, "rng_state", None), th.Tensor):
                out[f"comm.{name}.{mn}"] = m.rng_state
    return {k: v.clone() for k, v in out.items()}


def _differences(a, b):
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    return [k for k in a if not th.equal(a[k], b[k])]


# ---- 3. Evaluation against the loop written out ---------------------------------------------------------------------------------------
def _written_out(learner, env, episodes, eps, seed, enc):
    """run.py:63-74 for env.B environments at a time from public pieces; returns (table [K, episodes], actions and greedy actions per step)."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    single = not hasattr(env, "map_rng")
    n_agents = 1 if single else env.n_agents
    keys, B = _keys(env), env.B
    table = th.zeros(len(keys), episodes, dtype=th.float64, device="cuda")
    acts_log, greedy_log, random_log, step = [], [], [], 0
    with th.no_grad(), ops.frozen_weights():
        for r in range(episodes // B):
            env.reset() if single else env.reset_from_map()
            h = learner.init_hidden(B)
            for _ in range(env.episode_limit):
                obs = env.observations()["flat"] if single else env.graph(with_comm=learner.args.c is not None, static=True)
                logits, h = learner.policy_net(obs, h)
                logits = logits.contiguous()
                N = logits.shape[0]
                u_team, u_agent = R.draws(seed, step, N, n_agents)
                step += 1
                ut, ua = th.as_tensor(u_team).cuda(), th.as_tensor(u_agent).cuda()
                acts = th.empty(N, dtype=th.int64, device="cuda")
                L.check(L.lib().uavgnn_eps_greedy(logits.data_ptr(), logits.stride(0), N, learner.n_actions, n_agents, ut.data_ptr(),
                                                  ua.data_ptr(), float(np.float32(eps)), acts.data_ptr(), L.stream()), "uavgnn_eps_greedy")
                _, _, _, info = env.step(acts)
                acts_log.append(acts.clone()), greedy_log.append(logits.argmax(1))
                random_log.append(th.as_tensor(np.minimum((u_agent * np.float32(learner.n_actions)).astype(np.int64), learner.n_actions - 1)))
            for i, k in enumerate(keys):
                table[i, r * B:(r + 1) * B] = info[k]
    return table, acts_log, greedy_log, random_log, step


def _spy_on_steps(env):
    log, step = [], env.step

    def spy(acts):
        log.append(acts.clone())
        return step(acts)
    env.step = spy
    return log


@pytest.mark.parametrize("name", list(SETUPS))
def test_evaluation_is_the_loop_written_out(name):
    from uav_bs_ctrl_amd.graphs import Evaluation
    learner, _, _, kw, test_env = SETUPS[name]()
    for eps in (0.05, 0.0, 1.0):
        env_a, env_b = test_env(), test_env()
        ev = Evaluation(learner, env_a, 8, eps=eps, seed=SEED, enc=kw["enc"])
        log = _spy_on_steps(env_a)
        out = ev()
        table, acts, greedy, rand, steps = _written_out(learner, env_b, 8, eps, SEED, kw["enc"])
        assert list(out) == list(_keys(env_a)) and ev.rng.tolist() == [SEED, steps] and steps == 2 * env_a.episode_limit
        assert len(log) == len(acts) and all(th.equal(x, y) for x, y in zip(log, acts)), f"eps = {eps}: the actions differ"
        assert th.equal(th.stack([out[k] for k in out]), table), f"eps = {eps}: the table differs"
        assert not _differences(_sim_state(env_a), _sim_state(env_b))
        assert bool((out["EpLen"] == env_a.episode_limit).all()) and bool(th.isfinite(ev.table).all())
        if eps == 0.0:
            assert all(th.equal(x, g) for x, g in zip(log, greedy)), "eps = 0 did not select the maximum everywhere"
        if eps == 1.0:
            assert all(th.equal(x.cpu(), r) for x, r in zip(log, rand)), "eps = 1 did not select the random action everywhere"
            assert any(not th.equal(x, g) for x, g in zip(log, greedy))


# ---- 4. the graphed evaluation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETUPS))
def test_graphed_evaluation_replays_the_eager_one(name):
    from uav_bs_ctrl_amd.graphs import Evaluation, GraphedEvaluation
    from uav_bs_ctrl_amd.stats import EpochStats
    learner, _, _, kw, test_env = SETUPS[name]()
    env_e, env_g = test_env(), test_env()
    keys = ["Test" + k for k in _keys(env_e)]
    st_e, st_g = EpochStats(keys, "cuda"), EpochStats(keys, "cuda")
    params = learner.flat.flat.clone()
    eager = Evaluation(learner, env_e, 8, eps=0.3, seed=SEED, enc=kw["enc"], stats=st_e)
    graphed = GraphedEvaluation(learner, env_g, 8, eps=0.3, seed=SEED, enc=kw["enc"], stats=st_g)
    assert graphed.rng.tolist() == [SEED, 0] and th.equal(st_g.acc, st_e.acc), "the warm-up left its traces"
    assert th.equal(_sim_state(env_g)["rng"], _sim_state(env_e)["rng"])
    tables = []
    for call in range(2):
        out_e, out_g = eager(), graphed()
        tables.append(graphed.table.clone())
        assert th.equal(eager.table, graphed.table), f"call {call}: the tables differ"
        assert all(th.equal(out_e[k], out_g[k]) for k in out_e)
        assert th.equal(st_e.acc, st_g.acc) and th.equal(eager.rng, graphed.rng), f"call {call}"
        assert not _differences(_sim_state(env_e), _sim_state(env_g)), f"call {call}"
    assert not th.equal(tables[0], tables[1]), "both replays gave the same table: the counters are baked in"
    assert graphed.rng.tolist() == [SEED, 2 * 2 * env_g.episode_limit]
    row, acc = st_g.summary(), st_g.acc.cpu().numpy()
    assert row["NTestEpRet"] == 16 and row["NonFiniteTestEpRet"] == 0 and row["AverageTestEpLen"] == env_g.episode_limit
    both = th.cat(tables, 1).cpu().numpy()
    for i, k in enumerate(_keys(env_g)):
        assert row["MinTest" + k] == both[i].min() and row["MaxTest" + k] == both[i].max()
        tol_mean, tol_m2 = R.moment_tolerances(both[i])
        mean, m2 = R.two_pass(both[i])
        assert row["AverageTest" + k] == acc[i, 1] and abs(acc[i, 1] - mean) <= tol_mean and abs(acc[i, 2] - m2) <= tol_m2, k
    assert th.equal(learner.flat.flat, params), "an evaluation wrote a parameter"


# ---- 5. non-interference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,first", [("tarmac", False), ("disc", False), ("disc", True)], ids=["tarmac", "disc", "disc-evaluated-first"])
def test_evaluations_leave_the_training_run_untouched(c, first):
    """first: evaluations (eager and graphed) also run BEFORE the first training forward, when DiscreteComm's noise counter is not
    seeded yet - the evaluation seeds it for itself, and the training run must still draw the seed it draws without evaluations."""
    from uav_bs_ctrl_amd.graphs import Episode, Evaluation, GraphedEvaluation
    learner, env, rb, kw, _ = _multi(c)
    plain = Episode(learner, env, rb, **kw)
    for _ in range(3):
        plain()
    want = _train_state(learner, rb)
    if c == "disc":
        assert any(k.startswith("comm.policy") for k in want), "no in-kernel noise counter in this configuration"

    learner, env, rb, kw, test_env = _multi(c)       # seeded again: the same run, now with evaluations in between
    mixed = Episode(learner, env, rb, **kw)
    early = None
    if first:
        comm = [m for m in learner.policy_net.modules() if hasattr(m, "rng_state")]
        assert comm and all(m.rng_state is None for m in comm), "the noise counter is seeded before any forward"
        out = Evaluation(learner, test_env(), 8, seed=5, enc=kw["enc"])()
        early = GraphedEvaluation(learner, test_env(), 8, seed=5, enc=kw["enc"])
        assert th.equal(early()["EpRet"], out["EpRet"]), "eager and graphed evaluation of the unseeded policy differ"
        assert all(m.rng_state is None for m in comm), "an evaluation left the policy's noise counter seeded"
    mixed()
    planes = learner._rollout_planes
    keys_before = list(planes)
    out = Evaluation(learner, test_env(), 8, seed=5, enc=kw["enc"])()
    assert bool(th.isfinite(out["EpRet"]).all())
    mixed()
    gev = GraphedEvaluation(learner, test_env(), 8, seed=5, enc=kw["enc"])
    gev(), gev()
    if early is not None:
        early()                                      # captured before the policy was seeded: replays on its own counter
    assert learner._rollout_planes is planes and list(planes) == keys_before
    mixed()
    bad = _differences(want, _train_state(learner, rb))
    assert not bad, bad


@pytest.mark.parametrize("name", list(SETUPS))
def test_graphed_evaluation_follows_parameter_updates(name):
    """A graph captured BEFORE training evaluates the parameters of the moment it is replayed: after three training episodes its replay
    equals a fresh eager evaluation from the same {seed, step} and the same reset counter (a weight plane or a K1 parameter image baked
    into the capture would show here)."""
    from uav_bs_ctrl_amd.graphs import Episode, Evaluation, GraphedEvaluation
    learner, env, rb, kw, test_env = SETUPS[name]()
    env_g, env_e = test_env(), test_env()
    gev = GraphedEvaluation(learner, env_g, 8, eps=0.05, seed=SEED, enc=kw["enc"])
    env_rng = lambda e: e.map_rng if hasattr(e, "map_rng") else e.rng      # noqa: E731
    start = [gev.rng.clone(), env_rng(env_g).clone()]

    def rewind():
        gev.rng.copy_(start[0]), env_rng(env_g).copy_(start[1]), env_rng(env_e).copy_(start[1])

    def replay_equals_fresh_eager(what):
        rewind()
        gev()
        fresh = Evaluation(learner, env_e, 8, eps=0.05, seed=SEED, enc=kw["enc"])()
        assert all(th.equal(gev.out[k], fresh[k]) for k in fresh), f"{what}: the replay did not evaluate the current parameters"
        assert not _differences(_sim_state(env_g), _sim_state(env_e)), what
        return gev.table.clone()

    before = replay_equals_fresh_eager("as captured")
    p0 = learner.flat.flat.clone()
    train = Episode(learner, env, rb, **kw)
    for _ in range(3):
        train()
    assert not th.equal(learner.flat.flat, p0), "no update moved the parameters"
    replay_equals_fresh_eager("after three training episodes")
    # three small updates need not change a single greedy action of these tiny setups; a write that surely does shows that the
    # comparison above can fail: every parameter negated (in place, as an optimiser step writes them)
    learner.flat.flat.neg_()
    learner.invalidate_weight_cache()
    negated = replay_equals_fresh_eager("parameters negated")
    assert not th.equal(negated, before), "the evaluation does not depend on the parameters: the comparisons above show nothing"


# ---- 6. Episode(stats=...) ---------------------------------------------------------------------------------------------------------------
def test_episode_statistics_against_the_restatement():
    from uav_bs_ctrl_amd.graphs import Episode
    from uav_bs_ctrl_amd.stats import EpochStats
    learner, env, rb, kw, _ = _multi()
    plain = Episode(learner, env, rb, **kw)
    for _ in range(3):
        plain()
    want = _train_state(learner, rb)

    learner, env, rb, kw, _ = _multi()
    keys = list(_keys(env)) + ["LossQ"]
    st = EpochStats(keys, "cuda")
    ep = Episode(learner, env, rb, stats=st, **kw)
    ref, seen = R.stats_empty(len(keys)), {k: [] for k in keys}
    for _ in range(3):
        out = ep()
        vals = {k: ep.info[k].double().cpu().numpy() for k in _keys(env)}          # read back after the episode
        vals["LossQ"] = out["LossQ"].double().cpu().numpy().reshape(1)              # one update per episode here (T = the episode limit)
        for i, k in enumerate(keys):
            R.stats_push(ref[i:i + 1], vals[k][None])
            seen[k].append(vals[k])
    assert not _differences(want, _train_state(learner, rb)), "pushing statistics changed the training run"
    acc, row = st.acc.cpu().numpy(), st.summary()
    for i, k in enumerate(keys):
        allv = np.concatenate(seen[k])
        tol_mean, tol_m2 = R.moment_tolerances(allv)
        assert acc[i, 0] == ref[i, 0] == allv.size == row["N" + k] and acc[i, 5] == ref[i, 5] == 0
        assert acc[i, 3] == ref[i, 3] == row["Min" + k] and acc[i, 4] == ref[i, 4] == row["Max" + k]
        assert abs(acc[i, 1] - ref[i, 1]) <= tol_mean and abs(acc[i, 2] - ref[i, 2]) <= tol_m2, k
        mean, m2 = R.two_pass(allv)
        assert abs(acc[i, 1] - mean) <= tol_mean and abs(acc[i, 2] - m2) <= tol_m2, k
        assert row["Average" + k] == acc[i, 1] and row["Std" + k] == np.sqrt(acc[i, 2] / acc[i, 0])
    assert row["NEpRet"] == 3 * env.B and row["NLossQ"] == 3
    st.reset()
    assert st.acc.cpu().numpy().tolist() == R.stats_empty(len(keys)).tolist()


@pytest.mark.parametrize("name", list(SETUPS))
def test_graphed_episode_pushes_the_same_statistics(name):
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    from uav_bs_ctrl_amd.stats import EpochStats
    accs, states = [], []
    for cls in (Episode, GraphedEpisode):
        learner, env, rb, kw, _ = SETUPS[name]()
        st = EpochStats(list(_keys(env)) + ["LossQ"], "cuda")
        ep = cls(learner, env, rb, stats=st, **kw)
        assert st.summary()["NEpRet"] == 0, "the warm-up's pushes were not undone"
        for _ in range(3):
            ep()
        accs.append(st.acc.clone())
        state = _train_state(learner, rb)
        state.pop("gen")        # a generator registered with a capturing graph keeps its own offset bookkeeping (graphs._RngSnapshot)
        assert int(rb.state[1]) == rb.capacity, "the ring is compared whole only once it is full"
        states.append(state)
    assert th.equal(accs[0], accs[1]), (accs[0], accs[1])
    assert float(accs[0][-1, 0]) == 3 * env.episode_limit // rb.T, "LossQ: one value per update"
    assert not _differences(*states)


# ---- 7. arguments -----------------------------------------------------------------------------------------------------------------------
def test_arguments(monkeypatch):
    from uav_bs_ctrl_amd.graphs import Episode, Evaluation
    from uav_bs_ctrl_amd.stats import EpochStats
    learner, env, rb, kw, test_env = _exp1()
    for episodes in (0, 6, -4):
        with pytest.raises(ValueError, match="multiple"):
            Evaluation(learner, test_env(), episodes, enc=kw["enc"])
    st = EpochStats(["TestEpRet", "EpRet"], "cuda")
    with pytest.raises(ValueError, match="missing"):
        Evaluation(learner, test_env(), 4, enc=kw["enc"], stats=st)
    with pytest.raises(ValueError, match="missing"):
        Episode(learner, env, rb, stats=st, **kw)
    with pytest.raises(ValueError, match="unknown"):
        st.push(Other=th.zeros(2, device="cuda"))
    with pytest.raises(ValueError, match="equal"):
        st.push(TestEpRet=th.zeros(2, device="cuda"), EpRet=th.zeros(3, device="cuda"))
    st.push(EpRet=env.ep_ret, TestEpRet=env.t)           # float64 and int32 sources, one launch for the two adjacent keys
    st.push(EpRet=th.arange(100.0, device="cuda")[::25])     # a strided view; the staging buffer stays (4 <= cap)
    row = st.summary()
    assert (row["NEpRet"], row["NTestEpRet"], row["MaxEpRet"]) == (8, 4, 75.0)
    big = th.zeros(1000, device="cuda")
    monkeypatch.setattr(th.cuda, "is_current_stream_capturing", lambda: True)      # no capture is opened for an error path
    with pytest.raises(RuntimeError, match="capture"):
        st.push(EpRet=big)
    monkeypatch.undo()
    st.push(EpRet=big)                                       # outside a capture the staging buffer grows
    assert st.cap >= 1000 and st.summary()["NEpRet"] == 1008

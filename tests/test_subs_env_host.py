"""Experiment 1, host side (no GPU): the single-UBS environment's parameters against the reference's constants, the NumPy
restatement of its placement sampler against histograms of the reference's own draws, the `seen-by` graph builder against
``graph.batch`` of per-environment ``heterograph``s, and the sequence replay + ``QLearner.cache`` against the sequences the
reference's buffer stored (fixtures: tests/golden/make_golden_exp1.py)."""
import ast
import types

import numpy as np
import pytest
import torch as th

from tests import subs_sampler_ref as S
from tests.test_maps_registry import chi2_quantile, chi2_two_sample
from tests.util import GOLDEN

ENV_CASES = ["exp1_g2", "exp1_g4", "short_rb", "two_speeds", "m65"]


def env_case(case):
    """-> (npz, SingleUbsParams of the case, T)."""
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    z = np.load(f"{GOLDEN}/env_subs_cov.npz")
    c = {k.split(":")[-1]: float(z[k]) for k in z.files if k.startswith(f"{case}:const:")}
    p = SingleUbsParams(range_pos=c["range_pos"], episode_limit=int(c["episode_limit"]), n_grps=int(c["n_grps"]),
                        gts_per_grp=int(c["gts_per_grp"]), r_cov=c["r_cov"], n_rbs=int(c["n_rbs"]),
                        vels=tuple(z[f"{case}:vels"].tolist()), n_dirs=int(c["n_dirs"]))
    return z, p, c, int(z[f"{case}:steps"])


@pytest.mark.parametrize("case", ENV_CASES)
def test_params_reproduce_the_reference_constants(case):
    z, p, c, _ = env_case(case)
    assert p.n_gts == int(c["n_gts"]) and p.reward_scale_rate == c["reward_scale_rate"]
    assert abs(p.max_rate - c["max_rate"]) <= 1e-12 * c["max_rate"]
    moves = z[f"{case}:avail_moves"]
    assert p.avail_moves().shape == moves.shape and np.allclose(p.avail_moves(), moves, rtol=0.0, atol=1e-9)
    for k in ("dt", "h_ubs", "p_tx", "n0", "bw", "fc"):
        assert abs(getattr(p, k) - c[k]) <= 1e-12 * abs(c[k]), k
    assert p.chan() == (c["a"], c["b"], c["eta_los"], c["eta_nlos"])


# ---- the sampler's restatement against the reference's own draws ---------------------------------------------------------------------
SEED = 20251


@pytest.mark.parametrize("n_grps,gpg", [(2, 5), (4, 5)])
def test_sampler_restatement_against_the_reference_histograms(n_grps, gpg):
    """Two-sample chi-square of every histogram of subs_sampler_stats.npz (20 000 seeded reference draws) against the
    restatement's 20 000 environments at a fixed seed, below the chi-square quantile at 1 - 1e-6 (the rule of
    tests/test_maps_registry.py); and the same test REJECTS a sampler that leaves the GT rows unshuffled."""
    z = np.load(f"{GOLDEN}/subs_sampler_stats.npz")
    N = int(z["draws"])
    g, P, range_pos, r_cov = z[f"g{n_grps}x{gpg}:const"]
    assert (int(g), int(P)) == (n_grps, gpg)
    ubs, gts64, prior, order = S.sample64(n_grps, gpg, range_pos, r_cov, N, SEED, 0)
    gts = gts64.astype(np.float32)
    M = n_grps * gpg
    assert np.array_equal(np.sort(prior, axis=1), np.broadcast_to(np.arange(M), prior.shape)), "prior is no permutation"
    assert np.array_equal(np.sort(order, axis=1), np.broadcast_to(np.arange(M), order.shape))
    assert (gts >= 0).all() and (gts <= range_pos).all() and np.array_equal(ubs, np.full((N, 2), range_pos / 2))
    got = S.histograms(ubs, gts, prior, range_pos)
    bad = []
    for k, h in got.items():
        stat, df = chi2_two_sample(z[f"g{n_grps}x{gpg}:{k}"], h)
        bound = chi2_quantile(df)
        print(f"g{n_grps}x{gpg}:{k}: chi2 = {stat:.2f}, bound {bound:.2f} (df {df})")
        if not stat < bound:
            bad.append((k, stat, bound, df))
    assert not bad, bad
    # power: generation order instead of the shuffled rows -> rows 0 and 1 always share a group
    unshuffled = np.take_along_axis(gts, np.argsort(order, axis=1)[:, :, None], 1)
    h = S.histograms(ubs, unshuffled, prior, range_pos)
    stat, df = chi2_two_sample(z[f"g{n_grps}x{gpg}:pair_angle"], h["pair_angle"])
    assert stat > chi2_quantile(df)


def test_sampler_restatement_depends_on_seed_resets_and_environment_only():
    a = S.sample(2, 5, 1000.0, 100.0, 6, 11, 3)
    b = S.sample(2, 5, 1000.0, 100.0, 2, 11, 3, envs=[4, 1])
    for x, y in zip(a, b):
        assert np.array_equal(x[[4, 1]], y)
    c = S.sample(2, 5, 1000.0, 100.0, 6, 11, 4)
    assert not np.array_equal(a[1], c[1]) and not np.array_equal(a[2], c[2])


# ---- graph builder ----------------------------------------------------------------------------------------------------------------------
def assert_same_graph(got, ref):
    """Two HeteroBatches array for array: node counts, relations (offsets, source ids), features, graph offsets."""
    assert got._num_nodes == ref._num_nodes
    assert list(got._rels) == list(ref._rels)
    for c, r in ref._rels.items():
        g = got._rels[c]
        assert g.off.dtype == r.off.dtype == th.int32 and th.equal(g.off.cpu(), r.off.cpu()), c
        assert (g.src is None) == (r.src is None) and (g.eid is None) == (r.eid is None), c
    for nt, fr in ref._feat.items():
        assert th.equal(got._feat[nt]["feat"].cpu(), fr["feat"].cpu()), nt
    assert got.graph_off.dtype == th.int32 and th.equal(got.graph_off.cpu(), ref.graph_off.cpu())


def wrapper_graphs(gt, agent):
    """``graph.batch`` of B graphs built as the reference's wrapper builds them (drqn/utils/env_wrappers.py:63-77)."""
    from uav_bs_ctrl_amd import graph as G
    gs = []
    for b in range(gt.shape[0]):
        n_gts = gt.shape[1]
        data_dict = {("gt", "seen-by", "agent"): (th.arange(n_gts), th.zeros(n_gts, dtype=th.long))}
        g = G.heterograph(data_dict, num_nodes_dict={"gt": n_gts, "agent": 1})
        g.ndata["feat"] = {"gt": gt[b], "agent": agent[b].unsqueeze(0)}
        gs.append(g)
    return G.batch(gs)


@pytest.mark.parametrize("B,M", [(1, 10), (7, 65)])
def test_single_ubs_graph_builder_equals_batched_wrapper_graphs(B, M):
    from uav_bs_ctrl_amd import graph as G
    gen = th.Generator().manual_seed(3)
    gt, agent = th.randn(B, M, 4, generator=gen), th.randn(B, 2, generator=gen)
    g = G.from_single_ubs_obs(gt, agent)
    assert_same_graph(g, wrapper_graphs(gt, agent))
    x, off = g.relation_segments("seen-by")
    assert x.data_ptr() == gt.data_ptr() and g.agent_feat().data_ptr() == agent.data_ptr(), "the builder copied its inputs"
    assert G.from_single_ubs_obs(gt, agent)._rels[G.SEEN_BY].off.data_ptr() == off.data_ptr(), "offsets are cached"
    assert g.hints["max_deg:seen-by"] == M and g.hints["max_graph_agents"] == 1 and g.relation_order("seen-by") is None
    with pytest.raises(ValueError):
        G.from_single_ubs_obs(gt, agent[:-1] if B > 1 else th.zeros(2, 2))


# ---- replay + cache -----------------------------------------------------------------------------------------------------------------------
def drqn_fixture():
    z = np.load(f"{GOLDEN}/learner_update_drqn.npz")
    return z, ast.literal_eval(str(z["cfg"]))


def drqn_args(cfg, device):
    """The reference's DRQN config fields the learner reads (no ``dueling``, ``double_q`` or ``mixer``: algos/drqn/config.py)."""
    return types.SimpleNamespace(device=device, agent="gnn", hidden_size=cfg["hidden_size"], n_heads=cfg["n_heads"], n_layers=2,
                                 max_seq_len=cfg["T"], gamma=cfg["gamma"], polyak=cfg["polyak"], batch_size=cfg["B"], lr=cfg["lr"],
                                 anneal_lr=False, seed=0)


def replay_recorded_cache_calls(learner, buffer, z, device):
    """Feeds the recorded raw ``cache`` arguments of the reference rollout to ``learner.cache`` one call at a time."""
    f = lambda k, i: th.as_tensor(z["cache:" + k][i], dtype=th.float32, device=device)  # noqa: E731
    for i in range(z["cache:act"].shape[0]):
        learner.cache(buffer, dict(gt=f("gt", i)[None], agent=f("agent", i)[None]), f("h", i)[None], int(z["cache:act"][i]),
                      float(z["cache:rew"][i]), dict(gt=f("next_gt", i)[None], agent=f("next_agent", i)[None]), f("next_h", i)[None],
                      float(z["cache:done"][i]), float(z["cache:bad_mask"][i]))


def assert_stored_sequences(buffer, z):
    S_ = z["seq:gt"].shape[0]
    assert len(buffer) == S_
    for k in ("gt", "agent", "h", "rew", "done"):
        ref = th.as_tensor(z["seq:" + k]).float()            # the device stores float32: the same rounding of the float64 record
        assert th.equal(buffer.mem[k][:S_].cpu(), ref), k
    assert th.equal(buffer.mem["act"][:S_].cpu(), th.as_tensor(z["seq:act"]).long())


def test_replay_and_cache_reproduce_the_reference_buffer_on_the_cpu():
    from uav_bs_ctrl_amd.learner import QLearner
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    z, cfg = drqn_fixture()
    env_info = dict(obs_shape=dict(agent=2, gt=4), n_actions=cfg["n_actions"], episode_limit=cfg["episode_limit"])
    args = drqn_args(cfg, "cpu")
    learner = QLearner(env_info, args)
    assert not hasattr(args, "dueling") and not hasattr(args, "double_q"), "the caller's args were modified"
    assert learner.n_agents == 1 and learner.mixer is None and learner.double_q is False and learner.max_seq_len == cfg["T"]
    assert type(learner.policy_net).__name__ == "DrqnGnnAgent"
    assert list(dict(learner.policy_net.named_parameters())) == [str(n) for n in z["param_names"]]
    rnn = QLearner(dict(env_info, obs_shape=2 + 4 * cfg["n_gts"]), args)
    assert type(rnn.policy_net).__name__ == "RnnAgent" and rnn.policy_net.enc[0].in_features == 2 + 4 * cfg["n_gts"]
    buf = SingleUbsSequenceReplay(16, cfg["T"], cfg["n_gts"], cfg["hidden_size"], n_envs=1, device="cpu")
    replay_recorded_cache_calls(learner, buf, z, "cpu")
    assert_stored_sequences(buf, z)
    # an episode end inside the record: the raw done zeroes the stored next hidden state, the time-limit mask mutes the stored done
    ends = np.nonzero(z["cache:done"])[0]
    assert ends.size >= 1 and (z["cache:bad_mask"][ends] == 1).all() and float(buf.mem["done"].abs().max()) == 0.0
    s, t = divmod(int(ends[0]) + 1, cfg["T"])
    assert t == 0 and float(buf.mem["h"][s - 1, cfg["T"]].abs().max()) == 0.0 and float(np.abs(z["cache:next_h"][ends[0]]).max()) > 0
    # gather: both observation forms of the same sequences
    idx = th.as_tensor(z["indices"])
    b = buf.gather(idx, "gnn")
    assert len(b["obs"]) == cfg["T"] + 1 and b["acts"].shape == (cfg["T"], cfg["B"], 1) and b["h0"].shape == (cfg["B"], cfg["hidden_size"])
    ref_gt = th.as_tensor(z["seq:gt"]).float()[idx]
    for t in range(cfg["T"] + 1):
        assert_same_graph(b["obs"][t], wrapper_graphs(ref_gt[:, t], th.as_tensor(z["seq:agent"]).float()[idx][:, t]))
    f = buf.gather(idx, "rnn")
    for t in range(cfg["T"] + 1):
        want = th.cat((th.as_tensor(z["seq:agent"]).float()[idx][:, t], ref_gt[:, t].reshape(cfg["B"], -1)), 1)
        assert th.equal(f["obs"][t], want)
    assert th.equal(b["h1"], th.as_tensor(z["seq:h"]).float()[idx][:, 1])
    with pytest.raises(ValueError):
        buf.gather(idx, "mlp")

"""`-m gpu`: ``MultiAgentQLearner.accumulate`` with ``dueling=True`` (run_exp3.py's `duel` axis) at exp3 sizes: the dueling head stays on the
device path the plain head takes - the fused TarMAC step with the time-batched staging, csrc/head.hip for the forward, the folded weight
W_eff in the gate-gradient kernel - against the float64 oracle (oracle/restatement.py:madrqn_loss; float32 for the error floor), as one
replayed graph, and over a whole graphed training episode.  Modelled on tests/test_learner_comm_variants_gpu.py; helpers: tests/gpu_util.py."""
import functools
import json
import os
import types

import pytest
import torch as th

from tests.gpu_util import EXP3, UPDATE_CASES, _exp3_learner_and_sequence, _LibSpy, _oracle_at_gpu_branch
from tests.util import _GRAD_LOG, GRAD_BASE, GRAD_FACTOR, assert_close, grad_close

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 0.0       # as tests/test_gpu_parity.py: no blanket absolute floor
_OUT = os.path.dirname(_GRAD_LOG)
CASES = {label: (B, n, M, T) for label, B, n, M, T in UPDATE_CASES}


def _record(name, row):
    try:
        os.makedirs(_OUT, exist_ok=True)
        with open(os.path.join(_OUT, name), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def _learner(B, n, M, T, dist, dueling, c="tarmac"):
    """``_exp3_learner_and_sequence`` from a copy of bench.exp3_args with ``dueling`` set."""
    import bench
    real_args = bench.exp3_args

    def args(device, c="tarmac"):
        a = real_args(device, c=c)
        a.dueling = dueling
        return a
    mp = pytest.MonkeyPatch()
    mp.setattr(bench, "exp3_args", args)
    try:
        return _exp3_learner_and_sequence(B, n, M, T, dist, seed=3, c=c)
    finally:
        mp.undo()


def _spied_accumulate(learner, batch):
    """One accumulate -> (out, flat gradient buffer, C-ABI entries called (support queries aside), staged backward steps per
    end_sequence, th.cat calls that took a head parameter, calls of DuelingLayer.forward_torch)."""
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.agents import heads
    mp = pytest.MonkeyPatch()
    spy = _LibSpy(L.lib())
    staged, cats, torch_heads = [], [], []
    orig_end, orig_cat, orig_torch = ops.WeightGradSink.end_sequence, th.cat, heads.DuelingLayer.forward_torch
    head_ptrs = {p.data_ptr() for net in (learner.policy_net, learner.target_net) for p in net.f_out.parameters()}

    def end_spy(self):
        staged.append(0 if self.seq is None else len(self.seq.bwd_steps))
        return orig_end(self)

    def cat_spy(tensors, *a, **k):
        if any(isinstance(t, th.Tensor) and t.data_ptr() in head_ptrs for t in tensors):
            cats.append(len(tensors))
        return orig_cat(tensors, *a, **k)

    def torch_spy(self, x):
        torch_heads.append(tuple(x.shape))
        return orig_torch(self, x)
    mp.setattr(L, "lib", lambda: spy)
    mp.setattr(ops.WeightGradSink, "end_sequence", end_spy)
    mp.setattr(th, "cat", cat_spy)
    mp.setattr(heads.DuelingLayer, "forward_torch", torch_spy)
    # fresh graph objects: the indices a batch builds lazily and keeps (degree order, talk transpose) are built in this call, whoever ran first
    fb = dict(batch, obs=[g.fresh() for g in batch["obs"]])
    for k in ("obs_all", "obs_all_next"):
        if k in batch:
            fb[k] = batch[k].fresh()
    try:
        out = learner.accumulate(fb)
    finally:
        mp.undo()
    called = {nm for nm, _ in spy.calls if not nm.endswith("_supported")}
    return out, learner.grads.flat.clone(), called, staged, cats, torch_heads


@functools.lru_cache(maxsize=None)
def _tarmac_case(label, dist):
    """The dueling learner, its batch and one spied accumulate of it and of a ``dueling=False`` learner on the same batch (shared by the
    dispatch and the numerics test; nothing here moves a parameter)."""
    B, n, M, T = CASES[label]
    learner, batch = _learner(B, n, M, T, dist, True)
    plain, _ = _learner(B, n, M, T, dist, False)
    return dict(learner=learner, batch=batch, duel=_spied_accumulate(learner, batch), plain=_spied_accumulate(plain, batch))


def _grad_ratio(got, r64, r32):
    """max over the elements of |got - ref64| / grad_close's limit (<= 1 passes)."""
    a, r, r32 = got.detach().double().cpu(), r64.detach().double().cpu(), r32.detach().double().cpu()
    e32 = float((r32 - r).abs().max())
    lim = th.clamp(GRAD_BASE * (float(r.abs().max()) + r.abs()), min=max(GRAD_FLOOR, GRAD_FACTOR * e32))
    return float(((a - r).abs() / lim.clamp_min(1e-300)).max())


def _check_against_oracle(what, learner, batch, out, flat, T, N, cfg):
    """LossQ, every Q value, every slice of the flat gradient buffer; then the GraphedCycle replay against the eager buffer."""
    from uav_bs_ctrl_amd.graphs import GraphedCycle
    stats = {}
    l64, _, g64, _, g32 = _oracle_at_gpu_branch(learner, batch, out["QVals"].detach().cpu(), T, N, what, cfg=cfg, stats=stats)   # (asserts QVals)
    assert_close(out["LossQ"], l64, 1e-5, f"{what}: LossQ")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    worst = (0.0, "")
    ratios = {}
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        got = flat[o:o + prm.numel()].view_as(prm)
        ratios[k] = _grad_ratio(got, g64[k], g32[k])
        worst = max(worst, (ratios[k], k))
    _record("dueling_oracle.jsonl", dict(case=what, worst_grad_ratio=worst[0], worst_grad=worst[1],
                                         head_ratios={k: v for k, v in ratios.items() if k.startswith("f_out.")}, **stats))
    print(f"{what}: worst gradient ratio {worst[0]:.3f} ({worst[1]}); head: " +
          ", ".join(f"{k} {v:.3f}" for k, v in ratios.items() if k.startswith("f_out.")))
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        grad_close(flat[o:o + prm.numel()].view_as(prm), g64[k], f"learner.accumulate dueling {what}: grad {k}", ref32=g32[k], floor=GRAD_FLOOR)
    cyc = GraphedCycle(learner, lambda: learner.accumulate(batch))
    learner.grads.flat.fill_(float("nan"))
    out_g = cyc()
    th.cuda.synchronize()
    assert_close(out_g["LossQ"], l64, 1e-5, f"{what}: LossQ (graph replay)")
    assert th.equal(learner.grads.flat, flat), f"{what}: graph replay of accumulate differs from the eager run"


@pytest.mark.parametrize("dist", ["env", "dense"])
@pytest.mark.parametrize("label", ["1280 rows", "4096 rows"])
def test_tarmac_dueling_update_keeps_the_device_path(label, dist):
    """The C-ABI entries of one accumulate are those of the ``dueling=False`` learner on the same batch with the head kernel swapped for its
    dueling form - fused message kernel, f16x2 cell, gate-gradient kernel with the head gradient and column sums, time-batched staging."""
    case = _tarmac_case(label, dist)
    T = CASES[label][3]
    _, _, called, staged, cats, torch_heads = case["duel"]
    _, _, called_plain, staged_plain, _, _ = case["plain"]
    assert "uavgnn_head_fwd" in called_plain and "uavgnn_tarmac_msg_fwd_rowmax" in called_plain, "the plain learner left the path this test follows"
    assert called == (called_plain - {"uavgnn_head_fwd"}) | {"uavgnn_head_fwd_duel"}, \
        f"{label} {dist}: only dueling {sorted(called - called_plain)}, only plain {sorted(called_plain - called)}"
    assert staged == staged_plain and max(staged) == T + 1, f"{label} {dist}: staged backward steps {staged}, dueling=False {staged_plain}"
    assert not cats, f"{label} {dist}: th.cat over head parameters ({cats})"
    assert not torch_heads, f"{label} {dist}: the torch formulation of the head ran on {torch_heads}"


@pytest.mark.parametrize("dist", ["env", "dense"])
@pytest.mark.parametrize("label", ["1280 rows", "4096 rows"])
def test_tarmac_dueling_update_vs_oracle(label, dist):
    case = _tarmac_case(label, dist)
    B, n, M, T = CASES[label]
    out, flat = case["duel"][:2]
    _check_against_oracle(f"tarmac {label} {dist}", case["learner"], case["batch"], out, flat, T, B * n, dict(EXP3, dueling=True))


@pytest.mark.parametrize("label,B,n,M,T,unrolled", [("1280 rows", 160, 8, 20, 3, False), ("256 rows", 32, 8, 10, 3, True)])
def test_dueling_update_without_communication_vs_oracle(label, B, n, M, T, unrolled):
    """c=None: the head through ``_head`` - per step from 1024 rows, once over all steps (``_unroll``) below."""
    learner, batch = _learner(B, n, M, T, "env", True, c=None)
    out, flat, called, _, cats, torch_heads = _spied_accumulate(learner, batch)
    assert "uavgnn_head_fwd_duel" in called and not cats and not torch_heads
    assert ("uavgnn_gru_rec_fwd" in called) == unrolled
    _check_against_oracle(f"c=None {label} env", learner, batch, out, flat, T, B * n, dict(EXP3, c=None, dueling=True, exact_ties=True))


def _multi(seed=3):
    """tests/test_graphed_episode_gpu.py::_multi with a dueling head and H = 64 (the narrowest width csrc/head.hip covers)."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    from uav_bs_ctrl_amd.replay import SequenceReplay
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    th.manual_seed(seed)
    E, Hs = 4, 64
    env = BatchedUbsCoverageEnv.from_map("debug", E, seed=11)
    args = types.SimpleNamespace(device="cuda", hidden_size=Hs, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1,
                                 dueling=True, mixer=False, double_q=True, lr=1e-3, gamma=0.99, polyak=0.9, max_seq_len=None,
                                 batch_size=4, seed=seed)
    info = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=env.n_actions, n_agents=env.n_agents, episode_limit=env.episode_limit)
    learner = MultiAgentQLearner(info, args)
    rb = SequenceReplay(8, env.episode_limit, env.n_agents, env.n_gts, Hs, n_envs=E, state_dim=env.state_dim, r_comm=env.p.r_comm,
                        device_state=True, seed=21)
    return learner, env, rb, dict(batch_size=4, eps=(1.0, 0.05, 200.0), enc="gnn")


def test_graphed_episode_with_a_dueling_head_replays_the_eager_episode(monkeypatch):
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.graphs import Episode, GraphedEpisode
    spy = _LibSpy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    l_e, env_e, rb_e, kw = _multi()
    l_g, env_g, rb_g, _ = _multi()
    assert th.equal(l_e.flat.flat, l_g.flat.flat), "the two learners were not built from the same seed"
    p0 = l_e.flat.flat.clone()
    eager, graphed = Episode(l_e, env_e, rb_e, **kw), GraphedEpisode(l_g, env_g, rb_g, **kw)
    assert "uavgnn_head_fwd_duel" in spy.names, "the capture did not take the dueling head kernel"
    assert th.equal(l_g.flat.flat, p0), "the warm-up left its traces"
    out_e, out_g = eager(), graphed()
    th.cuda.synchronize()
    monkeypatch.undo()
    assert th.equal(out_e["LossQ"], out_g["LossQ"]) and bool(th.isfinite(out_g["LossQ"]))
    assert not th.equal(l_g.flat.flat, p0), "the episode did not train"
    size = int(rb_g.state[1])
    assert size > 0 and rb_g.state.tolist() == rb_e.state.tolist()
    assert th.equal(l_e.flat.flat, l_g.flat.flat), "parameters"
    assert th.equal(l_e.flat_target, l_g.flat_target), "target"
    bad = [k for k in rb_e.mem if not th.equal(rb_e.mem[k][:size], rb_g.mem[k][:size])]
    assert not bad, f"ring: {bad}"

"""`-m gpu`: the importance-weighted TD loss of a prioritised replay (``learner._td_loss`` with ``batch["weights"]``) against the float64
oracle: the test forms sum_b w_b (q - y)^2 / (T B n) itself from oracle/restatement.py:madrqn_loss's ``agent_out`` / ``target_out``, at the
double-Q choice and the ReLU pattern the GPU took (tests/gpu_util.py), and compares LossQ, ``last_td`` and every parameter gradient.
H = 32, six sequences: TarMAC and the agent without communication."""
import functools

import pytest
import torch as th

from oracle import restatement as R
from tests.gpu_util import EXP3, _exp3_learner_and_sequence, _gpu_relu_patterns, _oracle_at_gpu_branch, _oracle_obs, _ScriptedRelu
from tests.util import assert_close, grad_close

pytestmark = pytest.mark.gpu

H, B, N_AGENTS, M, T = 32, 6, 4, 10, 3


def _cfg(c):
    return dict(EXP3, c=c, hidden_size=H, msg_size=8, key_size=4, **({"exact_ties": True} if c is None else {}))


@functools.lru_cache(maxsize=None)
def _case(c):
    """The learner at H = 32, its batch and non-trivial weights (built once per variant; nothing here moves a parameter)."""
    import bench
    real_args = bench.exp3_args

    def args(device, c="tarmac"):
        a = real_args(device, c=c)
        a.hidden_size, a.msg_size, a.key_size = H, 8, 4
        return a
    mp = pytest.MonkeyPatch()
    mp.setattr(bench, "exp3_args", args)
    try:
        learner, batch = _exp3_learner_and_sequence(B, N_AGENTS, M, T, "env", seed=3, c=c)
    finally:
        mp.undo()
    gen = th.Generator(device="cuda").manual_seed(5)
    batch["h0"] = 0.1 * th.randn(B * N_AGENTS, H, device="cuda", generator=gen)
    batch["h1"] = 0.1 * th.randn(B * N_AGENTS, H, device="cuda", generator=gen)
    weights = th.tensor([1.0, 0.25, 0.7, 0.05, 0.5, 0.9], device="cuda")
    return learner, batch, weights


def _fresh(batch, **extra):
    fb = dict(batch, obs=[g.fresh() for g in batch["obs"]], **extra)
    for k in ("obs_all", "obs_all_next"):
        if k in batch:
            fb[k] = batch[k].fresh()
    return fb


def _weighted_oracle(learner, batch, w, dtype, next_acts, relu_masks, cfg):
    """(loss, td [T, B, n], gradients by name) with the weighted loss formed HERE from the oracle's Q values."""
    pp = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in learner.policy_net.state_dict().items()}
    pt = {k: v.detach().cpu().to(dtype) for k, v in learner.target_net.state_dict().items()}
    obs = [_oracle_obs(g, dtype) for g in batch["obs"]]
    f = lambda t: t.detach().cpu().to(dtype)   # noqa: E731
    acts, rews, dones = batch["acts"].cpu(), f(batch["rews"]), f(batch["dones"])
    script, real = _ScriptedRelu(relu_masks), R.F
    R.F = script
    try:
        _, agent_out, target_out = R.madrqn_loss(obs, f(batch["h0"]), f(batch["h1"]), acts, rews, dones, pp, pt, cfg, learner.gamma, True,
                                                 next_acts=next_acts)
    finally:
        R.F = real
    shp = (T, B, N_AGENTS)
    qvals = agent_out[:-1].gather(2, acts).view(shp)
    target = rews + learner.gamma * (1 - dones) * target_out.gather(2, next_acts).view(shp)
    td = qvals - target.expand(shp)
    loss = (f(w).view(1, B, 1) * td.square()).sum() / td.numel()
    names = [k for k, _ in learner.policy_net.named_parameters()]
    return loss.detach(), td.detach(), dict(zip(names, th.autograd.grad(loss, [pp[k] for k in names])))


@pytest.mark.parametrize("c", ["tarmac", None], ids=["tarmac", "no-comm"])
def test_weighted_update_vs_oracle(c):
    learner, batch, w = _case(c)
    cfg, what = _cfg(c), f"prioritised c={c}"
    out = learner.accumulate(_fresh(batch, weights=w))
    flat = learner.grads.flat.clone()
    assert len(learner.last_td) == 1 and tuple(learner.last_td[0].shape) == (T, B, N_AGENTS) and learner.last_td[0].is_contiguous()
    assert not learner.last_td[0].requires_grad
    q_gpu = out["QVals"].detach().cpu()
    _oracle_at_gpu_branch(learner, batch, q_gpu, T, B * N_AGENTS, what, cfg=cfg)          # QVals, and that the branch is float64's up to ties
    na_gpu, patterns = q_gpu[1:].argmax(2, keepdim=True), _gpu_relu_patterns(learner, batch, T, B * N_AGENTS)
    l64, td64, g64 = _weighted_oracle(learner, batch, w, th.float64, na_gpu, patterns, cfg)
    _, _, g32 = _weighted_oracle(learner, batch, w, th.float32, na_gpu, patterns, cfg)
    assert_close(out["LossQ"], l64, 1e-5, f"{what}: LossQ")
    assert_close(learner.last_td[0], td64, 1e-5, f"{what}: last_td")
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        grad_close(flat[o:o + prm.numel()].view_as(prm), g64[k], f"learner.accumulate {what}: grad {k}", ref32=g32[k])
    # a fixed-address TD buffer (what a captured update hands in) receives the same bits
    td_out = th.full((T, B, N_AGENTS), float("nan"), device="cuda")
    learner.accumulate(_fresh(batch, weights=w, td_out=td_out))
    assert learner.last_td[0].data_ptr() == td_out.data_ptr() and th.equal(td_out, learner.last_td[0])
    assert_close(td_out, td64, 1e-5, f"{what}: td_out")
    assert th.equal(learner.grads.flat, flat), "the TD buffer changed the gradient"


@pytest.mark.parametrize("c", ["tarmac", None], ids=["tarmac", "no-comm"])
def test_unit_weights_give_the_unweighted_loss_and_no_weights_leave_no_last_td(c):
    learner, batch, _ = _case(c)
    plain = learner.accumulate(_fresh(batch))
    assert not hasattr(learner, "last_td"), "a batch without weights left last_td"
    flat = learner.grads.flat.clone()
    ones = learner.accumulate(_fresh(batch, weights=th.ones(B, device="cuda")))
    assert len(learner.last_td) == 1
    assert_close(ones["LossQ"], plain["LossQ"], 1e-5, "unit weights: LossQ")
    assert th.equal(ones["QVals"], plain["QVals"])
    off = {id(q): o for q, o in zip(learner.grads.params, learner.grads.offsets)}
    for k, prm in learner.policy_net.named_parameters():
        o = off[id(prm)]
        grad_close(learner.grads.flat[o:o + prm.numel()], flat[o:o + prm.numel()], f"unit weights c={c}: grad {k}", floor=0.0)
    two = learner.accumulate([_fresh(batch, weights=th.ones(B, device="cuda")) for _ in range(2)])
    assert len(learner.last_td) == 2 and th.equal(learner.last_td[0], learner.last_td[1]), "one entry per chunk"
    assert_close(two["LossQ"], plain["LossQ"], 1e-5, "two chunks: LossQ")
    with pytest.raises(ValueError, match="some chunks carry importance weights"):
        learner.accumulate([_fresh(batch, weights=th.ones(B, device="cuda")), _fresh(batch)])
    learner.accumulate(_fresh(batch))
    assert not hasattr(learner, "last_td")
    for _ in range(2):                                   # `loss` on its own: the TD errors of that call alone, never a growing list
        learner.loss(_fresh(batch, weights=th.ones(B, device="cuda")))
        assert len(learner.last_td) == 1

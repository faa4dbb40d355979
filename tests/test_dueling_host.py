"""The algebra behind the dueling head's backward (uav_bs_ctrl_amd/ops.py: ``dueling_fold`` / ``dueling_split``) on the host, in float64:
the combine q = v + (adv - mean_a adv) of the reference's DuelingLayer (algos/madrqn/agents/dueling.py:13-16) is linear in the two heads'
outputs, so q = h W_eff^T + b_eff and the four parameter gradients are a split of G = dq^T h and g = colsum(dq).  Parameters: the
``f_out.*`` tensors of tests/golden/agent_tarmac_duel.npz; h and dq random."""
import torch as th

from tests.util import assert_close, load_golden
from uav_bs_ctrl_amd import ops

TOL = 1e-12


def _case(N=37, seed=5):
    _, _, p, cfg, _ = load_golden("agent_tarmac_duel", dtype=th.float64)
    Wa, ba, wv, bv = (p["f_out." + k].clone() for k in ("adv_head.weight", "adv_head.bias", "v_head.weight", "v_head.bias"))
    assert Wa.shape == (cfg["n_actions"], cfg["hidden_size"]) and wv.shape == (1, cfg["hidden_size"])
    gen = th.Generator().manual_seed(seed)
    h = th.randn(N, cfg["hidden_size"], generator=gen, dtype=th.float64)
    dq = th.randn(N, cfg["n_actions"], generator=gen, dtype=th.float64)
    return Wa, ba, wv, bv, h, dq


def _reference(h, Wa, ba, wv, bv):
    """dueling.py:14-16"""
    vals = th.nn.functional.linear(h, wv, bv)
    advs = th.nn.functional.linear(h, Wa, ba)
    return vals + (advs - advs.mean(-1, keepdim=True))


def test_the_fold_reproduces_the_reference_forward():
    Wa, ba, wv, bv, h, _ = _case()
    W_eff, b_eff = ops.dueling_fold(Wa, ba, wv, bv)
    assert W_eff.shape == Wa.shape and b_eff.shape == ba.shape
    assert_close(h @ W_eff.t() + b_eff, _reference(h, Wa, ba, wv, bv), TOL, "q from the fold")


def test_the_split_reproduces_the_reference_gradients():
    Wa, ba, wv, bv, h, dq = _case()
    leaves = [t.requires_grad_(True) for t in (h, Wa, ba, wv, bv)]
    ref = th.autograd.grad(_reference(*leaves), leaves, dq)
    with th.no_grad():
        W_eff, _ = ops.dueling_fold(Wa, ba, wv, bv)
        got = (dq @ W_eff,) + ops.dueling_split(dq.t() @ h, dq.sum(0))
    for name, a, r in zip(("d h", "d adv_head.weight", "d adv_head.bias", "d v_head.weight", "d v_head.bias"), got, ref):
        assert_close(a, r, TOL, name)


def test_one_action_leaves_the_value_head_alone():
    """A = 1: adv - mean is identically 0, so W_eff is the value row and the advantage head gets no gradient."""
    Wa, ba, wv, bv, h, dq = _case()
    W_eff, b_eff = ops.dueling_fold(Wa[:1], ba[:1], wv, bv)
    assert th.equal(W_eff, wv) and th.equal(b_eff, bv)
    dWa, dba, dwv, dbv = ops.dueling_split(dq[:, :1].t() @ h, dq[:, :1].sum(0))
    assert float(dWa.abs().max()) == 0.0 and float(dba.abs().max()) == 0.0
    assert_close(dwv, dq[:, :1].t() @ h, TOL, "d v_head.weight")
    assert_close(dbv, dq[:, :1].sum(0), TOL, "d v_head.bias")

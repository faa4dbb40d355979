"""Distributional Q (quantile regression) without a GPU: the third shared object and its table, the argument errors of its entries, the
torch arms in float64 against the NumPy restatement (tests/qr_ref.py, written from include/uavgnn_qr.h), closed forms of the loss, the
head module, the learner's and the run's option.  tests/test_quantile_gpu.py holds the kernels to the same restatement."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch as th
import torch.nn as nn

from tests import qr_ref as R
from tests.run_args import small_args
from tests.test_cabi_symbols import _exported
from uav_bs_ctrl_amd import _lib, ops
from uav_bs_ctrl_amd import build as BUILD
from uav_bs_ctrl_amd import run as RUN
from uav_bs_ctrl_amd.agents.heads import QuantileLinear, build_head, quantile_heads, quantile_mode

EINVAL, EUNSUPPORTED = -1000, -1001
ENTRIES = ["uavgnn_qr_loss_fwd", "uavgnn_qr_loss_partials", "uavgnn_qr_mean_fold", "uavgnn_qr_select_bwd", "uavgnn_qr_select_fwd",
           "uavgnn_qr_supported"]
NOISY = ["uavgnn_noisy_fold", "uavgnn_noisy_fold_bwd", "uavgnn_noisy_head_fwd", "uavgnn_noisy_head_supported", "uavgnn_noisy_noise"]


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_qr_library_builds_beside_the_other_two_and_exports_its_header(repo_root):
    main = BUILD.build_lib()
    assert main == BUILD.OUT, "build_lib still returns the main library's path"
    assert os.path.exists(BUILD.EXT_OUT) and os.path.exists(BUILD.QR_OUT)
    assert BUILD.QR_OBJ == os.path.join(BUILD.OBJ, "qr") and os.path.exists(os.path.join(BUILD.QR_OBJ, "quantile.o"))
    assert BUILD.EXTRA_CFLAGS["quantile.hip"] == BUILD.EXTRA_CFLAGS["td_return.hip"] == BUILD._NO_PK + ["-ffp-contract=off"]
    text = open(os.path.join(repo_root, "include", "uavgnn_qr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(uavgnn_[a-z0-9_]+)\s*\(", src)))
    assert declared == ENTRIES == sorted(_lib.QR_SIGNATURES) == _exported(BUILD.QR_OUT)
    assert _lib.parse_header(text)[1] == {}, "the error codes stay the main library's"
    assert not set(_lib.QR_SIGNATURES) & set(_lib.SIGNATURES) and not set(_lib.QR_SIGNATURES) & set(_lib.EXT_SIGNATURES)
    # the pins of the other two libraries
    assert len(_lib.SIGNATURES) == 130 and sorted(_lib.EXT_SIGNATURES) == NOISY == _exported(BUILD.EXT_OUT)
    assert (_lib.UAVGNN_EINVAL, _lib.UAVGNN_EUNSUPPORTED) == (EINVAL, EUNSUPPORTED)


def test_qr_library_passes_the_isa_audit(repo_root):
    import sys
    sys.path.insert(0, os.path.join(repo_root, "tools"))
    import isa_audit
    if not os.path.exists(isa_audit.OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain is not installed")
    BUILD.build_lib(verbose=False)
    rows = isa_audit.audit(BUILD.QR_OUT)
    # the audit lists a kernel only when it holds an MFMA or a packed fp32 instruction with an operand select: this library has neither
    assert [r for r in rows if r[0] != "ok"] == [] and [r for r in rows if r[4] != 0] == []
    assert any("qr_loss_fwd_kernel" in text for text in isa_audit.disassemble(BUILD.QR_OUT)), "the audit read this library's code"


def test_signatures_of_the_entries():
    I, P, LL, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float
    S = _lib.QR_SIGNATURES
    assert S["uavgnn_qr_supported"] == (I, [I, I])
    assert S["uavgnn_qr_mean_fold"] == (I, [P, I, P, I, I, I, P, P, P])
    assert S["uavgnn_qr_select_fwd"] == (I, [P, P, P, I, LL, I, I, I, P, P, P, P, P])
    assert S["uavgnn_qr_select_bwd"] == (I, [P, P, I, LL, I, I, P, P])
    assert S["uavgnn_qr_loss_fwd"] == (I, [P, P, P, I, P, P, I, I, I, I, F, I, F, P, P, P, P, I, P])
    assert S["uavgnn_qr_loss_partials"] == (I, [I, I, I, I])


@pytest.mark.parametrize("A,K,ok", [(1, 8, 1), (9, 16, 1), (64, 32, 1), (5, 64, 1), (65, 8, 0), (0, 8, 0), (9, 4, 0), (9, 12, 0), (9, 128, 0),
                                    (9, 0, 0), (-1, 32, 0)])
def test_supported_set(A, K, ok):
    assert _lib.qr().uavgnn_qr_supported(A, K) == ok


def test_argument_errors_are_codes_not_launches():
    """Fake non-NULL addresses: every call below is refused before anything is launched (no GPU is touched)."""
    Q = _lib.qr()
    p = 0x1000
    fold = dict(W=p, ld_w=32, b=p, A=9, K=8, H=32, W_bar=p, b_bar=p, stream=None)
    call = lambda fn, base, **k: getattr(Q, fn)(*{**base, **k}.values())      # noqa: E731
    for name in ("W", "b", "W_bar", "b_bar"):
        assert call("uavgnn_qr_mean_fold", fold, **{name: None}) == EINVAL, name
    for k in (dict(A=0), dict(K=0), dict(H=0), dict(ld_w=31), dict(A=-3)):
        assert call("uavgnn_qr_mean_fold", fold, **k) == EINVAL, k
    for k in (dict(A=65), dict(K=12), dict(K=128)):
        assert call("uavgnn_qr_mean_fold", fold, **k) == EUNSUPPORTED, k

    sel = dict(theta_pol=p, theta_tgt=p, acts=p, T=3, N=20, A=9, K=8, double_q=1, theta_a=p, theta_next=p, next_acts=p, q_pol=p, stream=None)
    for name in ("theta_pol", "theta_tgt", "acts", "theta_a", "theta_next"):
        assert call("uavgnn_qr_select_fwd", sel, **{name: None}) == EINVAL, name
    for k in (dict(T=0), dict(N=0), dict(A=0), dict(K=0), dict(N=-1)):
        assert call("uavgnn_qr_select_fwd", sel, **k) == EINVAL, k
    for k in (dict(A=65), dict(K=24)):
        assert call("uavgnn_qr_select_fwd", sel, **k) == EUNSUPPORTED, k
    assert call("uavgnn_qr_select_fwd", sel, N=2 ** 60) == EINVAL, "an element count past the index range"

    bwd = dict(d_theta_a=p, acts=p, T=3, N=20, A=9, K=8, d_theta_pol=p, stream=None)
    for name in ("d_theta_a", "acts", "d_theta_pol"):
        assert call("uavgnn_qr_select_bwd", bwd, **{name: None}) == EINVAL, name
    for k in (dict(T=0), dict(N=0), dict(A=0), dict(K=0)):
        assert call("uavgnn_qr_select_bwd", bwd, **k) == EINVAL, k
    for k in (dict(A=65), dict(K=24)):
        assert call("uavgnn_qr_select_bwd", bwd, **k) == EUNSUPPORTED, k

    G = Q.uavgnn_qr_loss_partials(3, 5, 3, 8)
    assert G == 2, "45 rows at 256 / 8 = 32 rows per workgroup"
    assert Q.uavgnn_qr_loss_partials(3, 5, 3, 64) == 12 and Q.uavgnn_qr_loss_partials(50, 4096, 8, 32) == 2048
    for bad in ((0, 5, 3, 8), (3, 0, 3, 8), (3, 5, 0, 8), (3, 5, 3, 0), (2 ** 20, 2 ** 10, 2, 8)):
        assert Q.uavgnn_qr_loss_partials(*bad) == EINVAL, bad
    assert Q.uavgnn_qr_loss_partials(3, 5, 3, 12) == EUNSUPPORTED
    loss = dict(theta_a=p, theta_next=p, rews=p, Cr=3, dones=p, weights=None, T=3, B=5, C=3, K=8, gamma=0.99, n_step=1, kappa=1.0, td=p, g=p,
                loss=p, workspace=p, G=G, stream=None)
    for name in ("theta_a", "theta_next", "rews", "dones", "td", "g", "loss", "workspace"):
        assert call("uavgnn_qr_loss_fwd", loss, **{name: None}) == EINVAL, name
    for k in (dict(T=0), dict(B=0), dict(C=0), dict(K=0), dict(Cr=2), dict(Cr=0), dict(n_step=0), dict(n_step=-1), dict(kappa=0.0),
              dict(kappa=-1.0), dict(kappa=float("nan")), dict(G=G + 1), dict(G=0)):
        assert call("uavgnn_qr_loss_fwd", loss, **k) == EINVAL, k
    assert call("uavgnn_qr_loss_fwd", loss, K=12) == EUNSUPPORTED
    assert _lib.lib().uavgnn_strerror(EUNSUPPORTED), "the codes are named by the main library"


# ---- the torch arms against the restatement ------------------------------------------------------------------------------------------
def _case(T, B, C, A, K, Cr, seed, scale=1.0):
    g = th.Generator().manual_seed(seed)
    N = B * C
    d = dict(theta_pol=scale * th.randn(T + 1, N, A, K, dtype=th.float64, generator=g),
             theta_tgt=scale * th.randn(T, N, A, K, dtype=th.float64, generator=g),
             acts=th.randint(0, A, (T, N, 1), generator=g),
             rews=th.randn(T, B, Cr, dtype=th.float64, generator=g),
             dones=th.zeros(T, B, 1, dtype=th.float64),
             weights=th.rand(B, dtype=th.float64, generator=g) + 0.5)
    d["dones"][0, 0] = 1.0
    d["dones"][T // 2, 1 % B] = 1.0
    d["dones"][T - 1, 2 % B] = 1.0
    return d


@pytest.mark.parametrize("T,B,C,A,K,Cr,double_q,n_step,weighted", [(3, 5, 3, 9, 8, 3, True, 1, True), (3, 5, 3, 9, 32, 1, False, 2, False),
                                                                   (1, 5, 1, 1, 64, 1, True, 7, True), (4, 3, 2, 5, 16, 2, False, 7, False),
                                                                   (4, 3, 2, 5, 8, 1, True, 3, True)])
def test_torch_arms_equal_the_restatement_in_float64(T, B, C, A, K, Cr, double_q, n_step, weighted):
    d = _case(T, B, C, A, K, Cr, seed=T + 10 * K, scale=2.0)
    pol = d["theta_pol"].clone().requires_grad_(True)
    theta_a, theta_next, next_acts, q_pol = ops.qr_select_torch(pol, d["theta_tgt"], d["acts"], double_q)
    ra, rn, racts, rq = R.select(d["theta_pol"], d["theta_tgt"], d["acts"], double_q)
    assert np.array_equal(theta_a.detach().numpy(), ra) and np.array_equal(theta_next.numpy(), rn)
    assert np.array_equal(next_acts.numpy(), racts) and np.abs(q_pol.numpy() - rq).max() <= 1e-12
    assert not theta_next.requires_grad and not q_pol.requires_grad
    w = d["weights"] if weighted else None
    loss, td = ops.qr_loss_torch(theta_a.view(T, B, C, K), theta_next.view(T, B, C, K), d["rews"], d["dones"], w, 0.9, n_step, 1.0)
    rl, rg, rtd, _, _ = R.loss(ra.reshape(T, B, C, K), rn.reshape(T, B, C, K), d["rews"], d["dones"], None if w is None else w.numpy(),
                               0.9, n_step, 1.0)
    assert abs(float(loss.detach()) - rl) <= 1e-12 * max(1.0, abs(rl)) and np.abs(td.numpy() - rtd).max() <= 1e-12 * np.abs(rtd).max()
    # autograd of the torch arm is the g formula, scattered to the taken action by the select
    loss.backward()
    want = R.select_bwd(rg.reshape(T, B * C, K), d["acts"], A)
    assert np.abs(pol.grad.numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-30)
    # ops.qr_select / ops.qr_loss route CPU float64 tensors to the same arms
    l2, td2 = ops.qr_loss(*[t.view(T, B, C, K) for t in ops.qr_select(d["theta_pol"], d["theta_tgt"], d["acts"], double_q)[:2]], d["rews"],
                          d["dones"], w, 0.9, n_step, 1.0, td_out=th.zeros(T, B, C, dtype=th.float64))
    assert float(l2) == float(loss.detach()) and th.equal(td2, td)


@pytest.mark.parametrize("kappa", [1.0, 0.5])
def test_autograd_of_the_torch_loss_is_the_g_formula_on_both_huber_branches(kappa):
    T, B, C, K = 2, 3, 2, 8
    d = _case(T, B, C, 1, K, C, seed=5, scale=3.0)       # |u| on both sides of kappa
    th_a = d["theta_pol"][:T, :, 0].reshape(T, B, C, K).clone().requires_grad_(True)
    th_n = d["theta_tgt"][:, :, 0].reshape(T, B, C, K)
    loss, _ = ops.qr_loss_torch(th_a, th_n, d["rews"], d["dones"], d["weights"], 0.95, 2, kappa)
    loss.backward()
    _, rg, _, _, y = R.loss(th_a.detach(), th_n, d["rews"], d["dones"], d["weights"].numpy(), 0.95, 2, kappa)
    u = y[..., None, :] - th_a.detach().numpy()[..., :, None]
    assert (np.abs(u) > kappa).any() and (np.abs(u) < kappa).any() and (u < 0).any() and (u > 0).any()
    assert np.abs(th_a.grad.numpy() - rg).max() <= 1e-12 * np.abs(rg).max()


def test_tau_and_the_restatement_of_the_mean_fold():
    for K in ops.QR_K:
        t = R.taus(K)
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t) and t[0] == 1 / (2 * K) and t[-1] == 1 - 1 / (2 * K)
    A, K, H = 3, 8, 5
    W, b = th.randn(A * K, H, dtype=th.float64), th.randn(A * K, dtype=th.float64)
    Wb, bb = ops.quantile_mean_fold(W, b, A, K)
    rW, rb = R.mean_fold(W, b, A, K)
    assert np.abs(Wb.numpy() - rW).max() <= 1e-12 and np.abs(bb.numpy() - rb).max() <= 1e-12
    with pytest.raises(_lib.UavGnnError):
        ops.quantile_mean_fold(W, b, A, 16)


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 64])
@pytest.mark.parametrize("u,kappa", [(0.75, 1.0), (1.0, 1.0), (0.3, 0.5)])
def test_equal_quantiles_and_equal_targets_give_k_half_u_squared_over_two_kappa(K, u, kappa):
    """All theta equal, all y equal, 0 < u <= kappa: every pair has L = u^2 / 2 and weight tau_i, sum_i tau_i = K / 2, so
    l = (1/K) K (K/2) u^2 / (2 kappa) = (K/2) u^2 / (2 kappa)."""
    T, B, C = 1, 2, 1
    theta = th.full((T, B, C, K), 0.25, dtype=th.float64)
    nxt = th.full((T, B, C, K), 5.0, dtype=th.float64)          # cut by the done: y = r
    rews = th.full((T, B, 1), 0.25 + u, dtype=th.float64)
    dones = th.ones(T, B, 1, dtype=th.float64)
    want = (K / 2) * u * u / (2 * kappa)
    loss, td = ops.qr_loss_torch(theta, nxt, rews, dones, None, 0.9, 1, kappa)
    rl, _, rtd, l, _ = R.loss(theta, nxt, rews, dones, None, 0.9, 1, kappa)
    assert abs(float(loss) - want) <= 1e-12 * want and abs(rl - want) <= 1e-12 * want and np.abs(l - want).max() <= 1e-12 * want
    assert np.abs(td.numpy() + u).max() <= 1e-12 and np.abs(rtd + u).max() <= 1e-12, "td = mean theta - mean y = -u"


def test_a_done_at_the_first_step_cuts_the_bootstrap_of_a_full_length_return():
    """n_step >= T with done_0 = 1: y_0 = r_0 whatever follows; without the done y_0 = r_0 + g r_1 + g^2 r_2 + g^3 theta_next[2]."""
    T, B, C, K, gam = 3, 2, 1, 8, 0.5
    nxt = th.arange(T * B * C * K, dtype=th.float64).view(T, B, C, K)
    rews = th.tensor([1.0, 2.0, 4.0], dtype=th.float64).view(T, 1, 1).expand(T, B, 1).contiguous()
    dones = th.zeros(T, B, 1, dtype=th.float64)
    dones[0, 0] = 1.0
    for n in (3, 7):
        y = R.targets(nxt, rews, dones, gam, n)
        assert np.array_equal(y[0, 0, 0], np.full(K, 1.0)), "sequence 0: cut at t = 0"
        assert np.allclose(y[0, 1, 0], 1.0 + gam * 2.0 + gam ** 2 * 4.0 + gam ** 3 * nxt[2, 1, 0].numpy(), rtol=0, atol=1e-12)
        assert np.allclose(y[1, 0, 0], 2.0 + gam * 4.0 + gam ** 2 * nxt[2, 0, 0].numpy(), rtol=0, atol=1e-12), "later steps are whole again"
        yt = ops.td_targets_torch(nxt, rews.unsqueeze(-1), dones.unsqueeze(-1), gam, ("nstep", n))
        assert np.abs(yt.numpy() - y).max() <= 1e-12
    theta = th.zeros(T, B, C, K, dtype=th.float64)
    _, td = ops.qr_loss_torch(theta, nxt, rews, dones, None, gam, 7, 1.0)
    assert float(td[0, 0, 0]) == -1.0


# ---- the head module -----------------------------------------------------------------------------------------------------------------
def test_quantile_linear_modes_on_the_cpu():
    th.manual_seed(0)
    m = QuantileLinear(32, 9, 8).double()
    assert not isinstance(m, nn.Linear), "the fused TarMAC step keys on nn.Linear and must not take this head"
    assert sorted(m.state_dict()) == ["bias", "weight"] and tuple(m.weight.shape) == (72, 32) and tuple(m.bias.shape) == (72,)
    x = th.randn(6, 32, dtype=th.float64)
    assert m.quantile_mode == "mean"
    q = m(x)
    with quantile_mode(m, "quantiles") as heads:
        assert heads == [m]
        theta = m(x)
    assert m.quantile_mode == "mean" and tuple(q.shape) == (6, 9) and tuple(theta.shape) == (6, 72)
    assert th.allclose(q, theta.view(6, 9, 8).mean(-1), rtol=0, atol=1e-13)
    q.sum().backward()
    assert m.weight.grad is not None and th.allclose(m.weight.grad.view(9, 8, 32).sum(1), x.sum(0).expand(9, 32), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="unknown mode"):
        with quantile_mode(m, "median"):
            pass
    for bad in (12, 0, True, 8.0, "8"):
        with pytest.raises(ValueError, match="quantiles"):
            QuantileLinear(32, 9, bad)
    with pytest.raises(ValueError, match="n_actions"):
        QuantileLinear(32, 65, 8)


def _args(**kw):
    base = dict(device="cpu", hidden_size=32, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1, dueling=False,
                mixer=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999, max_seq_len=5, seed=0, anneal_lr=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


INFO = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=9, n_agents=3, episode_limit=5)


def test_agents_build_the_head_and_refuse_the_pairs_that_do_not_exist():
    from uav_bs_ctrl_amd.agents import DrqnGnnAgent, GnnAgent, RnnAgent
    assert type(build_head(32, 9, _args())) is nn.Linear and type(build_head(32, 9, _args(quantiles=None))) is nn.Linear
    for cls, shape, kw in ((GnnAgent, INFO["obs_shape"], {}), (GnnAgent, INFO["obs_shape"], dict(c=None)), (RnnAgent, 14, dict(c=None, o="mlp")),
                           (DrqnGnnAgent, dict(gt=4, agent=2), {})):
        net = cls(shape, 9, _args(quantiles=8, **kw))
        assert isinstance(net.f_out, QuantileLinear) and net.f_out.K == 8 and quantile_heads(net) == [net.f_out], cls.__name__
        assert tuple(net.state_dict()["f_out.weight"].shape) == (72, 32) and tuple(net.state_dict()["f_out.bias"].shape) == (72,)
        assert type(cls(shape, 9, _args(**kw)).f_out) is nn.Linear and quantile_heads(cls(shape, 9, _args(**kw))) == []
        with pytest.raises(ValueError, match="quantiles together with dueling"):
            cls(shape, 9, _args(quantiles=8, dueling=True, **kw))
        with pytest.raises(ValueError, match="quantiles together with noisy"):
            cls(shape, 9, _args(quantiles=8, noisy=0.5, **kw))


def test_learner_option_and_its_refusals():
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner, QLearner
    args = _args()
    lr = MultiAgentQLearner(INFO, args, quantiles=8)
    assert not hasattr(args, "quantiles") and lr.args.quantiles == 8 and lr.quantiles == 8 and lr.QR_KAPPA == 1.0
    assert [type(m) for m in lr._quantile_heads] == [QuantileLinear, QuantileLinear]
    assert lr._quantile_heads[0] is lr.policy_net.f_out and lr._quantile_heads[1] is lr.target_net.f_out
    plain = MultiAgentQLearner(INFO, args)
    assert plain.quantiles is None and plain._quantile_heads == [] and type(plain.policy_net.f_out) is nn.Linear
    assert MultiAgentQLearner(INFO, args, quantiles=32, returns=("nstep", 3)).returns == ("nstep", 3)
    with pytest.raises(ValueError, match="quantile form of lambda returns does not exist"):
        MultiAgentQLearner(INFO, args, quantiles=8, returns=("lambda", 0.8))
    with pytest.raises(ValueError, match="quantile form of the QMIX mixer does not exist"):
        MultiAgentQLearner(dict(INFO, state_shape=10), _args(mixer=True, mixing_embed_dim=8, hypernet_embed=8), quantiles=8)
    with pytest.raises(ValueError, match="quantiles together with noisy"):
        MultiAgentQLearner(INFO, args, quantiles=8, noisy=0.5)
    with pytest.raises(ValueError, match="quantiles together with dueling"):
        MultiAgentQLearner(INFO, _args(dueling=True), quantiles=8)
    for bad in (12, "8", True, 8.0, (8,)):
        with pytest.raises(ValueError, match="quantiles"):
            MultiAgentQLearner(INFO, args, quantiles=bad)
    q_args = types.SimpleNamespace(device="cpu", agent="rnn", hidden_size=32, n_heads=4, n_layers=2, max_seq_len=5, gamma=0.99, polyak=0.9,
                                   batch_size=4, lr=1e-3, anneal_lr=False, seed=0)
    q = QLearner(dict(obs_shape=14, n_actions=5, episode_limit=10), q_args, quantiles=16)
    assert isinstance(q.policy_net.f_out, QuantileLinear) and q.policy_net.f_out.K == 16 and not hasattr(q_args, "quantiles")
    # `series` hands the option through the arguments
    assert MultiAgentQLearner(INFO, _args(quantiles=8)).quantiles == 8


def test_loss_of_a_cpu_learner_runs_both_networks_on_their_quantiles():
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    lr = MultiAgentQLearner(INFO, _args(c=None), quantiles=8)
    pol, tgt = lr.policy_net.f_out, lr.target_net.f_out
    seen = []
    lr._loss = lambda batch: seen.append((pol.quantile_mode, tgt.quantile_mode)) or "out"
    assert lr.loss({}) == "out" and seen == [("quantiles", "quantiles")]
    assert pol.quantile_mode == tgt.quantile_mode == "mean"


def test_td_tail_of_a_cpu_learner_is_the_torch_arm():
    """``_td_loss`` on hand-made quantiles: select -> loss, QVals = the means, weights / td_out / last_td as the scalar tail has them."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    T, B, n, A, K = 3, 2, 3, 9, 8
    for returns, n_step in ((None, 1), (("nstep", 2), 2)):
        lr = MultiAgentQLearner(INFO, _args(c=None), quantiles=K, returns=returns)
        d = _case(T, B, n, A, K, 1, seed=3)
        pol = d["theta_pol"].float().view(T + 1, B * n, A * K).requires_grad_(True)
        tgt = d["theta_tgt"].float().view(T, B * n, A * K)
        td_out = th.full((T, B, n), float("nan"))
        batch = dict(acts=d["acts"], rews=d["rews"].float(), dones=d["dones"].float(), weights=d["weights"].float(), td_out=td_out)
        loss, q_pol, target_out = lr._td_loss(batch, T, pol, tgt)
        a, nx, _, q = ops.qr_select_torch(pol.view(T + 1, B * n, A, K), tgt.view(T, B * n, A, K), d["acts"], True)
        want, td = ops.qr_loss_torch(a.view(T, B, n, K), nx.view(T, B, n, K), batch["rews"], batch["dones"], batch["weights"], lr.gamma, n_step)
        assert th.equal(loss, want) and th.equal(q_pol, q) and target_out is tgt and tuple(q_pol.shape) == (T + 1, B * n, A)
        assert lr.last_td[0] is td_out and th.equal(td_out, td)
        del batch["weights"]
        lr.__dict__.pop("last_td")
        lr._td_loss(batch, T, pol, tgt)
        assert not hasattr(lr, "last_td"), "no weights: no TD errors are kept"


def test_the_scalar_tail_still_runs_on_a_bare_namespace():
    """tests/test_td_return_gpu.py and tools/td_return_probe.py hand ``_td_loss`` a namespace with the one-step tail's fields only."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    T, B, n, A = 2, 3, 2, 5
    me = types.SimpleNamespace(returns=None, double_q=True, n_agents=n, mixer=None, gamma=0.9)
    agent_out, target_out = th.randn(T + 1, B * n, A), th.randn(T, B * n, A)
    batch = dict(acts=th.randint(0, A, (T, B * n, 1)), rews=th.randn(T, B, n), dones=th.zeros(T, B, 1))
    loss, a, t = MultiAgentQLearner._td_loss(me, batch, T, agent_out, target_out)
    assert bool(th.isfinite(loss)) and a is agent_out and t is target_out


# ---- the run option ------------------------------------------------------------------------------------------------------------------
def test_the_key_enters_config_json_only_when_set():
    ns = RUN.check_args("exp3", small_args("exp3"))
    off = RUN.run_config("exp3", "debug", ns, seed=3, n_envs=4, n_test_envs=2)
    assert "quantiles" not in off, "an absent key means off: existing run directories resume unchanged"
    on = RUN.run_config("exp3", "debug", ns, seed=3, n_envs=4, n_test_envs=2, quantiles=8)
    assert on["quantiles"] == 8 and {k: v for k, v in on.items() if k != "quantiles"} == off
    back = json.loads(RUN.config_text(dict(seed=3, args=ns, uav_bs_ctrl_amd=on)))["uav_bs_ctrl_amd"]
    assert back["quantiles"] == 8
    both = RUN.run_config("exp3", "debug", ns, prioritized=(0.6, 0.4, 0.9, 1e-3), compact_replay=True, returns=("nstep", 3), quantiles=32)
    assert both["quantiles"] == 32 and both["returns"] == ["nstep", 3] and both["compact_replay"] is True and "noisy" not in both
    for bad in (12, "8", True, 8.0, -8):
        with pytest.raises(ValueError, match="quantiles"):
            RUN.run_config("exp3", "debug", ns, quantiles=bad)
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    assert RUN.run_config("exp1", SingleUbsParams(), RUN.check_args("exp1", small_args("exp1")), quantiles=16)["quantiles"] == 16


def test_the_command_line_flag_and_the_series_key():
    from uav_bs_ctrl_amd import series
    ap = RUN._parser()
    base = ["--out", "d", "--exp", "exp3", "--env", "debug", "--args-json", "a.json"]
    assert ap.parse_args(base + ["--quantiles", "8"]).quantiles == 8 and ap.parse_args(base).quantiles is None
    assert ap.parse_args(base + ["--quantiles", "32", "--returns", "nstep", "3", "--compact-replay", "--prioritized", "0.6", "0.4", "0.9",
                                 "1e-3"]).quantiles == 32
    for words in (["--quantiles"], ["--quantiles", "12"], ["--quantiles", "many"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + words)
    assert "quantiles" in series.MODEL_KEYS

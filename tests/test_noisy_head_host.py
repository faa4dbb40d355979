"""The noisy-net Q head without a GPU: the second shared object and its table, the argument errors of its entries, the fold and the
module on the CPU against the NumPy restatement (tests/noisy_ref.py, written from include/uavgnn_ext.h), the stream's moments, and the
run option.  tests/test_noisy_head_gpu.py holds the kernels to the same restatement."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch as th
import torch.nn as nn

from tests import noisy_ref as R
from tests.run_args import small_args
from tests.test_cabi_symbols import _exported
from uav_bs_ctrl_amd import _lib, ops
from uav_bs_ctrl_amd import build as BUILD
from uav_bs_ctrl_amd import run as RUN
from uav_bs_ctrl_amd.agents.heads import NoisyLinear, build_head, noisy_heads, noisy_mode

EINVAL, EUNSUPPORTED = -1000, -1001
ENTRIES = ["uavgnn_noisy_fold", "uavgnn_noisy_fold_bwd", "uavgnn_noisy_head_fwd", "uavgnn_noisy_head_supported", "uavgnn_noisy_noise"]


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_ext_library_builds_beside_the_main_one_and_exports_its_header(repo_root):
    main = BUILD.build_lib()
    assert main == BUILD.OUT and os.path.exists(BUILD.EXT_OUT), "build_lib builds both and still returns the main library's path"
    text = open(os.path.join(repo_root, "include", "uavgnn_ext.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(uavgnn_[a-z0-9_]+)\s*\(", src)))
    assert declared == ENTRIES == sorted(_lib.EXT_SIGNATURES) == _exported(BUILD.EXT_OUT)
    assert _lib.parse_header(text)[1] == {}, "the error codes stay the main library's"
    assert _lib.ext().uavgnn_noisy_head_supported(256, 9) == 1


def test_ext_library_passes_the_isa_audit(repo_root):
    """tools/isa_audit.py on the second shared object: fp32 MFMAs only, and no packed fp32 with an operand select (`_NO_PK` took effect)."""
    import sys
    sys.path.insert(0, os.path.join(repo_root, "tools"))
    import isa_audit
    if not os.path.exists(isa_audit.OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain is not installed")
    BUILD.build_lib(verbose=False)
    rows = isa_audit.audit(BUILD.EXT_OUT)
    assert [r for r in rows if r[0] != "ok"] == []
    heads = {name: (n_mf, wide, n_sel) for _, name, n_mf, wide, n_sel, _ in rows if "noisy_head_fwd_kernel" in name}
    assert sorted(heads.values()) == [(32, False, 0), (64, False, 0), (128, False, 0)], heads      # 2 chains x 4 MFMAs x H / 16 loads


def test_the_main_table_is_unchanged():
    assert len(_lib.SIGNATURES) == 130 and _lib.UAVGNN_VERSION == 101
    assert not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES)
    assert (_lib.UAVGNN_EINVAL, _lib.UAVGNN_EUNSUPPORTED) == (EINVAL, EUNSUPPORTED)


def test_signatures_of_the_new_entries():
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    S = _lib.EXT_SIGNATURES
    assert S["uavgnn_noisy_head_supported"] == (I, [I, I])
    assert S["uavgnn_noisy_head_fwd"] == (I, [P, I, I, I, P, P, I, P, P, I, P, P, I, P])
    assert S["uavgnn_noisy_noise"] == (I, [P, I, I, I, P, P, P])
    assert S["uavgnn_noisy_fold"] == (I, [P, P, I, P, P, I, I, P, P, P, P, P, P])
    assert S["uavgnn_noisy_fold_bwd"] == (I, [P, I, P, P, P, I, I, P, P, P])
    assert LL not in sum((a for _, a in S.values()), []), "rng is a device pointer, not a host integer"


@pytest.mark.parametrize("H,A,ok", [(64, 1, 1), (128, 9, 1), (256, 16, 1), (256, 17, 0), (256, 0, 0), (32, 9, 0), (192, 9, 0), (512, 9, 0)])
def test_supported_set_is_the_plain_heads(H, A, ok):
    _lib.ext()
    BUILD.build_lib()
    assert _lib.ext().uavgnn_noisy_head_supported(H, A) == ok == _lib.lib().uavgnn_head_supported(H, A)


def test_argument_errors_are_codes_not_launches():
    """Fake non-NULL addresses: every call below is refused before anything is launched (no GPU is touched)."""
    E = _lib.ext()
    p, q = 0x1000, 0x1004       # 16-byte aligned / misaligned
    head = lambda **k: E.uavgnn_noisy_head_fwd(*[{**dict(h=p, ld_h=256, N=8, H=256, W_mu=p, W_sigma=p, ld_w=256, b_mu=p, b_sigma=p, A=9,   # noqa: E731
                                                          rng=p, q=p, ld_q=9, stream=None), **k}[n]
                                                 for n in ("h", "ld_h", "N", "H", "W_mu", "W_sigma", "ld_w", "b_mu", "b_sigma", "A", "rng", "q",
                                                           "ld_q", "stream")])
    for name in ("h", "W_mu", "W_sigma", "b_mu", "b_sigma", "rng", "q"):
        assert head(**{name: None}) == EINVAL, name
    assert head(ld_h=255) == EINVAL and head(ld_w=252) == EINVAL and head(ld_q=8) == EINVAL and head(N=-1) == EINVAL
    assert head(H=192, ld_h=192, ld_w=192) == EUNSUPPORTED and head(A=17, ld_q=17) == EUNSUPPORTED and head(A=0) == EUNSUPPORTED
    assert head(ld_h=258) == EUNSUPPORTED and head(ld_w=258) == EUNSUPPORTED
    for name in ("h", "W_mu", "W_sigma"):
        assert head(**{name: q}) == EUNSUPPORTED, name
    assert head(N=0) == 0, "no rows: nothing is launched"
    assert E.uavgnn_noisy_noise(None, 4, 8, 2, p, p, None) == EINVAL
    assert E.uavgnn_noisy_noise(p, -1, 8, 2, p, p, None) == EINVAL and E.uavgnn_noisy_noise(p, 4, 0, 2, p, p, None) == EINVAL
    assert E.uavgnn_noisy_noise(p, 4, 8, 0, p, p, None) == EINVAL and E.uavgnn_noisy_noise(p, 4, 4 * 0x10000 + 1, 2, p, p, None) == EINVAL
    assert E.uavgnn_noisy_noise(p, 0, 8, 2, p, p, None) == 0 and E.uavgnn_noisy_noise(p, 4, 8, 2, None, None, None) == 0
    fold = [p, p, 8, p, p, 2, 8, p, p, p, p, p, None]
    for i in (0, 1, 3, 4, 7, 8, 9, 10, 11):
        assert E.uavgnn_noisy_fold(*[None if k == i else v for k, v in enumerate(fold)]) == EINVAL, i
    assert E.uavgnn_noisy_fold(p, p, 7, p, p, 2, 8, p, p, p, p, p, None) == EINVAL
    assert E.uavgnn_noisy_fold(p, p, 8, p, p, 0, 8, p, p, p, p, p, None) == EINVAL
    assert E.uavgnn_noisy_fold(p, p, 8, p, p, 2, 0, p, p, p, p, p, None) == EINVAL
    bwd = [p, 8, p, p, p, 2, 8, p, p, None]
    for i in (0, 2, 3, 4, 7, 8):
        assert E.uavgnn_noisy_fold_bwd(*[None if k == i else v for k, v in enumerate(bwd)]) == EINVAL, i
    assert E.uavgnn_noisy_fold_bwd(p, 7, p, p, p, 2, 8, p, p, None) == EINVAL
    assert E.uavgnn_noisy_fold_bwd(p, 8, p, p, p, 0, 8, p, p, None) == EINVAL and E.uavgnn_noisy_fold_bwd(p, 8, p, p, p, 2, 0, p, p, None) == EINVAL
    assert _lib.lib().uavgnn_strerror(EUNSUPPORTED), "the codes are named by the main library"


# ---- the stream ----------------------------------------------------------------------------------------------------------------------
def test_restated_stream_has_normal_moments_and_f_inverts():
    seed, step = 2 ** 40 + 77, 3
    z_in, z_out = R.xi_in(seed, step, np.arange(2000), 256), R.xi_out(seed, step, np.arange(2000), 9)
    for z in (z_in, z_out):
        n = z.size
        assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
        assert abs((z ** 3).mean()) < 5 * np.sqrt(15 / n) and abs((z ** 4).mean() - 3) < 5 * np.sqrt(96 / n)
        fz = R.f(z)
        assert np.abs(fz * np.abs(fz) - z).max() <= 4 * np.finfo(np.float64).eps * np.abs(z).max()
    assert abs(np.corrcoef(z_in[:, 0], z_out[:, 0])[0, 1]) < 5 / np.sqrt(2000), "xi_in and xi_out come from different blocks"
    # (seed, step, row, column) only: a sub-range equals the same rows of the whole, and every key word matters
    assert np.array_equal(R.xi_in(seed, step, [5, 1999], 256), z_in[[5, 1999]])
    assert np.array_equal(R.xi_in(seed, step, [7], 9), z_in[[7], :9]), "ragged last block: a prefix of the same columns"
    for other in (R.xi_in(seed + 1, step, [0], 8), R.xi_in(seed, step + 1, [0], 8), R.xi_in(seed + 2 ** 32, step, [0], 8),
                  R.xi_in(seed, step + 2 ** 32, [0], 8), R.xi_in(seed, step, [1], 8), R.xi_out(seed, step, [0], 8)):
        assert not np.any(other == z_in[:1, :8])


def test_float32_box_muller_stays_close_to_float64():
    """What the device tolerance (2e-5) leaves room for: float32 evaluation of the same uniforms, both ends of u included."""
    u = R.uniforms(11, 0, np.arange(4000), np.arange(16))
    u[0, 0] = [2.0 ** -24, 1 - 2.0 ** -24, 1 - 2.0 ** -24, 2.0 ** -24]
    z64, z32 = R.box_muller(u), R.box_muller(u, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z64).max() < 5e-6


# ---- the fold and the module on the CPU ----------------------------------------------------------------------------------------------
def _module(H=32, A=9, sigma0=0.5, dtype=th.float64, seed=0):
    th.manual_seed(seed)
    m = NoisyLinear(H, A, sigma0).to(dtype)
    with th.no_grad():
        m.weight_sigma.mul_(1 + th.rand_like(m.weight_sigma))       # distinct sigmas: a swapped index would show
        m.bias_sigma.mul_(1 + th.rand_like(m.bias_sigma))
    return m


def _np(t):
    return t.detach().numpy()


def test_initialisation():
    th.manual_seed(3)
    H, A = 64, 9
    m = NoisyLinear(H, A, 0.5)
    assert [n for n, _ in m.named_parameters()] == ["weight", "bias", "weight_sigma", "bias_sigma"]
    assert m.weight.shape == m.weight_sigma.shape == (A, H) and m.bias.shape == m.bias_sigma.shape == (A,)
    assert th.equal(m.weight_sigma, th.full((A, H), 0.5 / np.sqrt(H))) and th.equal(m.bias_sigma, th.full((A,), 0.5 / np.sqrt(H)))
    b = 1 / np.sqrt(H)
    for p in (m.weight, m.bias):
        assert float(p.abs().max()) <= b
    assert float(m.weight.abs().max()) > 0.9 * b and abs(float(m.weight.mean())) < 5 * b / np.sqrt(3 * A * H)
    assert m.noisy_mode == "off" and m.rng_state is None and "rng_state" not in m.state_dict()
    assert sorted(m.state_dict()) == ["bias", "bias_sigma", "weight", "weight_sigma"]
    with pytest.raises(TypeError):
        NoisyLinear(H, A)       # no default sigma0 in the package


def test_a_plain_heads_state_dict_fills_the_means_only():
    m, plain = _module(dtype=th.float32), nn.Linear(32, 9)
    sig = m.weight_sigma.detach().clone()
    res = m.load_state_dict(plain.state_dict(), strict=False)
    assert sorted(res.missing_keys) == ["bias_sigma", "weight_sigma"] and not res.unexpected_keys
    assert th.equal(m.weight, plain.weight) and th.equal(m.bias, plain.bias) and th.equal(m.weight_sigma, sig)


def test_bare_forward_is_the_plain_head_on_the_means():
    m = _module()
    x = th.randn(7, 32, dtype=th.float64)
    assert th.equal(m(x), nn.functional.linear(x, m.weight, m.bias))
    assert m.rng_state is None, "mode off consumes nothing"


def test_shared_mode_with_injected_noise_is_the_restatement():
    m = _module()
    H, A = 32, 9
    x = th.randn(7, H, dtype=th.float64)
    f_in, f_out = R.f(R.xi_in(5, 0, [0], H)[0]), R.f(R.xi_out(5, 0, [0], A)[0])
    m.noise = (th.from_numpy(f_in), th.from_numpy(f_out))
    with noisy_mode(m, "shared") as heads:
        assert heads == [m] and m.noisy_mode == "shared" and m.noise is None, "the fold is drawn on entry"
        q1, q2 = m(x), m(x)
    assert m.noisy_mode == "off" and th.equal(q1, q2), "one draw for the whole scope"
    W, b = R.fold(_np(m.weight), _np(m.weight_sigma), _np(m.bias), _np(m.bias_sigma), f_in, f_out)
    assert np.abs(_np(q1) - (_np(x) @ W.T + b)).max() <= 1e-13
    # the transpose: autograd through the fold equals the restatement's
    q1.backward(th.ones_like(q1) * th.arange(1, A + 1, dtype=th.float64))
    dq = np.ones((7, A)) * np.arange(1, A + 1)
    dW, dWs, db, dbs = R.fold_transpose(dq.T @ _np(x), dq.sum(0), f_in, f_out)
    for name, want in (("weight", dW), ("weight_sigma", dWs), ("bias", db), ("bias_sigma", dbs)):
        assert np.abs(_np(getattr(m, name).grad) - want).max() <= 1e-12, name
    got = ops.noisy_fold_bwd(th.from_numpy(dW), th.from_numpy(db), th.from_numpy(f_in), th.from_numpy(f_out))
    assert np.abs(_np(got[0]) - dWs).max() <= 1e-13 and np.abs(_np(got[1]) - dbs).max() <= 1e-13


def test_gradcheck_of_the_fold():
    th.manual_seed(1)
    A, H = 3, 5
    params = [th.randn(A, H, dtype=th.float64, requires_grad=True), th.rand(A, H, dtype=th.float64, requires_grad=True),
              th.randn(A, dtype=th.float64, requires_grad=True), th.rand(A, dtype=th.float64, requires_grad=True)]
    noise = (ops.noisy_f(th.randn(H, dtype=th.float64)), ops.noisy_f(th.randn(A, dtype=th.float64)))
    assert th.autograd.gradcheck(lambda *p: ops.noisy_fold(*p, noise=noise)[:2], params)
    out = ops.noisy_fold(*params, noise=noise)
    assert th.equal(out[2], noise[0]) and th.equal(out[3], noise[1])


def test_rows_mode_with_injected_noise_is_the_restatement():
    m = _module()
    N, H, A = 6, 32, 9
    x = th.randn(N, H, dtype=th.float64)
    f_in, f_out = R.f(R.xi_in(9, 2, np.arange(N), H)), R.f(R.xi_out(9, 2, np.arange(N), A))
    m.noise = (th.from_numpy(f_in), th.from_numpy(f_out))
    with noisy_mode(m, "rows"), th.no_grad():
        q = m(x)
    want, S = R.head_rows(_np(x), _np(m.weight), _np(m.weight_sigma), _np(m.bias), _np(m.bias_sigma), f_in, f_out)
    assert (np.abs(_np(q) - want) <= 1e-14 * S).all()
    per_row = np.stack([_np(x)[r] @ R.fold(_np(m.weight), _np(m.weight_sigma), _np(m.bias), _np(m.bias_sigma), f_in[r], f_out[r])[0].T
                        + R.fold(_np(m.weight), _np(m.weight_sigma), _np(m.bias), _np(m.bias_sigma), f_in[r], f_out[r])[1] for r in range(N)])
    assert (np.abs(want - per_row) <= 1e-14 * S).all(), "the factorised form IS a different weight matrix per row"
    with noisy_mode(m, "rows"), pytest.raises(_lib.UavGnnError, match="rollout"):
        m(x)            # with grad enabled
    with pytest.raises(ValueError, match="mode"):
        with noisy_mode(m, "on"):
            pass


def test_torch_draws_differ_between_scopes_and_rows():
    m = _module()
    x = th.ones(4, 32, dtype=th.float64)
    with noisy_mode(m, "shared"):
        a = m(x)
    with noisy_mode(m, "shared"):
        b = m(x)
    assert not th.equal(a, b) and th.equal(a[0], a[1])
    with noisy_mode(m, "rows"), th.no_grad():
        c = m(x)
    assert not th.equal(c[0], c[1]), "rows: every row has its own draw"
    assert m.rng_state is None, "no device pair on the CPU"


# ---- the agents and the learner ------------------------------------------------------------------------------------------------------
def _args(**kw):
    base = dict(device="cpu", hidden_size=32, c="tarmac", n_heads=4, n_layers=2, msg_size=8, key_size=4, n_rounds=1, dueling=False,
                mixer=False, double_q=True, lr=5e-4, gamma=0.99, polyak=0.999, max_seq_len=5, seed=0, anneal_lr=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


INFO = dict(obs_shape=dict(agent=2, ubs=2, gt=4), n_actions=9, n_agents=3, episode_limit=5)


def test_agents_build_the_head_their_args_ask_for():
    from uav_bs_ctrl_amd.agents import DrqnGnnAgent, GnnAgent, RnnAgent
    from uav_bs_ctrl_amd.agents.heads import DuelingLayer
    assert type(build_head(32, 9, _args())) is nn.Linear and type(build_head(32, 9, _args(dueling=True))) is DuelingLayer
    assert type(build_head(32, 9, _args(noisy=None))) is nn.Linear
    for cls, shape, kw in ((GnnAgent, INFO["obs_shape"], {}), (GnnAgent, INFO["obs_shape"], dict(c=None)), (RnnAgent, 14, dict(c=None, o="mlp")),
                           (DrqnGnnAgent, dict(gt=4, agent=2), {})):
        net = cls(shape, 9, _args(noisy=0.4, **kw))
        assert isinstance(net.f_out, NoisyLinear) and net.f_out.sigma0 == 0.4 and noisy_heads(net) == [net.f_out], cls.__name__
        assert type(cls(shape, 9, _args(**kw)).f_out) is nn.Linear
        with pytest.raises(ValueError, match="dueling together with noisy"):
            cls(shape, 9, _args(noisy=0.4, dueling=True, **kw))


def test_learner_option_leaves_the_callers_args_alone():
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner, QLearner
    args = _args()
    lr = MultiAgentQLearner(INFO, args, noisy=0.5)
    assert not hasattr(args, "noisy") and lr.args.noisy == 0.5
    assert len(lr._noisy_policy) == 1 and len(lr._noisy_target) == 1 and lr._noisy_policy[0] is lr.policy_net.f_out
    sd = lr.target_net.state_dict()
    assert th.equal(sd["f_out.weight_sigma"], lr.policy_net.f_out.weight_sigma), "the target network carries the sigmas too"
    assert lr.policy_net.f_out.weight_sigma.requires_grad and not lr.target_net.f_out.weight_sigma.requires_grad
    plain = MultiAgentQLearner(INFO, args)
    assert plain._noisy_policy == [] and type(plain.policy_net.f_out) is nn.Linear
    with plain.rollout_noise():
        pass
    for bad in ("0.5", True, (0.5,)):
        with pytest.raises(ValueError, match="sigma0"):
            MultiAgentQLearner(INFO, args, noisy=bad)
    with pytest.raises(ValueError, match="dueling together with noisy"):
        MultiAgentQLearner(INFO, _args(dueling=True), noisy=0.5)
    q_args = types.SimpleNamespace(device="cpu", agent="rnn", hidden_size=32, n_heads=4, n_layers=2, max_seq_len=5, gamma=0.99, polyak=0.9,
                                   batch_size=4, lr=1e-3, anneal_lr=False, seed=0)
    q = QLearner(dict(obs_shape=14, n_actions=5, episode_limit=10), q_args, noisy=0.3)
    assert isinstance(q.policy_net.f_out, NoisyLinear) and not hasattr(q_args, "noisy")


def test_modes_of_a_cpu_learner():
    """``rollout_noise`` sets the policy's heads to "rows" for its scope and nothing else; ``loss`` runs both networks "shared"."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    lr = MultiAgentQLearner(INFO, _args(c=None), noisy=0.5)
    pol, tgt = lr.policy_net.f_out, lr.target_net.f_out
    with lr.rollout_noise():
        assert pol.noisy_mode == "rows" and tgt.noisy_mode == "off"
    assert pol.noisy_mode == "off"
    seen = []
    lr._loss = lambda batch: seen.append((pol.noisy_mode, tgt.noisy_mode, pol._fold is not None, tgt._fold is not None)) or "out"
    assert lr.loss({}) == "out" and seen == [("shared", "shared", True, True)]
    assert pol.noisy_mode == tgt.noisy_mode == "off" and pol._fold is None


# ---- the run option ------------------------------------------------------------------------------------------------------------------
def test_the_key_enters_config_json_only_when_set():
    ns = RUN.check_args("exp3", small_args("exp3"))
    off = RUN.run_config("exp3", "debug", ns, seed=3, n_envs=4, n_test_envs=2)
    assert "noisy" not in off, "an absent key means off: existing run directories resume unchanged"
    on = RUN.run_config("exp3", "debug", ns, seed=3, n_envs=4, n_test_envs=2, noisy=0.5)
    assert on["noisy"] == 0.5 and {k: v for k, v in on.items() if k != "noisy"} == off
    back = json.loads(RUN.config_text(dict(seed=3, args=ns, uav_bs_ctrl_amd=on)))["uav_bs_ctrl_amd"]
    assert back["noisy"] == 0.5
    both = RUN.run_config("exp3", "debug", ns, prioritized=(0.6, 0.4, 0.9, 1e-3), compact_replay=True, returns=("nstep", 2), noisy=1)
    assert both["noisy"] == 1.0 and isinstance(both["noisy"], float) and both["returns"] == ["nstep", 2] and both["compact_replay"] is True
    for bad in (-0.1, "0.5", True, float("nan")):
        with pytest.raises(ValueError, match="noisy"):
            RUN.run_config("exp3", "debug", ns, noisy=bad)
    from uav_bs_ctrl_amd.sim import SingleUbsParams
    assert RUN.run_config("exp1", SingleUbsParams(), RUN.check_args("exp1", small_args("exp1")), noisy=0.5)["noisy"] == 0.5


def test_the_command_line_flag():
    ap = RUN._parser()
    base = ["--out", "d", "--exp", "exp3", "--env", "debug", "--args-json", "a.json"]
    assert ap.parse_args(base + ["--noisy", "0.5"]).noisy == 0.5 and ap.parse_args(base).noisy is None
    assert ap.parse_args(base + ["--noisy", "0.5", "--returns", "nstep", "3", "--compact-replay"]).noisy == 0.5
    for words in (["--noisy"], ["--noisy", "much"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + words)

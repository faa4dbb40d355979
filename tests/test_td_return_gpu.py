"""`-m gpu`: the TD-tail kernels (csrc/td_return.hip) through ``ops`` and the C ABI against the NumPy float64 restatement
(tests/td_return_ref.py) fed the fp32 inputs.

Cases: a thinned product of T in {1, 2, 7}, (B, C) in {(3, 8), (37, 1), (130, 8)} (24, 37 and 1040 threads: under one wavefront, a ragged
wavefront, several workgroups with a ragged tail), A in {5, 9}, Cr in {1, C}, weights absent / given, double_q on / off and returns in
{nstep 1, 2, 3, T, T + 5; lambda 0, 0.5, 1}; every value of every axis is hit (checked below).

The TD-error bound |td - td64| <= 8 T 2^-24 max(1, S), S = max|r| + max|V| + max|y64| + max|q|, is derived: each step of either recursion
makes at most six roundings of quantities bounded by S, and the carried error is multiplied by c lambda <= 1."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch as th

from tests import td_return_ref as R
from tests.util import assert_close

pytestmark = pytest.mark.gpu

GAMMA = 0.99
EPS = 2.0 ** -24
TS, BCS, AS = (1, 2, 7), ((3, 8), (37, 1), (130, 8)), (5, 9)
RETURNS = ("n1", "n2", "n3", "nT", "nT+5", "l0", "l0.5", "l1")


def _returns(tag, T):
    return {"n1": ("nstep", 1), "n2": ("nstep", 2), "n3": ("nstep", 3), "nT": ("nstep", T), "nT+5": ("nstep", T + 5), "l0": ("lambda", 0.0),
            "l0.5": ("lambda", 0.5), "l1": ("lambda", 1.0)}[tag]


def _cases():
    out, k = [], 0
    for T in TS:
        for B, C in BCS:
            for _ in range(4):
                out.append((T, B, C, AS[k % 2], bool((k // 2) % 2), bool((k // 3) % 2), bool((k // 5) % 2), RETURNS[(3 * k + k // 8) % 8]))
                k += 1
    return out


CASES = _cases()           # (T, B, C, A, per-agent rewards, weights, double_q, returns)
for _axis, _values in ((0, TS), (3, AS), (4, (False, True)), (5, (False, True)), (6, (False, True)), (7, RETURNS)):
    assert {c[_axis] for c in CASES} == set(_values), f"axis {_axis} of the case list misses a value"
assert {(c[1], c[2]) for c in CASES} == set(BCS)
for _T in TS:                   # every kind of return at every T, every thread count with and without weights
    assert {c[7] for c in CASES if c[0] == _T} >= {"n1", "nT+5", "l0.5"} or _T == 1
assert {c[7] for c in CASES if c[0] == 7} == set(RETURNS), "the longest sequence runs every target"
IDS = ["T{}-B{}-C{}-A{}-{}-{}-{}-{}".format(T, B, C, A, "rC" if pa else "r1", "w" if w else "now", "dq" if dq else "max", r)
       for T, B, C, A, pa, w, dq, r in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(T, B, C, A, per_agent, weighted, seed):
    """fp32 inputs on the host (NumPy) - Q values O(1) with a sign mix, dones with probability 0.2 forced on at t = 0 and t = T - 1, the
    maximum duplicated in two columns of some rows of both Q tensors."""
    rng = np.random.default_rng(seed)
    N = B * C
    agent_out = rng.standard_normal((T + 1, N, A)).astype(np.float32)
    target_out = rng.standard_normal((T, N, A)).astype(np.float32)
    for q in (agent_out[1:], target_out):
        rows = rng.random((T, N)) < 0.3
        j1, j2 = rng.integers(0, A, (T, N)), rng.integers(0, A, (T, N))
        top = q.max(2) + np.float32(0.5)
        for j in (j1, j2):
            cur = np.take_along_axis(q, j[..., None], 2)[..., 0]
            np.put_along_axis(q, j[..., None], np.where(rows, top, cur)[..., None], 2)
    acts = rng.integers(0, A, (T, N, 1)).astype(np.int64)
    rews = rng.standard_normal((T, B, C if per_agent else 1)).astype(np.float32)
    dones = (rng.random((T, B, 1)) < 0.2).astype(np.float32)
    dones[0, 0, 0] = 1.0
    dones[T - 1, B - 1, 0] = 1.0
    weights = (rng.random(B).astype(np.float32) + np.float32(0.05)) if weighted else None
    return agent_out, target_out, acts, rews, dones, weights


@functools.lru_cache(maxsize=None)
def _reference(T, B, C, A, per_agent, weighted, double_q, tag, seed):
    agent_out, target_out, acts, rews, dones, weights = _inputs(T, B, C, A, per_agent, weighted, seed)
    q, v, na = R.select(agent_out, target_out, acts, double_q)
    q3, v3 = q.reshape(T, B, C), v.reshape(T, B, C)
    y = R.targets(v3, rews, dones, np.float64(np.float32(GAMMA)), _returns(tag, T))
    loss, td, g = R.loss_and_td(q3, y, weights)
    S = float(np.abs(rews).max() + np.abs(v3).max() + np.abs(y).max() + np.abs(q3).max())
    return dict(q=q, v=v, na=na, y=y, loss=loss, td=td, g=g, bound=8 * T * EPS * max(1.0, S))


def _dev(x):
    return None if x is None else th.from_numpy(x).cuda()


def _default_td(agent_out, target_out, acts, rews, dones, weights, C, double_q):
    """TD errors of ``learner._td_loss``'s default (one-step) path on the same tensors."""
    from uav_bs_ctrl_amd.learner import MultiAgentQLearner
    me = types.SimpleNamespace(returns=None, double_q=double_q, n_agents=C, mixer=None, gamma=GAMMA)
    batch = dict(acts=acts, rews=rews, dones=dones, weights=weights if weights is not None else th.ones(rews.shape[1], device="cuda"))
    MultiAgentQLearner._td_loss(me, batch, target_out.shape[0], agent_out, target_out)
    return me.last_td[0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_against_float64(case):
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    T, B, C, A, per_agent, weighted, double_q, tag = case
    seed = CASES.index(case)
    N, returns = B * C, _returns(tag, T)
    ref = _reference(T, B, C, A, per_agent, weighted, double_q, tag, seed)
    agent_out, target_out, acts, rews, dones, weights = (_dev(x) for x in _inputs(T, B, C, A, per_agent, weighted, seed))
    what = IDS[seed]

    # select: copies and indices are exact, ties go to the first index
    a = agent_out.clone().requires_grad_(True)
    q, v, na = ops.td_select(a, target_out, acts, double_q, return_acts=True)
    assert na.dtype == th.int32 and np.array_equal(na.cpu().numpy(), ref["na"]), f"{what}: next_acts"
    assert np.array_equal(q.detach().cpu().numpy().astype(np.float64), ref["q"]), f"{what}: qvals"
    assert np.array_equal(v.cpu().numpy().astype(np.float64), ref["v"]), f"{what}: next_vals"
    assert q.requires_grad and not v.requires_grad

    # targets, TD errors, loss
    loss, td = ops.td_return_loss(q.view(T, B, C), v.view(T, B, C), rews, dones, weights, GAMMA, returns)
    err = float(np.abs(td.cpu().numpy().astype(np.float64) - ref["td"]).max())
    print(f"{what}: max |td - td64| = {err:.3e} (bound {ref['bound']:.3e}); loss {float(loss.detach()):.8e} vs {ref['loss']:.8e}")
    assert tuple(td.shape) == (T, B, C) and not td.requires_grad and loss.dim() == 0
    assert err <= ref["bound"], f"{what}: TD error {err:.3e} above {ref['bound']:.3e}"
    assert_close(loss, th.tensor(ref["loss"], dtype=th.float64), 1e-5, f"{what}: loss")

    # d_agent_out through the C ABI into a NaN-filled buffer: every element is written
    g, = th.autograd.grad(loss, q, retain_graph=True)
    w64 = np.ones(B) if weights is None else weights.cpu().numpy().astype(np.float64)
    coef = (2.0 * w64 / (T * B * C)).reshape(1, B, 1)
    g_err = np.abs(g.view(T, B, C).cpu().numpy().astype(np.float64) - ref["g"])
    assert (g_err <= coef * ref["bound"] + 4 * EPS * np.abs(ref["g"])).all(), f"{what}: g, worst {g_err.max():.3e}"
    d_out = th.full((T + 1, N, A), float("nan"), device="cuda")
    rc = L.lib().uavgnn_td_select_bwd(g.data_ptr(), acts.data_ptr(), None, T, N, A, d_out.data_ptr(), L.stream())
    assert rc == 0
    d64 = R.d_agent_out(ref["g"].reshape(T, N), acts.cpu().numpy(), A)
    chosen = np.zeros((T + 1, N, A), dtype=bool)
    np.put_along_axis(chosen[:-1], acts.cpu().numpy(), True, 2)
    got = d_out.cpu().numpy()
    assert (got[~chosen] == 0.0).all() and not np.isnan(got).any(), f"{what}: d_agent_out off the chosen actions / in row T"
    lim = (np.repeat(coef, C, axis=2) * ref["bound"]).reshape(1, N, 1) + 4 * EPS * np.abs(d64)
    assert (np.abs(got.astype(np.float64) - d64) <= lim)[chosen].all(), f"{what}: d_agent_out at the chosen actions"
    # the optional device scalar: a power of two scales exactly; autograd takes the same route
    half = th.full((T + 1, N, A), float("nan"), device="cuda")
    scale = th.tensor([0.5], device="cuda")
    assert L.lib().uavgnn_td_select_bwd(g.data_ptr(), acts.data_ptr(), scale.data_ptr(), T, N, A, half.data_ptr(), L.stream()) == 0
    assert th.equal(half, d_out * 0.5)
    loss.backward()
    assert th.equal(a.grad, d_out), f"{what}: autograd's d_agent_out"

    # determinism: a second call gives the same bits (td straight into a caller's buffer)
    td_out = th.full((T, B, C), float("nan"), device="cuda")
    q2, v2 = ops.td_select(agent_out, target_out, acts, double_q)
    loss2, td2 = ops.td_return_loss(q2.view(T, B, C), v2.view(T, B, C), rews, dones, weights, GAMMA, returns, td_out=td_out, workspace={})
    assert td2.data_ptr() == td_out.data_ptr() and th.equal(td2, td) and th.equal(loss2, loss.detach()), f"{what}: two calls differ"

    if tag in ("n1", "l0") or (tag == "nT" and T == 1):
        assert th.equal(td, _default_td(agent_out, target_out, acts, rews, dones, weights, C, double_q)), f"{what}: not the default path's bits"


def test_one_step_settings_are_the_default_paths_bits_at_every_shape():
    from uav_bs_ctrl_amd import ops
    for i, (T, (B, C), A) in enumerate([(T, bc, A) for T in TS for bc in BCS for A in AS]):
        per_agent, weighted, double_q = bool(i % 2), bool((i // 2) % 2), bool((i // 3) % 2)
        agent_out, target_out, acts, rews, dones, weights = (_dev(x) for x in _inputs(T, B, C, A, per_agent, weighted, 100 + i))
        want = _default_td(agent_out, target_out, acts, rews, dones, weights, C, double_q)
        q, v = ops.td_select(agent_out, target_out, acts, double_q)
        for returns in (("nstep", 1), ("lambda", 0.0)):
            _, td = ops.td_return_loss(q.view(T, B, C), v.view(T, B, C), rews, dones, weights, GAMMA, returns)
            assert th.equal(td, want), f"T={T} B={B} C={C} A={A} {returns}"


def test_argument_errors_are_codes_and_launch_nothing():
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    T, B, C, A = 2, 3, 4, 5
    N = B * C
    f = lambda *s: th.full(s, 7.0, device="cuda")   # noqa: E731
    ao, to, acts = f(T + 1, N, A), f(T, N, A), th.zeros(T, N, dtype=th.int64, device="cuda")
    q, v, na = f(T, N), f(T, N), th.full((T, N), 7, dtype=th.int32, device="cuda")
    p = lambda t: t.data_ptr()   # noqa: E731
    EINVAL = L.UAVGNN_EINVAL
    assert lib.uavgnn_td_select_fwd(None, p(to), p(acts), T, N, A, 1, p(q), p(v), p(na), None) == EINVAL
    assert lib.uavgnn_td_select_fwd(p(ao), None, p(acts), T, N, A, 1, p(q), p(v), p(na), None) == EINVAL
    assert lib.uavgnn_td_select_fwd(p(ao), p(to), None, T, N, A, 1, p(q), p(v), p(na), None) == EINVAL
    assert lib.uavgnn_td_select_fwd(p(ao), p(to), p(acts), T, N, A, 1, None, p(v), p(na), None) == EINVAL
    assert lib.uavgnn_td_select_fwd(p(ao), p(to), p(acts), 0, N, A, 1, p(q), p(v), p(na), None) == EINVAL
    assert lib.uavgnn_td_select_fwd(p(ao), p(to), p(acts), T, 0, A, 1, p(q), p(v), p(na), None) == EINVAL
    assert lib.uavgnn_td_select_fwd(p(ao), p(to), p(acts), T, N, 0, 1, p(q), p(v), p(na), None) == EINVAL
    d = f(T + 1, N, A)
    assert lib.uavgnn_td_select_bwd(None, p(acts), None, T, N, A, p(d), None) == EINVAL
    assert lib.uavgnn_td_select_bwd(p(q), None, None, T, N, A, p(d), None) == EINVAL
    assert lib.uavgnn_td_select_bwd(p(q), p(acts), None, T, N, A, None, None) == EINVAL
    assert lib.uavgnn_td_select_bwd(p(q), p(acts), None, T, N, -1, p(d), None) == EINVAL
    G = lib.uavgnn_td_return_partials(B, C)
    assert G == 1 and lib.uavgnn_td_return_partials(130, 8) == 17 and lib.uavgnn_td_return_partials(0, 8) == EINVAL
    q3, v3, r, dn, w = f(T, B, C), f(T, B, C), f(T, B, 1), f(T, B, 1), f(B)
    td, g, loss, ws = f(T, B, C), f(T, B, C), f(1), f(G)

    def ret(qq=q3, vv=v3, rr=r, Cr=1, dd=dn, ww=w, T_=T, B_=B, C_=C, mode=0, n=2, lam=0.5, td_=td, g_=g, loss_=loss, ws_=ws, G_=G):
        g0 = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return lib.uavgnn_td_return_fwd(g0(qq), g0(vv), g0(rr), Cr, g0(dd), g0(ww), T_, B_, C_, GAMMA, mode, n, lam, g0(td_), g0(g_), g0(loss_),
                                        g0(ws_), G_, None)
    for kw in (dict(qq=None), dict(vv=None), dict(rr=None), dict(dd=None), dict(td_=None), dict(g_=None), dict(loss_=None), dict(ws_=None),
               dict(Cr=2), dict(Cr=0), dict(T_=0), dict(B_=0), dict(C_=0), dict(mode=2), dict(mode=-1), dict(n=0), dict(mode=1, lam=1.5),
               dict(mode=1, lam=-0.1), dict(mode=1, lam=float("nan")), dict(G_=G + 1), dict(G_=0)):
        assert ret(**kw) == EINVAL, kw
    th.cuda.synchronize()
    for t in (q, v, td, g, loss, ws, d):
        assert bool((t == 7.0).all()), "a refused call wrote an output"
    assert bool((na == 7).all())
    assert ret(ww=None) == 0 and ret(mode=1, n=0) == 0 and ret(Cr=C, rr=q3) == 0, "weights may be NULL; lam / n_step are read by their mode only"
    th.cuda.synchronize()
    assert bool(th.isfinite(loss).all())

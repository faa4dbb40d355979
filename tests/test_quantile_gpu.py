"""The kernels of csrc/qr/quantile.hip on the GPU against the NumPy float64 restatement of include/uavgnn_qr.h (tests/qr_ref.py), through
raw ``_lib.qr()`` calls and through ``ops``.

Bound: the project's parity rule ``assert_close(..., 1e-5)`` (rtol = 1e-5, atol = 1e-5 max|ref|) for theta_a,
theta_next, q_pol, td, g, loss and the select's backward.  A plain fp32 evaluation with sequential sums needs at most 1e-7 under that rule
at K = 8 ... 64 on N(0, 1) and N(0, 25) inputs, so the bound leaves 100 x margin; the gradient is continuous at u = 0 and |u| = kappa, so
no branch of the loss needs special handling.  Every output is filled with NaN (-1 for the int32 actions) before a call: an element that
the header says is written and is not shows.  Every call is launched twice and the bits compared."""
import os
import re

import numpy as np
import pytest
import torch as th

from tests import qr_ref as R
from tests.util import assert_close

pytestmark = pytest.mark.gpu

GAMMA = 0.9


def _qr():
    from uav_bs_ctrl_amd import _lib as L
    return L, L.qr()


def _constants():
    """kThreads and kGridCap of csrc/qr/quantile.hip: the past-the-cap cases are sized from the kernel's own numbers."""
    from uav_bs_ctrl_amd import build
    text = open(os.path.join(build.QR_CSRC, "quantile.hip")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) for name in ("kThreads", "kGridCap"))


def _inputs(T, B, C, A, K, seed, scale=1.0):
    g = th.Generator().manual_seed(seed)
    N = B * C
    d = dict(theta_pol=scale * th.randn(T + 1, N, A, K, generator=g), theta_tgt=scale * th.randn(T, N, A, K, generator=g),
             acts=th.randint(0, A, (T, N), generator=g), rews_1=th.randn(T, B, 1, generator=g), rews_C=th.randn(T, B, C, generator=g),
             dones=th.zeros(T, B, 1), weights=th.rand(B, generator=g) + 0.5)
    d["dones"][0, 0] = 1.0                      # t = 0
    d["dones"][T // 2, 1] = 1.0                 # mid-sequence
    d["dones"][T - 1, 2] = 1.0                  # the last step
    return d


def _raw_select(theta_pol, theta_tgt, acts, double_q, with_acts=True, with_q=True):
    L, Q = _qr()
    T1, N, A, K = theta_pol.shape
    T = T1 - 1
    outs = []
    for _ in range(2):
        theta_a = th.full((T, N, K), float("nan"), device="cuda")
        theta_next = th.full((T, N, K), float("nan"), device="cuda")
        next_acts = th.full((T, N), -1, dtype=th.int32, device="cuda")
        q_pol = th.full((T1, N, A), float("nan"), device="cuda")
        rc = Q.uavgnn_qr_select_fwd(theta_pol.data_ptr(), theta_tgt.data_ptr(), acts.data_ptr(), T, N, A, K, int(double_q), theta_a.data_ptr(),
                                    theta_next.data_ptr(), next_acts.data_ptr() if with_acts else None, q_pol.data_ptr() if with_q else None,
                                    L.stream())
        L.check(rc, "uavgnn_qr_select_fwd")
        outs.append((theta_a, theta_next, next_acts, q_pol))
    th.cuda.synchronize()
    for a, b in zip(*outs):
        assert th.equal(a.view(th.int32), b.view(th.int32)), "two launches, equal bits"
    return outs[0]


def _raw_select_bwd(d_theta_a, acts, A):
    L, Q = _qr()
    T, N, K = d_theta_a.shape
    outs = []
    for _ in range(2):
        out = th.full((T + 1, N, A, K), float("nan"), device="cuda")
        L.check(Q.uavgnn_qr_select_bwd(d_theta_a.data_ptr(), acts.data_ptr(), T, N, A, K, out.data_ptr(), L.stream()), "uavgnn_qr_select_bwd")
        outs.append(out)
    th.cuda.synchronize()
    assert th.equal(outs[0].view(th.int32), outs[1].view(th.int32)), "two launches, equal bits"
    return outs[0]


def _raw_loss(theta_a, theta_next, rews, dones, weights, n_step, kappa=1.0, gamma=GAMMA):
    L, Q = _qr()
    T, B, C, K = theta_a.shape
    G = Q.uavgnn_qr_loss_partials(T, B, C, K)
    assert G >= 1
    outs = []
    for _ in range(2):
        td = th.full((T, B, C), float("nan"), device="cuda")
        g = th.full((T, B, C, K), float("nan"), device="cuda")
        loss = th.full((1,), float("nan"), device="cuda")
        ws = th.full((G,), float("nan"), device="cuda")
        rc = Q.uavgnn_qr_loss_fwd(theta_a.data_ptr(), theta_next.data_ptr(), rews.data_ptr(), rews.shape[-1], dones.data_ptr(),
                                  None if weights is None else weights.data_ptr(), T, B, C, K, gamma, n_step, kappa, td.data_ptr(),
                                  g.data_ptr(), loss.data_ptr(), ws.data_ptr(), G, L.stream())
        L.check(rc, "uavgnn_qr_loss_fwd")
        outs.append((td, g, loss, ws))
    th.cuda.synchronize()
    for a, b in zip(*outs):
        assert th.equal(a.view(th.int32), b.view(th.int32)), "two launches, equal bits"
    return outs[0][:3]


def _no_nan(*tensors):
    for t in tensors:
        assert not bool(th.isnan(t).any()), "an element the header says is written was not"


# ---- select --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 32, 64])
@pytest.mark.parametrize("A", [1, 9])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("T", [1, 3])
def test_select_and_its_backward_against_the_restatement(K, A, C, T):
    B = 5                                       # T B C rows: no multiple of 64 / K rows per wavefront at any K
    d = _inputs(T, B, C, A, K, seed=K + A + 7 * C + T)
    pol, tgt, acts = d["theta_pol"].cuda(), d["theta_tgt"].cuda(), d["acts"].cuda()
    for double_q in (True, False):
        theta_a, theta_next, next_acts, q_pol = _raw_select(pol, tgt, acts, double_q)
        ra, rn, racts, rq = R.select(d["theta_pol"], d["theta_tgt"], d["acts"], double_q)
        _no_nan(theta_a, theta_next, q_pol)
        assert np.array_equal(next_acts.cpu().numpy(), racts), "random rows have no near-tie: the fp32 choice is the float64 one"
        assert_close(theta_a, th.from_numpy(ra), 1e-5, "theta_a")
        assert_close(theta_next, th.from_numpy(rn), 1e-5, "theta_next")
        assert_close(q_pol, th.from_numpy(rq), 1e-5, "q_pol")
        assert th.equal(theta_a.cpu(), th.from_numpy(ra).float()) and th.equal(theta_next.cpu(), th.from_numpy(rn).float()), "copies"
        # the optional outputs: NULL changes nothing of the others
        a2, n2, acts2, q2 = _raw_select(pol, tgt, acts, double_q, with_acts=False, with_q=False)
        assert th.equal(a2, theta_a) and th.equal(n2, theta_next) and bool((acts2 == -1).all()) and bool(th.isnan(q2).all())
    d_theta_a = th.randn(T, B * C, K, generator=th.Generator().manual_seed(1)).cuda()
    got = _raw_select_bwd(d_theta_a, acts, A)
    want = R.select_bwd(d_theta_a.cpu().numpy(), d["acts"], A)
    _no_nan(got)
    assert_close(got, th.from_numpy(want), 1e-5, "select backward")
    assert bool((got[T] == 0).all()) and int((got != 0).sum()) == int((d_theta_a != 0).sum()), "exact zeros off the taken action and in row T"


@pytest.mark.parametrize("K", [8, 64])
def test_ties_nans_and_out_of_range_actions(K):
    T, B, C, A = 3, 5, 3, 9
    N = B * C
    d = _inputs(T, B, C, A, K, seed=3)
    pol, tgt = d["theta_pol"].clone(), d["theta_tgt"].clone()
    # a tie in the action means: two actions with the same quantiles, above everything else -> the first wins
    pol[1, 0, 6], pol[1, 0, 2] = 50.0 + pol[1, 0, 4], 50.0 + pol[1, 0, 4]
    tgt[0, 0, 7], tgt[0, 0, 3] = 50.0 + tgt[0, 0, 5], 50.0 + tgt[0, 0, 5]
    # a NaN counts as the maximum, the first NaN wins
    pol[2, 1, 5, K - 1], pol[2, 1, 8, 0] = float("nan"), float("nan")
    tgt[1, 1, 4, 1], tgt[1, 1, 6, 2] = float("nan"), float("nan")
    acts = d["acts"].clone()
    acts[2, 1] = 0                                   # not one of the NaN rows above
    acts[0, 2], acts[T - 1, N - 1] = A, -1           # outside [0, A)
    pc, tc, ac = pol.cuda(), tgt.cuda(), acts.cuda()
    for double_q in (True, False):
        theta_a, theta_next, next_acts, q_pol = _raw_select(pc, tc, ac, double_q)
        ra, rn, racts, rq = R.select(pol, tgt, acts, double_q)
        got_acts = next_acts.cpu().numpy()
        assert np.array_equal(got_acts, racts)
        if double_q:
            assert got_acts[0, 0] == 2 and got_acts[1, 1] == 5
        else:
            assert got_acts[0, 0] == 3 and got_acts[1, 1] == 4
        nan_rows = th.isnan(theta_a).all(-1).cpu()
        assert nan_rows[0, 2] and nan_rows[T - 1, N - 1] and int(nan_rows.sum()) == 2 and int(th.isnan(theta_a).sum()) == 2 * K, \
            "an index outside [0, A): a NaN row, nothing else disturbed"
        assert np.array_equal(theta_a.cpu().numpy(), ra.astype(np.float32), equal_nan=True)
        assert np.array_equal(theta_next.cpu().numpy(), rn.astype(np.float32), equal_nan=True)
        assert_close(th.nan_to_num(q_pol, nan=0.0), th.nan_to_num(th.from_numpy(rq), nan=0.0), 1e-5, "q_pol")
        assert np.array_equal(np.isnan(q_pol.cpu().numpy()), np.isnan(rq))
    d_theta_a = th.ones(T, N, K, device="cuda")
    got = _raw_select_bwd(d_theta_a, ac, A)
    assert th.equal(got.cpu(), th.from_numpy(R.select_bwd(np.ones((T, N, K)), acts, A)).float()) and float(got.sum()) == (T * N - 2) * K


# ---- loss ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 32, 64])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_loss_against_the_restatement(K, C, T, scale):
    B, A = 5, 1
    d = _inputs(T, B, C, A, K, seed=11 * K + C + T, scale=scale)
    theta_a = d["theta_pol"][:T, :, 0].reshape(T, B, C, K).contiguous()
    theta_next = d["theta_tgt"][:, :, 0].reshape(T, B, C, K).contiguous()
    ta, tn, dones = theta_a.cuda(), theta_next.cuda(), d["dones"].cuda()
    for n_step in (1, 2, 7):                    # 7 > T: the whole rest of the sequence
        for rews in (d["rews_1"], d["rews_C"]):
            for weights in (None, d["weights"]):
                td, g, loss = _raw_loss(ta, tn, rews.cuda(), dones, None if weights is None else weights.cuda(), n_step)
                rl, rg, rtd, _, _ = R.loss(theta_a, theta_next, rews, d["dones"], None if weights is None else weights.numpy(), GAMMA, n_step, 1.0)
                _no_nan(td, g, loss)
                what = f"K={K} C={C} T={T} n_step={n_step} Cr={rews.shape[-1]} weights={weights is not None}"
                assert_close(td, th.from_numpy(rtd), 1e-5, "td " + what)
                assert_close(g, th.from_numpy(rg), 1e-5, "g " + what)
                assert_close(loss, th.tensor([rl], dtype=th.float64), 1e-5, "loss " + what)


@pytest.mark.parametrize("kappa", [0.5, 2.0])
def test_loss_at_other_thresholds(kappa):
    T, B, C, K = 3, 5, 3, 32
    d = _inputs(T, B, C, 1, K, seed=5, scale=2.0)
    theta_a = d["theta_pol"][:T, :, 0].reshape(T, B, C, K).contiguous()
    theta_next = d["theta_tgt"][:, :, 0].reshape(T, B, C, K).contiguous()
    td, g, loss = _raw_loss(theta_a.cuda(), theta_next.cuda(), d["rews_C"].cuda(), d["dones"].cuda(), d["weights"].cuda(), 2, kappa)
    rl, rg, rtd, _, _ = R.loss(theta_a, theta_next, d["rews_C"], d["dones"], d["weights"].numpy(), GAMMA, 2, kappa)
    assert_close(td, th.from_numpy(rtd), 1e-5, "td")
    assert_close(g, th.from_numpy(rg), 1e-5, "g")
    assert_close(loss, th.tensor([rl], dtype=th.float64), 1e-5, "loss")


def test_closed_form_on_the_device():
    """All theta equal, all y equal, 0 < u <= kappa: l = (K/2) u^2 / (2 kappa) (tests/test_quantile_host.py has the derivation)."""
    for K in (8, 16, 32, 64):
        T, B, C, u = 1, 5, 1, 0.75
        theta = th.full((T, B, C, K), 0.25, device="cuda")
        nxt = th.full((T, B, C, K), 5.0, device="cuda")
        rews = th.full((T, B, 1), 0.25 + u, device="cuda")
        td, g, loss = _raw_loss(theta, nxt, rews, th.ones(T, B, 1, device="cuda"), None, 1)
        want = (K / 2) * u * u / 2
        assert abs(float(loss) - want) <= 1e-6 * want and bool((td == -u).all())


# ---- through ops: autograd, td_out, workspace ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,double_q,n_step", [(8, True, 2), (32, False, 1), (64, True, 7)])
def test_ops_chain_and_its_gradient(K, double_q, n_step):
    from uav_bs_ctrl_amd import ops
    T, B, C, A = 3, 5, 3, 9
    d = _inputs(T, B, C, A, K, seed=K)
    pol = d["theta_pol"].cuda().requires_grad_(True)
    tgt, acts = d["theta_tgt"].cuda(), d["acts"].cuda().unsqueeze(-1)
    ws, td_out = {}, th.full((T, B, C), float("nan"), device="cuda")
    theta_a, theta_next, next_acts, q_pol = ops.qr_select(pol, tgt, acts, double_q)
    assert theta_a.requires_grad and not theta_next.requires_grad and not q_pol.requires_grad and next_acts.dtype == th.int32
    loss, td = ops.qr_loss(theta_a.view(T, B, C, K), theta_next.view(T, B, C, K), d["rews_1"].cuda(), d["dones"].cuda(), d["weights"].cuda(),
                           GAMMA, n_step, td_out=td_out, workspace=ws)
    assert td is td_out and len(ws) == 1
    (3.0 * loss).backward()
    ra, rn, racts, rq = R.select(d["theta_pol"], d["theta_tgt"], d["acts"], double_q)
    rl, rg, rtd, _, _ = R.loss(ra.reshape(T, B, C, K), rn.reshape(T, B, C, K), d["rews_1"], d["dones"], d["weights"].numpy(), GAMMA, n_step, 1.0)
    assert_close(loss, th.tensor(rl, dtype=th.float64), 1e-5, "loss")
    assert_close(td_out, th.from_numpy(rtd), 1e-5, "td")
    assert_close(q_pol, th.from_numpy(rq), 1e-5, "q_pol")
    assert_close(pol.grad, th.from_numpy(3.0 * R.select_bwd(rg.reshape(T, B * C, K), d["acts"], A)), 1e-5, "d theta_pol")
    # the torch arm on the device in float64 agrees too (what the probe compares against)
    a64, n64, acts64, _ = ops.qr_select(pol.detach().double(), tgt.double(), acts, double_q)
    l64, td64 = ops.qr_loss(a64.view(T, B, C, K), n64.view(T, B, C, K), d["rews_1"].cuda().double(), d["dones"].cuda().double(),
                            d["weights"].cuda().double(), GAMMA, n_step)
    assert abs(float(l64) - rl) <= 1e-12 * abs(rl) and th.equal(acts64.cpu(), th.from_numpy(racts))
    # a second call reuses the workspace buffer and gives the same bits
    loss2, td2 = ops.qr_loss(theta_a.detach().view(T, B, C, K), theta_next.view(T, B, C, K), d["rews_1"].cuda(), d["dones"].cuda(),
                             d["weights"].cuda(), GAMMA, n_step, workspace=ws)
    assert len(ws) == 1 and th.equal(loss2, loss.detach()) and th.equal(td2, td_out)


@pytest.mark.parametrize("K", [8, 32, 64])
def test_mean_fold_and_the_head_modes(K):
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.agents.heads import QuantileLinear, quantile_mode
    L, Q = _qr()
    A, H, ld = 9, 32, 40
    g = th.Generator().manual_seed(K)
    Wp = th.randn(A * K, ld, generator=g).cuda()
    b = th.randn(A * K, generator=g).cuda()
    W_bar, b_bar = th.full((A, H), float("nan"), device="cuda"), th.full((A,), float("nan"), device="cuda")
    L.check(Q.uavgnn_qr_mean_fold(Wp.data_ptr(), ld, b.data_ptr(), A, K, H, W_bar.data_ptr(), b_bar.data_ptr(), L.stream()), "mean_fold")
    rW, rb = R.mean_fold(Wp[:, :H].cpu().numpy(), b.cpu().numpy(), A, K)
    _no_nan(W_bar, b_bar)
    assert_close(W_bar, th.from_numpy(rW), 1e-5, "W_bar (row stride > H)")
    assert_close(b_bar, th.from_numpy(rb), 1e-5, "b_bar")
    W2, b2 = ops.quantile_mean_fold(Wp[:, :H], b, A, K)
    assert th.equal(W2, W_bar) and th.equal(b2, b_bar), "ops passes the row stride on"
    th.manual_seed(0)
    m = QuantileLinear(H, A, K).cuda()
    x = th.randn(21, H, device="cuda")
    with th.no_grad():
        q = m(x)
        with quantile_mode(m, "quantiles"):
            theta = m(x)
    assert tuple(q.shape) == (21, A) and tuple(theta.shape) == (21, A * K)
    assert_close(q, theta.double().view(21, A, K).mean(-1), 1e-5, "mean mode against the quantiles' mean")
    q_grad = m(x)                               # under grad: the torch expression
    assert q_grad.requires_grad
    assert_close(q_grad, q, 1e-5, "mean mode with and without autograd")


# ---- past the grid caps --------------------------------------------------------------------------------------------------------------
def test_select_kernels_past_their_grid_caps():
    from uav_bs_ctrl_amd import ops
    threads, cap = _constants()
    K, A, T = 8, 2, 3
    N = (cap * (threads // K)) // (T + 1) + 3 * (threads // K) + 5        # (T + 1) N row groups: past the cap, ragged
    assert (T + 1) * N > cap * (threads // K) and ((T + 1) * N) % (threads // K) != 0
    assert (T + 1) * N * A * K > cap * threads, "the backward's element count is past its cap too"
    g = th.Generator().manual_seed(0)
    pol, tgt = th.randn(T + 1, N, A, K, generator=g), th.randn(T, N, A, K, generator=g)
    acts = th.randint(0, A, (T, N), generator=g)
    for double_q in (True, False):
        theta_a, theta_next, next_acts, q_pol = _raw_select(pol.cuda(), tgt.cuda(), acts.cuda(), double_q)
        wa, wn, wacts, wq = ops.qr_select_torch(pol.double(), tgt.double(), acts, double_q)
        _no_nan(theta_a, theta_next, q_pol)
        # rows whose two action means differ by less than fp32 can tell may choose either
        pick = (pol[1:] if double_q else tgt).double().sum(-1)
        clear = ((pick[..., 0] - pick[..., 1]).abs() > 1e-5 * pick.abs().max()).numpy()
        assert clear.mean() > 0.999 and np.array_equal(next_acts.cpu().numpy()[clear], wacts.numpy()[clear])
        assert th.equal(theta_a.cpu(), wa.float())
        assert th.equal(theta_next.cpu()[th.from_numpy(clear)], wn.float()[th.from_numpy(clear)])
        assert_close(q_pol, wq, 1e-5, "q_pol")
    d_theta_a = th.randn(T, N, K, generator=g)
    got = _raw_select_bwd(d_theta_a.cuda(), acts.cuda(), A)
    _no_nan(got)
    want = th.zeros(T + 1, N, A, K)
    want[:T].scatter_(2, acts.view(T, N, 1, 1).expand(T, N, 1, K), d_theta_a.view(T, N, 1, K))
    assert th.equal(got.cpu(), want)


def test_loss_kernel_past_its_grid_cap():
    from uav_bs_ctrl_amd import ops
    L, Q = _qr()
    threads, cap = _constants()
    K, T, C = 8, 3, 1
    B = (cap * (threads // K)) // T + 3 * (threads // K) + 5
    rows = T * B * C
    assert rows > cap * (threads // K) and rows % (threads // K) != 0 and Q.uavgnn_qr_loss_partials(T, B, C, K) == cap
    g = th.Generator().manual_seed(1)
    theta_a, theta_next = th.randn(T, B, C, K, generator=g), th.randn(T, B, C, K, generator=g)
    rews, weights = th.randn(T, B, 1, generator=g), th.rand(B, generator=g) + 0.5
    dones = (th.rand(T, B, 1, generator=g) < 0.2).float()
    td, gr, loss = _raw_loss(theta_a.cuda(), theta_next.cuda(), rews.cuda(), dones.cuda(), weights.cuda(), 2)
    _no_nan(td, gr, loss)
    ta64 = theta_a.double().requires_grad_(True)          # the float64 torch arm: held to the restatement at 1e-12 by the host tests
    l64, td64 = ops.qr_loss_torch(ta64, theta_next.double(), rews.double(), dones.double(), weights.double(), GAMMA, 2, 1.0)
    l64.backward()
    assert_close(td, td64, 1e-5, "td")
    assert_close(gr, ta64.grad, 1e-5, "g")
    assert_close(loss, l64.detach().view(1), 1e-5, "loss")


def test_mean_fold_past_its_grid_cap():
    L, Q = _qr()
    threads, cap = _constants()
    A, K = 64, 8
    H = (cap * threads) // A + 11
    assert A * H + A > cap * threads
    g = th.Generator().manual_seed(2)
    W, b = th.randn(A * K, H, generator=g), th.randn(A * K, generator=g)
    Wc, bc = W.cuda(), b.cuda()
    W_bar, b_bar = th.full((A, H), float("nan"), device="cuda"), th.full((A,), float("nan"), device="cuda")
    L.check(Q.uavgnn_qr_mean_fold(Wc.data_ptr(), H, bc.data_ptr(), A, K, H, W_bar.data_ptr(), b_bar.data_ptr(), L.stream()), "mean_fold")
    _no_nan(W_bar, b_bar)
    assert_close(W_bar, W.double().view(A, K, H).sum(1) / K, 1e-5, "W_bar")
    assert_close(b_bar, b.double().view(A, K).sum(1) / K, 1e-5, "b_bar")

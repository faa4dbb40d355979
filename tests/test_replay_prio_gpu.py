"""`-m gpu`: the prioritised replay's kernels (csrc/replay_prio.hip) through the C ABI against the NumPy restatement of their rules
(tests/replay_prio_ref.py): the drawn slots bit for bit, the weights within two float32 ulps, the updated priorities within one
fixed-point unit (exactly at alpha = 0 and 1), and every word the entries must not touch."""
import numpy as np
import pytest
import torch as th

from tests import replay_prio_ref as P

pytestmark = pytest.mark.gpu

SEED = (0x1234_5678 << 32) | 0x9abc_def1                                         # both key words in use
BETA = 0.4
GUARD = 0x5A5A5A5A


def _lib():
    from uav_bs_ctrl_amd import _lib as L
    return L


def _dev_u32(values):
    """uint32 values as the int32 device tensor the entries take the address of."""
    return th.from_numpy(np.asarray(values, dtype=np.uint64).astype(np.uint32).view(np.int32).copy()).cuda()


def _host_u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.uint64)


def _workspace(capacity, B, fill=None):
    n = _lib().lib().uavgnn_replay_prio_workspace_bytes(capacity, B)
    assert n > 0 and n % 16 == 0
    ws = th.empty(n, dtype=th.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws


def _tensors(size, draws, seed=SEED):
    return (th.tensor([3, size], dtype=th.int64, device="cuda"), th.tensor([seed, draws], dtype=th.int64, device="cuda"),
            th.zeros(1, dtype=th.int32, device="cuda"))


def _draw(state, rng, prio, B, status, ws, beta=BETA):
    """One draw through the C ABI with one guard word on either side of idx and of weights."""
    L = _lib()
    idx = th.full((B + 2,), -7, dtype=th.int64, device="cuda")
    w = th.full((B + 2,), -7.0, dtype=th.float32, device="cuda")
    before = prio.clone()
    L.check(L.lib().uavgnn_replay_prio_sample(state.data_ptr(), rng.data_ptr(), prio.numel(), B, prio.data_ptr(), beta, idx.data_ptr() + 8,
                                              w.data_ptr() + 4, status.data_ptr(), ws.data_ptr(), L.stream()), "uavgnn_replay_prio_sample")
    assert idx[0] == -7 and idx[-1] == -7 and w[0] == -7 and w[-1] == -7, "the sampler wrote outside idx / weights"
    assert th.equal(prio, before), "the sampler wrote a priority"
    return idx[1:-1].cpu().numpy(), w[1:-1].cpu().numpy()


def _check_weights(got, want32):
    assert got.dtype == np.float32 and np.isfinite(got).all()
    ulps = np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(want32).astype(np.float64)
    assert ulps.max() <= 2.0, f"weights differ by {ulps.max()} float32 ulps"


def _check_draw(prio_host, size, B, draws, got, seed=SEED, beta=BETA):
    idx, w32, _, bit = P.sample(seed, draws, prio_host, size, B, beta)
    assert np.array_equal(got[0], idx), f"size {size}, B {B}, draws {draws}"
    _check_weights(got[1], w32)
    return bit


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
def test_sixty_four_consecutive_draws_on_the_96_slot_case():
    q = P.slots96()
    prio = _dev_u32(q)
    state, rng, status = _tensors(96, (1 << 32) - 3)             # the counter crosses its low word
    ws = _workspace(96, 8)
    for d in range(64):
        draws = (1 << 32) - 3 + d
        got = _draw(state, rng, prio, 8, status, ws)
        assert rng.tolist() == [SEED, draws + 1], "the draw counter did not advance on the device (once)"
        _check_draw(q, 96, 8, draws, got)
    assert int(status) == 0 and state.tolist() == [3, 96]


@pytest.mark.parametrize("size", [(1 << j) + d for j in range(6, 14) for d in (-1, 0, 1)])
def test_sizes_around_powers_of_two_never_read_beyond_size(size):
    """A ring 17 slots larger than ``size`` whose tail holds 2^32 - 1: around the wavefront's 64 slots and the workgroup's 4096."""
    cap, B = size + 17, 32
    q = np.random.default_rng(size).integers(1, 1 << 24, cap, dtype=np.uint64)
    q[size:] = P.PRIO_TOP
    prio = _dev_u32(q)
    state, rng, status = _tensors(size, 5)
    got = _draw(state, rng, prio, B, status, _workspace(cap, B))
    assert got[0].max() < size
    assert _check_draw(q, size, B, 5, got) == 0 and int(status) == 0 and rng.tolist() == [SEED, 6]


def test_one_sequence_in_the_ring():
    prio = _dev_u32([77, P.PRIO_TOP, P.PRIO_TOP])
    state, rng, status = _tensors(1, 2)
    got = _draw(state, rng, prio, 4, status, _workspace(3, 4))
    assert got[0].tolist() == [0] * 4 and (got[1] == 1.0).all() and int(status) == 0 and rng.tolist() == [SEED, 3]


def test_an_empty_ring_sets_status_and_advances_the_counter():
    prio = _dev_u32([P.PRIO_TOP] * 9)
    state, rng, status = _tensors(0, 7)
    got = _draw(state, rng, prio, 5, status, _workspace(9, 5, fill=0xFF))
    assert got[0].tolist() == [0] * 5 and (got[1] == 1.0).all() and int(status) == 1 and rng.tolist() == [SEED, 8]


def test_empty_strata_take_their_lower_end():
    q = [1, 1, 1, 9, 9]
    state, rng, status = _tensors(3, 11)
    got = _draw(state, rng, _dev_u32(q), 8, status, _workspace(5, 8))
    assert got[0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and (got[1] == 1.0).all()
    assert _check_draw(q, 3, 8, 11, got) == 0 and int(status) == 0


def test_a_dominant_slot_repeats_in_ascending_order():
    q = np.full(5, P.PRIO_ONE, dtype=np.uint64)
    q[2] = P.PRIO_TOP
    state, rng, status = _tensors(5, 0, seed=12345)
    got = _draw(state, rng, _dev_u32(q), 8, status, _workspace(5, 8))
    assert got[0].tolist() == [2] * 8 and (np.diff(got[0]) >= 0).all()
    _check_draw(q, 5, 8, 0, got, seed=12345)
    # and a heavy slot among many light ones: repeats beside other slots
    q = np.full(300, 1000, dtype=np.uint64)
    q[123] = 100000
    state, rng, status = _tensors(300, 1)
    got = _draw(state, rng, _dev_u32(q), 16, status, _workspace(300, 16))
    assert (np.diff(got[0]) >= 0).all() and (got[0] == 123).sum() >= 2 and len(set(got[0].tolist())) > 1
    _check_draw(q, 300, 16, 1, got)
    assert got[1][got[0] == 123].max() < 1.0 and got[1].max() == 1.0, "the heavy slot carries the smaller weight"


def test_a_full_ring_of_a_million_slots_over_the_whole_32_bit_range():
    cap, B = (1 << 20) + 4097, 256
    q = np.random.default_rng(7).integers(1, 1 << 32, cap, dtype=np.uint64)
    assert int(q.sum()) > 1 << 50, "precondition: the sum needs the 64-bit split"
    prio = _dev_u32(q)
    state, rng, status = _tensors(cap, (1 << 32) - 1)
    ws = _workspace(cap, B)
    got = _draw(state, rng, prio, B, status, ws)
    assert _check_draw(q, cap, B, (1 << 32) - 1, got) == 0 and int(status) == 0 and rng.tolist() == [SEED, 1 << 32]


def test_the_draw_does_not_depend_on_what_the_workspace_held():
    cap, size, B = 9000, 8200, 33
    q = np.random.default_rng(3).integers(1, 1 << 22, cap, dtype=np.uint64)
    prio = _dev_u32(q)
    state, rng, status = _tensors(size, 4)
    ws = _workspace(cap, B, fill=0xFF)
    a = _draw(state, rng, prio, B, status, ws)
    rng.copy_(th.tensor([SEED, 4], dtype=th.int64))
    b = _draw(state, rng, prio, B, status, ws)           # on what the first draw left behind
    _check_draw(q, size, B, 4, a)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and int(status) == 0


def test_argument_errors_are_codes():
    lib = _lib().lib()
    assert lib.uavgnn_replay_prio_workspace_bytes(0, 4) == 0 and lib.uavgnn_replay_prio_workspace_bytes(8, 65536) == 0
    assert lib.uavgnn_replay_prio_workspace_bytes((1 << 30) + 1, 4) == 0 and lib.uavgnn_replay_prio_workspace_bytes(1 << 30, 65535) > 0
    t = th.zeros(64, dtype=th.int64, device="cuda")
    p = t.data_ptr()
    assert lib.uavgnn_replay_prio_sample(p, p, 8, 0, p, BETA, p, p, p, p, None) == -1000
    assert lib.uavgnn_replay_prio_sample(p, p, 8, 65536, p, BETA, p, p, p, p, None) == -1001
    assert lib.uavgnn_replay_prio_sample(p, p, (1 << 30) + 1, 4, p, BETA, p, p, p, p, None) == -1001
    assert lib.uavgnn_replay_prio_sample(p, p, 8, 4, p, BETA, p, p, p, p + 8, None) == -1000, "a workspace off its 16-byte alignment"
    assert lib.uavgnn_replay_prio_sample(p, p, 8, 4, None, BETA, p, p, p, p, None) == -1000
    for beta in (-0.1, 16.5, float("inf"), float("nan")):     # beyond 16 a weight's power could leave double's range
        assert lib.uavgnn_replay_prio_sample(p, p, 8, 4, p, beta, p, p, p, p, None) == -1000, beta
    assert lib.uavgnn_replay_prio_update(p, 0, 4, 2, p, 8, 0.6, 0.9, 1e-3, p, p, p, None) == -1000
    assert lib.uavgnn_replay_prio_update(p, 3, 4, 2, p, 8, float("nan"), 0.9, 1e-3, p, p, p, None) == -1000
    assert lib.uavgnn_replay_prio_commit(p, 9, 8, p, p, None) == -1000
    assert not t.any()


# ---- the update ----------------------------------------------------------------------------------------------------------------------
def _update(td, idx, capacity, alpha, eta, eps, prio0, top0):
    """One update through the C ABI on prio [capacity] between four guard words on either side; (prio', prio_max', status)."""
    L = _lib()
    T, B, C = td.shape
    buf = _dev_u32([GUARD] * 4 + list(prio0) + [GUARD] * 4)
    top = _dev_u32([GUARD, top0, GUARD])
    status = th.zeros(1, dtype=th.int32, device="cuda")
    td_d, idx_d = th.from_numpy(td).cuda(), th.tensor(idx, dtype=th.int64, device="cuda")
    L.check(L.lib().uavgnn_replay_prio_update(td_d.data_ptr(), T, B, C, idx_d.data_ptr(), capacity, alpha, eta, eps, buf.data_ptr() + 16,
                                              top.data_ptr() + 4, status.data_ptr(), L.stream()), "uavgnn_replay_prio_update")
    out, t = _host_u32(buf), _host_u32(top)
    assert (out[:4] == GUARD).all() and (out[-4:] == GUARD).all() and t[0] == GUARD and t[2] == GUARD, "a guard word was written"
    assert th.equal(td_d.cpu().view(th.int32), th.from_numpy(td).view(th.int32)) and idx_d.tolist() == list(idx)      # bits: a NaN row stays
    return out[4:-4], int(t[1]), int(status)


# (3, 300, 1): more sequences than one workgroup owns at C = 1; (2, 3, 300): C beyond a workgroup, one sequence each; (3, 70, 7): 256 % C != 0
@pytest.mark.parametrize("T,B,C", [(3, 5, 2), (50, 32, 8), (3, 300, 1), (2, 3, 300), (3, 70, 7)])
@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0])
def test_update_against_the_restatement(T, B, C, alpha):
    rng = np.random.default_rng(100 * T + B)
    td = (rng.standard_normal((T, B, C)) * np.where(rng.random((1, B, 1)) < 0.2, 30.0, 0.5)).astype(np.float32)
    cap = 2 * B + 3
    idx = np.sort(rng.integers(0, cap, B))
    idx[1] = idx[2] = idx[0]                              # a run of three equal indices at the front, whatever was drawn
    idx[-1] = idx[-2]                                     # and a run of two that ends the batch
    idx = np.sort(idx)
    prio0 = rng.integers(1, 1 << 22, cap, dtype=np.uint64)
    eta, eps = 0.9, 1e-3
    got, top, status = _update(td, idx.tolist(), cap, alpha, eta, eps, prio0, P.PRIO_ONE)
    want, want_top, bit = P.update(td, idx, cap, alpha, eta, eps, prio0, P.PRIO_ONE)
    tol = 0 if alpha in (0.0, 1.0) else 1                 # a last-bit difference of pow moves llrint by one unit at most
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert diff.max() <= tol, f"priorities differ by {diff.max()} fixed-point units"
    untouched = np.setdiff1d(np.arange(cap), idx)
    assert np.array_equal(got[untouched], prio0[untouched]), "a slot outside the batch was written"
    assert abs(top - want_top) <= tol and top >= P.PRIO_ONE and status == bit == 0
    q, _ = P.priority(td, alpha, eta, eps)
    last = {int(s): b for b, s in enumerate(idx)}         # the last row of every run
    for s, b in last.items():
        assert abs(int(got[s]) - int(q[b])) <= tol, f"slot {s} does not hold the priority of its last row {b}"
    if alpha == 0.0:
        assert (got[idx] == P.PRIO_ONE).all() and top == P.PRIO_ONE


def test_update_skips_a_nan_row_and_an_index_at_capacity():
    T, B, C, cap = 3, 6, 2, 9
    td = np.random.default_rng(2).standard_normal((T, B, C)).astype(np.float32)
    td[1, 2, 0] = np.nan
    td[2, 3, 1] = np.inf
    idx = [1, 3, 4, 5, 7, cap]
    prio0 = [7] * cap
    got, top, status = _update(td, idx, cap, 0.6, 0.9, 1e-3, prio0, 5 * P.PRIO_ONE)
    want, want_top, bit = P.update(td, idx, cap, 0.6, 0.9, 1e-3, prio0, 5 * P.PRIO_ONE)
    assert status == bit == 2, "status bit 1"
    assert got[4] == 7 and got[5] == 7, "a non-finite row wrote"
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1 and got[1] != 7 and got[3] != 7 and got[7] != 7
    assert top == max(5 * P.PRIO_ONE, top) and abs(top - want_top) <= 1, "prio_max only grows"
    # a skipped LAST row of a run leaves the slot as it was: the run's earlier rows do not write
    got, _, status = _update(td, [1, 1, 1, 5, 6, 7], cap, 0.6, 0.9, 1e-3, prio0, P.PRIO_ONE)
    assert status == 2 and got[1] == 7 and got[5] == 7 and got[6] != 7


def test_prio_max_only_grows():
    td = np.full((2, 3, 1), 1e-3, dtype=np.float32)
    got, top, status = _update(td, [0, 1, 2], 3, 1.0, 0.9, 0.0, [9, 9, 9], 7 * P.PRIO_ONE)
    assert top == 7 * P.PRIO_ONE and status == 0 and (got == P.priority(td, 1.0, 0.9, 0.0)[0]).all() and got[0] < P.PRIO_ONE
    td = np.full((2, 3, 1), 1e6, dtype=np.float32)
    got, top, _ = _update(td, [0, 1, 2], 3, 1.0, 0.9, 0.0, [9, 9, 9], 7 * P.PRIO_ONE)
    assert top == P.PRIO_TOP and (got == P.PRIO_TOP).all(), "the upper clamp"


# ---- the commit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head,E,cap", [(0, 3, 8), (6, 5, 8), (7, 8, 8), (299, 300, 301)])
def test_commit_writes_exactly_the_wrapped_slots(head, E, cap):
    L = _lib()
    prio0 = np.arange(10, 10 + cap, dtype=np.uint64)
    buf = _dev_u32([GUARD] * 4 + list(prio0) + [GUARD] * 4)
    top = _dev_u32([123456])
    state = th.tensor([head, 2], dtype=th.int64, device="cuda")
    L.check(L.lib().uavgnn_replay_prio_commit(state.data_ptr(), E, cap, buf.data_ptr() + 16, top.data_ptr(), L.stream()),
            "uavgnn_replay_prio_commit")
    out = _host_u32(buf)
    assert (out[:4] == GUARD).all() and (out[-4:] == GUARD).all() and state.tolist() == [head, 2] and _host_u32(top)[0] == 123456
    assert np.array_equal(out[4:-4], P.commit(prio0, head, E, cap, 123456))


# ---- through the class ---------------------------------------------------------------------------------------------------------------
def test_commit_draw_and_update_through_the_replay_class():
    from uav_bs_ctrl_amd.replay import PRIO_ONE, SingleUbsSequenceReplay
    pr = (0.6, BETA, 0.9, 1e-3)
    cap, T, E, B = 12, 2, 4, 4
    rb = SingleUbsSequenceReplay(cap, T, 3, 8, n_envs=E, device="cuda", device_state=True, seed=9, prioritized=pr)
    assert rb.prio.tolist() == [PRIO_ONE] * cap and rb.prio_max.tolist() == [PRIO_ONE] and rb.is_weights is None
    rb.prio_max.fill_(3 * PRIO_ONE)
    rb.prio.fill_(5)
    for _ in range(2):
        rb._commit()
    assert rb.state.tolist() == [8, 8] and rb.prio.tolist() == [3 * PRIO_ONE] * 8 + [5] * 4
    idx = rb.sample_indices(B)
    want = P.sample(9, 0, _host_u32(rb.prio), 8, B, BETA)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and rb.rng.tolist() == [9, 1] and tuple(rb.is_weights.shape) == (B,)
    _check_weights(rb.is_weights.cpu().numpy(), want[1])
    td = th.randn(T, B, 1, device="cuda")
    before = _host_u32(rb.prio)
    rb.update_priorities(idx, td)
    after, _, bit = P.update(td.cpu().numpy(), idx.tolist(), cap, pr[0], pr[2], pr[3], before, 3 * PRIO_ONE)
    assert np.abs(_host_u32(rb.prio).astype(np.int64) - after.astype(np.int64)).max() <= 1 and bit == 0
    rb.check()
    with pytest.raises(ValueError, match="is_weights holds"):
        rb.sample_indices(B + 1)
    rb.update_priorities(idx, th.full((T, B, 1), float("nan"), device="cuda"))
    with pytest.raises(_lib().UavGnnError, match="bit 1"):
        rb.check()
    off = SingleUbsSequenceReplay(cap, T, 3, 8, n_envs=E, device="cuda", device_state=True, seed=9)
    assert off.prioritized is None and not hasattr(off, "prio")

"""`-m gpu`: the many-workgroup replay sampler (csrc/replay_wide.hip) bit for bit against the NumPy restatement of THE RULE
(tests/replay_sampler_ref.py) - past the one-workgroup kernel's 65 536 slots, on a tie at the threshold key, at its edges, against
the one-workgroup kernel where both apply, on a workspace full of 0xFF, inside a captured graph and through the replay classes."""
import functools

import numpy as np
import pytest
import torch as th

from tests import replay_sampler_ref as R

pytestmark = pytest.mark.gpu

SEED = (0x1234_5678 << 32) | 0x9abc_def1                                         # both key words in use
NARROW = 65536


@functools.lru_cache(maxsize=None)
def _ref(seed, draws, size, B):
    """The restatement's batch, computed once per (seed, draws, size, B) and never written to."""
    out = R.sample(seed, draws, size, B)
    out.setflags(write=False)
    return out


def _slots():
    from uav_bs_ctrl_amd import _lib as L
    return L.lib().uavgnn_replay_sample_wide_slots_per_workgroup()


def _workspace(capacity, fill=None):
    from uav_bs_ctrl_amd import _lib as L
    n = L.lib().uavgnn_replay_sample_wide_workspace_bytes(capacity)
    assert n > 0
    ws = th.empty(n, dtype=th.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws


def _tensors(size, draws, seed=SEED):
    return (th.tensor([3, size], dtype=th.int64, device="cuda"), th.tensor([seed, draws], dtype=th.int64, device="cuda"),
            th.zeros(1, dtype=th.int32, device="cuda"))


def _draw(state, rng, capacity, B, status, ws, wide=True):
    """One draw through the C ABI with one guard word on either side of idx."""
    from uav_bs_ctrl_amd import _lib as L
    idx = th.full((B + 2,), -7, dtype=th.int64, device="cuda")
    if wide:
        L.check(L.lib().uavgnn_replay_sample_wide(state.data_ptr(), rng.data_ptr(), capacity, B, idx.data_ptr() + 8, status.data_ptr(),
                                                  ws.data_ptr(), L.stream()), "uavgnn_replay_sample_wide")
    else:
        L.check(L.lib().uavgnn_replay_sample(state.data_ptr(), rng.data_ptr(), capacity, B, idx.data_ptr() + 8, status.data_ptr(),
                                             L.stream()), "uavgnn_replay_sample")
    assert idx[0] == -7 and idx[-1] == -7, "the sampler wrote outside idx"
    return idx[1:-1].cpu().numpy()


# ---- 1. agreement with the restatement over three draws ------------------------------------------------------------------------------
def _cases():
    fixed = [(65537, 65537, 32), (5000, 1048579, 32), (200001, 262144, 32), (1048579, 1048579, 4096)]
    return fixed + ["2S-1", "2S", "2S+1"]


@pytest.mark.parametrize("case", _cases(), ids=str)
def test_wide_sampler_equals_the_restatement_over_three_draws(case):
    if isinstance(case, str):                           # around the boundary of the second workgroup's chunk
        S = _slots()
        size, capacity, B = {"2S-1": 2 * S - 1, "2S": 2 * S, "2S+1": 2 * S + 1}[case], max(2 * S + 1, NARROW + 1), 33
    else:
        size, capacity, B = case
    first = (1 << 32) - 2                               # the counter crosses its low word
    state, rng, status = _tensors(size, first)
    ws = _workspace(capacity)
    for d in range(3):
        draws = first + d
        got = _draw(state, rng, capacity, B, status, ws)
        assert rng.tolist() == [SEED, draws + 1], "the draw counter did not advance on the device (once)"
        assert np.array_equal(got, _ref(SEED, draws, size, B)), f"size {size}, capacity {capacity}, B {B}, draw {d}"
    assert int(status) == 0 and state.tolist() == [3, size]


# ---- 2. a tie at the threshold key -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,draws", [(70001, 0), (200001, (1 << 32) - 2), (1048579, (1 << 32) - 1)])
def test_a_tie_at_the_threshold_key_is_broken_by_slot(size, draws):
    keys = R.keys(SEED, [draws], size)[0]
    order = np.lexsort((np.arange(size), keys))         # by key, ties by slot
    tied = np.nonzero(keys[order][1:] == keys[order][:-1])[0]
    assert tied.size > 0, "precondition: the draw holds no two slots with one key - the case checks nothing"
    r = int(tied[0])                                    # 0-based rank of the first element of the first tied pair
    B, lower, higher = r + 1, int(order[r]), int(order[r + 1])
    assert lower < higher and keys[lower] == keys[higher]
    state, rng, status = _tensors(size, draws)
    got = _draw(state, rng, size, B, status, _workspace(size))
    assert lower in got and higher not in got, (B, lower, higher)
    assert np.array_equal(got, np.sort(order[:B])) and np.array_equal(got, _ref(SEED, draws, size, B))
    assert int(status) == 0 and rng.tolist() == [SEED, draws + 1]


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------
def test_the_whole_ring_as_one_batch():
    n = NARROW + 1
    state, rng, status = _tensors(n, 5)
    got = _draw(state, rng, n, n, status, _workspace(n))
    assert np.array_equal(got, np.arange(n)) and int(status) == 0 and rng.tolist() == [SEED, 6]


def test_a_batch_larger_than_the_ring_wraps_and_sets_status():
    cap = 70001
    state, rng, status = _tensors(100, 7)
    ws = _workspace(cap)
    got = _draw(state, rng, cap, 128, status, ws)
    assert np.array_equal(got, _ref(SEED, 7, 100, 128)) and got.max() < 100
    assert int(status) == 1 and rng.tolist() == [SEED, 8]
    good = _draw(state, rng, cap, 64, status, ws)
    assert np.array_equal(good, _ref(SEED, 8, 100, 64)) and rng.tolist() == [SEED, 9]
    assert int(status) == 1, "a kernel cleared the status word"


def test_an_empty_ring():
    state, rng, status = _tensors(0, 7)
    got = _draw(state, rng, 70001, 5, status, _workspace(70001))
    assert got.tolist() == [0] * 5 and int(status) == 1 and rng.tolist() == [SEED, 8]


def test_an_empty_batch_advances_the_counter_and_writes_nothing():
    from uav_bs_ctrl_amd import _lib as L
    for size in (0, 70001):
        state, rng, status = _tensors(size, 7)
        ws = _workspace(70001)
        assert _draw(state, rng, 70001, 0, status, ws).size == 0
        assert L.lib().uavgnn_replay_sample_wide(state.data_ptr(), rng.data_ptr(), 70001, 0, None, status.data_ptr(), ws.data_ptr(),
                                                 L.stream()) == 0, "a null idx at B == 0"
        assert rng.tolist() == [SEED, 9] and int(status) == 0 and state.tolist() == [3, size]


# ---- 4. same bits as the one-workgroup kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,B", [(8, 8), (9, 8), (40, 8), (5000, 32), (65536, 4096)])
def test_wide_and_narrow_kernels_write_the_same_bits(size, B):
    draws = (1 << 32) - 1
    ws = _workspace(NARROW)
    state, rng_w, status = _tensors(size, draws)
    rng_n = rng_w.clone()
    wide = _draw(state, rng_w, NARROW, B, status, ws)
    narrow = _draw(state, rng_n, NARROW, B, status, None, wide=False)
    want = _ref(SEED, draws, size, B)
    assert np.array_equal(wide, narrow) and np.array_equal(wide, want)
    assert rng_w.tolist() == rng_n.tolist() == [SEED, draws + 1] and int(status) == 0


# ---- 5. workspace and repeatability --------------------------------------------------------------------------------------------------------
def test_the_draw_does_not_depend_on_what_the_workspace_held():
    size, cap, B, draws = 200001, 262144, 32, (1 << 32) - 2
    state, rng, status = _tensors(size, draws)
    ws = _workspace(cap, fill=0xFF)
    a = _draw(state, rng, cap, B, status, ws)
    rng.copy_(th.tensor([SEED, draws], dtype=th.int64))
    b = _draw(state, rng, cap, B, status, ws)           # on what the first draw left behind
    want = _ref(SEED, draws, size, B)
    assert np.array_equal(a, want) and np.array_equal(b, want) and int(status) == 0


# ---- 6. capture ----------------------------------------------------------------------------------------------------------------------------
def test_three_captured_draws_replay_at_the_current_counter():
    from uav_bs_ctrl_amd.graphs import _warm_up_and_capture, _Window
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    cap, B = 70001, 8
    rb = SingleUbsSequenceReplay(cap, 2, 3, 8, n_envs=2, device="cuda", device_state=True, seed=9)
    rb.state.copy_(th.tensor([0, cap], device="cuda"))
    window = _Window()
    out = _warm_up_and_capture(2, lambda: [rb.sample_indices(B) for _ in range(3)], window, state=[rb.rng])
    assert rb.rng.tolist() == [9, 0], "the warm-up left its draws"
    assert len(window.graphs) == 1
    got = []
    for _ in range(2):
        window.graphs[0].replay()
        got += [o.cpu().numpy() for o in out]
    assert rb.rng.tolist() == [9, 6]
    for d, g in enumerate(got):
        assert np.array_equal(g, _ref(9, d, cap, B)), f"draw {d}"
    rb.check()


# ---- 7. through the class --------------------------------------------------------------------------------------------------------------------
def test_sample_and_gather_through_sequence_replay():
    from tests.test_replay_device_gpu import MULTI_NAMES, _fake_learner
    from uav_bs_ctrl_amd.graphs import GraphedUpdate
    from uav_bs_ctrl_amd.replay import SequenceReplay
    cap, T, n, M, B = 70001, 2, 3, 5, 8
    rb = SequenceReplay(cap, T, n, M, 8, n_envs=3, state_dim=3, device="cuda", device_state=True, seed=1)
    assert rb._sample_ws is not None and rb._sample_ws.dtype == th.uint8
    gen = th.Generator(device="cuda").manual_seed(4)
    for v in rb.mem.values():
        v.copy_(th.randint(0, 9, v.shape, generator=gen, device="cuda") if v.dtype == th.int64
                else th.randn(v.shape, generator=gen, device="cuda"))
    rb.state.copy_(th.tensor([5, cap], device="cuda"))
    ref, got = (GraphedUpdate(_fake_learner("tarmac"), B, T, n, M, capture=False) for _ in range(2))
    idx = rb.sample_indices(B)
    assert np.array_equal(idx.cpu().numpy(), _ref(1, 0, cap, B)) and rb.rng.tolist() == [1, 1]
    ref.load({k: v.index_select(0, idx) for k, v in rb.mem.items()})
    rb.gather_into(idx, got)
    for name in MULTI_NAMES:
        owner_g, owner_r, attr = (got.obs, ref.obs, name[4:]) if name.startswith("obs.") else (got, ref, name)
        assert th.equal(getattr(owner_g, attr), getattr(owner_r, attr)), name
    rb.check()

"""`-m gpu`: the kernels of the device-resident replay state (csrc/replay.hip) - the ring commit against the host-state replay's, the
sampler bit for bit against its NumPy restatement (tests/replay_sampler_ref.py), the one-launch gather against ``index_select`` +
``load``, the exploration schedule against the restated formula."""
import ctypes
import types

import numpy as np
import pytest
import torch as th

from tests import replay_sampler_ref as R

pytestmark = pytest.mark.gpu

H = 8


def _multi(n, M, T, E, cap, device_state, state_dim=3, **kw):
    from uav_bs_ctrl_amd.replay import SequenceReplay
    return SequenceReplay(cap, T, n, M, H, n_envs=E, state_dim=state_dim, device="cuda", device_state=device_state, **kw)


def _single(M, T, E, cap, device_state, **kw):
    from uav_bs_ctrl_amd.replay import SingleUbsSequenceReplay
    return SingleUbsSequenceReplay(cap, T, M, H, n_envs=E, device="cuda", device_state=device_state, **kw)


def _transition(rb, gen):
    """A random transition in the shapes of ``rb``'s fields (every value distinct with overwhelming probability)."""
    tr = {}
    for k, v in rb.cur.items():
        shape = (v.shape[0],) + tuple(v.shape[2:])
        if v.dtype == th.int64:
            tr[k] = th.randint(0, 1 << 40, shape, generator=gen, device="cuda")
        else:
            tr[k] = th.randn(shape, generator=gen, device="cuda")
            if k not in ("act", "rew", "done"):
                tr["next_" + k] = th.randn(shape, generator=gen, device="cuda")
    return tr


# ---- commit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make,commits", [
    (lambda ds, **kw: _multi(3, 5, 4, 3, 7, ds, **kw), 6),       # gt: 5 steps x 300 B = 1500 B per sequence - the 4-byte path; heads 0 3 6 2 5 1 4
    (lambda ds, **kw: _multi(4, 4, 2, 4, 8, ds, **kw), 3),       # every field a multiple of 16 B - the 16-byte path
    (lambda ds, **kw: _single(5, 3, 3, 7, ds, **kw), 6),
    (lambda ds, **kw: _single(3, 3, 2, 5, ds, **kw), 4),
], ids=["multi-3x5-ring7", "multi-4x4-ring8", "single-M5", "single-M3"])
def test_commit_equals_the_host_state_commit(make, commits):
    host, dev = make(False), make(True, seed=1)
    gen = th.Generator(device="cuda").manual_seed(5)
    for c in range(commits):
        for _ in range(host.T):
            tr = _transition(host, gen)
            host.push(tr), dev.push(tr)
        assert dev.ptr == 0 and dev.state.tolist() == [host.head, host.size], f"commit {c}"
        for k in host.mem:
            assert th.equal(host.mem[k], dev.mem[k]), f"commit {c}: {k}"
    assert len(dev) == len(host) == host.capacity and int(dev.status) == 0
    dev.check()


def test_commit_of_more_sequences_than_the_ring_holds_is_an_error_code():
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd.replay import SequenceReplay
    with pytest.raises(ValueError, match="capacity"):
        SequenceReplay(2, 2, 2, 3, H, n_envs=3, device="cuda", device_state=True)
    src, dst, state = th.ones(9, 4, device="cuda"), th.zeros(8, 4, device="cuda"), th.zeros(2, dtype=th.int64, device="cuda")
    fields = (ctypes.c_longlong * 3)(src.data_ptr(), dst.data_ptr(), 16)
    assert L.lib().uavgnn_replay_commit(fields, 1, 9, 8, state.data_ptr(), L.stream()) == L.UAVGNN_EINVAL
    th.cuda.synchronize()
    assert not dst.any() and state.tolist() == [0, 0], "the refused commit launched"
    fields = (ctypes.c_longlong * 3)(src.data_ptr(), dst.data_ptr(), 6)          # no multiple of 4 bytes
    assert L.lib().uavgnn_replay_commit(fields, 1, 2, 8, state.data_ptr(), L.stream()) == L.UAVGNN_EINVAL
    assert L.lib().uavgnn_replay_sample(state.data_ptr(), state.data_ptr(), 65537, 4, dst.data_ptr(), dst.data_ptr(),
                                        L.stream()) == L.UAVGNN_EUNSUPPORTED


# ---- sampler --------------------------------------------------------------------------------------------------------------------
def _draw(state, rng, capacity, B, status):
    from uav_bs_ctrl_amd import _lib as L
    idx = th.full((B + 2,), -7, dtype=th.int64, device="cuda")                   # one guard word on either side
    L.check(L.lib().uavgnn_replay_sample(state.data_ptr(), rng.data_ptr(), capacity, B, idx.data_ptr() + 8, status.data_ptr(),
                                         L.stream()), "uavgnn_replay_sample")
    assert idx[0] == -7 and idx[-1] == -7, "the sampler wrote outside idx"
    return idx[1:-1].cpu().numpy()


@pytest.mark.parametrize("size,B", [(8, 8), (9, 8), (40, 8), (5000, 32), (50000, 32), (65536, 4096)])
def test_sampler_equals_the_restatement_over_three_draws(size, B):
    seed = (0x1234_5678 << 32) | 0x9abc_def1                                      # both key words in use
    state = th.tensor([3, size], dtype=th.int64, device="cuda")
    rng = th.tensor([seed, (1 << 32) - 2], dtype=th.int64, device="cuda")         # the counter crosses its low word
    status = th.zeros(1, dtype=th.int32, device="cuda")
    for d in range(3):
        draws = (1 << 32) - 2 + d
        got = _draw(state, rng, 65536, B, status)
        assert rng.tolist() == [seed, draws + 1], "the draw counter did not advance on the device"
        assert np.array_equal(got, R.sample(seed, draws, size, B)), f"size {size}, B {B}, draw {d}"
    assert int(status) == 0 and state.tolist() == [3, size]


def test_a_batch_larger_than_the_ring_sets_status_and_stays_inside_it():
    from uav_bs_ctrl_amd import _lib as L
    rb = _single(3, 2, 2, 6, True, seed=9)
    gen = th.Generator(device="cuda").manual_seed(2)
    for _ in range(2 * rb.T):
        rb.push(_transition(rb, gen))
    assert len(rb) == 4
    rb.check()
    idx = rb.sample_indices(4)
    assert sorted(idx.tolist()) == [0, 1, 2, 3] and int(rb.status) == 0
    idx = rb.sample_indices(6)
    assert int(rb.status) == 1 and rb.rng.tolist() == [9, 2]
    assert int(idx.min()) >= 0 and int(idx.max()) < 4 and np.array_equal(idx.cpu().numpy(), R.sample(9, 1, 4, 6))
    with pytest.raises(L.UavGnnError, match="status"):
        rb.check()
    rb.sample_indices(2)
    assert int(rb.status) == 1, "a kernel cleared the status word"
    with pytest.raises(ValueError, match="generator"):
        rb.sample_indices(2, generator=gen)
    empty = _single(3, 2, 2, 6, True, seed=9)
    assert empty.sample_indices(3).tolist() == [0, 0, 0] and int(empty.status) == 1


# ---- gather ---------------------------------------------------------------------------------------------------------------------
GUARD = -12345.0


def _guarded(t, offset):
    """A NaN-filled (int64: -1) stand-in of buffer ``t`` inside a larger allocation whose other words hold a guard value; offset: the
    guard words in front (64: the stand-in stays 16-byte aligned; 1: it is only 4-byte / 8-byte aligned)."""
    buf = th.full((t.numel() + 2 * offset,), -99 if t.dtype == th.int64 else GUARD, dtype=t.dtype, device=t.device)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.fill_(-1 if t.dtype == th.int64 else float("nan"))
    return buf, view


def _fill_ring(rb, seed):
    gen = th.Generator(device="cuda").manual_seed(seed)
    for k, v in rb.mem.items():
        if v.dtype == th.int64:
            v.copy_(th.randint(0, 9, v.shape, generator=gen, device="cuda"))
        else:
            v.copy_(th.randn(v.shape, generator=gen, device="cuda"))
    rb.state.copy_(th.tensor([0, rb.capacity], device="cuda"))


def _check_gather(rb, ref, got, names, offset):
    cap = rb.capacity
    idx = th.tensor([cap - 1, 0, 2, 2, 0], dtype=th.int64, device="cuda")      # repeats, the first and the last slot
    ref.load({k: v.index_select(0, idx) for k, v in rb.mem.items()})
    bufs = {}
    for name in names:
        owner, attr = (got.obs, name[4:]) if name.startswith("obs.") else (got, name)
        if getattr(owner, attr) is None:
            continue
        bufs[name], view = _guarded(getattr(owner, attr), offset)
        setattr(owner, attr, view)
    rb.gather_into(idx, got)
    for name, buf in bufs.items():
        owner, attr = (got.obs, name[4:]) if name.startswith("obs.") else (got, name)
        r_owner = ref.obs if name.startswith("obs.") else ref
        out, want = getattr(owner, attr), getattr(r_owner, attr)
        if out.dtype != th.int64:
            assert not th.isnan(out).any(), f"{name}: a word of the destination was not written"
        assert th.equal(out, want), name
        guard = -99 if buf.dtype == th.int64 else GUARD
        assert (buf[:offset] == guard).all() and (buf[offset + out.numel():] == guard).all(), f"{name}: a guard word changed"
    return idx


def _fake_learner(c):
    return types.SimpleNamespace(fused_tail=True, device=th.device("cuda"), args=types.SimpleNamespace(hidden_size=H, c=c))


MULTI_NAMES = ("obs.gt", "obs.ubs", "obs.agent", "obs.d_u2u", "h0", "h1", "acts", "rews", "dones")


@pytest.mark.parametrize("offset", [64, 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("n,M", [(3, 5), (4, 4)], ids=["3x5-slab300B", "4x4-slab320B"])
@pytest.mark.parametrize("enc,c", [("gnn", "tarmac"), ("mlp", None)])
def test_gather_into_a_graphed_update_layout_equals_index_select_and_load(enc, c, n, M, offset):
    from uav_bs_ctrl_amd.graphs import GraphedUpdate
    T, B, cap = 4, 5, 7
    rb = _multi(n, M, T, 2, cap, True, seed=1)
    _fill_ring(rb, 11)
    ref, got = (GraphedUpdate(_fake_learner(c), B, T, n, M, enc=enc, capture=False) for _ in range(2))
    assert (got.obs.d_u2u is None) == (enc == "mlp")
    idx = _check_gather(rb, ref, got, MULTI_NAMES, offset)
    # the replay's own gather of the same sequences
    m = {k: v.index_select(0, idx) for k, v in rb.mem.items()}
    assert th.equal(got.h0, m["h"][:, 0].reshape(B * n, -1)) and th.equal(got.h1, m["h"][:, 1].reshape(B * n, -1))
    assert th.equal(got.acts, m["act"].permute(1, 0, 2).reshape(T, B * n, 1))
    assert th.equal(got.obs.gt, m["gt"].transpose(0, 1)) and th.equal(got.rews, m["rew"].transpose(0, 1))
    # a `states` buffer, when the target has one, is filled time-major as well
    got.states = th.full((T + 1, B, 3), float("nan"), device="cuda")
    got.load_from(rb, idx)
    assert th.equal(got.states, m["state"].transpose(0, 1))


@pytest.mark.parametrize("offset", [64, 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("M", [5, 4], ids=["M5-slab80B", "M4-slab64B"])
@pytest.mark.parametrize("enc", ["gnn", "rnn"])
def test_gather_into_a_graphed_single_ubs_update_layout_equals_gather_and_load(enc, M, offset):
    from uav_bs_ctrl_amd.graphs import GraphedSingleUbsUpdate
    T, B, cap = 3, 5, 6
    rb = _single(M, T, 2, cap, True, seed=1)
    _fill_ring(rb, 12)
    ref, got = (GraphedSingleUbsUpdate(_fake_learner(None), B, T, M, enc, capture=False) for _ in range(2))
    idx = _check_gather(rb, ref, got, ("gt", "agent", "h0", "h1", "acts", "rews", "dones"), offset)
    own = rb.gather(idx, enc, time_batched=False)
    for k in ("h0", "h1", "acts", "rews", "dones"):
        assert th.equal(getattr(got, k), own[k]), k
    if enc == "rnn":
        flat = got._batch()["obs"]
        for t in range(T + 1):
            assert th.equal(flat[t], own["obs"][t]), t


def test_gather_refuses_a_buffer_of_another_shape():
    from uav_bs_ctrl_amd.graphs import GraphedSingleUbsUpdate
    rb = _single(4, 3, 2, 6, True, seed=1)
    got = GraphedSingleUbsUpdate(_fake_learner(None), 5, 3, 4, "gnn", capture=False)
    with pytest.raises(ValueError, match="gt"):
        rb.gather_into(th.zeros(4, dtype=th.int64, device="cuda"), got)          # B = 4 against buffers of 5 rows


# ---- exploration schedule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [50000, 200000])
def test_eps_schedule_kernel_equals_the_restated_formula(decay):
    from uav_bs_ctrl_amd import _lib as L
    ts = [0, 1, decay // 2, decay - 1, decay, decay + 10, 3 * 10 ** 6]
    want = R.eps_schedule(ts, 1.0, 0.05, decay)
    buf = th.zeros(3, dtype=th.float32, device="cuda")                            # eps between two guard words
    for t0, w in zip(ts, want):
        t = th.tensor([t0], dtype=th.int64, device="cuda")
        L.check(L.lib().uavgnn_eps_schedule(t.data_ptr(), 32, 1.0, 0.05, float(decay), buf.data_ptr() + 4, L.stream()),
                "uavgnn_eps_schedule")
        got = buf.cpu().numpy()
        assert got[1].tobytes() == w.tobytes(), (t0, got[1], w)
        assert got[0] == 0 and got[2] == 0 and int(t) == t0 + 32
    t = th.zeros(1, dtype=th.int64, device="cuda")
    assert L.lib().uavgnn_eps_schedule(t.data_ptr(), 1, 1.0, 0.05, 0.0, buf.data_ptr(), L.stream()) == L.UAVGNN_EINVAL

"""NumPy restatement of the device replay sampler and of the exploration schedule, written from the header comment of
uav_bs_ctrl_amd/csrc/replay.hip - not from its code: slot s of the ring is keyed by the first Philox4x32-10 word at counter
(s, 0, draws_lo, draws_hi) under the key (seed_lo, seed_hi); the B smallest (key, slot) pairs are the sample, written in ascending slot
order; a batch larger than the ring wraps (idx[i] = i % max(size, 1)).  Vectorised over draws.

Also the co-inclusion counts that tests/golden/make_replay_sample_stats.py (on the reference's ``ReplayBuffer.sample``) and
tests/test_replay_device_host.py (on the restatement) share."""
import numpy as np

from tests.map_sampler_ref import philox4x32_10

_M64 = 2 ** 64 - 1


def keys(seed, draws, size):
    """uint64 [len(draws), size] (32-bit values): the key of every slot at every draw counter of `draws`."""
    seed = int(seed) & _M64
    d = np.atleast_1d(np.asarray(draws)).astype(np.uint64)[:, None]
    s = np.arange(size, dtype=np.uint64)[None]
    return philox4x32_10(s, np.uint64(0), d & np.uint64(0xFFFFFFFF), d >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)[0]


def sample(seed, draws, size, B):
    """int64 [B]: the batch the kernel writes at {seed, draws} from a ring holding `size` sequences."""
    return sample_many(seed, [draws], size, B)[0]


def sample_many(seed, draws, size, B):
    """int64 [len(draws), B]: one batch per draw counter."""
    n = len(draws)
    if size < B:
        return np.broadcast_to(np.arange(B, dtype=np.int64) % max(size, 1), (n, B)).copy()
    k = keys(seed, draws, size)
    slot = np.broadcast_to(np.arange(size, dtype=np.int64), k.shape)
    out = np.empty((n, B), dtype=np.int64)
    for i in range(n):
        out[i] = np.sort(np.lexsort((slot[i], k[i]))[:B])
    return out


def eps_schedule64(t, eps_start, eps_end, decay_steps):
    """float64: max(eps_end, eps_start - (eps_start - eps_end) / decay_steps * t), every operation rounded to double on its own."""
    t = np.asarray(t, dtype=np.int64).astype(np.float64)
    slope = (np.float64(eps_start) - np.float64(eps_end)) / np.float64(decay_steps)
    return np.maximum(np.float64(eps_end), np.float64(eps_start) - slope * t)


def eps_schedule(t, eps_start, eps_end, decay_steps):
    """float32: the word the kernel writes - the double value rounded once."""
    return eps_schedule64(t, eps_start, eps_end, decay_steps).astype(np.float32)


def inclusion_counts(batches, size):
    """(per-slot inclusion counts [size], pair co-inclusion counts [size (size - 1) / 2] over the pairs i < j) of batches [N, B]."""
    batches = np.asarray(batches, dtype=np.int64)
    member = np.zeros((batches.shape[0], size), dtype=np.int64)
    np.put_along_axis(member, batches, 1, 1)
    assert (member.sum(1) == batches.shape[1]).all(), "a batch holds a slot twice"
    pair = member.T @ member
    return member.sum(0), pair[np.triu_indices(size, 1)]

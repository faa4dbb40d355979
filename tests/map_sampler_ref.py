"""NumPy restatement of the reset-time placement sampler, written from the header comment of
uav_bs_ctrl_amd/csrc/map_sample.hip (draw slots, integer / uniform conversions, partial Fisher-Yates over a virtual identity
array, stable-argsort shuffles, the per-kind placement formulas) - not from its code: vectorised over environments, the sparse
table is an append-only log searched for the LAST write, the ranks come from np.argsort(kind="stable").

Also the histograms and structural invariants that tests/golden/make_map_fixtures.py (on the reference's own draws) and
tests/test_maps_registry.py / tests/test_map_sampler_gpu.py (on the restatement's / the kernel's) share."""
import numpy as np

SLOT_SPOT, SLOT_PICK, SLOT_GT = 16, 1024, 2048
UNIFORM_LATTICE, FIXED, HOTSPOT, DENSE_HOTSPOT, DENSE_HOTSPOT_V2 = range(5)
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit values; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _words(env, slot, seed, resets):
    seed, resets = int(seed) & (2 ** 64 - 1), int(resets) & (2 ** 64 - 1)
    return philox4x32_10(env, slot, resets & 0xFFFFFFFF, resets >> 32, seed & 0xFFFFFFFF, seed >> 32)


def _below(w, m):
    """integer in [0, m) from 32-bit words: floor(w m / 2^32)"""
    return ((w * np.asarray(m, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def _unit(w):
    return ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def _sample_distinct(words, C):
    """words [B, count] -> ordered samples of `count` distinct points of [0, C) per row: partial Fisher-Yates over a[p] = p."""
    B, count = words.shape
    log_pos, log_val = np.full((B, count), -1, dtype=np.int64), np.zeros((B, count), dtype=np.int64)

    def read(pos, k):                                     # a[pos]: the last write to pos among the first k log entries, else pos
        out = pos.copy()
        for i in range(k):
            out = np.where(log_pos[:, i] == pos, log_val[:, i], out)
        return out
    picks = np.zeros((B, count), dtype=np.int64)
    for k in range(count):
        j = k + _below(words[:, k], C - k)
        picks[:, k] = read(j, k)
        log_val[:, k] = read(np.full(B, k, dtype=np.int64), k)
        log_pos[:, k] = j
    return picks


def sample(int_consts, f64_consts, B, seed, resets, fixed_ubs=None, fixed_gts=None, envs=None):
    """(pos_ubs [B,n,2] f64, pos_gts [B,M,2] f32, prior [B,M] i32) of environments 0..B-1 (or `envs`) at {seed, resets}."""
    kind, n, M, L_u, L_s, r, n_picks, gpg, origin = (int(v) for v in int_consts)
    range_pos, pitch_u, pitch_s, pitch_c, spread = (float(v) for v in f64_consts)
    env = np.arange(B, dtype=np.uint64) if envs is None else np.asarray(envs, dtype=np.uint64)
    B = env.shape[0]
    e1 = env[:, None]
    w_gt = _words(e1, np.uint64(SLOT_GT) + np.arange(M, dtype=np.uint64)[None], seed, resets)       # 4 x [B, M]

    def lattice(count, slot0, L):
        w0 = _words(e1, np.uint64(slot0) + np.arange(count, dtype=np.uint64)[None], seed, resets)[0]
        p = _sample_distinct(w0, L * L)
        return np.stack((p // L, p % L), -1)                                                         # [B, count, 2] integers

    if kind == FIXED:
        ubs = np.broadcast_to(np.asarray(fixed_ubs, dtype=np.float64).reshape(1, n, 2), (B, n, 2))
        gts = np.broadcast_to(np.asarray(fixed_gts, dtype=np.float64).reshape(1, M, 2), (B, M, 2))
    else:
        ubs = pitch_u * lattice(n, 0, L_u)
        if kind == UNIFORM_LATTICE:
            gts = pitch_u * lattice(M, SLOT_PICK, L_u)
        else:
            q = _below(_words(env, SLOT_SPOT, seed, resets)[0], L_s * L_s)
            spot = pitch_s * (origin + np.stack((q // L_s, q % L_s), -1))[:, None, :]                # [B, 1, 2]
            cell = lattice(n_picks, SLOT_PICK, r)[:, np.arange(M) // gpg] if n_picks > 0 else np.zeros((B, M, 2))
            gts = spot + pitch_c * cell + spread * (np.stack((_unit(w_gt[0]), _unit(w_gt[1])), -1) - 0.5)
            order = np.argsort(w_gt[2], axis=1, kind="stable")          # output row i holds generated GT order[i]
            gts = np.take_along_axis(gts, order[:, :, None], 1)
    prior = np.argsort(w_gt[3], axis=1, kind="stable").astype(np.int32)
    return (np.ascontiguousarray(np.clip(ubs, 0.0, range_pos)), np.clip(gts, 0.0, range_pos).astype(np.float32), prior)


# ---- what the fixture generator and the tests share ---------------------------------------------------------------------------
def histograms(kind, pos_ubs, pos_gts, prior, range_pos, ubs_pitch):
    """Integer histograms of a batch of placements, from the positions alone (the reference hands out nothing else).
    kind: 'hotspot' (4 GTs on the 2 x 2 block), 'dense_hotspot' (groups on a 4 x 4 block of 200 m cells) or 'dense_hotspot_v2'."""
    pos_ubs, pos_gts, prior = np.asarray(pos_ubs, dtype=np.float64), np.asarray(pos_gts, dtype=np.float64), np.asarray(prior)
    B, M = prior.shape
    L_u = int(range_pos // ubs_pitch)
    iu = np.rint(pos_ubs / ubs_pitch).astype(np.int64)
    h = {"ubs_x": np.bincount(iu[..., 0].ravel(), minlength=L_u), "ubs_y": np.bincount(iu[..., 1].ravel(), minlength=L_u),
         "prior0": np.bincount(prior[:, 0], minlength=M)}
    if kind == "dense_hotspot_v2":                        # spot = midrange of the GTs, to the nearest multiple of 400 (1 .. 14)
        mid = np.rint((pos_gts.min(1) + pos_gts.max(1)) / 2 / 400.0).astype(np.int64) - 1
        L_s = int(range_pos // 400) - 1
        h["spot"] = np.bincount(mid[:, 0] * L_s + mid[:, 1], minlength=L_s * L_s)
        return h
    cen = np.rint(pos_gts / 200.0).astype(np.int64)       # lattice cell of every GT
    r = 2 if kind == "hotspot" else 4
    L_s = int(range_pos // 200) // r
    spot = cen.min(1) // r                                # [B, 2]
    h["spot"] = np.bincount(spot[:, 0] * L_s + spot[:, 1], minlength=L_s * L_s)
    rel = cen - r * spot[:, None, :]                      # cell inside the block
    cell = rel[..., 0] * r + rel[..., 1]
    if kind == "hotspot":
        h["gt0_cell"] = np.bincount(cell[:, 0], minlength=r * r)
    else:
        held = np.zeros((B, r * r), dtype=bool)
        np.put_along_axis(held, np.clip(cell, 0, r * r - 1), True, 1)
        h["group_cells"] = held.sum(0)
        off = pos_gts - 200.0 * cen                       # in [-50, 50]
        ob = np.clip(np.floor((off + 50.0) / 10.0).astype(np.int64), 0, 9)
        h["offset_x"], h["offset_y"] = np.bincount(ob[..., 0].ravel(), minlength=10), np.bincount(ob[..., 1].ravel(), minlength=10)
        h["gt01_share_group"] = np.bincount((cell[:, 0] == cell[:, 1]).astype(np.int64), minlength=2)
    return {k: v.astype(np.int64) for k, v in h.items()}


def check_ubs(pos_ubs, range_pos, pitch):
    """UBSs on the lattice, inside [0, range_pos), pairwise distinct within an environment."""
    pos_ubs = np.asarray(pos_ubs, dtype=np.float64)
    idx = np.rint(pos_ubs / pitch)
    assert np.array_equal(idx * pitch, pos_ubs), "a UBS is off the lattice"
    assert (pos_ubs >= 0).all() and (pos_ubs < range_pos).all(), "a UBS is outside [0, range_pos)"
    L = int(range_pos // pitch)
    flat = np.sort((idx[..., 0] * L + idx[..., 1]).astype(np.int64), axis=1)
    assert (np.diff(flat, axis=1) > 0).all(), "two UBSs of an environment share a lattice point"


def check_prior(prior):
    prior = np.asarray(prior)
    assert np.array_equal(np.sort(prior, axis=1), np.broadcast_to(np.arange(prior.shape[1]), prior.shape)), "prior is no permutation"


def check_hotspot(pos_gts, range_pos=2000.0):
    """4 GTs: the GT set is exactly s + 200 {(0,0),(1,0),(0,1),(1,1)}, s a multiple of 400, s <= 1600."""
    g = np.asarray(pos_gts, dtype=np.float64)
    assert g.shape[1:] == (4, 2)
    s = g.min(1)
    assert np.array_equal(np.rint(s / 400.0) * 400.0, s) and (s >= 0).all() and (s <= 1600.0).all(), "hotspot origin"
    rel = g - s[:, None, :]
    code = np.sort(rel[..., 0] / 200.0 * 2 + rel[..., 1] / 200.0, axis=1)
    assert np.array_equal(code, np.broadcast_to(np.arange(4.0), code.shape)), "the GTs are not the 2 x 2 block"


def check_dense_hotspot(pos_gts, n_grps=10, gts_per_grp=5):
    """n_grps distinct centres (nearest multiples of 200) with gts_per_grp GTs each, every GT within 50 m of its centre, all centres
    in one 800 m block whose origin is a multiple of 800 and <= 4800."""
    g = np.asarray(pos_gts, dtype=np.float64)
    cen = np.rint(g / 200.0).astype(np.int64)
    assert (np.abs(g - 200.0 * cen) <= 50.0).all(), "a GT is farther than 50 m from its centre"
    code = np.sort(cen[..., 0] * 1000 + cen[..., 1], axis=1).reshape(g.shape[0], n_grps, gts_per_grp)
    assert (code == code[:, :, :1]).all(), "a centre does not hold gts_per_grp GTs"
    assert (np.diff(code[:, :, 0], axis=1) > 0).all(), "fewer than n_grps distinct centres"
    blk = cen // 4
    assert (blk == blk[:, :1, :]).all() and (blk >= 0).all() and (blk * 800 <= 4800).all(), "centres leave one 800 m block"

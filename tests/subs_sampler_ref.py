"""NumPy restatement of the reset-time placement sampler of the single-UBS environment, written from the header comment of
uav_bs_ctrl_amd/csrc/subs_env.hip (draw slots, the uniform conversion, group angles / radii, Box-Muller offsets, stable-argsort
shuffle and priorities) - not from its code: vectorised over environments, float64 throughout, rounded to float32 once.  The
Philox generator and its keying are those of tests/map_sampler_ref.py (the kernel reuses csrc/map_sample.hip's).

Also the histograms that tests/golden/make_golden_exp1.py (on the reference's own draws) and tests/test_subs_env_host.py (on
the restatement's) share.  Every histogram takes ONE sample per environment (GT row 0, or a per-environment index): the GTs of
one environment share their group centres, so pooling them would break the independence the chi-square test assumes."""
import numpy as np

from tests.map_sampler_ref import _unit, _words

SLOT_ANGLE, SLOT_GROUP, SLOT_GT = 0, 1024, 2048
TWO_PI = 6.283185307179586
N_BINS = 32


def sample64(n_grps, gts_per_grp, range_pos, r_cov, B, seed, resets, envs=None):
    """(pos_ubs [B,2] f64, pos_gts [B,M,2] f64 BEFORE the rounding to float32, prior [B,M] i32, order [B,M]: output row i holds
    generated GT order[i]) of environments 0..B-1 (or `envs`) at {seed, resets}."""
    G, P = int(n_grps), int(gts_per_grp)
    M = G * P
    env = np.arange(B, dtype=np.uint64) if envs is None else np.asarray(envs, dtype=np.uint64)
    B = env.shape[0]
    e1 = env[:, None]
    u = _unit(_words(env, SLOT_ANGLE, seed, resets)[0])[:, None]                                          # [B, 1]
    u_g = _unit(_words(e1, np.uint64(SLOT_GROUP) + np.arange(G, dtype=np.uint64)[None], seed, resets)[0])  # [B, G]
    w = _words(e1, np.uint64(SLOT_GT) + np.arange(M, dtype=np.uint64)[None], seed, resets)                 # 4 x [B, M]
    centre = np.array([range_pos / 2, range_pos / 2], dtype=np.float64)
    theta = (u + np.arange(G, dtype=np.float64)[None] / float(G)) * TWO_PI
    r_min, r_max = 0.2 * range_pos, 0.3 * range_pos
    r_g = r_min + u_g * (r_max - r_min)
    cg = centre + r_g[..., None] * np.stack((np.cos(theta), np.sin(theta)), -1)                            # [B, G, 2]
    rho, phi = np.sqrt(-2.0 * np.log(_unit(w[0]))), TWO_PI * _unit(w[1])
    z = rho[..., None] * np.stack((np.cos(phi), np.sin(phi)), -1)                                          # [B, M, 2]
    gts = np.clip(cg[:, np.arange(M) // P] + 0.25 * r_cov * z, 0.0, range_pos)
    order = np.argsort(w[2], axis=1, kind="stable")
    gts = np.take_along_axis(gts, order[:, :, None], 1)
    prior = np.argsort(w[3], axis=1, kind="stable").astype(np.int32)
    return np.broadcast_to(centre, (B, 2)).copy(), gts, prior, order


def sample(n_grps, gts_per_grp, range_pos, r_cov, B, seed, resets, envs=None):
    """(pos_ubs [B,2] f64, pos_gts [B,M,2] f32, prior [B,M] i32): what uavgnn_subs_env_sample writes."""
    ubs, gts, prior, _ = sample64(n_grps, gts_per_grp, range_pos, r_cov, B, seed, resets, envs)
    return ubs, gts.astype(np.float32), prior


def histograms(pos_ubs, pos_gts, prior, range_pos):
    """Integer histograms of a batch of placements, one sample per environment each: GT row 0's x, y, distance from and angle
    about the UBS (32 bins each), the angle between GT rows 0 and 1 as seen from the UBS (32 bins: the group structure), the row at
    which the GT nearest the UBS lands (M bins: the shuffle) and prior[0] (M bins)."""
    pos_ubs, pos_gts, prior = np.asarray(pos_ubs, dtype=np.float64), np.asarray(pos_gts, dtype=np.float64), np.asarray(prior)
    B, M = prior.shape
    rel = pos_gts - pos_ubs[:, None, :]
    dist, ang = np.hypot(rel[..., 0], rel[..., 1]), np.arctan2(rel[..., 1], rel[..., 0])

    def hist(v, lo, hi):
        idx = np.clip(np.floor((v - lo) / (hi - lo) * N_BINS).astype(np.int64), 0, N_BINS - 1)
        return np.bincount(idx, minlength=N_BINS).astype(np.int64)
    return {"gt_x": hist(pos_gts[:, 0, 0], 0.0, range_pos), "gt_y": hist(pos_gts[:, 0, 1], 0.0, range_pos),
            "gt_dist": hist(dist[:, 0], 0.1 * range_pos, 0.4 * range_pos), "gt_angle": hist(ang[:, 0], -np.pi, np.pi),
            "pair_angle": hist(np.mod(ang[:, 1] - ang[:, 0], TWO_PI), 0.0, TWO_PI),
            "nearest_row": np.bincount(np.argmin(dist, axis=1), minlength=M).astype(np.int64),
            "prior0": np.bincount(prior[:, 0], minlength=M).astype(np.int64)}

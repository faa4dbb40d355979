"""The reference's map registry on our side (uav_bs_ctrl_amd/sim.py: MAPS, MapSpec, dense_hotspot_v2) and the DISTRIBUTION of the
reset-time placement sampler, on the CPU: the sampler is checked here through its NumPy restatement (tests/map_sampler_ref.py,
written from the header of csrc/map_sample.hip); tests/test_map_sampler_gpu.py checks the kernel bit for bit against that
restatement.

  * registry against tests/golden/maps_registry.json (the reference's get_params(), avail_moves, max_rate);
  * structural invariants of every placement kind on 2 000 environments (the reference's own set_positions satisfies the same);
  * two-sample chi-square of every histogram of tests/golden/map_sampler_stats.npz (20 000 seeded reference draws) against the
    restatement's 20 000 environments at a fixed seed, below the chi-square quantile at 1 - 1e-6 (Wilson-Hilferty)."""
import dataclasses
import json
import math

import numpy as np
import pytest

from tests import map_sampler_ref as R
from tests.util import GOLDEN
from uav_bs_ctrl_amd import sim

NAMES = ["test", "debug", "inf", "r400", "r800", "4ubs", "6ubs", "8ubs"]
SEED = 0x5EED0FACE


def _num(v):
    return math.inf if v == "inf" else v


def test_registry_holds_exactly_the_reference_names():
    assert list(sim.MAPS) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_registry_matches_the_reference_parameters(name):
    ref = json.load(open(f"{GOLDEN}/maps_registry.json"))[name]
    spec = sim.MAPS[name]
    p, seen = spec.params, set()
    for k, v in ref["params"].items():
        if k in ("n_grps", "gts_per_grp"):
            assert getattr(spec, k) == v, (name, k)
            continue
        seen.add(k)
        got = getattr(p, k)
        if k == "vels":
            assert [float(x) for x in got] == [float(x) for x in np.atleast_1d(v)], (name, k, got, v)
        else:
            assert float(got) == float(_num(v)), (name, k, got, v)
    assert {"range_pos", "episode_limit", "dt", "n_ubs", "n_gts", "r_cov", "n_rbs", "r_sns", "r_comm", "vels", "n_dirs",
            "reward_scale_rate"} <= seen
    defaults = sim.MapParams(n_ubs=p.n_ubs, n_gts=p.n_gts)                 # what no map overrides: the env's class constants
    for f in dataclasses.fields(sim.MapParams):
        if f.name not in seen:
            assert getattr(p, f.name) == getattr(defaults, f.name), (name, f.name)
    assert np.abs(p.avail_moves() - np.asarray(ref["avail_moves"])).max() <= 1e-9
    assert p.avail_moves().shape == np.asarray(ref["avail_moves"]).shape
    assert abs(p.max_rate - ref["max_rate"]) <= 1e-12 * ref["max_rate"]


def test_placement_kinds_of_the_registry():
    kinds = {k: v.kind for k, v in sim.MAPS.items()}
    assert kinds == dict(test="uniform_lattice", debug="fixed", inf="hotspot", r400="hotspot", r800="hotspot",
                         **{f"{n}ubs": "dense_hotspot" for n in (4, 6, 8)})
    v2 = sim.dense_hotspot_v2()
    assert (v2.kind, v2.params.n_gts, v2.params.n_rbs, v2.params.episode_limit, v2.params.dt) == ("dense_hotspot_v2", 100, 10, 100, 10.0)
    assert sim.dense_hotspot_v2(n_ubs=6).params.n_ubs == 6
    # lattice sizes by the reference's integer arithmetic: spots per axis, block side
    assert sim.MAPS["inf"].sampler_consts()[0][3:6] == [10, 5, 2]
    assert sim.MAPS["8ubs"].sampler_consts()[0][3:6] == [30, 7, 4]
    assert v2.sampler_consts()[0][3:5] == [60, 14]
    np.testing.assert_array_equal(np.asarray(sim.MAPS["debug"].fixed_ubs), 100.0 * np.array([[3, 3], [8, 2], [8, 9]]))
    np.testing.assert_array_equal(np.asarray(sim.MAPS["debug"].fixed_gts), 100.0 * np.array([[3, 4], [4, 2], [3, 1], [6, 9]]))


def _draw(spec, B, resets=0):
    ic, fc = spec.sampler_consts()
    return R.sample(ic, fc, B, SEED, resets, spec.fixed_ubs, spec.fixed_gts)


def check_structure(spec, ubs, gts, prior):
    """The invariants of a placement kind (shared with the GPU test's large-batch case)."""
    p = spec.params
    R.check_prior(prior)
    assert gts.dtype == np.float32 and ubs.dtype == np.float64 and (gts >= 0).all() and (gts <= p.range_pos).all()
    if spec.kind == "fixed":
        assert (ubs == np.asarray(spec.fixed_ubs)).all() and (gts == np.asarray(spec.fixed_gts, dtype=np.float32)).all()
        return
    R.check_ubs(ubs, p.range_pos, {"uniform_lattice": 1.0, "dense_hotspot_v2": float(spec.ubs_pitch)}.get(spec.kind, float(spec.min_dist)))
    if spec.kind == "uniform_lattice":
        R.check_ubs(gts, p.range_pos, 1.0)                                  # GTs: distinct lattice points too
    elif spec.kind == "hotspot":
        R.check_hotspot(gts)
    elif spec.kind == "dense_hotspot":
        R.check_dense_hotspot(gts, spec.n_grps, spec.gts_per_grp)
    else:                                                                   # one 800 m square around a multiple of 400 in 400 .. 5600
        mid = np.rint((gts.min(1).astype(np.float64) + gts.max(1)) / 800.0) * 400.0
        assert (mid >= 400).all() and (mid <= p.range_pos - 400).all() and (np.abs(gts - mid[:, None, :]) <= 400.0).all()


@pytest.mark.parametrize("name", ["test", "debug", "inf", "8ubs", "6ubs", "dense_hotspot_v2", "lattice_16x40"])
def test_structural_invariants_of_the_restatement(name):
    if name == "lattice_16x40":                 # the base map with many picks from a small lattice: the sparse table is hit often
        spec = sim.MapSpec(sim.MapParams(n_ubs=16, n_gts=40, range_pos=7.0), "uniform_lattice")
    else:
        spec = sim.dense_hotspot_v2() if name == "dense_hotspot_v2" else sim.MAPS[name]
    check_structure(spec, *_draw(spec, 2000))


def chi2_quantile(df, z=4.753424308822899):
    """Wilson-Hilferty approximation of the chi-square quantile; z = the standard normal quantile at 1 - 1e-6."""
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def chi2_two_sample(a, b):
    """Two-sample chi-square statistic of two count vectors with EQUAL totals, and its degrees of freedom."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.sum() == b.sum()
    keep = (a + b) > 0
    return float((((a - b) ** 2)[keep] / (a + b)[keep]).sum()), int(keep.sum()) - 1


STAT_MAPS = [("inf", "hotspot", 200.0), ("8ubs", "dense_hotspot", 200.0), ("dense_hotspot_v2", "dense_hotspot_v2", 100.0)]


@pytest.mark.parametrize("name,kind,pitch", STAT_MAPS)
def test_distribution_against_the_reference_histograms(name, kind, pitch):
    """Measured chi-square statistic / bound (degrees of freedom) at the committed seeds:
      inf               gt0_cell 0.93 / 32.81 (3), prior0 3.52 / 32.81 (3), spot 19.64 / 72.89 (24), ubs_x 7.26 / 45.97 (9),
                        ubs_y 15.88 / 45.97 (9)
      8ubs              group_cells 3.99 / 57.36 (15), gt01_share_group 1.11 / 27.50 (1), offset_x 9.37 / 45.97 (9),
                        offset_y 4.14 / 45.97 (9), prior0 53.97 / 111.57 (49), spot 38.58 / 110.10 (48), ubs_x 32.12 / 81.02 (29),
                        ubs_y 15.57 / 81.02 (29)
      dense_hotspot_v2  prior0 99.40 / 181.08 (99), spot 176.95 / 303.84 (195), ubs_x 70.84 / 126.05 (59), ubs_y 45.30 / 126.05 (59)
    """
    z = np.load(f"{GOLDEN}/map_sampler_stats.npz")
    N = int(z["n_draws"])
    assert N == 20000
    spec = sim.dense_hotspot_v2() if name == "dense_hotspot_v2" else sim.MAPS[name]
    got = R.histograms(kind, *_draw(spec, N), spec.params.range_pos, pitch)
    keys = sorted(k.split(":", 1)[1] for k in z.files if k.startswith(name + ":"))
    assert keys == sorted(got) and len(keys) >= 4
    bad = []
    for k in keys:
        stat, df = chi2_two_sample(z[f"{name}:{k}"], got[k])
        bound = chi2_quantile(df)
        print(f"{name}:{k}: chi2 = {stat:.2f}, bound {bound:.2f} (df {df})")
        if not stat < bound:
            bad.append((k, stat, bound, df))
    assert not bad, bad


def test_sampling_cells_with_replacement_is_caught():
    """The approximation the end-to-end benchmark carries (group cells drawn WITH replacement) fails the distinct-centres
    invariant, the shared-group histogram and the group-cell counts: the checks above are able to tell."""
    z = np.load(f"{GOLDEN}/map_sampler_stats.npz")
    rs = np.random.RandomState(5)
    B, spec = 20000, sim.MAPS["8ubs"]
    ubs, gts, prior = _draw(spec, B)
    spot = 800.0 * rs.randint(0, 7, (B, 1, 2))
    cells = 200.0 * rs.randint(0, 4, (B, 10, 2)).repeat(5, axis=1)
    bad_gts = (spot + cells + 100.0 * (rs.rand(B, 50, 2) - 0.5)).clip(0, 6000).astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_dense_hotspot(bad_gts)
    h = R.histograms("dense_hotspot", ubs, bad_gts, prior, 6000.0, 200.0)
    stat, df = chi2_two_sample(z["8ubs:gt01_share_group"], h["gt01_share_group"])
    assert stat > chi2_quantile(df)
    held = h["group_cells"].sum()
    assert held < 0.8 * z["8ubs:group_cells"].sum()              # about 7.6 of 16 cells held instead of exactly 10

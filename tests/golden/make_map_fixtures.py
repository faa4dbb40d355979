#!/usr/bin/env python
"""Generates the fixtures of the map registry and the reset-time placement sampler from the REFERENCE's own modules
(envs/mubs_cov/maps.py and mubs_cov.py imported unchanged from /root/reference, over oracle/gym_standin).  Runs only in the build
container (the reference cannot travel).  Data only:

  maps_registry.json      get_params() of the eight registered maps + avail_moves and max_rate as MultiUbsCoverageEnv computes
                          them (infinity encoded as the string "inf")
  map_sampler_stats.npz   integer histograms (tests/map_sampler_ref.py:histograms) over N = 20 000 seeded draws of
                          set_positions() + np.random.permutation(n_gts) for 'inf', '8ubs' and DenseHotSpotV2(); keys
                          "<map>:<histogram>".  'test' is left out: its 250 000-point list costs about 50 ms per draw.
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path[:0] = [os.path.join(ROOT, "oracle", "dgl_standin"), os.path.join(ROOT, "oracle", "gym_standin"), REF, ROOT]

from envs.mubs_cov.maps import MAPS, DenseHotSpotV2  # noqa: E402
from envs.mubs_cov.mubs_cov import MultiUbsCoverageEnv  # noqa: E402

from tests.map_sampler_ref import histograms  # noqa: E402

N_DRAWS = 20000
SEED = 20240


def _plain(v):
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_plain(x) for x in np.asarray(v).tolist()]
    if isinstance(v, (float, np.floating)):
        return "inf" if np.isinf(v) else float(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    return v


def registry():
    out = {}
    for map_id, m in MAPS.items():
        env = MultiUbsCoverageEnv(map_id, record=False)
        out[map_id] = dict(params={k: _plain(v) for k, v in m.get_params().items()},
                           avail_moves=_plain(env.avail_moves), max_rate=float(env.max_rate))
    path = os.path.join(HERE, "maps_registry.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"maps_registry.json -> {os.path.getsize(path)} B")


def stats():
    out = {}
    for name, m, kind, pitch in (("inf", MAPS["inf"], "hotspot", 200.0), ("8ubs", MAPS["8ubs"], "dense_hotspot", 200.0),
                                 ("dense_hotspot_v2", DenseHotSpotV2(), "dense_hotspot_v2", 100.0)):
        random.seed(SEED), np.random.seed(SEED)
        ubs, gts, prior = [], [], []
        for _ in range(N_DRAWS):
            pos = m.set_positions()                              # mubs_cov.py:94-96
            ubs.append(np.asarray(pos["ubs"], dtype=np.float64)), gts.append(np.asarray(pos["gt"], dtype=np.float32))
            prior.append(np.random.permutation(m.n_gts))
        for k, v in histograms(kind, np.stack(ubs), np.stack(gts), np.stack(prior), float(m.range_pos), pitch).items():
            out[f"{name}:{k}"] = v.astype(np.int32)
        print(name, {k: int(v.sum()) for k, v in out.items() if k.startswith(name + ":")})
    out["n_draws"] = np.int32(N_DRAWS)
    path = os.path.join(HERE, "map_sampler_stats.npz")
    np.savez_compressed(path, **out)
    print(f"map_sampler_stats.npz -> {os.path.getsize(path)} B")


if __name__ == "__main__":
    for part in (sys.argv[1:] or ["registry", "stats"]):
        dict(registry=registry, stats=stats)[part]()

"""Trajectory films, the host side (uav_bs_ctrl_amd/film.py), without a GPU.

  1. ``Film.write`` fed with the REFERENCE's film arrays (tests/golden/film_files.npz: the recorders of both simulators run unchanged,
     tests/golden/make_film_fixtures.py) reproduces the three CSV files the reference's ``replay(save_dir=...)`` wrote: parsed with the
     ``csv`` module, the same rows and cells, every header and index cell equal as a string, every numeric cell equal as a parsed
     float64; the multi-UBS ``others.csv`` (an empty frame) byte for byte;
  2. a film refuses an environment of another shape;
  3. the header, the ctypes table and the built library agree on the two new entries;
  4. ``plot=True`` writes a PNG."""
import csv
import functools
import io
import os
import re

import numpy as np
import pytest
import torch as th

from tests.util import GOLDEN

CSV_FILES = ("path_ubs.csv", "pos_gts.csv", "others.csv")
HEADER_ROWS = {"path_ubs.csv": 3, "pos_gts.csv": 1, "others.csv": 1}


@functools.lru_cache(maxsize=None)
def film_npz():
    return np.load(os.path.join(GOLDEN, "film_files.npz"))


def film_arrays(case):
    z = film_npz()
    return {k.split(":")[-1]: z[k] for k in z.files if k.startswith(f"{case}:film:")}


def host_env(case, B=1, **kw):
    """The device simulators' classes on the CPU: their buffers only, nothing is launched."""
    from uav_bs_ctrl_amd.sim import BatchedSingleUbsCoverageEnv, BatchedUbsCoverageEnv, SingleUbsParams
    if case == "mubs":
        return BatchedUbsCoverageEnv.from_map(kw.get("map_id", "debug"), B, device="cpu", seed=0)
    p = SingleUbsParams(n_grps=kw.get("n_grps", 2), gts_per_grp=2, episode_limit=kw.get("episode_limit", int(film_npz()["subs:steps"])))
    return BatchedSingleUbsCoverageEnv(p, B, device="cpu", seed=0)


def reference_film(case):
    from uav_bs_ctrl_amd.film import Film
    z = film_npz()
    film = Film(host_env(case), 2)
    film.put(1, pos_gts=z[f"{case}:pos_gts"], **film_arrays(case))       # episode 1 of 2: the episode offset enters the read-back
    return film


def _rows(text):
    return list(csv.reader(io.StringIO(text, newline="")))


@pytest.mark.parametrize("case", ["mubs", "subs"])
def test_write_reproduces_the_reference_csv_files(case, tmp_path):
    z = film_npz()
    film = reference_film(case)
    film.write(str(tmp_path), 1)
    assert sorted(os.listdir(tmp_path)) == sorted(CSV_FILES), "plot=False writes the three CSV files only"
    n_numeric = 0
    for name in CSV_FILES:
        want_bytes = bytes(z[f"{case}:csv:{name}"])
        with open(tmp_path / name, "rb") as f:
            got_bytes = f.read()
        got, want = _rows(got_bytes.decode()), _rows(want_bytes.decode())
        assert len(got) == len(want), (name, len(got), len(want))
        for r, (g, w) in enumerate(zip(got, want)):
            assert len(g) == len(w), (name, r, g, w)
            for c, (gc, wc) in enumerate(zip(g, w)):
                if r < HEADER_ROWS[name] or c == 0:
                    assert gc == wc, f"{name} row {r} cell {c}: {gc!r} != {wc!r}"
                else:
                    assert float(gc) == float(wc), f"{name} row {r} cell {c}: {gc!r} parses to another float64 than {wc!r}"
                    n_numeric += 1
        if case == "mubs" and name == "others.csv":
            assert got_bytes == want_bytes, "the empty frame's file differs"
    steps, n = int(z[f"{case}:steps"]), 3 if case == "mubs" else 1
    assert n_numeric == (steps + 1) * 2 * n + 4 * 2 + (0 if case == "mubs" else 2 * steps)
    # the float32 GT positions were printed as float32s: the reference's text holds at most 9 significant digits per cell
    if case == "subs":
        with open(tmp_path / "pos_gts.csv") as f:
            cells = [c for row in _rows(f.read())[1:] for c in row[1:]]
        assert all(len(c.replace(".", "").lstrip("0")) <= 9 for c in cells), cells


def test_cells():
    from uav_bs_ctrl_amd.film import _cell
    assert _cell(np.float32(0.1), True) == "0.1" and _cell(np.float64(np.float32(0.1)), False) == "0.10000000149011612"
    assert _cell(0.25000279538720427, False) == "0.25000279538720427" and _cell(300.0, False) == "300.0"
    assert _cell(float("nan"), False) == "" and _cell(np.float32("nan"), True) == ""


def test_episode_and_unwritten_slots():
    film = reference_film("subs")
    host = film.numpy()
    ep0, ep1 = film.episode(0, host), film.episode(1)
    assert all(np.isnan(v).all() for v in ep0.values()), "an episode nobody wrote holds something else than the fill value"
    want = film_arrays("subs")
    assert set(ep1) == set(want) | {"pos_gts"}
    for k, v in want.items():
        assert ep1[k].shape == v.shape and np.array_equal(ep1[k], v.astype(ep1[k].dtype)), k
    assert ep1["pos_ubs"].dtype == np.float64 and ep1["rate_per_gt"].dtype == np.float32 and ep1["pos_gts"].dtype == np.float32
    assert int(host["status"][0]) == 0
    film.check(host), film.check()
    host["status"][0] = 1
    from uav_bs_ctrl_amd._lib import UavGnnError
    with pytest.raises(UavGnnError, match="outside the film"):
        film.check(host)
    with pytest.raises(IndexError):
        film.episode(2)
    film.clear()
    assert all(bool(th.isnan(v).all()) for v in film.fields.values()) and int(film.status) == 0


def test_film_refuses_another_environment_shape():
    from uav_bs_ctrl_amd._lib import UavGnnError
    from uav_bs_ctrl_amd.film import Film
    film = Film(host_env("mubs"), 3)
    film.match(host_env("mubs"))
    for other, what in ((host_env("mubs", B=2), "B = 2"), (host_env("mubs", map_id="r800"), "n = 4"), (host_env("subs"), "single-UBS")):
        with pytest.raises(ValueError, match=what):
            film.reload(other, 0)
        with pytest.raises(ValueError, match="another environment shape"):
            film.click(other, None, 0)
    single = Film(host_env("subs"), 1)
    for other, what in ((host_env("subs", n_grps=3), "M = 6"), (host_env("subs", episode_limit=7), "episode_limit = 7"),
                        (host_env("mubs"), "single-UBS")):
        with pytest.raises(ValueError, match=what):
            single.reload(other, 0)
    with pytest.raises(ValueError, match="actions"):
        single.click(host_env("subs"), None, 0)
    with pytest.raises(ValueError, match="at least one"):
        Film(host_env("mubs"), 0)
    with pytest.raises(UavGnnError, match="no CPU fallback"):          # a film on the host is for reading and writing files only
        film.reload(host_env("mubs"), 0)


def test_header_ctypes_table_and_library_agree_on_the_film_entries(repo_root):
    import ctypes

    from uav_bs_ctrl_amd import _lib
    from uav_bs_ctrl_amd.build import build_lib
    src = open(os.path.join(repo_root, "include", "uavgnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    handle = ctypes.CDLL(build_lib())
    for name in ("uavgnn_film_click_mubs", "uavgnn_film_click_subs"):
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in include/uavgnn.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = ctypes.c_void_p if ("*" in p or "uavgnn_stream_t" in p) else ctypes.c_double if p.startswith("double") else ctypes.c_int
            assert a is want, (name, p, a)
        assert hasattr(handle, name), f"{name} is not exported"
    assert os.path.exists(os.path.join(repo_root, "uav_bs_ctrl_amd", "csrc", "film.hip"))


@pytest.mark.parametrize("case", ["mubs", "subs"])
def test_plot_writes_a_png(case, tmp_path):
    pytest.importorskip("matplotlib")
    film = reference_film(case)
    film.write(str(tmp_path), 1, plot=True)
    png = tmp_path / "trajectories.png"
    assert png.exists() and png.stat().st_size > 1000
    with open(png, "rb") as f:
        assert f.read(8) == b"\x89PNG\r\n\x1a\n"
    assert sorted(os.listdir(tmp_path)) == sorted(CSV_FILES + ("trajectories.png",))

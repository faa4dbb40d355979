"""`-m gpu`: the additions to the resident K1 backward (gatv2_bwd_resident_kernel<LEAN, HT>, csrc/gatv2_bwd_mfma.hip) against
the kernel without them, through the C ABI: the instruction-count changes of the tile loop (UAVGNN_K1_BWD_LEAN, default on) and
the last trip of at most 16 edges run on one score tile (UAVGNN_K1_BWD_HALFTRIP, default on).  Both are bit-identical by
construction, so every comparison against the all-off path is `th.equal` on all seven gradients; the generic kernel is the
independent reference under the rule of tests/test_k1_bwd_resident.py.  (The edge prefetch through LDS this file was planned
for was built, passed these same cases with its own switch, measured flat and was taken out again: DESIGN.md section 8.  The
case with the 1e30 rows was written for it and stays: it holds for any staging that pads a chunk.)

That the two names select different code is not asserted here (nothing to observe through the C ABI but the gradients, which
are equal by design): the four template instances are four kernel symbols, and the kernel traces
profiles/k1_bwd_prefetch_standalone_* show <true, true> by default, <false, true> under UAVGNN_K1_BWD_LEAN=0,
<true, false> under UAVGNN_K1_BWD_HALFTRIP=0.

The grid is 512 workgroups x 4 wavefronts: 8192 + 37 destinations give every wavefront four or five, i.e. every hand-over
(first of a wavefront, next in class, out-of-class skipped, last)."""
import contextlib
import functools
import os

import pytest
import torch as th

pytestmark = pytest.mark.gpu

H = 256
NAMES = ["dW_s", "db_s", "dW_d", "db_d", "dattn", "dW_r", "db_r"]
SLOPE = 0.2
N_MIX = 8192 + 37
SWITCHES = ("UAVGNN_K1_BWD_LEAN", "UAVGNN_K1_BWD_HALFTRIP")


def _problem(deg, seed, ld_out=512, order=None, poison=None):
    """Forward of one `seen`-shaped relation with the given in-degrees on the GPU; returns run(fn) -> the seven gradients.
    `order`: the destinations to process (dst_order of the C ABI; the others are segments nobody owns); `poison`: a mask over
    the segments whose x_src / a_save rows are set to 1e30 behind the forward."""
    from uav_bs_ctrl_amd import _lib as L
    S = int(deg.numel())
    dev = "cuda"
    off = th.zeros(S + 1, dtype=th.int64)
    off[1:] = th.cumsum(deg.to(th.int64), 0)
    E = int(off[-1])
    N = S if order is None else int(order.numel())
    assert E >= 16 * N, "the matrix-core path is chosen for a mean in-degree of 16 or more"
    gen = th.Generator(device=dev).manual_seed(seed)
    x_src = th.rand(E, 4, generator=gen, device=dev) * 2 - 1
    x_dst = th.rand(S, 2, generator=gen, device=dev)
    prm = [0.5 * th.randn(s, generator=gen, device=dev) for s in ((H, 4), (H,), (H, 2), (H,), (H,), (H, 2), (H,))]
    out = th.zeros(S, ld_out, device=dev)
    a_save = th.zeros(E, 4, device=dev)
    lib, st, offd = L.lib(), L.stream(), off.to(th.int32).to(dev)
    ordd = None if order is None else order.to(th.int32).to(dev)

    def optr():   # `ordd` stays referenced by run(): its memory must not go back to the allocator while the kernels read it
        return None if ordd is None else ordd.data_ptr()

    rc = lib.uavgnn_gatv2_fwd(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), optr(), N, *[t.data_ptr() for t in prm],
                              4, 64, SLOPE, out.data_ptr(), ld_out, a_save.data_ptr(), st)
    assert rc == 0
    th.cuda.synchronize()
    if poison is not None:
        rows = th.repeat_interleave(poison.to(dev), deg.to(dev))
        x_src[rows] = 1e30
        a_save[rows] = 1e30
    d_out = th.randn(S, ld_out, generator=gen, device=dev)
    wsb = lib.uavgnn_gatv2_bwd_workspace_bytes(4, H)
    ws = th.empty(wsb // 4, device=dev)

    def run(fn):
        g = [th.full_like(t, float("nan")) for t in prm]
        rc = fn(x_src.data_ptr(), E, 4, x_dst.data_ptr(), 2, offd.data_ptr(), optr(), N, *[t.data_ptr() for t in prm[:5]], 4, 64,
                SLOPE, out.data_ptr(), d_out.data_ptr(), ld_out, a_save.data_ptr(), *[t.data_ptr() for t in g], ws.data_ptr(), wsb,
                st)
        assert rc == 0, rc
        th.cuda.synchronize()
        return g

    return run, lib


@contextlib.contextmanager
def _switches(lean, halftrip):
    """The two A/B switches for the calls inside (the launcher reads them at every call)."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ.update(dict(zip(SWITCHES, (str(int(lean)), str(int(halftrip))))))
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _degrees(pattern):
    gen = th.Generator().manual_seed(5)
    if pattern == "alternating":        # (a) a short destination behind a long one: its upper slots hold the long one's data
        deg = th.full((N_MIX,), 128, dtype=th.int64)
        deg[1::2] = 16
        return deg
    if pattern == "uniform":            # (b)
        return th.randint(16, 129, (N_MIX,), generator=gen)
    if pattern == "out_of_class":       # (c) a quarter outside the class, skipped between two in-class destinations
        deg = th.randint(16, 129, (N_MIX,), generator=gen)
        out = th.rand(N_MIX, generator=gen) < 0.25
        low = th.rand(N_MIX, generator=gen) < 0.5
        deg = th.where(out & low, th.randint(0, 16, (N_MIX,), generator=gen), deg)
        deg = th.where(out & ~low, th.randint(129, 201, (N_MIX,), generator=gen), deg)
        return deg
    return th.full((N_MIX,), int(pattern), dtype=th.int64)   # (d) exact degrees


@functools.lru_cache(maxsize=None)
def _results(pattern):
    """One problem per degree pattern, its gradients with both additions (default environment) and with neither."""
    run, lib = _problem(_degrees(pattern), seed=len(pattern) + 31)
    for k in SWITCHES:
        assert os.environ.get(k) is None, f"{k} is set in the test environment"
    g_new = run(lib.uavgnn_gatv2_bwd)
    with _switches(0, 0):
        g_off = run(lib.uavgnn_gatv2_bwd)
    return run, lib, g_new, g_off


def _identical(g, g_ref, what):
    for a, b, nm in zip(g, g_ref, NAMES):
        assert bool(th.isfinite(a).all()), f"{nm}: {what}"
        assert th.equal(a, b), f"{nm} ({what}): differs in {int((a != b).sum())} elements, worst {float((a - b).abs().max()):.3e}"


def _agree(g_new, g_ref, what):
    for a, b, nm in zip(g_new, g_ref, NAMES):
        assert bool(th.isfinite(a).all()), f"{nm}: {what}"
        scale = float(b.abs().max())
        err = (a - b).abs()
        loose = int((err > 2e-5 * scale).sum())
        assert loose <= 8 and float(err.max()) <= 1e-3 * scale, (
            f"{nm} ({what}): {loose} elements beyond 2e-5 of max|ref|, worst {float(err.max()) / scale:.3e} of max|ref|")


@pytest.mark.parametrize("pattern", ["alternating", "uniform", "out_of_class", "80", "48", "16", "112", "96"])
def test_lean_loop_and_half_trip_bit_identical_to_the_parent_path(pattern):
    """Default (both on) against UAVGNN_K1_BWD_LEAN=0 UAVGNN_K1_BWD_HALFTRIP=0, all seven gradients, and bit-exact over three
    more launches.  Exact degrees: 80 (third trip half), 48 (second trip half), 16 (a half trip only), 112, 96 (no half trip)."""
    run, lib, g_new, g_off = _results(pattern)
    _identical(g_new, g_off, f"default vs both switches off, {pattern}")
    for rep in range(3):
        _identical(run(lib.uavgnn_gatv2_bwd), g_new, f"launch {rep + 2}, {pattern}")


@pytest.mark.parametrize("lean,halftrip", [(1, 0), (0, 1), (1, 1)])
def test_each_switch_alone_at_degree_80(lean, halftrip):
    """Degree 80, 8192 destinations: each addition alone and both together (set explicitly) against neither."""
    run, lib = _problem(th.full((8192,), 80, dtype=th.int64), seed=80)
    with _switches(0, 0):
        g_off = run(lib.uavgnn_gatv2_bwd)
    with _switches(lean, halftrip):
        g = run(lib.uavgnn_gatv2_bwd)
    _identical(g, g_off, f"LEAN={lean} HALFTRIP={halftrip} vs both off")


@pytest.mark.parametrize("pattern", ["uniform", "out_of_class"])
def test_against_the_generic_kernel(pattern):
    run, lib, g_new, _ = _results(pattern)
    _agree(g_new, run(lib.uavgnn_gatv2_bwd_generic), f"default vs generic, {pattern}")


def test_padded_lanes_read_only_their_own_destination():
    """Segments 128, 16, 48 repeating; the 48-edge segments belong to no destination (dst_order leaves them out) and their
    x_src / a_save rows are 1e30.  They lie right behind the rows of a 16-edge destination, where lanes 16..63 of a chunk load
    would land if the padded lanes were not held inside the destination: 0 x 1e30 stays finite, but the de / Sb / T sums would
    move, and the gradients with them.  The 16-edge destinations are half trips whose second-tile V words in LDS are what the
    128-edge destination before them left.  Nothing is read out of bounds either way."""
    groups = (N_MIX + 1) // 2
    deg = th.tensor([128, 16, 48], dtype=th.int64).repeat(groups)
    seg = th.arange(3 * groups)
    run, lib = _problem(deg, seed=4, order=seg[seg % 3 != 2], poison=seg % 3 == 2)
    g_new = run(lib.uavgnn_gatv2_bwd)
    with _switches(0, 0):
        g_off = run(lib.uavgnn_gatv2_bwd)
    _identical(g_new, g_off, "poisoned neighbours, default vs both switches off")

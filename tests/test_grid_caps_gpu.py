"""`-m gpu`: the streaming kernels PAST their grid cap.  Almost every memory-bound kernel in csrc/ launches ``capped_grid(work, per_block,
cap)`` workgroups and walks the rest of its work in a grid-stride loop; the other test files check them where the loop body runs once.
Here every case is larger than the cap it names and ragged (no multiple of the grid: the last trip is partial), as narrow as the kernel
allows, and compared with a host reference of the same operation - the rule of the kernel's own test file, the reference computed once.

What a single-trip test cannot see: a stride that is not the grid size, an index formed in 32 bits, a per-thread accumulator that assumes
the stride keeps its column (the column sums of the fused gate backward), a wave reduction inside the loop that assumes a full wave (its
row maxima), a carry between scan rounds, a barrier that not every thread reaches on the last trip.

Every case asserts the cap it passes with literal numbers.  Outputs the wrapper lets a caller pass are filled with NaN (-1 for integers)
before the call, so an element that is never written shows.  profiles/grid_caps.txt lists every capped launch of csrc/ with the case that
takes it past its cap."""
import functools

import numpy as np
import pytest
import torch as th

from oracle import restatement as R
from tests import graph_builder_ref as GB
from tests import td_return_ref as TD
from tests.util import assert_close, grad_close, needed_rel

pytestmark = pytest.mark.gpu


def _nan(*shape):
    return th.full(shape, float("nan"), device="cuda")


def _close(actual, ref, rel, what, floor=0.0):
    """tests.util.assert_close, with the measured figure printed first (the table in profiles/grid_caps.txt is made from these lines)."""
    print(f"{what}: passes at rel = {needed_rel(actual, ref, floor):.2e} (bound {rel:g})")
    assert_close(actual, ref, rel, what, floor)


# ---- graph builder (csrc/build_graph.hip): index and byte work, every comparison exact ---------------------------------------------------
# obs_degrees / obs_compact: 4096 workgroups of 4 waves, one agent per wave -> 16 384 agents; talk_degrees / talk_compact /
# csc_transpose_env: the same grid over environments -> 16 384 environments; offsets_scan4: rounds of 8192 elements per array, up to
# 2^17 rows, torch.cumsum above.
#               B      n  M   distances set exactly to r_comm per environment
GRAPH_CASES = [(1024, 8, 70, 1),      # N = 8192: exactly one scan round; two ballot trips per agent (M > 64); the static multi-launch path
               (4097, 2, 5, 0),       # N = 8194: a second scan round of two elements, with its carry
               (16389, 2, 3, 1),      # N = 32 778: the observation kernels' loop with a ragged third trip; B > 16 384: the talk kernels' loop;
               #                        five scan rounds over the agents, three over the environments
               (65539, 2, 2, 0)]      # N = 131 078 > 2^17: the cumsum branch
GRAPH_R_COMM = 0.75


@functools.lru_cache(maxsize=None)
def _graph_case(B, n, M, exact):
    rng = np.random.default_rng(B + M)
    raw = GB.random_obs(rng, B, n, M, r_comm=GRAPH_R_COMM, exact=exact)
    ref = GB.build(*raw, GRAPH_R_COMM)
    for a in list(raw) + list(ref.values()):
        a.setflags(write=False)
    return raw, ref


def _graph_arrays(g, flat=False):
    out = {}
    if not flat:
        out["x_a"] = g.agent_feat()
        out["x_gt"], out["seen_off"] = g.relation_segments("seen")
        out["x_ubs"], out["near_off"] = g.relation_segments("near")
    out["talk_off"], out["talk_src"] = g.talk_csc()
    out["talk_eid"], out["graph_off"] = g.talk_eid(), g.graph_off
    return {k: v.cpu().numpy() for k, v in out.items()}


def _first_difference(a, b):
    """None when the arrays are equal (a NaN - an element never written - equals nothing), else a line that says where they are not."""
    if a.shape != b.shape:
        return f"shape {a.shape} vs {b.shape}"
    a, b = a.reshape(-1, a.shape[-1] if a.ndim > 1 else 1), b.reshape(-1, b.shape[-1] if b.ndim > 1 else 1)
    bad = np.flatnonzero((a != b).any(1))
    return f"{bad.size} of {a.shape[0]} rows differ, the first at row {bad[0]}: got {a[bad[0]]}, expected {b[bad[0]]}" if bad.size else None


OFFSETS = ("seen_off", "near_off", "talk_off", "graph_off")
EDGE_ARRAYS = (("x_gt", "seen_off"), ("x_ubs", "near_off"), ("talk_src", "talk_off"), ("talk_eid", "talk_off"))


@pytest.mark.parametrize("B,n,M,exact", GRAPH_CASES, ids=[f"B{c[0]}-n{c[1]}-M{c[2]}" for c in GRAPH_CASES])
def test_device_graph_builder_past_its_caps(B, n, M, exact):
    from uav_bs_ctrl_amd import from_padded_obs, from_padded_obs_flat
    N = B * n
    assert N > 4096, "above the single-launch builder: the multi-launch path, static or not"
    if (B, n, M) == (1024, 8, 70):
        assert N == 8192 and M > 64, "one full scan round of 8192; a second ballot trip over the GT rows"
    elif (B, n, M) == (4097, 2, 5):
        assert 8192 < N == 8194, "the second scan round holds two elements"
    elif (B, n, M) == (16389, 2, 3):
        assert N == 32778 and N > 2 * 16384 and N % 16384 == 10, "obs kernels: 4096 x 4 agents per trip, a ragged third trip"
        assert B > 16384 and B % 16384 == 5, "talk kernels: 4096 x 4 environments per trip, a ragged second trip"
        assert 4 * 8192 < N <= 5 * 8192 and 2 * 8192 < B <= 3 * 8192, "five scan rounds over the agents, three over the environments"
    else:
        assert (B, n, M) == (65539, 2, 2) and N == 131078 and N > 2 ** 17, "above the one-launch scans: the cumsum branch"
    raw, ref = _graph_case(B, n, M, exact)
    if exact:
        assert ((raw[3] == np.float32(GRAPH_R_COMM)) & ~np.eye(n, dtype=bool)[None]).any(), "no distance exactly equal to r_comm"
    dev = [th.tensor(a).cuda() for a in raw]          # a copy: the cached arrays are read-only
    # every graph stays alive until the end, so that no later call is handed a freed block that already holds the right values
    g_dyn = from_padded_obs(*dev, r_comm=GRAPH_R_COMM)
    got = _graph_arrays(g_dyn)
    for k in GB.KEYS:
        assert got[k].dtype == ref[k].dtype, f"{k}: {got[k].dtype}"
        assert (d := _first_difference(got[k], ref[k])) is None, f"from_padded_obs {k}: {d}"
    assert g_dyn.number_of_edges("talk") == ref["talk_src"].size
    g_static = from_padded_obs(*dev, r_comm=GRAPH_R_COMM, static=True)
    got = _graph_arrays(g_static)
    for k in OFFSETS + ("x_a",):
        assert (d := _first_difference(got[k], ref[k])) is None, f"static {k}: {d}"
    for k, ko in EDGE_ARRAYS:
        E = int(ref[ko][-1])
        assert got[k].shape[0] >= E and (d := _first_difference(got[k][:E], ref[k])) is None, f"static {k}: {d}"
        assert not got[k][E:].any(), f"static {k}: a row behind the last edge was written"
    g_flat = from_padded_obs_flat(*dev, r_comm=GRAPH_R_COMM)
    got = _graph_arrays(g_flat, flat=True)
    for k in ("talk_off", "talk_src", "talk_eid", "graph_off"):
        assert (d := _first_difference(got[k], ref[k])) is None, f"from_padded_obs_flat {k}: {d}"
    if B == 16389:       # csc_transpose_env: one wave per graph, 4096 x 4 graphs per trip
        assert g_dyn.hints["max_graph_agents"] == 2 and g_dyn.graph_off.numel() - 1 == B > 16384
        want = GB.transpose(ref["talk_off"], ref["talk_src"])
        for nm, a, b in zip(("t_off", "t_dst", "t_pos"), g_dyn.talk_transpose(), want):
            assert (d := _first_difference(a.cpu().numpy(), b)) is None, f"talk_transpose {nm}: {d}"


# ---- TD tail (csrc/td_return.hip) -----------------------------------------------------------------------------------------------------------
def test_td_tail_past_the_select_caps_and_the_partial_sum_loop():
    """td_select_fwd / td_select_bwd: 2048 workgroups of 256 threads = 524 288 rows / elements per trip; td_loss_sum: one workgroup adds
    the G per-wavefront partials in steps of 256.  Select and its backward are copies and indices: exact.  TD errors under the derived
    bound of tests/test_td_return_gpu.py.  Loss at 1e-5: its terms are non-negative and each passes through at most about 35 fp32
    additions (two fused steps, six wave levels, 17 partials per thread, six levels, four adds): about 2e-6 relative at worst."""
    from tests.test_td_return_gpu import GAMMA, _dev, _inputs, _reference
    from uav_bs_ctrl_amd import _lib as L
    from uav_bs_ctrl_amd import ops
    T, B, C, A = 2, 32771, 8, 3
    N, rows = B * C, T * B * C
    assert rows == 524336 and rows > 2048 * 256 and rows % (2048 * 256) == 48, "select forward: a ragged second trip"
    total = (T + 1) * N * A
    assert total == 2359512 and total > 4 * 2048 * 256 and total % (2048 * 256) != 0, "select backward: a ragged fifth trip"
    G = L.lib().uavgnn_td_return_partials(B, C)
    assert G == 4097 and G > 16 * 256 and G % 256 == 1, "the partial sums: 17 trips, the last one of a single thread"
    seed = 7
    for double_q in (True, False):
        ref = _reference(T, B, C, A, True, True, double_q, "n2", seed)
        agent_out, target_out, acts, rews, dones, weights = (_dev(x) for x in _inputs(T, B, C, A, True, True, seed))
        q, v, na = _nan(T, N), _nan(T, N), th.full((T, N), -1, dtype=th.int32, device="cuda")
        L.check(L.lib().uavgnn_td_select_fwd(agent_out.data_ptr(), target_out.data_ptr(), acts.data_ptr(), T, N, A, int(double_q), q.data_ptr(),
                                             v.data_ptr(), na.data_ptr(), L.stream()), "td_select_fwd")
        for nm, got, want in (("next_acts", na, ref["na"]), ("qvals", q, ref["q"]), ("next_vals", v, ref["v"])):
            assert (d := _first_difference(got.cpu().numpy().astype(want.dtype), want)) is None, f"double_q={double_q} {nm}: {d}"
        q2, v2, na2 = ops.td_select(agent_out, target_out, acts, double_q, return_acts=True)
        assert th.equal(q2, q) and th.equal(v2, v) and th.equal(na2, na), "ops.td_select"
    # the backward on its own: exact against the restatement (a copy to the chosen action, zero elsewhere and in row T)
    d_q = th.randn(T, N, generator=th.Generator().manual_seed(3)).cuda()
    d_out = _nan(T + 1, N, A)
    L.check(L.lib().uavgnn_td_select_bwd(d_q.data_ptr(), acts.data_ptr(), None, T, N, A, d_out.data_ptr(), L.stream()), "td_select_bwd")
    want = TD.d_agent_out(d_q.cpu().numpy().astype(np.float64), acts.cpu().numpy(), A)
    assert (d := _first_difference(d_out.cpu().numpy().astype(np.float64), want)) is None, f"d_agent_out: {d}"
    # targets, TD errors and the loss (double_q off from the last pass of the loop above)
    for tag, returns in (("n2", ("nstep", 2)), ("l0.5", ("lambda", 0.5))):
        ref = _reference(T, B, C, A, True, True, False, tag, seed)
        td_out = _nan(T, B, C)
        loss, td = ops.td_return_loss(q.view(T, B, C), v.view(T, B, C), rews, dones, weights, GAMMA, returns, td_out=td_out, workspace={})
        err = float(np.abs(td.cpu().numpy().astype(np.float64) - ref["td"]).max())
        rel = abs(float(loss) - ref["loss"]) / ref["loss"]
        print(f"td tail {tag}: max |td - td64| = {err:.3e} (bound {ref['bound']:.3e}); loss {float(loss):.8e} vs {ref['loss']:.8e} (rel {rel:.2e})")
        assert td.data_ptr() == td_out.data_ptr() and not bool(th.isnan(td).any())
        assert err <= ref["bound"], f"{tag}: TD error {err:.3e} above {ref['bound']:.3e}"
        _close(loss, th.tensor(ref["loss"], dtype=th.float64), 1e-5, f"{tag}: loss")


# ---- AdamW + clip + polyak through the C ABI (csrc/optim.hip) -------------------------------------------------------------------------------
ADAMW_N = 1048576 + 2051
#               n        n_clip          target clip  t
ADAMW_CASES = [(ADAMW_N, 524289, True, 0.05, 1),            # a clip boundary inside a float4
               (ADAMW_N, ADAMW_N - 1, False, 0.05, 1000),   # a clip boundary inside the scalar tail; no target
               (ADAMW_N, ADAMW_N, True, 0.05, 1000),
               (ADAMW_N, 0, True, 0.05, 1),
               (ADAMW_N, 524289, False, 0.0, 1000),         # clip == 0: nothing is clipped whatever n_clip says
               (ADAMW_N, ADAMW_N, True, 0.0, 1),
               (7, 7, True, 0.05, 1), (7, 5, False, 0.05, 1000), (7, 0, True, 0.0, 1000)]    # all tail behind one float4


@functools.lru_cache(maxsize=None)
def _adamw_inputs(n):
    gen = th.Generator().manual_seed(n)
    return (th.randn(n, generator=gen), 0.2 * th.randn(n, generator=gen), 0.1 * th.rand(n, generator=gen), 0.05 * th.rand(n, generator=gen),
            th.randn(n, generator=gen))       # p, g, m >= 0, v >= 0, target


@pytest.mark.parametrize("n,n_clip,with_target,clip,t", ADAMW_CASES)
def test_adamw_polyak_kernel_tail_clip_boundaries_and_stride_loop(n, n_clip, with_target, clip, t):
    """One step of uavgnn_adamw_polyak from random state against the same update in float64 (torch.optim.AdamW on double tensors,
    clip_grad_value_ on the first n_clip elements, the polyak line): the branches FusedAdamW cannot reach because FlatParams pads every
    parameter to four floats - the scalar tail, a clip boundary inside a float4 and inside the tail - and the grid-stride loop (1024
    workgroups x 256 threads x 4 floats).  One step is a handful of roundings: the bound of the existing test, 2e-6 (floor 1e-7)."""
    from uav_bs_ctrl_amd import _lib as L
    if n > 7:
        assert n == 1050627 and n > 1024 * 256 * 4 and n % (1024 * 256 * 4) == 2051 and n % 4 == 3, "a ragged second trip that ends in a tail"
        assert n_clip in (524289, n - 1, n, 0) and 524289 % 4 == 1
    else:
        assert n % 4 == 3 and n // 4 == 1
    f32 = lambda x: float(np.float32(x))      # noqa: E731  the kernel takes these as C floats: the reference gets the same values
    lr, b1, b2, eps, wd, polyak = f32(3e-3), 0.9, 0.999, f32(1e-8), f32(1e-2), f32(0.9)
    host = _adamw_inputs(n)
    GUARD = 4
    bufs = []
    for x in host:
        b = _nan(n + GUARD)
        b[:n] = x.cuda()
        assert b.data_ptr() % 16 == 0
        bufs.append(b)
    p, g, m, v, targ = bufs
    hyper = th.tensor([lr, float(t)], device="cuda")
    L.check(L.lib().uavgnn_adamw_polyak(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), targ.data_ptr() if with_target else None, n,
                                        n_clip, hyper.data_ptr(), b1, b2, eps, wd, f32(clip), polyak, L.stream()), "uavgnn_adamw_polyak")
    for nm, b in zip(("p", "g", "m", "v", "target"), bufs):
        assert bool(th.isnan(b[n:]).all()), f"{nm}: the guard behind element n was written"
    # float64 reference
    p64, g64, m64, v64, t64 = (x.double().clone() for x in host)
    par = th.nn.Parameter(p64)
    par.grad = g64
    if clip > 0 and n_clip > 0:
        par.grad[:n_clip].clamp_(-f32(clip), f32(clip))        # clip_grad_value_ on the first n_clip elements
    opt = th.optim.AdamW([par], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[par] = dict(step=th.tensor(float(t - 1)), exp_avg=m64, exp_avg_sq=v64)
    opt.step()
    t64 = polyak * t64 + (1 - polyak) * par.data
    what = f"n={n} n_clip={n_clip} clip={clip} t={t}"
    _close(p[:n], par.data, 2e-6, f"{what}: p", floor=1e-7)
    _close(m[:n], opt.state[par]["exp_avg"], 2e-6, f"{what}: exp_avg", floor=1e-7)
    _close(v[:n], opt.state[par]["exp_avg_sq"], 2e-6, f"{what}: exp_avg_sq", floor=1e-7)
    if with_target:
        _close(targ[:n], t64, 2e-6, f"{what}: target", floor=1e-7)
    else:
        assert th.equal(targ[:n].cpu(), host[4]), "a NULL target was written"
    # the gradient written back, bit for bit: clamp below n_clip, the input above it
    want_g = host[1].clone()
    if clip > 0:
        want_g[:n_clip] = want_g[:n_clip].clamp(-f32(clip), f32(clip))
        assert n_clip == 0 or bool((want_g[:n_clip] != host[1][:n_clip]).any()), "no gradient above the clip value"
    assert (d := _first_difference(g[:n].cpu().numpy(), want_g.numpy())) is None, f"{what}: gradient written back: {d}"


# ---- epsilon-greedy selection (csrc/act_select.hip, csrc/eval_stats.hip) --------------------------------------------------------------------
def test_eps_greedy_entries_past_the_cap_with_a_partial_last_team():
    """2048 workgroups x 256 threads = 524 288 agents per trip.  Three-level Q rows (ties are the norm: the first maximum wins), teams
    of 3 with a partial last one.  uavgnn_eps_greedy / _dev: the torch expression of the existing test on the same uniforms;
    uavgnn_eps_greedy_philox: tests/eval_ref.py."""
    from tests import eval_ref
    from tests.test_eval_device_gpu import SEED, _select
    from uav_bs_ctrl_amd import _lib as L
    N, A, n_agents, eps = 524288 + 515, 3, 3, 0.25          # 0.25: the same number as a float and as a double
    assert N == 524803 and N > 2048 * 256 and N % (2048 * 256) == 515 and N % n_agents == 1, "a ragged second trip; the last team has one agent"
    teams = (N + n_agents - 1) // n_agents
    gen = th.Generator().manual_seed(N)
    q_host = th.randint(0, 3, (N, A + 1), generator=gen).float()                     # row stride A + 1
    u_host = th.rand(teams + N, generator=gen)
    q, u = q_host.cuda(), u_host.cuda()
    explore = (u_host[:teams] <= eps).repeat_interleave(n_agents)[:N]
    rand = (u_host[teams:] * A).long().clamp(max=A - 1)
    greedy = q_host[:, :A].argmax(1)
    assert th.equal(greedy, th.as_tensor(np.argmax(q_host[:, :A].numpy(), 1))), "argmax on the host: the first maximum"
    assert 0.3 < float((q_host[:, :A] == q_host[:, :A].max(1, keepdim=True).values).sum(1).gt(1).float().mean()), "ties are common"
    want = th.where(explore, rand, greedy)
    assert 0.2 < float(explore.float().mean()) < 0.3
    eps_dev = th.tensor([eps], device="cuda")
    G = 8
    for name in ("uavgnn_eps_greedy", "uavgnn_eps_greedy_dev"):
        buf = th.full((N + 2 * G,), -1, dtype=th.int64, device="cuda")
        L.check(getattr(L.lib(), name)(q.data_ptr(), q.stride(0), N, A, n_agents, u.data_ptr(), u.data_ptr() + 4 * teams,
                                       float(eps) if name == "uavgnn_eps_greedy" else eps_dev.data_ptr(), buf.data_ptr() + 8 * G, L.stream()), name)
        out = buf.cpu()
        assert bool((out[:G] == -1).all()) and bool((out[G + N:] == -1).all()), f"{name}: a guard word was written"
        assert (d := _first_difference(out[G:G + N].numpy(), want.numpy())) is None, f"{name}: {d}"
    step = 2 ** 32 + 9
    rng = th.tensor([SEED, step], dtype=th.int64, device="cuda")
    q_np = q_host.numpy()
    for on_device in (False, True):
        got = _select(q, N, A, n_agents, rng, eps, on_device)
        assert (d := _first_difference(got, eval_ref.eps_greedy_philox(q_np, A, n_agents, SEED, step, eps))) is None, f"philox: {d}"
        step += 1


# ---- K5 (csrc/disc_comm.hip) ----------------------------------------------------------------------------------------------------------------
def test_gumbel_noise_past_the_cap():
    """gumbel_noise_kernel: 4096 workgroups x 256 threads = 2^20 (edge, channel) pairs per trip.  The last 40 edges against the NumPy
    Philox of tests/test_gpu_parity.py under that test's tolerance; every pair is written."""
    from tests.test_gpu_parity import _philox4x32_10
    from uav_bs_ctrl_amd import _lib as L
    E, M = 16400, 64
    assert E * M == 1049600 and E * M > 4096 * 256 and (E * M) % (4096 * 256) == 1024, "a ragged second trip"
    seed = 0x1234567890ABCDEF & (2 ** 62 - 1)
    rng = th.tensor([seed, 7], dtype=th.int64, device="cuda")
    noise = _nan(E, M, 2)
    L.check(L.lib().uavgnn_gumbel_noise(rng.data_ptr(), E, M, noise.data_ptr(), L.stream()), "uavgnn_gumbel_noise")
    assert not bool(th.isnan(noise).any()), "a pair was never written"
    e_idx, i_idx = np.meshgrid(np.arange(E - 40, E), np.arange(M), indexing="ij")
    ctr = np.stack([e_idx.ravel(), i_idx.ravel(), np.full(e_idx.size, 7), np.zeros(e_idx.size)], 1).astype(np.uint32)
    r = _philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    u = ((r[:, :2] >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
    ref = -np.log(-np.log(u))
    got = noise[E - 40:].cpu().double().numpy().reshape(-1, 2)
    assert np.allclose(got, ref, rtol=2e-5, atol=2e-5), float(np.abs(got - ref).max())
    x = noise.double()
    assert abs(float(x.mean()) - 0.5772156649) < 5 * (1.6449 / x.numel()) ** 0.5 and abs(float(x.var()) - 1.6449340668) < 0.02


def _talk_only(N, max_deg, seed):
    from tests.test_gpu_parity import _random_talk
    g, off, src = _random_talk(N, max_deg, seed)
    deg = (off[1:] - off[:-1])
    assert int(deg.max()) == max_deg and 0.1 < float((deg == 0).float().mean()), "in-degrees 0 .. max_deg, a good share without in-edges"
    return g.to("cuda"), off, src, R.seg_ids(off)


def test_disc_comm_past_the_cap():
    """disc_comm_fwd walks destinations, disc_comm_bwd sources (the transposed CSC): 4096 workgroups x 4 waves = 16 384 of either per
    trip.  Injected noise, msg = 3; the float64 restatement of oracle/restatement.py (disc_comm's message and its exact-tie ownership
    rule: the first in-edge whose hard bit is set owns the channel) under the rules of test_exp3_disc_comm_vs_oracle: 1e-5 forward,
    grad_close with the float32 restatement.  Logits and noise are multiples of 1/64 whose class difference is an odd multiple, so
    logit + noise is exact in both precisions and the hard choice - a discontinuity of the forward - is the same bit in both."""
    from uav_bs_ctrl_amd import ops
    N, msg, tau = 16384 + 70, 3, 0.5
    assert N == 16454 and N > 4096 * 4 and N % (4096 * 4) == 70, "a ragged second trip over destinations and over sources"
    g, off, src, dst = _talk_only(N, 3, seed=N)
    E = src.numel()
    gen = th.Generator().manual_seed(5)
    logits = th.randint(-64, 65, (N, 2 * msg), generator=gen).float() / 32
    gum = th.randint(-96, 97, (E, msg, 2), generator=gen).float() / 32
    gum[..., 1] += 1.0 / 64
    w = th.randn(N, 2 * msg, generator=gen)
    t = logits[src.long()].view(E, msg, 2) + gum
    assert bool((t[..., 0] != t[..., 1]).all()) and bool((t.double() == logits.double()[src.long()].view(E, msg, 2) + gum.double()).all())

    def ref(dtype):
        lg = logits.to(dtype).requires_grad_(True)
        y = th.softmax((lg.index_select(0, src.long()).view(E, msg, 2) + gum.to(dtype)) / tau, -1)
        y_hard = th.zeros_like(y).scatter_(-1, y.max(-1, keepdim=True)[1], 1.0)
        m = (y_hard - y.detach() + y).flatten(1)
        c = R.segment_max_first(m, dst, N, key=y_hard.flatten(1))
        return c, th.autograd.grad((c * w.to(dtype)).sum(), lg)[0], y_hard
    c64, g64, hard64 = ref(th.float64)
    _, g32, hard32 = ref(th.float32)
    assert th.equal(hard64.float(), hard32), "the hard choice differs between the precisions"
    ld = logits.cuda().requires_grad_(True)
    c = ops.disc_comm_aggregate(ld, gum.cuda(), g, tau=tau)
    _close(c, c64, 1e-5, "disc c")
    deg = off[1:] - off[:-1]
    assert bool((c[(deg == 0).cuda()] == 0).all()), "a destination without in-edges receives zeros"
    got, = th.autograd.grad((c * w.cuda()).sum(), ld)
    grad_close(got, g64, f"K5 N={N} msg={msg}: d_logits", ref32=g32)


# ---- K3b (csrc/talk_attn.hip, csrc/talk_attn_env.hip) ---------------------------------------------------------------------------------------
def _k3b_check(graphs, src, dst, N, K, M, what):
    """The comparison of test_talk_attention_kernel_vs_oracle on every graph of ``graphs`` (containers of the same talk relation):
    float64 restatement, assert_close at 1e-5 forward, grad_close with the float32 CPU restatement; attention and uniform form."""
    from uav_bs_ctrl_amd import ops
    gen = th.Generator().manual_seed(1)
    s, q, v = (th.randn(N, d, generator=gen) for d in (K, K, M))
    w = th.randn(N, M, generator=gen)
    src = src.long()

    def ref(s_, q_, v_, uniform):
        if uniform:
            return R.segment_mean(v_[src], dst, N)
        e = (s_[src] * q_[dst]).sum(-1, keepdim=True) / K
        return R.segment_sum(v_[src] * R.segment_softmax(e, dst, N), dst, N)

    for uniform in (False, True):
        s64, q64, v64 = (t.double().requires_grad_(True) for t in (s, q, v))
        c64 = ref(s64, q64, v64, uniform)
        g64 = th.autograd.grad((c64 * w.double()).sum(), [v64] if uniform else [s64, q64, v64])
        s32, q32, v32 = (t.clone().requires_grad_(True) for t in (s, q, v))
        g32 = th.autograd.grad((ref(s32, q32, v32, uniform) * w).sum(), [v32] if uniform else [s32, q32, v32])
        for name, g in graphs:
            sd, qd, vd = (t.cuda().requires_grad_(True) for t in (s, q, v))
            c = ops.talk_attention(None if uniform else sd, None if uniform else qd, vd, g, 1.0 / K)
            _close(c, c64, 1e-5, f"{what} {name}: c uniform={uniform}")
            got = th.autograd.grad((c * w.cuda()).sum(), [vd] if uniform else [sd, qd, vd])
            for a, b, b32, nm in zip(got, g64, g32, ["d_v"] if uniform else ["d_s", "d_q", "d_v"]):
                grad_close(a, b, f"{what} {name}: {nm} uniform={uniform}", ref32=b32)


def test_talk_attention_per_destination_kernels_past_the_cap():
    """talk_attn_fwd and the destination pass of its backward walk destinations, the source pass walks sources (the transposed CSC):
    4096 workgroups x 4 waves = 16 384 of either per trip."""
    from uav_bs_ctrl_amd import ops
    N, K, M = 16384 + 70, 4, 8
    assert N == 16454 and N > 4096 * 4 and N % (4096 * 4) == 70, "a ragged second trip over destinations and over sources"
    g, off, src, dst = _talk_only(N, 3, seed=N + 1)
    assert ops._talk_env(g, M, K) is None, "no graph_off: the per-destination kernels"
    _k3b_check([("per destination", g)], src, dst, N, K, M, f"K3b N={N} K={K} M={M}")


def test_talk_attention_per_graph_kernels_past_the_cap():
    """talk_attn_env_fwd / _bwd: one wave per graph, at most 8192 workgroups.  A workgroup has at most 16 waves, so 8192 x 16 graphs are
    past the cap whatever wave count the LDS budget gives.  Graphs of 1 or 2 agents, self loops allowed, some without any edge."""
    from uav_bs_ctrl_amd import ops
    from uav_bs_ctrl_amd.graph import HeteroBatch
    B, K, M = 8192 * 16 + 8192 + 5, 2, 4
    assert B == 139269 and B > 8192 * 16 and B % 8192 == 5 and B % (8192 * 4) != 0, "ragged at every wave count 1, 2, 4, 8, 16"
    rng = np.random.default_rng(B)
    sizes = rng.integers(1, 3, B)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    N = int(bounds[-1])
    i, j = np.meshgrid(np.arange(2), np.arange(2), indexing="ij")
    keep = (i.ravel()[None] < sizes[:, None]) & (j.ravel()[None] < sizes[:, None]) & (rng.random((B, 4)) < 0.6)     # [B, (i, j)]
    gi, slot = np.nonzero(keep)
    src, dst = bounds[gi] + i.ravel()[slot], bounds[gi] + j.ravel()[slot]
    order = np.argsort(dst * N + src, kind="stable")
    src, dst = th.as_tensor(src[order]), th.as_tensor(dst[order])
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(th.bincount(dst, minlength=N), 0)
    assert 0.05 < float((~keep.any(1)).mean()), "some graphs have no edge at all"
    kw = dict(x_a=th.zeros(N, 2), talk_off=off, talk_src=src.to(th.int32))
    g_env = HeteroBatch.from_arrays(**kw, graph_off=bounds, device="cuda")
    assert ops._talk_env(g_env, M, K) is not None and g_env.hints["max_graph_agents"] == 2, "the per-graph kernels"
    _k3b_check([("per graph", g_env)], src, dst, N, K, M, f"K3b per graph B={B} K={K} M={M}")
    assert "talkT" not in g_env._cache, "the per-graph backward never builds the transpose"


# ---- GRU gates (csrc/gru.hip, csrc/gru_fused.hip) -------------------------------------------------------------------------------------------
def _gru_ref(gi_, gh_, h_, H):
    r = th.sigmoid(gi_[:, :H] + gh_[:, :H])
    z = th.sigmoid(gi_[:, H:2 * H] + gh_[:, H:2 * H])
    n = th.tanh(gi_[:, 2 * H:] + r * gh_[:, 2 * H:])
    return (1 - z) * n + z * h_


@pytest.mark.parametrize("N,H", [(8197, 256), (17480, 30)])
def test_gru_gates_kernels_past_the_cap(N, H):
    """gru_gates_fwd / _bwd: 2048 workgroups x 256 threads per trip, one float4 (H % 4 == 0) or one float per thread.  The float64
    expression and the rules of test_gru_gates_kernel_vs_oracle."""
    from uav_bs_ctrl_amd import ops
    if H == 256:
        assert N * (H // 4) == 524608 and N * (H // 4) > 2048 * 256 and (N * (H // 4)) % (2048 * 256) == 320, "float4 kernels: a ragged second trip"
    else:
        assert H % 4 != 0 and N * H == 524400 and N * H > 2048 * 256 and (N * H) % (2048 * 256) == 112, "scalar kernels: a ragged second trip"
    gen = th.Generator().manual_seed(H)
    gi, gh, h, w = (th.randn(N, d, generator=gen) for d in (3 * H, 3 * H, H, H))
    a64 = [t.double().requires_grad_(True) for t in (gi, gh, h)]
    o64 = _gru_ref(*a64, H)
    g64 = th.autograd.grad((o64 * w.double()).sum(), a64)
    ad = [t.cuda().requires_grad_(True) for t in (gi, gh, h)]
    o = ops.gru_gates(*ad)
    _close(o, o64, 1e-5, "h'")
    for a, b, nm in zip(th.autograd.grad((o * w.cuda()).sum(), ad), g64, ("d_gi", "d_gh", "d_h")):
        _close(a, b, 1e-5, nm, floor=1e-7)


def test_fused_gate_backward_entries_past_the_cap():
    """gru_gates_bwd_fused_kernel, every instantiation the C ABI reaches (_fused, _fused_head, _fused_sums with and without the head,
    _fused_sums_rowmax unpacked and packed): 2048 workgroups x 256 threads, one float4 per thread -> 524 288 float4 per trip; N = 8197
    rows of H = 256 are 524 608, so 320 threads make a second trip and the rest do not.  Against float64: the gate gradients and d_h
    (the rule of test_gru_gates_kernel_vs_oracle, 1e-5 with a floor of 1e-7); the per-workgroup column sums folded over their rows
    against the float64 column sums within 2e-6 of the column's sum of magnitudes (the rule of test_gate_gradient_kernel_column_sums;
    an element is off by a few fp32 roundings of itself plus, through 1 - n^2, about 2.4e-7 |d (1 - z) n|: summed with one sign that
    is below 1e-6 of the sum of magnitudes for standard normal pre-activations, and the fp32 additions add at most depth x 6e-8); the
    row maxima exactly max |.| of the row the call wrote (the rule of the existing row-maximum test).  The variants agree bit for bit
    where the existing tests say so."""
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    N, H, A = 8197, 256, 9
    total = N * (H // 4)
    assert total == 524608 and total > 2048 * 256 and total % (2048 * 256) == 320 and N % 4 != 0, "a ragged second trip"
    G = lib.uavgnn_gru_gates_bwd_sum_rows(N, H)
    assert G == 2048
    gen = th.Generator().manual_seed(N)
    pre, h, dho = th.randn(N, 4 * H, generator=gen), th.tanh(th.randn(N, H, generator=gen)), th.randn(N, H, generator=gen)
    dq, W = th.randn(N, A, generator=gen), 0.3 * th.randn(A, H, generator=gen)

    def ref64(head):
        p64, h64 = pre.double().requires_grad_(True), h.double().requires_grad_(True)
        r, z = th.sigmoid(p64[:, :H]), th.sigmoid(p64[:, H:2 * H])
        n = th.tanh(p64[:, 2 * H:3 * H] + r * p64[:, 3 * H:])
        d_tot = dho.double() + (dq.double() @ W.double() if head else 0.0)
        dp, dh = th.autograd.grad((((1 - z) * n + z * h64) * d_tot).sum(), [p64, h64])
        return dict(d_gi=dp[:, :3 * H], d_gh=th.cat((dp[:, :2 * H], dp[:, 3 * H:]), 1), d_h=dh, d_tot=d_tot,
                    sums=dp.sum(0), scale=dp.abs().sum(0))           # sums: d_r | d_z | d_n (input side) | d_n (hidden side)
    refs = {False: ref64(False), True: ref64(True)}
    pre_d, h_d, dho_d, dq_d, W_d = (t.cuda() for t in (pre, h, dho, dq, W))
    st = L.stream()

    def run(entry, head, packed=False):
        if packed:
            pack = _nan(N, 4 * H)
            d_gi_ptr, d_gh_ptr = pack.data_ptr() + 4 * H, pack.data_ptr()
        else:
            d_gi, d_gh = _nan(N, 3 * H), _nan(N, 3 * H)
            d_gi_ptr, d_gh_ptr = d_gi.data_ptr(), d_gh.data_ptr()
        d_h, sums, rowmax = _nan(N, H), _nan(G, 4 * H), th.full((N,), -1.0, device="cuda")
        hd = (dq_d.data_ptr(), A, W_d.data_ptr()) if head else (None, 0, None)
        common = (N, H, d_gi_ptr, d_gh_ptr, d_h.data_ptr())
        if entry == "fused":          # the head's term handed in as part of d_hout, rounded once
            tot = refs[head]["d_tot"].float().cuda()
            rc = lib.uavgnn_gru_gates_bwd_fused(pre_d.data_ptr(), h_d.data_ptr(), tot.data_ptr(), *common, st)
        elif entry == "head":
            rc = lib.uavgnn_gru_gates_bwd_fused_head(pre_d.data_ptr(), h_d.data_ptr(), dho_d.data_ptr(), *hd, *common, st)
        elif entry == "sums":
            rc = lib.uavgnn_gru_gates_bwd_fused_sums(pre_d.data_ptr(), h_d.data_ptr(), dho_d.data_ptr(), *hd, *common, sums.data_ptr(), st)
        else:
            rc = lib.uavgnn_gru_gates_bwd_fused_sums_rowmax(pre_d.data_ptr(), h_d.data_ptr(), dho_d.data_ptr(), *hd, *common, sums.data_ptr(),
                                                            rowmax.data_ptr(), st)
        L.check(rc, f"gate gradients: {entry}")
        th.cuda.synchronize()
        if packed:                    # G = [dn_h | dr | dz | dn_i]
            d_gi, d_gh = pack[:, H:], th.cat((pack[:, H:3 * H], pack[:, :H]), 1)
        return dict(d_gi=d_gi, d_gh=d_gh, d_h=d_h, sums=sums, rowmax=rowmax)

    def against_float64(out, head, what, sums, rowmax):
        ref = refs[head]
        for k in ("d_gi", "d_gh", "d_h"):
            assert not bool(th.isnan(out[k]).any()), f"{what}: {k} has elements that were never written"
            _close(out[k], ref[k], 1e-5, f"{what}: {k}", floor=1e-7)
        if sums:
            assert not bool(th.isnan(out["sums"]).any()), f"{what}: a column sum was never written"
            worst = float(((out["sums"].double().sum(0).cpu() - ref["sums"]).abs() / ref["scale"]).max())
            print(f"{what}: column sums off by {worst:.2e} of the column's sum of magnitudes (bound 2e-6)")
            assert worst < 2e-6, f"{what}: column sums off by {worst:.2e} of the sum of magnitudes"
        if rowmax:
            assert th.equal(out["rowmax"], th.maximum(out["d_gi"].abs().max(1).values, out["d_gh"].abs().max(1).values)), f"{what}: row maxima"

    plain = run("fused", False)
    against_float64(plain, False, "fused", False, False)
    sums0 = run("sums", False)
    against_float64(sums0, False, "fused_sums without head", True, False)
    head = run("head", True)
    against_float64(head, True, "fused_head", False, False)
    via_tot = run("fused", True)
    sums1 = run("sums", True)
    against_float64(sums1, True, "fused_sums with head", True, False)
    rm = run("rowmax", True)
    against_float64(rm, True, "fused_sums_rowmax", True, True)
    rm_packed = run("rowmax", True, packed=True)
    against_float64(rm_packed, True, "fused_sums_rowmax packed", True, True)
    rm0_packed = run("rowmax", False, packed=True)
    against_float64(rm0_packed, False, "fused_sums_rowmax packed without head", True, True)
    for k in ("d_gi", "d_gh", "d_h"):
        assert th.equal(plain[k], sums0[k]) and th.equal(sums0[k], rm0_packed[k]), f"without head: {k} differs between the entries"
        assert th.equal(head[k], sums1[k]) and th.equal(sums1[k], rm[k]) and th.equal(rm[k], rm_packed[k]), f"with head: {k} differs between the entries"
        _close(head[k], via_tot[k], 2e-6, f"head folded in vs handed in: {k}")
    assert th.equal(sums1["sums"], rm["sums"]) and th.equal(rm["sums"], rm_packed["sums"]) and th.equal(sums0["sums"], rm0_packed["sums"])
    assert th.equal(rm["rowmax"], rm_packed["rowmax"])


# ---- the other capped launches no test had taken past their cap -----------------------------------------------------------------------------
def test_head_kernel_past_the_cap():
    """head_fwd: 4096 workgroups of 4 waves, one 16-row tile per wave -> 16 384 tiles (262 144 rows) per trip.  (The dueling form has
    its own case at this size in tests/test_dueling_head_gpu.py.)  The rule of test_head_kernel_vs_float64: the error of a K = H fp32
    accumulation relative to |h| |W|^T + |b| stays below 4e-7; the narrowest supported head, H = 64."""
    from uav_bs_ctrl_amd import _lib as L
    N, H, A = 262144 + 21, 64, 9
    tiles = (N + 15) // 16
    assert tiles == 16386 and tiles > 4096 * 4 and tiles % (4096 * 4) == 2 and N % 16 == 5, "two waves make a second trip, the last tile is partial"
    gen = th.Generator().manual_seed(N)
    h, W, b = th.randn(N, H, generator=gen).cuda(), (0.2 * th.randn(A, H, generator=gen)).cuda(), th.randn(A, generator=gen).cuda()
    q = _nan(N, A)
    L.check(L.lib().uavgnn_head_fwd(h.data_ptr(), H, N, H, W.data_ptr(), H, b.data_ptr(), A, q.data_ptr(), A, L.stream()), "uavgnn_head_fwd")
    assert not bool(th.isnan(q).any()), "a row was never written"
    ref = h.double() @ W.double().t() + b.double()
    scale = h.double().abs() @ W.double().abs().t() + b.double().abs()
    err = float(((q.double() - ref).abs() / scale).max())
    print(f"head past the cap: error {err:.2e} of |h| |W|^T + |b| (bound 4e-7)")
    assert err < 4e-7, err


def test_valu_k1_forward_past_the_cap():
    """gatv2_fwd_kernel (the forward of head layouts without a matrix-core instantiation; here 4 heads of 8): 4096 workgroups x 4 waves
    = 16 384 destinations per trip.  The float64 restatement of oracle/restatement.py under the parity rule (1e-5); the attention
    weights sum to one per destination with in-edges (the rule of test_mfma_and_valu_kernels_agree_and_order_is_only_a_schedule)."""
    from uav_bs_ctrl_amd import _lib as L
    N, FS, nh, D = 16384 + 70, 4, 4, 8
    H = nh * D
    assert N == 16454 and N > 4096 * 4 and N % (4096 * 4) == 70, "a ragged second trip"
    gen = th.Generator().manual_seed(N)
    deg = th.randint(0, 4, (N,), generator=gen)
    off = th.zeros(N + 1, dtype=th.int32)
    off[1:] = th.cumsum(deg, 0)
    E = int(off[-1])
    assert 0.1 < float((deg == 0).float().mean())
    x_src, x_dst = th.randn(E, FS, generator=gen), th.randn(N, 2, generator=gen)
    p = {"fc_src.weight": 0.5 * th.randn(H, FS, generator=gen), "fc_src.bias": 0.1 * th.randn(H, generator=gen),
         "fc_dst.weight": 0.5 * th.randn(H, 2, generator=gen), "fc_dst.bias": 0.1 * th.randn(H, generator=gen),
         "attn": th.randn(1, nh, D, generator=gen), "res_fc.weight": 0.5 * th.randn(H, 2, generator=gen), "res_fc.bias": 0.1 * th.randn(H, generator=gen)}
    ref = R.gatv2_conv_seg(x_src.double(), x_dst.double(), off, {k: v.double() for k, v in p.items()}, nh).reshape(N, H)
    dev = [p[k].cuda().contiguous() for k in ("fc_src.weight", "fc_src.bias", "fc_dst.weight", "fc_dst.bias", "attn", "res_fc.weight", "res_fc.bias")]
    xs, xd, off_d = x_src.cuda(), x_dst.cuda(), off.cuda()
    out, a_save = _nan(N, H), _nan(E, nh)
    rc = L.lib().uavgnn_gatv2_fwd(xs.data_ptr(), E, FS, xd.data_ptr(), 2, off_d.data_ptr(), None, N, *[t.data_ptr() for t in dev], nh, D, 0.2,
                                  out.data_ptr(), H, a_save.data_ptr(), L.stream())
    assert rc == 0, rc
    assert not bool(th.isnan(out).any()) and not bool(th.isnan(a_save).any()), "an element was never written"
    _close(out, ref, 1e-5, f"K1 forward N={N} nh={nh} D={D}")
    seg = th.repeat_interleave(th.arange(N), deg).cuda()
    sums = th.zeros(N, nh, device="cuda").index_add_(0, seg, a_save)
    has = (deg > 0).cuda()
    _close(sums[has], th.ones_like(sums[has]), 1e-6, "attention weights sum to one per destination")


def test_replay_rebuild_past_the_cap():
    """replay_rebuild_kernel: one workgroup per (step, sampled row), at most 16 384 workgroups, two barriers per item and one before
    the next.  The kernel's own test (tests/test_replay_rebuild_kernel_gpu.py): the rebuilt data IS what the simulator wrote, so every
    comparison is torch.equal.  The 'debug' map (n = 3, M = 4), 7 steps, 2341 sampled rows."""
    from tests import test_replay_rebuild_kernel_gpu as K
    from uav_bs_ctrl_amd.sim import BatchedUbsCoverageEnv
    B, T1 = 2341, K.STEPS + 1
    assert T1 * B == 16387 and T1 * B > 16384 and (T1 * B) % 16384 == 3, "three workgroups make a second trip"
    env = BatchedUbsCoverageEnv.from_map("debug", K.E, seed=5)
    env.reset_from_map()
    ring, rec = K._record(env, seed=1)
    assert K._both(rec["gt"][..., 0]), "the case is vacuous: every GT is seen, or none"
    idx = th.randint(0, K.E + 2, (B,), generator=th.Generator().manual_seed(B)).tolist()       # some beyond the 5 sequences: clamped
    code, got = K._rebuild(env, ring, idx=idx)
    assert code == 0, code
    rows = th.tensor([min(i, K.E - 1) for i in idx], device="cuda")
    for k, v in got.items():
        want = rec[k].index_select(1, rows)
        assert v.shape == want.shape, (k, v.shape, want.shape)
        assert not bool(th.isnan(v).any()), f"{k}: an element of the destination was not written"
        assert th.equal(v, want), f"{k}: {int((v != want).sum())} of {v.numel()} elements differ from what the simulator wrote"


def _film_slots(rng, B, T):
    """Step counters with every slot 0 .. T, and a few outside (those environments write nothing and raise the status bit)."""
    t = rng.integers(0, T + 1, B).astype(np.int32)
    t[rng.integers(0, B, 5)] = T + 1
    t[rng.integers(0, B, 5)] = -1
    t[B - 1], t[B - 2] = T, 0           # the tail of the last trip records
    return t


def _same_with_nan(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), \
        f"{what}: {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} of {got.size} elements differ"


def test_film_click_kernels_past_the_cap():
    """film_click_mubs / film_click_subs: 2048 workgroups x 256 threads = 524 288 (environment, element) pairs per trip.  A slot is a
    copy (the rule of tests/test_film_gpu.py): the NumPy statement of the contract at the head of csrc/film.hip, bit for bit, on a
    NaN-filled film - what an environment does not record stays NaN, an environment outside the film writes nothing.  The reward of
    two agents is (r0 + r1) / 2 in double on both sides; the move table holds 3-4-5 triangles, so the velocity is exact."""
    from uav_bs_ctrl_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(11)
    f64 = lambda a: th.as_tensor(np.ascontiguousarray(a), dtype=th.float64).cuda()      # noqa: E731
    f32 = lambda a: th.as_tensor(np.ascontiguousarray(a), dtype=th.float32).cuda()      # noqa: E731
    nan64 = lambda *s: th.full(s, float("nan"), dtype=th.float64, device="cuda")        # noqa: E731
    # multi-UBS: 2 n + 2 + 2 M elements per environment
    B, n, M, T = 65536 + 3, 2, 1, 2
    W = 2 * n + 2 + 2 * M
    assert B * W == 524312 and B * W > 2048 * 256 and (B * W) % (2048 * 256) == 24, "mubs: a ragged second trip"
    t = _film_slots(rng, B, T)
    pos, gts, run, rew = rng.random((B, n, 2)), rng.random((B, M, 2)).astype(np.float32), rng.random((B, 4)).astype(np.float32), rng.random((B, n))
    film = dict(pos_ubs=nan64(B, T + 1, n, 2), fair_idx=nan64(B, T), reward=nan64(B, T), pos_gts=_nan(B, M, 2))
    status = th.zeros(1, dtype=th.int32, device="cuda")
    dev = [th.as_tensor(t).cuda(), f64(pos), f32(gts), f32(run), f64(rew)]
    rc = lib.uavgnn_film_click_mubs(B, n, M, T, B, 0, *[x.data_ptr() for x in dev], film["pos_ubs"].data_ptr(), film["fair_idx"].data_ptr(),
                                    film["reward"].data_ptr(), film["pos_gts"].data_ptr(), status.data_ptr(), L.stream())
    assert rc == 0, rc
    ok, e = (t >= 0) & (t <= T), np.arange(B)
    want = dict(pos_ubs=np.full((B, T + 1, n, 2), np.nan), fair_idx=np.full((B, T), np.nan), reward=np.full((B, T), np.nan),
                pos_gts=np.full((B, M, 2), np.nan, dtype=np.float32))
    want["pos_ubs"][e[ok], t[ok]] = pos[ok]
    step = ok & (t >= 1)
    want["fair_idx"][e[step], t[step] - 1] = run[step, 2].astype(np.float64)
    want["reward"][e[step], t[step] - 1] = (rew[step, 0] + rew[step, 1]) / 2.0
    want["pos_gts"][ok & (t == 0)] = gts[ok & (t == 0)]
    assert int(status) == 1, "environments outside the film were not reported"
    for k in film:
        _same_with_nan(film[k], want[k], f"mubs {k}")
    # single UBS: 7 + 3 M elements per environment
    B, M, T, A, dt = 52429, 1, 2, 3, 2.0
    W = 7 + 3 * M
    assert B * W == 524290 and B * W > 2048 * 256 and (B * W) % (2048 * 256) == 2, "subs: a ragged second trip"
    t = _film_slots(rng, B, T)
    acts = rng.integers(0, A, B)
    moves = np.array([[3.0, 4.0], [0.0, -2.0], [-6.0, 8.0]])
    pos, gts, run, rew, rate = (rng.random((B, 2)), rng.random((B, M, 2)).astype(np.float32), rng.random((B, 4)), rng.random(B),
                                rng.random((B, M)).astype(np.float32))
    names = ("pos_ubs", "total_throughput", "fair_idx", "global_utility", "reward", "rate_per_gt", "velocity", "pos_gts")
    film = dict(pos_ubs=nan64(B, T + 1, 2), total_throughput=nan64(B, T), fair_idx=nan64(B, T), global_utility=nan64(B, T), reward=nan64(B, T),
                rate_per_gt=_nan(B, T, M), velocity=nan64(B, T), pos_gts=_nan(B, M, 2))
    status.zero_()
    dev = [th.as_tensor(t).cuda(), th.as_tensor(acts, dtype=th.int64).cuda(), f64(moves), f64(pos), f32(gts), f64(run), f64(rew), f32(rate)]
    rc = lib.uavgnn_film_click_subs(B, M, T, A, dt, B, 0, *[x.data_ptr() for x in dev], *[film[k].data_ptr() for k in names], status.data_ptr(),
                                    L.stream())
    assert rc == 0, rc
    ok, e = (t >= 0) & (t <= T), np.arange(B)
    step = ok & (t >= 1)
    want = {k: np.full(tuple(film[k].shape), np.nan, dtype=np.float32 if film[k].dtype == th.float32 else np.float64) for k in names}
    want["pos_ubs"][e[ok], t[ok]] = pos[ok]
    for k, col in (("total_throughput", 0), ("fair_idx", 2), ("global_utility", 3)):
        want[k][e[step], t[step] - 1] = run[step, col]
    want["reward"][e[step], t[step] - 1] = rew[step]
    want["rate_per_gt"][e[step], t[step] - 1] = rate[step]
    want["velocity"][e[step], t[step] - 1] = np.array([5.0, 2.0, 10.0])[acts[step]] / dt
    want["pos_gts"][ok & (t == 0)] = gts[ok & (t == 0)]
    assert int(status) == 1
    for k in names:
        _same_with_nan(film[k], want[k], f"subs {k}")

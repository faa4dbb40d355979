"""``torch.autograd.Function`` wrappers over the C-ABI kernels (include/uavgnn.h).

Each op checks dtype / contiguity / device, takes PyTorch's current HIP stream and calls ``libuavgnn.so`` through
ctypes.  No op has a CPU or eager-PyTorch fallback: CPU tensors raise ``UavGnnError``.
"""
from __future__ import annotations

import os
import torch as th

from . import _lib as L

NEG_SLOPE = 0.2  # DGL GATv2Conv default, not overridden at gnn_agents.py:93-96
K1_IMAGE = os.environ.get("UAVGNN_K1_IMAGE", "1") != "0"   # prepared parameter image inside frozen_weights() scopes (A/B switch)
HETERO_FUSED = True   # K1 forward of both encoder relations in one launch (csrc/gatv2_hetero.hip); False: per relation
# K1's score GEMM on the bf16 matrix cores (exact three-way splits: fp32-level accuracy); False: the fp32-MFMA kernel of rounds 1-3
# (csrc/gatv2_hetero_f32.hip, a source of its own) - the A/B reference and the K1 part of bench.py's strict-fp32 leg
K1_BF16Z = os.environ.get("UAVGNN_K1_BF16Z", "1") != "0"
# row maxima out of the time-batched K1 launches (more than K1_ROWMAX_MIN_ROWS destinations) for an f16x2 f_aggr forward (A/B switch)
K1_ROWMAX = os.environ.get("UAVGNN_K1_ROWMAX", "1") != "0"
K1_ROWMAX_MIN_ROWS = 1 << 17
# ... and out of ANY launch whose `seen` relation has this mean in-degree (a compute-bound launch) from the row count at which the f_aggr
# product behind it takes the f16x2 kernel (GEMM_X3_SMALL_GRID tiles of 256 x 128 for H = 256 output columns)
K1_ROWMAX_DENSE_DEG = int(os.environ.get("UAVGNN_K1_ROWMAX_DENSE_DEG", "16"))
K1_ROWMAX_DENSE_MIN_ROWS = 16384


class _KernelTimer:
    """Optional HIP-event timing of the C-ABI launches (bench.py's live roofline measurement).  Events are recorded
    on PyTorch's current stream, which is the stream every launch is issued on."""

    def __init__(self):
        self.enabled = False
        self.only = None
        self._spans = {}

    def reset(self, enabled=True, only=None):
        """only: names of the spans to time (None = all).  A span costs two event creations + records on the launch
        thread (~15 us) and two timestamp packets on the stream: timing EVERY launch of a cycle makes its rollout phase
        host-bound (tools/launch_bound_probe.py), so a timed benchmark region instruments the kernel it grades only."""
        self._spans = {}
        self.enabled = enabled
        self.only = None if only is None else frozenset(only)

    class _Span:
        def __init__(self, timer, name, work=None):
            self.t, self.name, self.work = timer, name, work

        def __enter__(self):
            self.on = self.t.enabled and (self.t.only is None or self.name in self.t.only)
            if self.on:
                self.e0 = th.cuda.Event(enable_timing=True)
                self.e1 = th.cuda.Event(enable_timing=True)
                self.e0.record()
            return self

        def __exit__(self, *exc):
            if self.on:
                self.e1.record()
                self.t._spans.setdefault(self.name, []).append((self.e0, self.e1, self.work))
            return False

    def span(self, name, work=None):
        """work: optional tuple describing the launch (edges, destinations, saves-attention flag) for byte accounting."""
        return _KernelTimer._Span(self, name, work)

    def summary(self):
        th.cuda.synchronize()
        out = {}
        for name, pairs in self._spans.items():
            ms = [a.elapsed_time(b) for a, b, _ in pairs]
            out[name] = dict(count=len(ms), avg_ms=sum(ms) / len(ms), total_ms=sum(ms), ms=ms,
                             work=[w for _, _, w in pairs if w is not None])
        return out


KERNEL_TIMER = _KernelTimer()


class _HeteroGATv2(th.autograd.Function):
    """K1 over R relations that share the destination nodes.  Returns [N, R*H]: relation i owns columns [i*H, (i+1)*H)
    (so the th.cat of gnn_agents.py:106 never happens).  Per relation the flat argument list carries
    x_src, seg_off, dst_order, attn, W_s, b_s, W_d, b_d, W_r, b_r  (b_r and dst_order may be None)."""

    PER_REL = 10
    last_rowmax = None      # (address of the output, rowmax_near, rowmax_seen) of the forward that just ran, for hetero_gatv2()

    @staticmethod
    def forward(ctx, x_dst, nh, train, *rel_args):
        R = len(rel_args) // _HeteroGATv2.PER_REL
        L.require_gpu(x_dst, *[t for t in rel_args if isinstance(t, th.Tensor)])
        x_dst = L.f32c(x_dst)
        N = x_dst.shape[0]
        H = rel_args[4].shape[0]
        D = H // nh
        out = th.empty((N, R * H), dtype=th.float32, device=x_dst.device)
        saved, meta, has_order = [x_dst], [], []
        # both relations of the observation encoder in ONE launch when the shape has a fused instantiation
        fused = (HETERO_FUSED and R == 2 and N > 0 and rel_args[4].shape[1] == 4 and rel_args[14].shape[1] == 2 and
                 bool(L.lib().uavgnn_gatv2_hetero_supported(4, 2, x_dst.shape[1], nh, D)))
        prepared = []
        for i in range(R):
            x_src, seg_off, order, attn, W_s, b_s, W_d, b_d, W_r, b_r = rel_args[i * 10:(i + 1) * 10]
            x_src = L.f32c(x_src)
            FS = W_s.shape[1]
            if W_s.shape[0] != H or x_src.shape[0] and x_src.shape[1] != FS:
                raise L.UavGnnError("hetero_gatv2: inconsistent relation shapes")
            p = [L.f32c(t.detach()) for t in (W_s, b_s, W_d, b_d, attn, W_r)]
            b_r_c = None if b_r is None else L.f32c(b_r.detach())
            # ctx.needs_input_grad stays True for parameters under torch.no_grad(): `train` (grad mode at the call site)
            # decides whether the attention weights are saved - a rollout / target-network forward must not pay for them
            need = train and any(ctx.needs_input_grad[3 + i * 10 + 3: 3 + i * 10 + 10])
            a_save = th.empty((max(x_src.shape[0], 1), nh), dtype=th.float32, device=x_dst.device) if need else None
            prepared.append((x_src, seg_off, order, p, b_r_c, need, a_save, FS, b_r is not None))
            fused = fused and all(t.data_ptr() % 16 == 0 for t in p + ([b_r_c] if b_r_c is not None else []))
        if fused:
            (xs, so, oo, pS, brS, needS, aS, _, _), (xn, no, _, pN, brN, needN, aN, _, _) = prepared
            lib, pa_s, pa_n = L.lib(), L.ptr_array(pS + [brS]), L.ptr_array(pN + [brN])
            phases = 3 if K1_BF16Z else 3 | 256
            image = None
            if _PLANES is not None and K1_BF16Z and K1_IMAGE:
                # the parameter image of the kernel's prologue, built once per scope instead of by every workgroup of every launch
                # (csrc/gatv2_hetero.hip, K1Image: -0.85 us of a 20-us rollout launch).  Keyed by storage AND version counters.
                ws = pS + pN + [t for t in (brS, brN) if t is not None]
                image = _weight_planes("k1img", ws, (nh, D), lib.uavgnn_gatv2_hetero_image_bytes(),
                                       lambda buf: L.check(lib.uavgnn_gatv2_hetero_prepare(pa_s, pa_n, nh, D, NEG_SLOPE, buf.data_ptr(),
                                                                                           L.stream()), "uavgnn_gatv2_hetero_prepare"))
            with KERNEL_TIMER.span("gatv2_hetero_fwd", (xs.shape[0], xn.shape[0], N, int(needS), int(needN))):
                head = (L.ptr(xs), xs.shape[0], L.ptr(so), L.ptr(oo), L.ptr(xn), xn.shape[0], L.ptr(no), L.ptr(x_dst), N, pa_s, pa_n,
                        nh, D, NEG_SLOPE)
                tail = (out.data_ptr(), R * H, L.ptr(aS), L.ptr(aN), phases, L.stream())
                _HeteroGATv2.last_rowmax = None
                if K1_ROWMAX and K1_BF16Z and GEMM_H2 and GEMM_X3 and (N > K1_ROWMAX_MIN_ROWS or
                                                                       (N >= K1_ROWMAX_DENSE_MIN_ROWS and xs.shape[0] >= K1_ROWMAX_DENSE_DEG * N)):
                    # time-batched launch: the maxima of the two halves of every output row on the way (+9 % on this launch) - the f_aggr
                    # product behind it runs on the f16x2 kernel (-25 %); the store-bound rollout launch on env-realistic degrees would pay
                    # +1.9 us of 18: plain there.  A rollout launch on DENSE degrees (mean in-degree of `seen` >= 16, known from the shapes:
                    # every `gt` source has one out-edge) is compute-bound at 85-90 us: +2 % there, -17 us on the 58-us GEMM behind it
                    rmA, rmB = th.empty(N, dtype=th.float32, device=x_dst.device), th.empty(N, dtype=th.float32, device=x_dst.device)
                    rc = lib.uavgnn_gatv2_hetero_fwd_rowmax(*head, L.ptr(image), out.data_ptr(), R * H, L.ptr(aS), L.ptr(aN), rmA.data_ptr(),
                                                            rmB.data_ptr(), phases, L.stream())
                    if rc == 0:     # a declined launch wrote nothing: the per-relation kernels below fill `out`, and no maxima exist
                        _HeteroGATv2.last_rowmax = (out.data_ptr(), rmA, rmB)
                elif image is not None:
                    rc = lib.uavgnn_gatv2_hetero_fwd_image(*head, image.data_ptr(), *tail)
                else:
                    rc = lib.uavgnn_gatv2_hetero_fwd_phases(*head, *tail)
            if rc == L.UAVGNN_EUNSUPPORTED:
                fused = False
            else:
                L.check(rc, "uavgnn_gatv2_hetero_fwd")
        for i in range(R):
            x_src, seg_off, order, p, b_r_c, need, a_save, FS, has_br = prepared[i]
            if not fused:
                with KERNEL_TIMER.span(f"gatv2_fwd[F={FS}]", (x_src.shape[0], N, int(need))):
                    rc = L.lib().uavgnn_gatv2_fwd(L.ptr(x_src), x_src.shape[0], FS, L.ptr(x_dst), x_dst.shape[1],
                                                  L.ptr(seg_off), L.ptr(order), N, *[L.ptr(t) for t in p], L.ptr(b_r_c), nh,
                                                  D, NEG_SLOPE, out.data_ptr() + 4 * i * H, R * H, L.ptr(a_save), L.stream())
                L.check(rc, "uavgnn_gatv2_fwd")
            saved += [x_src, seg_off, order if order is not None else seg_off, *p,
                      a_save if a_save is not None else x_dst]
            has_order.append(order is not None)
            meta.append((FS, need, has_br, has_order[-1]))
        ctx.nh, ctx.meta, ctx.H = nh, meta, H
        ctx.save_for_backward(*saved, out)
        return out

    @staticmethod
    def backward(ctx, d_out):
        saved = ctx.saved_tensors
        x_dst, out = saved[0], saved[-1]
        nh, H = ctx.nh, ctx.H
        R = len(ctx.meta)
        N, dev = x_dst.shape[0], x_dst.device
        d_out = L.f32c(d_out)
        grads = [None, None, None]
        for i, (FS, need, has_br, has_ord) in enumerate(ctx.meta):
            x_src, seg_off, order, W_s, b_s, W_d, b_d, attn, W_r, a_save = saved[1 + i * 10: 1 + (i + 1) * 10]
            if not need or N == 0:
                grads += [None] * 10
                continue
            g = [th.empty_like(W_s), th.empty_like(b_s), th.empty_like(W_d), th.empty_like(b_d),
                 th.empty_like(attn), th.empty_like(W_r), th.empty(H, dtype=th.float32, device=dev)]
            ws_bytes = L.lib().uavgnn_gatv2_bwd_workspace_bytes(FS, H)
            ws = th.empty(ws_bytes // 4, dtype=th.float32, device=dev)
            with KERNEL_TIMER.span(f"gatv2_bwd[F={FS}]"):
                rc = L.lib().uavgnn_gatv2_bwd(L.ptr(x_src), x_src.shape[0], FS, L.ptr(x_dst), x_dst.shape[1], L.ptr(seg_off),
                                              L.ptr(order) if has_ord else None, N, L.ptr(W_s), L.ptr(b_s), L.ptr(W_d), L.ptr(b_d), L.ptr(attn), nh, H // nh,
                                              NEG_SLOPE, out.data_ptr() + 4 * i * H, d_out.data_ptr() + 4 * i * H,
                                              R * H, L.ptr(a_save), *[L.ptr(t) for t in g], ws.data_ptr(), ws_bytes,
                                              L.stream())
            L.check(rc, "uavgnn_gatv2_bwd")
            dW_s, db_s, dW_d, db_d, dattn, dW_r, db_r = g
            grads += [None, None, None, dattn, dW_s, db_s, dW_d, db_d, dW_r, db_r if has_br else None]
        return tuple(grads)


def hetero_gatv2(x_dst, nh, relations):
    """relations: list of (x_src [E,F], seg_off [N+1] int32, dst_order [N] int32 or None, conv) with conv exposing attn,
    fc_src, fc_dst, res_fc."""
    flat = []
    for x_src, seg_off, order, conv in relations:
        flat += [x_src, seg_off, order, conv.attn, conv.fc_src.weight, conv.fc_src.bias, conv.fc_dst.weight,
                 conv.fc_dst.bias, conv.res_fc.weight, conv.res_fc.bias]
    _HeteroGATv2.last_rowmax = None
    out = _HeteroGATv2.apply(x_dst, nh, th.is_grad_enabled(), *flat)
    rm, _HeteroGATv2.last_rowmax = _HeteroGATv2.last_rowmax, None
    if rm is not None and rm[0] == out.data_ptr():
        # (row maxima of the `near` / `seen` halves: read by linear_relu right behind this call) + the version counter they hold for:
        # an in-place edit of `out` in between leaves them stale
        out._uavgnn_rowmax = (rm[1], rm[2], _version_of(out))
    return out


def _version_of(t):
    """t's version counter (None for an inference tensor, which has none: reading it raises)."""
    try:
        return t._version
    except RuntimeError:
        return None


def _talk_transpose_if_needed(g, *tensors):
    """The transpose of the talk CSC is a backward-only index: skip building it for no-grad forwards (act, target)."""
    if th.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        return g.talk_transpose()
    return None, None, None


def _talk_env(g, M, K):
    """(graph_off, B, n_max) when the batch is made of small graphs the per-graph K3b kernels cover, else None."""
    go, n_max = g.graph_off, g.hints.get("max_graph_agents")
    if go is None or not go.is_cuda or n_max is None or n_max < 1:
        return None
    if not L.lib().uavgnn_talk_attn_env_supported(int(n_max), int(M), int(K)):
        return None
    return go, go.numel() - 1, int(n_max)


def _launch_talk_fwd(env, s, ld_s, q, ld_q, v, ld_v, K, M, talk_off, talk_src, N, scale, c, ld_c, a_save, x_copy, ld_x,
                     n_copy):
    """K3b forward on raw pointers: per-graph kernel when `env` describes the batch, per-destination kernel otherwise."""
    with KERNEL_TIMER.span("talk_attn_fwd"):
        if env is not None:
            go, B, n_max = env
            rc = L.lib().uavgnn_talk_attn_env_fwd(s, ld_s, q, ld_q, v, ld_v, K, M, L.ptr(talk_off), L.ptr(talk_src),
                                                  go.data_ptr(), B, n_max, scale, c, ld_c, a_save, x_copy, ld_x, n_copy,
                                                  L.stream())
        else:
            rc = L.lib().uavgnn_talk_attn_fwd(s, ld_s, q, ld_q, v, ld_v, K, M, L.ptr(talk_off), L.ptr(talk_src), N,
                                              scale, c, ld_c, a_save, x_copy, ld_x, n_copy, L.stream())
    L.check(rc, "uavgnn_talk_attn_fwd")


def _launch_talk_bwd(env, s, ld_s, q, ld_q, v, ld_v, K, M, talk_off, talk_src, transpose, N, scale, a_save, d_c, ld_dc,
                     d_s, ld_ds, d_q, ld_dq, d_v, ld_dv):
    with KERNEL_TIMER.span("talk_attn_bwd"):
        if env is not None:
            go, B, n_max = env
            rc = L.lib().uavgnn_talk_attn_env_bwd(s, ld_s, q, ld_q, v, ld_v, K, M, L.ptr(talk_off), L.ptr(talk_src),
                                                  go.data_ptr(), B, n_max, scale, a_save.data_ptr(), d_c, ld_dc, d_s,
                                                  ld_ds, d_q, ld_dq, d_v, ld_dv, L.stream())
        else:
            t_off, t_dst, t_pos = transpose
            de = th.empty_like(a_save) if s is not None else None
            rc = L.lib().uavgnn_talk_attn_bwd(s, ld_s, q, ld_q, v, ld_v, K, M, L.ptr(talk_off), L.ptr(talk_src),
                                              L.ptr(t_off), L.ptr(t_dst), L.ptr(t_pos), N, scale, a_save.data_ptr(),
                                              d_c, ld_dc, d_s, ld_ds, d_q, ld_dq, d_v, ld_dv, L.ptr(de), L.stream())
    L.check(rc, "uavgnn_talk_attn_bwd")


class _TalkAttention(th.autograd.Function):
    """K3b.  c_v = sum_u softmax_u(<s_u, q_v> * scale) v_u over the talk relation; s = q = None -> mean."""

    @staticmethod
    def forward(ctx, s, q, v, talk_off, talk_src, t_off, t_dst, t_pos, scale, env=None):
        L.require_gpu(v, talk_off, talk_src, s, q)
        N, M = v.shape
        K = 0 if s is None else s.shape[1]
        for t in (s, q, v):
            if t is not None and (t.dtype != th.float32 or t.stride(1) != 1):
                raise L.UavGnnError("talk_attention: float32 row-major inputs required")
        E = talk_src.shape[0]
        c = th.empty((N, M), dtype=th.float32, device=v.device)
        a_save = th.empty(max(E, 1), dtype=th.float32, device=v.device)
        _launch_talk_fwd(env, L.ptr(s), 0 if s is None else s.stride(0), L.ptr(q), 0 if q is None else q.stride(0),
                         L.ptr(v), v.stride(0), K, M, talk_off, talk_src, N, float(scale), c.data_ptr(), c.stride(0),
                         a_save.data_ptr(), None, 0, 0)
        ctx.scale, ctx.uniform, ctx.env = float(scale), s is None, env
        ctx.save_for_backward(*(t for t in (s, q) if t is not None), v, talk_off, talk_src, t_off, t_dst, t_pos, a_save)
        return c

    @staticmethod
    def backward(ctx, d_c):
        if ctx.uniform:
            v, talk_off, talk_src, t_off, t_dst, t_pos, a_save = ctx.saved_tensors
            s = q = None
        else:
            s, q, v, talk_off, talk_src, t_off, t_dst, t_pos, a_save = ctx.saved_tensors
        N, M = v.shape
        K = 0 if s is None else s.shape[1]
        d_c = d_c.contiguous()
        d_v = th.empty((N, M), dtype=th.float32, device=v.device)
        d_s = d_q = None
        if not ctx.uniform:
            d_s = th.empty((N, K), dtype=th.float32, device=v.device)
            d_q = th.empty((N, K), dtype=th.float32, device=v.device)
        _launch_talk_bwd(ctx.env, L.ptr(s), 0 if s is None else s.stride(0), L.ptr(q), 0 if q is None else q.stride(0),
                         L.ptr(v), v.stride(0), K, M, talk_off, talk_src, (t_off, t_dst, t_pos), N, ctx.scale, a_save,
                         d_c.data_ptr(), d_c.stride(0), L.ptr(d_s), K, L.ptr(d_q), K, d_v.data_ptr(), M)
        return d_s, d_q, d_v, None, None, None, None, None, None, None


def talk_attention(s, q, v, g, scale=1.0):
    """g: HeteroBatch carrying the talk relation."""
    off, src = g.talk_csc()
    env = _talk_env(g, v.shape[1], 0 if s is None else s.shape[1])
    t_off, t_dst, t_pos = (None, None, None) if env is not None else _talk_transpose_if_needed(g, s, q, v)
    return _TalkAttention.apply(s, q, v, off, src, t_off, t_dst, t_pos, scale, env)


class _GruGates(th.autograd.Function):
    """K4 pointwise half: h' from the two [N,3H] pre-activation blocks of a GRU cell."""

    @staticmethod
    def forward(ctx, gi, gh, h):
        L.require_gpu(gi, gh, h)
        gi, gh, h = L.f32c(gi), L.f32c(gh), L.f32c(h)
        N, H = h.shape
        h_out = th.empty_like(h)
        with KERNEL_TIMER.span("gru_gates_fwd"):
            rc = L.lib().uavgnn_gru_gates_fwd(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), N, H, h_out.data_ptr(),
                                              L.stream())
        L.check(rc, "uavgnn_gru_gates_fwd")
        ctx.save_for_backward(gi, gh, h)
        return h_out

    @staticmethod
    def backward(ctx, d_hout):
        gi, gh, h = ctx.saved_tensors
        N, H = h.shape
        d_hout = L.f32c(d_hout)
        d_gi, d_gh, d_h = th.empty_like(gi), th.empty_like(gh), th.empty_like(h)
        with KERNEL_TIMER.span("gru_gates_bwd"):
            rc = L.lib().uavgnn_gru_gates_bwd(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), d_hout.data_ptr(), N, H,
                                              d_gi.data_ptr(), d_gh.data_ptr(), d_h.data_ptr(), L.stream())
        L.check(rc, "uavgnn_gru_gates_bwd")
        return d_gi, d_gh, d_h


def gru_gates(gi, gh, h):
    return _GruGates.apply(gi, gh, h)


def _mc_operand(t) -> bool:
    """What every matrix-core wrapper asks of a row-major fp32 operand: unit inner stride, rows of whole float4s, a 16-byte base."""
    return t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


GRU_FUSED = True   # K4 as one kernel (csrc/gru_fused.hip); False: vendor GEMMs + the gate kernel (A/B, tools/gru_probe.py)


GRU_FUSED_MIN_ROWS = 1024   # below: a handful of workgroups walk 18 K slices serially (25 us at 8 rows; vendor GEMMs + gates: 15 us)


def gru_cell_supported(inp, h) -> bool:
    return bool(GRU_FUSED and inp.shape[0] >= GRU_FUSED_MIN_ROWS and inp.is_cuda and inp.dtype == th.float32 and h.dtype == th.float32 and _mc_operand(inp)
                and L.lib().uavgnn_gru_cell_supported(inp.shape[1], h.shape[1]))


GRU_X3 = os.environ.get("UAVGNN_GRU_X3", "1") != "0"   # the cell's GEMMs as bf16x3 splits on the bf16 matrix cores (csrc/gru_x3.hip)
# ... as exactly scaled two-term f16 splits, three products per fp32 product (csrc/gru_h2.hip), where the producer of the cell's input
# hands over the row maxima (the TarMAC step); UAVGNN_GRU_H2=0: the bf16x3 cell everywhere (A/B)
GRU_H2 = os.environ.get("UAVGNN_GRU_H2", "1") != "0"

# bf16 planes of weight matrices (and the parameter image of the fused K1 forward), reused ONLY inside a `frozen_weights()`
# scope.  A drop-in module's weights may change behind any cache (`.data` writes bump no version counter), so by default every
# call splits its weights again (3-5 us, one launch).  The learner's loss forward + backward is one call during which nobody
# can touch the parameters: 101 recurrent steps and 51 backward steps share their planes there (~250 launches, ~1.1 ms of a C3
# cycle).  A rollout between two optimiser steps is the other such interval: ``MultiAgentQLearner.act`` passes a store that
# lives until the learner itself changes the parameters (``apply`` / ``load_checkpoint`` / ``invalidate_weight_cache``).
_PLANES = None
_PLANES_MAX = 128


class frozen_weights:
    """Scope in which the caller guarantees that no parameter changes: weight planes are built once per (storage, layout).

    ``store``: a dict owned by the caller that outlives the scope (entries are reused by later scopes over the same dict until
    the caller clears it); default: a store that dies with the outermost scope."""

    def __init__(self, store=None):
        self.store = store

    def __enter__(self):
        global _PLANES
        self.prev = _PLANES
        if self.store is not None:
            _PLANES = self.store
        elif _PLANES is None:
            _PLANES = {}
        return self

    def __exit__(self, *exc):
        global _PLANES
        _PLANES = self.prev
        return False


def _cached_planes(key, nbytes, device, build, keep=()):
    """planes tensor for `key`; `build(planes)` launches the split when the scope has not seen the key yet.

    The key holds device ADDRESSES of the weights, so an entry also holds strong references to them (`keep`): while the
    entry lives the caching allocator cannot hand those addresses to another tensor, i.e. a hit IS the same storage.  (A
    temporary weight - TarMAC's stacked projection built by th.cat on every call - freed after a no-grad target-network
    step would otherwise let the next policy step's temporary of the same shape land on the same address and pick up the
    TARGET network's planes.)"""
    if _PLANES is not None:
        hit = _PLANES.pop(key, None)
        if hit is not None:
            _PLANES[key] = hit              # most recently used last (dicts keep insertion order)
            return hit[0]
    planes = th.empty(nbytes, dtype=th.uint8, device=device)
    build(planes)
    if _PLANES is not None:
        # a long-lived store fed with temporaries (weights built by th.cat per call) must not grow without bound: the least
        # recently used entries go, one by one - never the whole store in the middle of a scope, and never the K1 parameter image
        while len(_PLANES) >= _PLANES_MAX:
            victim = next((k for k in _PLANES if k[0] != "k1img"), None)
            if victim is None:
                break
            del _PLANES[victim]
        _PLANES[key] = (planes, tuple(keep))
    return planes


def _weight_planes(tag, weights, dims, nbytes, build):
    """``_cached_planes`` under THE key of a prepared form of `weights`: the tag (first: the eviction exempts "k1img"), per weight its
    address, version counter and strides, then `dims` (the layout integers the form depends on).  The entry keeps the weights."""
    key = [tag]
    for W in weights:
        key += (W.data_ptr(), _version_of(W), W.stride())
    key += dims
    return _cached_planes(tuple(key), nbytes, weights[0].device, build, keep=weights)


def gru_cell_two_piece_supported(x, c, h) -> bool:
    """The bf16x3 cell takes its input as [x || c] from two buffers (no concatenated copy) when both pieces are multiples of
    32 columns wide, 16-byte aligned with row strides of whole float4s."""
    K1, K2, H = x.shape[1], c.shape[1], h.shape[1]
    return bool(GRU_X3 and K1 >= 32 and K1 % 32 == 0 and K2 % 32 == 0 and _mc_operand(x) and _mc_operand(c)
                and L.lib().uavgnn_gru_cell_x3_supported(K1 + K2, H)
                and 4 * x.shape[0] * max(x.stride(0), c.stride(0), H) < 2 ** 32)


def gru_cell_h2_supported(K_in, H, N, ld_max) -> bool:
    """The f16x2 cell (csrc/gru_h2.hip) covers this call - given a `row_absmax` from the kernel that produced the input."""
    return bool(GRU_H2 and GRU_X3 and N >= GRU_FUSED_MIN_ROWS and L.lib().uavgnn_gru_cell_h2_supported(K_in, H)
                and 4 * N * max(ld_max, H) < 2 ** 32)


def _gru_cell_launch(inp, h, W_ih, b_ih, W_hh, b_hh, save, inp2=None, h2_out=None, rowmax=None):
    """h' (and the [N, 4H] pre-activation sets when `save`) of the fused GRU cell.  inp2: second piece of the input
    ([inp || inp2] is what W_ih multiplies; the caller checked gru_cell_two_piece_supported).  h2_out: contiguous [N, H]
    buffer h' is written into (a slot of the time-batched staging of a BPTT sequence).  rowmax [N]: max |.| over every row of
    [inp || inp2 || h], written by the kernel that produced the input (the fused TarMAC message launch) - selects the f16x2 cell
    (csrc/gru_h2.hip: half the matrix-core work of the bf16x3 cell; the caller checked gru_cell_h2_supported)."""
    N, H = h.shape
    h2 = th.empty_like(h) if h2_out is None else h2_out
    pre = th.empty((N, 4 * H), dtype=th.float32, device=h.device) if save else None
    if rowmax is not None or inp2 is not None or (GRU_X3 and L.lib().uavgnn_gru_cell_x3_supported(inp.shape[1], H)
                                                  and 4 * N * max(inp.stride(0), H) < 2 ** 32):   # 32-bit byte offsets inside the kernel (3.3 M rows at K_in = 320)
        lib, K1, K2 = L.lib(), inp.shape[1], (0 if inp2 is None else inp2.shape[1])
        K_in = K1 + K2
        # the two matrix-core cells differ in their entries and in one argument: the row maxima in front of the planes (f16x2), the
        # flag word behind the outputs (bf16x3)
        if rowmax is not None:
            tag, arith, ws_bytes, split, fwd = ("gruh2", "f16x2", "uavgnn_gru_cell_h2_workspace_bytes", "uavgnn_gru_split_weights_h2",
                                                "uavgnn_gru_cell_fwd_h2")
            scales, flags = (rowmax.data_ptr(),), ()
        else:
            tag, arith, ws_bytes, split, fwd = ("gru", "bf16x3", "uavgnn_gru_cell_x3_workspace_bytes", "uavgnn_gru_split_weights",
                                                "uavgnn_gru_cell_fwd_x3_opts")
            scales, flags = (), (GRU_X3_FLAGS,)
        with KERNEL_TIMER.span("gru_cell_fwd", (N, K_in, H, arith)):
            # the planes are rebuilt on every call outside a frozen_weights() scope: nothing observable tells when a drop-in
            # module's weights changed
            planes = _weight_planes(tag, (W_ih, W_hh), (K_in, H), getattr(lib, ws_bytes)(K_in, H),
                                    lambda p: L.check(getattr(lib, split)(W_ih.data_ptr(), K_in, W_hh.data_ptr(), H, p.data_ptr(),
                                                                          L.stream()), split))
            rc = getattr(lib, fwd)(inp.data_ptr(), inp.stride(0), K1, L.ptr(inp2), 0 if inp2 is None else inp2.stride(0), K2,
                                   h.data_ptr(), N, H, *scales, planes.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), h2.data_ptr(),
                                   L.ptr(pre), *flags, L.stream())
        L.check(rc, fwd)
        return h2, pre
    with KERNEL_TIMER.span("gru_cell_fwd", (N, inp.shape[1], H, "f32")):
        rc = L.lib().uavgnn_gru_cell_fwd(inp.data_ptr(), inp.stride(0), inp.shape[1], h.data_ptr(), N, H, W_ih.data_ptr(),
                                         b_ih.data_ptr(), W_hh.data_ptr(), b_hh.data_ptr(), h2.data_ptr(), L.ptr(pre),
                                         L.stream())
    L.check(rc, "uavgnn_gru_cell_fwd")
    return h2, pre


def _gru_gates_bwd_from_pre(pre, h, d_hout, d_gi=None, d_gh=None, head=None, sums=None, rowmax=None):
    """Gate gradients from the saved pre-activation sets.  ``head`` = (dq [N, n_out], W_out [n_out, H]): the gradient of h' is
    d_hout (None = 0) + dq W_out, formed inside the kernel (uavgnn_gru_gates_bwd_fused_head).  ``sums``: a
    [uavgnn_gru_gates_bwd_sum_rows(N, H), 4H] buffer that receives the launch's per-workgroup column sums (the bias gradients'
    share of this step)."""
    N, H = h.shape
    if d_gi is None:
        d_gi = th.empty((N, 3 * H), dtype=th.float32, device=h.device)
    if d_gh is None:
        d_gh = th.empty_like(d_gi)
    dh = th.empty_like(h)
    # four entries over one kernel template, named by the optional outputs: _sums (+ _rowmax: the row maxima of d_gi / d_gh, `rowmax` [N],
    # H = 256) take the head's operands whether there is a head or not (NULL, 0, NULL), _head has no optional output, the plain one neither
    if sums is not None:
        entry, outs = ("_sums_rowmax", (sums, rowmax)) if rowmax is not None else ("_sums", (sums,))
    else:
        entry, outs = ("_head" if head is not None else ""), ()
    dq, W_out = head if head is not None else (None, None)
    head_args = (L.ptr(dq), 0 if dq is None else dq.shape[1], L.ptr(W_out)) if entry else ()
    with KERNEL_TIMER.span("gru_gates_bwd"):
        rc = getattr(L.lib(), "uavgnn_gru_gates_bwd_fused" + entry)(pre.data_ptr(), h.data_ptr(), L.ptr(d_hout), *head_args, N, H,
                                                                    d_gi.data_ptr(), d_gh.data_ptr(), dh.data_ptr(),
                                                                    *(t.data_ptr() for t in outs), L.stream())
    L.check(rc, "uavgnn_gru_gates_bwd_fused")
    return d_gi, d_gh, dh


class _GruCellFused(th.autograd.Function):
    """nn.GRUCell as ONE forward launch (K4); backward = gate kernel on the saved pre-activations + vendor GEMMs."""

    @staticmethod
    def forward(ctx, inp, h, W_ih, b_ih, W_hh, b_hh, train, rowmax=None):
        inp, h = L.f32c(inp), L.f32c(h)
        p = [L.f32c(t.detach()) for t in (W_ih, b_ih, W_hh, b_hh)]
        h2, pre = _gru_cell_launch(inp, h, *p, save=bool(train), rowmax=rowmax)
        ctx.have_pre = bool(train)
        if train:
            ctx.save_for_backward(inp, h, pre, p[0], p[2])
        return h2

    @staticmethod
    def backward(ctx, d_h2):
        if not ctx.have_pre:
            raise L.UavGnnError("gru_cell: backward through a forward that saved no pre-activations (train=False)")
        inp, h, pre, W_ih, W_hh = ctx.saved_tensors
        d_gi, d_gh, dh = _gru_gates_bwd_from_pre(pre, h, L.f32c(d_h2))
        d_inp = _mm_nn(d_gi, W_ih) if ctx.needs_input_grad[0] else None
        if ctx.needs_input_grad[1]:
            _mm_nn(d_gh, W_hh, out=dh, accumulate=True)
        else:
            dh = None
        gWih = _wgrad(d_gi, inp) if ctx.needs_input_grad[2] else None
        gbih = _colsum(d_gi) if ctx.needs_input_grad[3] else None
        gWhh = _wgrad(d_gh, h) if ctx.needs_input_grad[4] else None
        gbhh = _colsum(d_gh) if ctx.needs_input_grad[5] else None
        return d_inp, dh, gWih, gbih, gWhh, gbhh, None, None


def row_absmax(*pieces, out=None):
    """[N] = max |.| per row over up to three row-major fp32 matrices with N rows each (Inf for a row that holds Inf / NaN): the
    `rowmax` of the f16x2 GRU cell for callers whose producer does not hand it over (one extra pass over the operand)."""
    ps = [L.f32c(t) for t in pieces]
    N = ps[0].shape[0]
    if out is None:
        out = th.empty(N, dtype=th.float32, device=ps[0].device)
    args = []
    for i in range(3):
        t = ps[i] if i < len(ps) else None
        args += [L.ptr(t), 0 if t is None else t.stride(0), 0 if t is None else t.shape[1]]
    L.check(L.lib().uavgnn_row_absmax(*args, N, out.data_ptr(), L.stream()), "uavgnn_row_absmax")
    return out


def gru_cell(inp, h, cell, rowmax=None):
    """nn.GRUCell(inp, h) with `cell`'s parameters: fused kernel when the shape has an instantiation, else vendor GEMMs +
    the gate kernel.  rowmax [N] (``row_absmax(inp, h)`` or a producer's): the f16x2 cell where it covers the shape."""
    if gru_cell_supported(inp, h):
        # ANY differentiable input makes autograd run the backward, which reads the saved [N, 4H] pre-activation sets
        train = th.is_grad_enabled() and any(t.requires_grad for t in (inp, h, cell.weight_ih, cell.bias_ih,
                                                                       cell.weight_hh, cell.bias_hh))
        if rowmax is not None and not gru_cell_h2_supported(inp.shape[1], h.shape[1], inp.shape[0], inp.stride(0)):
            rowmax = None
        return _GruCellFused.apply(inp, h, cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, train, rowmax)
    gi = linear(inp, cell.weight_ih, cell.bias_ih)
    gh = linear(h, cell.weight_hh, cell.bias_hh)
    return gru_gates(gi, gh, h)


# The recurrence of an agent WITHOUT a communication block over a whole sequence (csrc/gru_rec.hip): the input projection of all steps
# in one GEMM, one launch per step for h W_hh^T + gates, one launch per backward step.  False: the per-step launches of `gru_cell`
# (A/B, tools/exp1_probe.py)
GRU_SEQ = os.environ.get("UAVGNN_GRU_SEQ", "1") != "0"


def gru_unroll_supported(N, H) -> bool:
    """`gru_unroll` covers N rows per step: below the row count from which the fused cells run (they win there)."""
    return bool(GRU_SEQ and 0 < N < GRU_FUSED_MIN_ROWS and L.lib().uavgnn_gru_rec_supported(H))


class _GruRecurrence(th.autograd.Function):
    """h_1 .. h_T1 from the time-batched input pre-activations gi_all [T1 N, 3H] (b_ih included) and h_0 [N, H]."""

    @staticmethod
    def forward(ctx, gi_all, h0, W_hh, b_hh, T1, train):
        L.require_gpu(gi_all, h0, W_hh, b_hh)
        gi_all, W, b = L.f32c(gi_all), L.f32c(W_hh.detach()), L.f32c(b_hh.detach())
        N, H = h0.shape
        if gi_all.shape != (T1 * N, 3 * H):
            raise L.UavGnnError(f"gru_unroll: gi_all {tuple(gi_all.shape)} is not [T1 N, 3H] = [{T1 * N}, {3 * H}]")
        lib, st = L.lib(), L.stream()
        # slot 0 is h_0: the h of every step is a view of the buffer its h' went into
        hbuf = th.empty((T1 + 1, N, H), dtype=th.float32, device=h0.device)
        hbuf[0].copy_(h0)
        pre = th.empty((T1, N, 4 * H), dtype=th.float32, device=h0.device) if train else None
        gi_p, h_p, pre_p = gi_all.data_ptr(), hbuf.data_ptr(), L.ptr(pre)
        with KERNEL_TIMER.span("gru_rec_fwd", (T1, N, H)):
            for t in range(T1):
                rc = lib.uavgnn_gru_rec_fwd(gi_p + 12 * t * N * H, 3 * H, h_p + 4 * t * N * H, H, N, H, W.data_ptr(), b.data_ptr(),
                                            h_p + 4 * (t + 1) * N * H, H, None if pre is None else pre_p + 16 * t * N * H, st)
                L.check(rc, "uavgnn_gru_rec_fwd")
        ctx.have_pre = bool(train)
        if train:
            ctx.save_for_backward(hbuf, pre, W)
        ctx.T1 = T1
        return hbuf[1:]

    @staticmethod
    def backward(ctx, d_hall):
        if not ctx.have_pre:
            raise L.UavGnnError("gru_unroll: backward through a forward that saved no pre-activations (train=False)")
        hbuf, pre, W = ctx.saved_tensors
        T1 = ctx.T1
        N, H = hbuf.shape[1], hbuf.shape[2]
        d_hall = L.f32c(d_hall)
        dev = hbuf.device
        d_gi = th.empty((T1, N, 3 * H), dtype=th.float32, device=dev)
        d_gh = th.empty((T1, N, 3 * H), dtype=th.float32, device=dev)
        carry = th.empty((2, N, H), dtype=th.float32, device=dev)       # step t writes carry[t & 1] and reads carry[(t + 1) & 1]
        lib, st = L.lib(), L.stream()
        pre_p, h_p, dh_p, gi_p, gh_p, c_p = (t.data_ptr() for t in (pre, hbuf, d_hall, d_gi, d_gh, carry))
        with KERNEL_TIMER.span("gru_rec_bwd", (T1, N, H)):
            for t in range(T1 - 1, -1, -1):
                rc = lib.uavgnn_gru_rec_bwd(pre_p + 16 * t * N * H, h_p + 4 * t * N * H, H, dh_p + 4 * t * N * H,
                                            None if t == T1 - 1 else c_p + 4 * ((t + 1) & 1) * N * H, N, H, W.data_ptr(),
                                            gi_p + 12 * t * N * H, gh_p + 12 * t * N * H, c_p + 4 * (t & 1) * N * H, st)
                L.check(rc, "uavgnn_gru_rec_bwd")
        d_gh2 = d_gh.view(T1 * N, 3 * H)
        dW = _wgrad(d_gh2, hbuf[:T1].view(T1 * N, H)) if ctx.needs_input_grad[2] else None
        db = _colsum(d_gh2) if ctx.needs_input_grad[3] else None
        return d_gi.view(T1 * N, 3 * H), (carry[0] if ctx.needs_input_grad[1] else None), dW, db, None, None


def gru_unroll(x_all, h0, cell, T1):
    """h_all [T1, N, H]: nn.GRUCell with `cell`'s parameters unrolled over the T1 time-major steps of x_all [T1 N, K] from h0 [N, H]
    (or [1, H]).  The input projection is ONE `linear` over all steps (so are its weight, bias and input gradients), the recurrence one
    launch per step and direction (csrc/gru_rec.hip), dW_hh / db_hh one reduction over the time-batched gate gradients."""
    N = x_all.shape[0] // T1
    if h0.shape[0] != N:
        h0 = h0.expand(N, -1)
    H = h0.shape[1]
    if not L.lib().uavgnn_gru_rec_supported(H):
        raise L.UavGnnError(f"gru_unroll: no instantiation for H = {H} (uavgnn_gru_rec_supported)")
    gi_all = linear(x_all, cell.weight_ih, cell.bias_ih)
    train = th.is_grad_enabled() and any(t.requires_grad for t in (gi_all, h0, cell.weight_hh, cell.bias_hh))
    return _GruRecurrence.apply(gi_all, h0, cell.weight_hh, cell.bias_hh, T1, train)


def _row_blocks(n, cap=256, min_rows=32):
    """Largest power-of-two block count <= cap that divides n with >= min_rows rows per block."""
    S = 1
    while S < cap and n % (2 * S) == 0 and n // (2 * S) >= min_rows:
        S *= 2
    return S


def _colsum_partial(dy):
    """[S, C] partial column sums of a (possibly column-sliced) [n, C] matrix.  torch's one-pass column reduction
    over 10^4..10^5 rows runs at 0.01-3 TB/s depending on C (48 us for [32768, 9], 34 us for [32768, 768]); blocking
    the rows S = 256 ways first reaches ~5 TB/s for every width (tools/colsum_probe.py), fixed order."""
    n = dy.shape[0]
    S = _row_blocks(n)
    return dy.unflatten(0, (S, n // S)).sum(1)


def _colsum(dy):
    return _colsum_partial(dy).sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# Dense layers on the bf16 matrix cores (csrc/gemm_x3.hip): fp32 in / out, six exact bf16 products per fp32 product
# ---------------------------------------------------------------------------------------------------------------------
GEMM_X3 = os.environ.get("UAVGNN_GEMM_X3", "1") != "0"   # False: vendor fp32 GEMMs (A/B, tools/gemm_x3_probe.py)
# Measured against the recorded vendor solutions at C3 (tools/gemm_x3_probe.py, profiles/r02_gemm_x3_probe.txt): 1.10-1.30x on
# outputs that tile by 128 columns (256, 512), 1.01x on 320 (2.5 tiles), 0.84x on 96: only the first group takes the kernel.


# A/B variants of the bf16x3 kernels are PER-CALL flag words of the C ABI (include/uavgnn.h: the library keeps no process-wide
# state); the probes set these module attributes, the environment seeds them: GEMM 8 (default) / 9 (staging interleaved) / 4
# (128 x 128 tiles), GRU cell 1 (default: staging interleaved) / 0 (staging in blocks)
GEMM_X3_FLAGS = {"8": 0, "9": L.UAVGNN_GEMM_STAGING_INTERLEAVED, "4": L.UAVGNN_GEMM_TILE_128}.get(os.environ.get("UAVGNN_GEMM_X3_VARIANT", "8"), 0)
GRU_X3_FLAGS = L.UAVGNN_GRU_STAGING_BLOCKS if os.environ.get("UAVGNN_GRU_X3_VARIANT", "1") == "0" else 0


GEMM_X3_SMALL_GRID = 128   # fewer 256 x 128 tiles than this: 128 x 128 tiles instead


GEMM_X3_MIN_ROWS = 4096   # fewer rows: the vendor GEMM


def _gemm_epilogue(accumulate, relu) -> int:
    return (L.UAVGNN_GEMM_ACCUMULATE if accumulate else 0) | (L.UAVGNN_GEMM_RELU if relu else 0)


def gemm_x3_supported(a, n_out, k) -> bool:
    return bool(GEMM_X3 and a.is_cuda and a.dtype == th.float32 and a.dim() == 2 and _mc_operand(a) and n_out % 128 == 0
                and a.shape[0] >= GEMM_X3_MIN_ROWS
                and a.shape[0] * a.stride(0) < 2 ** 31 and L.lib().uavgnn_gemm_x3_supported(a.shape[0], n_out, k))


def gemm_x3(a, W, transpose_w=False, bias=None, out=None, accumulate=False, relu=False, rowmax_out=None):
    """out = a @ W.T (transpose_w=False, W [n_out, k]) or a @ W (transpose_w=True, W [k, n_out]) (+ bias) (+ out) (relu).
    `W` may be a strided view with unit inner stride; its bf16 planes are rebuilt on every call (3-5 us: nothing observable
    tells when a drop-in module's weights changed) unless the caller opened a frozen_weights() scope.  Caller checks gemm_x3_supported()."""
    lib = L.lib()
    M, K = a.shape
    R, C = W.shape
    n_out = C if transpose_w else R
    assert (R if transpose_w else C) == K and W.stride(1) == 1
    if out is None:
        out = th.empty((M, n_out), dtype=th.float32, device=a.device)
    with KERNEL_TIMER.span("gemm_x3", (M, n_out, K)):
        planes = _weight_planes("mat", (W,), (R, C, int(transpose_w)), 6 * R * C,
                                lambda p: L.check(lib.uavgnn_split_bf16x3(W.data_ptr(), W.stride(0), R, C, int(transpose_w),
                                                                          p.data_ptr(), L.stream()), "uavgnn_split_bf16x3"))
        flags = GEMM_X3_FLAGS
        if not (flags & L.UAVGNN_GEMM_TILE_128) and ((M + 255) // 256) * ((n_out + 127) // 128) < GEMM_X3_SMALL_GRID:
            # C2-size batches (N_a = 4096): the 256 x 128 tiles of the eight-wave kernel are 32 workgroups on 256 CUs (58 us for
            # [4096, 768] x [768, 256]); the four-wave kernel's 128 x 128 tiles double the workgroups (UAVGNN_GEMM_TILE_128)
            flags |= L.UAVGNN_GEMM_TILE_128
            if ((M + 127) // 128) * ((n_out + 127) // 128) < GEMM_X3_SMALL_GRID:
                flags = (flags & ~L.UAVGNN_GEMM_TILE_128) | L.UAVGNN_GEMM_TILE_64         # still under half the CUs: 64 x 128 tiles
        epi = _gemm_epilogue(accumulate, relu) | flags
        # ... + max |.| over every row of `a`, a by-product of the staging (the 256 x 128-tile kernel only)
        if rowmax_out is not None and not (flags & (L.UAVGNN_GEMM_TILE_128 | L.UAVGNN_GEMM_TILE_64)):
            rc = lib.uavgnn_gemm_nt_x3_rowmax(a.data_ptr(), a.stride(0), M, K, planes.data_ptr(), n_out, L.ptr(bias), out.data_ptr(),
                                              out.stride(0), epi, rowmax_out.data_ptr(), L.stream())
        else:
            if rowmax_out is not None:
                rowmax_out.copy_(a.abs().amax(1))
            rc = lib.uavgnn_gemm_nt_x3(a.data_ptr(), a.stride(0), M, K, planes.data_ptr(), n_out, L.ptr(bias), out.data_ptr(),
                                       out.stride(0), epi, L.stream())
    L.check(rc, "uavgnn_gemm_nt_x3")
    return out


def _mm_nt(x, W, b=None, relu=False):
    """x @ W.T (+ b) (relu): bf16x3 kernel when the shape has one, else the vendor GEMM."""
    if gemm_x3_supported(x, W.shape[0], W.shape[1]) and W.stride(1) == 1 and (b is None or b.is_contiguous()):
        return gemm_x3(x, W, False, bias=b, relu=relu)
    if relu:
        return th._addmm_activation(b, x, W.t())
    return th.addmm(b, x, W.t()) if b is not None else th.mm(x, W.t())


def _mm_nn(dy, W, out=None, accumulate=False, rowmax=None):
    """dy @ W (+ out when accumulate).  rowmax: the row maxima of dy from its producer -> the f16x2 kernel where it covers the shape."""
    operands_ok = W.stride(1) == 1 and (out is None or (out.stride(1) == 1 and out.dtype == th.float32))    # what both kernels ask of W / out
    if rowmax is not None and gemm_h2_supported(dy, W.shape[1], W.shape[0]) and operands_ok:
        return gemm_h2(dy, W, rowmax, True, out=out, accumulate=accumulate)
    if gemm_x3_supported(dy, W.shape[1], W.shape[0]) and operands_ok:
        return gemm_x3(dy, W, True, out=out, accumulate=accumulate)
    if out is None:
        return th.mm(dy, W)
    return out.addmm_(dy, W) if accumulate else th.mm(dy, W, out=out)


def gemm_x3_cat_supported(a1, a2, n_out) -> bool:
    K1, K2 = a1.shape[1], a2.shape[1]
    return bool(a2.is_cuda and a2.dtype == th.float32 and a2.dim() == 2 and a2.shape[0] == a1.shape[0] and K1 % 32 == 0
                and K2 % 32 == 0 and _mc_operand(a2)
                and a2.shape[0] * a2.stride(0) < 2 ** 31 and gemm_x3_supported(a1, n_out, K1 + K2)
                and ((a1.shape[0] + 255) // 256) * ((n_out + 127) // 128) >= GEMM_X3_SMALL_GRID and not (GEMM_X3_FLAGS & L.UAVGNN_GEMM_TILE_128))


def gemm_x3_cat(a1, a2, W1, W2, out):
    """out = a1 @ W1 + a2 @ W2 (W1 [K1, n_out], W2 [K2, n_out], unit inner strides) as ONE bf16x3 product over the contraction
    [a1 || a2] (csrc/gemm_x3.hip, two-source loader; the stacked weight is split once per weight version inside a
    frozen_weights() scope).  Caller checks gemm_x3_cat_supported()."""
    lib = L.lib()
    M, K1 = a1.shape
    K2, n_out = a2.shape[1], W1.shape[1]
    K = K1 + K2
    assert W1.shape[0] == K1 and W2.shape == (K2, n_out) and W1.stride(1) == 1 and W2.stride(1) == 1

    def build(p):
        Wc = th.cat((W1, W2), 0)                                  # [K, n_out], contiguous
        L.check(lib.uavgnn_split_bf16x3(Wc.data_ptr(), n_out, K, n_out, 1, p.data_ptr(), L.stream()), "uavgnn_split_bf16x3")
    with KERNEL_TIMER.span("gemm_x3", (M, n_out, K)):
        planes = _weight_planes("matcat", (W1, W2), (K1, K2, n_out), 6 * K * n_out, build)
        rc = lib.uavgnn_gemm_nt_x3_cat(a1.data_ptr(), a1.stride(0), K1, a2.data_ptr(), a2.stride(0), M, K, planes.data_ptr(), n_out,
                                       None, out.data_ptr(), out.stride(0), GEMM_X3_FLAGS & L.UAVGNN_GEMM_STAGING_INTERLEAVED, L.stream())
    L.check(rc, "uavgnn_gemm_nt_x3_cat")
    return out


# The input-gradient products of the recurrent step and of f_aggr on the f16x2 arithmetic (csrc/gemm_h2.hip: three f16 products per fp32
# product) where the kernel that produced the activation operand hands over its row maxima; UAVGNN_GEMM_H2=0: bf16x3 everywhere (A/B)
GEMM_H2 = os.environ.get("UAVGNN_GEMM_H2", "1") != "0"


def gemm_h2_supported(a, n_out, k) -> bool:
    """The eight-wave f16x2 kernel covers y = a B^T: what gemm_x3_supported asks, and a grid that fills the chip with 256 x 128 tiles
    (the bf16x3 path switches to smaller tiles below; the f16x2 kernel has none)."""
    return bool(GEMM_H2 and gemm_x3_supported(a, n_out, k) and L.lib().uavgnn_gemm_h2_supported(a.shape[0], n_out, k)
                and ((a.shape[0] + 255) // 256) * ((n_out + 127) // 128) >= GEMM_X3_SMALL_GRID)


def gemm_h2(a, W, rowmax, transpose_w=False, bias=None, out=None, accumulate=False, relu=False, a2=None, W2=None, rowmax2=None,
            rowmax2_out=None):
    """out = a @ W.T (transpose_w=False) or a @ W (transpose_w=True) (+ bias) (+ out) (relu) on the f16x2 kernel; with a2 / W2:
    [a || a2] @ [W; W2] (W [K1, n_out], W2 [K2, n_out], transposed form only).  rowmax (and rowmax2): per row an upper bound of
    max |.| over the row of the activation operand, from its producer(s); rowmax2_out [M] instead of rowmax2: the launch takes the row
    maxima of a2 itself and leaves them there (uavgnn_gemm_nt_h2_rm2).  Caller checks gemm_h2_supported()."""
    lib = L.lib()
    M, K1 = a.shape
    if a2 is not None:
        assert transpose_w and W2 is not None and W.stride(1) == 1 and W2.stride(1) == 1
        K2, n_out = a2.shape[1], W.shape[1]
        K = K1 + K2
        tag, weights, dims = "h2cat", (W, W2), (K1, K2, n_out)

        def build(p):
            Wc = th.cat((W, W2), 0)                                   # [K, n_out], contiguous
            L.check(lib.uavgnn_split_h2(Wc.data_ptr(), n_out, K, n_out, 1, p.data_ptr(), L.stream()), "uavgnn_split_h2")
    else:
        R, C = W.shape
        n_out, K = (C, R) if transpose_w else (R, C)
        assert K == K1 and W.stride(1) == 1
        tag, weights, dims = "h2mat", (W,), (R, C, int(transpose_w))      # (gemm_h2_n64 reuses these planes: the same tag and dims there)

        def build(p):
            L.check(lib.uavgnn_split_h2(W.data_ptr(), W.stride(0), R, C, int(transpose_w), p.data_ptr(), L.stream()), "uavgnn_split_h2")
    if out is None:
        out = th.empty((M, n_out), dtype=th.float32, device=a.device)
    with KERNEL_TIMER.span("gemm_h2", (M, n_out, K)):
        planes = _weight_planes(tag, weights, dims, lib.uavgnn_split_h2_bytes(n_out, K), build)
        fn, rm2 = (lib.uavgnn_gemm_nt_h2, rowmax2) if rowmax2_out is None else (lib.uavgnn_gemm_nt_h2_rm2, rowmax2_out)
        rc = fn(a.data_ptr(), a.stride(0), K1, L.ptr(a2), 0 if a2 is None else a2.stride(0), M, K, rowmax.data_ptr(),
                L.ptr(rm2), planes.data_ptr(), n_out, L.ptr(bias), out.data_ptr(), out.stride(0),
                _gemm_epilogue(accumulate, relu) | (GEMM_X3_FLAGS & L.UAVGNN_GEMM_STAGING_INTERLEAVED), L.stream())
    L.check(rc, "uavgnn_gemm_nt_h2")
    return out


# The gate gradients of a staged BPTT step as ONE [N, 4H] buffer G = [dn_h | dr | dz | dn_i] (packed mode of
# uavgnn_gru_gates_bwd_fused_sums_rowmax) instead of d_gi / d_gh [N, 3H] each, whose r / z columns hold the same numbers: a third of the
# kernel's gate-gradient writes and of the stage buffers; the consumers read strided views.  A/B switch
G4 = os.environ.get("UAVGNN_G4", "1") != "0"
# d c = d_gi W_ih[:, H:] of the recurrent step on the f16x2 arithmetic, 128 x 64 output tiles (csrc/gemm_h2.hip); 0: vendor fp32 GEMM (A/B)
DC_H2 = os.environ.get("UAVGNN_DC_H2", "1") != "0"
GEMM_H2_N64_MIN_GRID = 128   # fewer 128 x 64 tiles than this (half the CUs): the vendor GEMM


def gemm_h2_n64_supported(a, n_out, k) -> bool:
    """The 128 x 64-tile f16x2 kernel covers y = a B^T with n_out % 64 == 0 on a grid that fills at least half the chip."""
    return bool(DC_H2 and GEMM_H2 and a.is_cuda and a.dtype == th.float32 and a.dim() == 2 and _mc_operand(a) and a.shape[1] == k
                and n_out % 64 == 0 and k % 64 == 0 and a.shape[0] * a.stride(0) < 2 ** 31
                and L.lib().uavgnn_gemm_h2_supported(a.shape[0], n_out, k)
                and ((a.shape[0] + 127) // 128) * (n_out // 64) >= GEMM_H2_N64_MIN_GRID)


def gemm_h2_n64(a, W, rowmax, out=None):
    """out = a @ W (W [k, n_out], a view with unit inner stride) on the 128 x 64-tile f16x2 kernel.  rowmax: per row an upper bound of
    max |.| over the row of `a`, from its producer.  Caller checks gemm_h2_n64_supported()."""
    lib = L.lib()
    M, K = a.shape
    R, n_out = W.shape
    assert R == K and W.stride(1) == 1
    if out is None:
        out = th.empty((M, n_out), dtype=th.float32, device=a.device)
    with KERNEL_TIMER.span("gemm_h2_n64", (M, n_out, K)):
        # the planes of gemm_h2(a, W, ., transpose_w=True): whichever kernel meets W first in a scope splits it for both
        planes = _weight_planes("h2mat", (W,), (R, n_out, 1), lib.uavgnn_split_h2_bytes(n_out, K),
                                lambda p: L.check(lib.uavgnn_split_h2(W.data_ptr(), W.stride(0), R, n_out, 1, p.data_ptr(), L.stream()),
                                                  "uavgnn_split_h2"))
        rc = lib.uavgnn_gemm_nt_h2_n64(a.data_ptr(), a.stride(0), M, K, rowmax.data_ptr(), planes.data_ptr(), n_out, out.data_ptr(),
                                       out.stride(0), L.stream())
    L.check(rc, "uavgnn_gemm_nt_h2_n64")
    return out


# Weight gradients on the bf16 matrix cores (csrc/gemm_tn_x3.hip).
# Measured against the vendor's batched split-K fp32 GEMM (tools/gemm_tn_probe.py, profiles/r03_gemm_tn_probe.txt): BOTH operands
# have to be split and transposed inside the kernel, which bounds it at 95-108 TFLOP/s fp32-equivalent = the vendor's 106-108
# at the per-step shapes (32 768 rows; 0.4-0.6 x on the 96- and 9-row outputs), 142 vs 134 at the time-batched encoder shape
# (1.67 M rows).  Only the latter takes the kernel; its error against float64 is 0.5-0.8 x the vendor's on every shape.
GEMM_TN_MIN_ROWS = 1 << 18
# ... on the f16x2 arithmetic with LDS transposing reads (csrc/gemm_tn_h2.hip): the recurrent weights of a staged BPTT sequence
# (A/B switch: bench.py's result line names UAVGNN_GEMM_TN_H2=0 as the way back to bf16x3 / the vendor GEMM)
GEMM_TN_H2 = os.environ.get("UAVGNN_GEMM_TN_H2", "1") != "0"
# ... on 256 x 160 / 256 x 96 output tiles where such a width divides the input width and 128 does not (dW_ih, dWp: no padded MFMA column
# tile; uavgnn_gemm_tn_h2_width).  A/B switch: UAVGNN_GEMM_TN_TILES=0 runs every product on the 128-wide tiles at their chunk count
GEMM_TN_TILES = os.environ.get("UAVGNN_GEMM_TN_TILES", "1") != "0"


def _max_two_stage(t):
    """max over all elements as row maxima of a [S, numel / S] view, then the maximum of the S row maxima - neither stage takes torch's
    multi-block semaphore path, whose final write did not always land inside a replayed hipGraph (learner._mse)."""
    n = t.numel()
    S = 1
    while S < 1024 and n % (2 * S) == 0 and n // (2 * S) >= 256:
        S *= 2
    return t.reshape(S, n // S).max(1).values.max()


def _gemm_tn_h2_shape(n, Mo, Ko, min_in=128) -> bool:
    """csrc/gemm_tn_h2.hip (256 x 128 output tiles) takes an [Mo, Ko] = [n, Mo]^T [n, Ko] product of CUDA fp32 operands - the shape half
    of gemm_tn_h2_supported, for a forward that asks before the gradient operand exists (_LinearReLU)."""
    return bool(GEMM_X3 and GEMM_H2 and GEMM_TN_H2 and n >= GEMM_TN_MIN_ROWS
                and Mo >= 256 and Ko >= min_in       # (a 9-row output leaves most of a 256 x 128 tile idle: the vendor GEMM)
                and L.lib().uavgnn_gemm_tn_h2_supported(n, Mo, Ko))


def gemm_tn_h2_supported(dy, x, min_in=128) -> bool:
    """dy^T x on csrc/gemm_tn_h2.hip.  min_in: the narrowest `x` worth a 128-wide tile - 128 by default; the 96-column projections pass
    96 with the operands SWAPPED (x^T d_proj = dWp^T: three quarters of a tile instead of three eighths)."""
    return bool(dy.is_cuda and dy.dtype == th.float32 and x.dtype == th.float32 and dy.dim() == 2 and x.dim() == 2
                and dy.shape[0] == x.shape[0] and _mc_operand(dy) and _mc_operand(x)
                and _gemm_tn_h2_shape(dy.shape[0], dy.shape[1], x.shape[1], min_in))


def gemm_tn_x3_supported(dy, x) -> bool:
    return bool(GEMM_X3 and dy.is_cuda and dy.dtype == th.float32 and x.dtype == th.float32 and dy.dim() == 2
                and x.dim() == 2 and dy.shape[0] == x.shape[0] and dy.shape[0] >= GEMM_TN_MIN_ROWS and dy.stride(1) == 1
                and x.stride(1) == 1 and dy.shape[1] > 0 and x.shape[1] > 0)


def gemm_tn_x3(dy, x, partials=None, accumulate=False):
    """partials [S, out, in] (+)= chunked dy^T x (csrc/gemm_tn_x3.hip; the caller sums over S).  Caller checks
    gemm_tn_x3_supported()."""
    lib = L.lib()
    n, Mo, Ko = dy.shape[0], dy.shape[1], x.shape[1]
    if partials is None:
        S = lib.uavgnn_gemm_tn_x3_chunks(n, Mo, Ko)
        partials = th.empty((S, Mo, Ko), dtype=th.float32, device=dy.device)
    with KERNEL_TIMER.span("gemm_tn_x3", (n, Mo, Ko)):
        rc = lib.uavgnn_gemm_tn_x3(dy.data_ptr(), dy.stride(0), Mo, x.data_ptr(), x.stride(0), Ko, n, partials.data_ptr(),
                                   partials.shape[0], int(accumulate), L.stream())
    L.check(rc, "uavgnn_gemm_tn_x3")
    return partials


def _wgrad_partials(dy, x, bounds=None, allow_tn=True, slot=None):
    """[S, out, in] partials of the weight gradient dy^T x, the reduction over the rows split into S chunks (the caller sums over S, in
    a fixed order: deterministic, no atomics) - THE place that picks the arithmetic of a weight gradient and launches it:
    f16x2 (csrc/gemm_tn_h2.hip) when the caller hands over ``bounds`` = (bound_y, bound_x), 0-dim device tensors that bound max |.| over
    ALL of dy / x - the column scales of the split; the caller checked ``gemm_tn_h2_supported`` (of both products of a pair, with its
    operands swapped or not: see WeightGradSink.step_grads);
    bf16x3 (csrc/gemm_tn_x3.hip) where ``allow_tn`` and that kernel takes the shape;
    else the vendor's fp32 GEMM batched over ``WeightGradSink._chunks`` row chunks (a plain call leaves most CUs idle on a tiny output
    over 10^4..10^6 rows: 400 us for 768 x 320 x 32768).
    slot: ``slot(tag, shape) -> (partials, accumulate)`` names the buffer to launch into and whether to add to what it holds (the
    sink's slots; tag: "tnh2", "tn" or None for the vendor product); default: a fresh buffer."""
    n, Mo, Ko = dy.shape[0], dy.shape[1], x.shape[1]
    if bounds is not None:
        tag = "tnh2"
        S = L.lib().uavgnn_gemm_tn_h2_chunks(n, Mo, Ko) if GEMM_TN_TILES else L.lib().uavgnn_gemm_tn_h2_chunks_tj(n, Mo, Ko, 128)
    elif allow_tn and gemm_tn_x3_supported(dy, x):      # (is_cuda first: the sink's host tests run on CPU tensors, without the library)
        tag, S = "tn", L.lib().uavgnn_gemm_tn_x3_chunks(n, Mo, Ko)
    else:
        tag, S = None, WeightGradSink._chunks(n)
    part, accumulate = slot(tag, (S, Mo, Ko)) if slot is not None else (None, False)
    if part is None and tag is not None:
        part = th.empty((S, Mo, Ko), dtype=th.float32, device=x.device)
    if tag == "tnh2":
        cy, cx = bounds[0].expand(Mo).contiguous(), bounds[1].expand(Ko).contiguous()
        with KERNEL_TIMER.span("gemm_tn_h2", (n, Mo, Ko)):
            args = (dy.data_ptr(), dy.stride(0), Mo, x.data_ptr(), x.stride(0), Ko, n, cy.data_ptr(), cx.data_ptr(), part.data_ptr(), S,
                    int(accumulate))
            rc = (L.lib().uavgnn_gemm_tn_h2(*args, L.stream()) if GEMM_TN_TILES
                  else L.lib().uavgnn_gemm_tn_h2_tj(*args, 128, L.stream()))
        L.check(rc, "uavgnn_gemm_tn_h2")
    elif tag == "tn":
        gemm_tn_x3(dy, x, part, accumulate)
    elif S > 1:         # (a buffer handed in: beta = 0 ignores what it holds)
        xc = x if x.is_contiguous() else x.contiguous()
        a, b = dy.view(S, n // S, -1).transpose(1, 2), xc.view(S, n // S, -1)
        part = th.bmm(a, b) if part is None else part.baddbmm_(a, b, beta=int(accumulate))
    elif part is None:
        part = th.mm(dy.t(), x).unsqueeze(0)
    else:
        part[0].addmm_(dy.t(), x, beta=int(accumulate))
    return part


def _wgrad(dy, x, bounds=None):
    """dy^T x: ``_wgrad_partials`` into a fresh buffer, then the sum over the chunks."""
    part = _wgrad_partials(dy, x, bounds)
    return part[0] if part.shape[0] == 1 else part.sum(0)


class _LinearSplitK(th.autograd.Function):
    """y = x W^T (+ b) on the vendor GEMM (hipBLASLt/rocBLAS fp32), with a weight-gradient path shaped for this
    workload: N_a is 10^4..10^5 rows while W is at most 768 x 512, so dW = dY^T X has a tiny output and a huge
    reduction dimension.  A plain GEMM call leaves most CUs idle there (measured: 400 us for 768x320x32768); the
    reduction is split into S row chunks run as ONE batched GEMM [S, out, in] followed by a fixed-order sum over S
    (deterministic, no atomics)."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        ctx.has_bias = b is not None
        return _mm_nt(x, W, b)

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        return _LinearSplitK._grads(ctx, x, W, dy, ctx.has_bias)

    @staticmethod
    def _grads(ctx, x, W, dy, has_bias, rowmax=None, x_rowmax=None):
        dy = dy.contiguous()
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = _mm_nn(dy, W, rowmax=rowmax)
        if ctx.needs_input_grad[1]:
            # f16x2 where the producers left row maxima: their global maxima bound every column (see WeightGradSink.step_grads)
            h2 = rowmax is not None and x_rowmax is not None and gemm_tn_h2_supported(dy, x)
            dW = _wgrad(dy, x, (_max_two_stage(rowmax), _max_two_stage(x_rowmax)) if h2 else None)
        if has_bias and ctx.needs_input_grad[2]:
            db = _colsum(dy)
        return dx, dW, db


def linear(x, W, b=None):
    return _LinearSplitK.apply(x, W, b)


# ---------------------------------------------------------------------------------------------------------------------
# QMIX mixing tail (csrc/qmix.hip): everything of the mixer behind its hyper-network GEMM in one launch per direction
# ---------------------------------------------------------------------------------------------------------------------
QMIX_MAX_AGENTS, QMIX_MAX_EMBED = 16, 128


class _QmixMix(th.autograd.Function):
    """q_tot [rows] of mixers.py:31-45 from the stacked projection proj [rows, (n+3) e] and qs [rows, n].  The forward saves its inputs
    only; the backward recomputes the hidden layer (one launch) and sums the per-workgroup partials of d V[2] in a fixed order."""

    @staticmethod
    def forward(ctx, proj, qs, v2w, v2b):
        L.require_gpu(proj, qs, v2w, v2b)
        proj, qs, v2w, v2b = L.f32c(proj), L.f32c(qs), L.f32c(v2w), L.f32c(v2b)
        rows, n = qs.shape
        e = v2w.numel()
        q_tot = th.empty(rows, dtype=th.float32, device=proj.device)
        with KERNEL_TIMER.span("qmix_mix_fwd", (rows, n, e)):
            rc = L.lib().uavgnn_qmix_mix_fwd(proj.data_ptr(), proj.stride(0), qs.data_ptr(), v2w.data_ptr(), v2b.data_ptr(), rows, n, e,
                                             q_tot.data_ptr(), L.stream())
        L.check(rc, "uavgnn_qmix_mix_fwd")
        ctx.save_for_backward(proj, qs, v2w)
        ctx.v2w_shape, ctx.v2b_shape = v2w.shape, v2b.shape
        return q_tot

    @staticmethod
    def backward(ctx, d_qtot):
        proj, qs, v2w = ctx.saved_tensors
        lib = L.lib()
        rows, n = qs.shape
        e = v2w.numel()
        d_qtot = L.f32c(d_qtot)
        d_proj, d_qs = th.empty_like(proj), th.empty_like(qs)
        G = lib.uavgnn_qmix_mix_bwd_partials(rows, e)
        part = th.empty((G, e + 1), dtype=th.float32, device=proj.device)
        if rows == 0:
            part.zero_()
        with KERNEL_TIMER.span("qmix_mix_bwd", (rows, n, e)):
            rc = lib.uavgnn_qmix_mix_bwd(proj.data_ptr(), proj.stride(0), qs.data_ptr(), d_qtot.data_ptr(), v2w.data_ptr(), rows, n, e,
                                         d_proj.data_ptr(), d_proj.stride(0), d_qs.data_ptr(), part.data_ptr(), G, L.stream())
        L.check(rc, "uavgnn_qmix_mix_bwd")
        tot = part.sum(0)
        return d_proj, d_qs, tot[:e].reshape(ctx.v2w_shape), tot[e:].reshape(ctx.v2b_shape)


def qmix_mix(proj, qs, v2_weight, v2_bias):
    """proj [rows, (n+3) e], qs [rows, n], v2_weight [e] or [1, e], v2_bias [1] -> q_tot [rows]; CUDA float32,
    n <= QMIX_MAX_AGENTS, e <= QMIX_MAX_EMBED (the caller checks: ``agents.qmix.QMixer.forward``)."""
    return _QmixMix.apply(proj, qs, v2_weight, v2_bias)


# ---------------------------------------------------------------------------------------------------------------------
# TD tail behind the Q head (csrc/td_return.hip): action select, multi-step targets, TD errors, loss and its gradient
# ---------------------------------------------------------------------------------------------------------------------
def normalize_returns(returns):
    """``None`` (the reference's one-step target, learner.py:150), ``("nstep", n)`` with an integer n >= 1 or ``("lambda", lam)`` with
    0 <= lam <= 1 -> None or the pair with n an int / lam a float.  Anything else is a ValueError that names the value."""
    if returns is None:
        return None
    try:
        kind, value = returns
    except (TypeError, ValueError):
        raise ValueError(f"returns: None, ('nstep', n) or ('lambda', lam) expected, got {returns!r}") from None
    if kind == "nstep":
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not 1 <= value <= 2 ** 30 or value != int(value):
            raise ValueError(f"returns=('nstep', n): n must be an integer >= 1, got {value!r}")
        return "nstep", int(value)
    if kind == "lambda":
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 <= float(value) <= 1.0:
            raise ValueError(f"returns=('lambda', lam): lam must be a number in [0, 1], got {value!r}")
        return "lambda", float(value)
    raise ValueError(f"returns: the kind is 'nstep' or 'lambda', got {kind!r} in {returns!r}")


def td_targets_torch(next_vals, rews, dones, gamma, returns):
    """The two multi-step targets in torch ops (what runs on CPU tensors, and the comparison arm of tools/td_return_probe.py).
    next_vals [T, B, C], rews [T, B, C] or [T, B, 1], dones [T, B, 1] -> y [T, B, C]; with c_t = gamma (1 - done_t):
      ('nstep', n):    y_t = sum_{k<m} (prod_{j<k} c_{t+j}) r_{t+k} + (prod_{j<m} c_{t+j}) V_{t+m-1}, m = min(n, T - t), as min(n, T) passes
                       over the whole sequence: y^(1) = r + c V, y^(k)_t = r_t + c_t y^(k-1)_{t+1} (t < T - 1), y^(k)_{T-1} = y^(1)_{T-1};
      ('lambda', lam): G_{T-1} = r_{T-1} + c_{T-1} V_{T-1}, G_t = r_t + c_t ((1 - lam) V_t + lam G_{t+1}), a loop over T."""
    kind, p = normalize_returns(returns)
    T = next_vals.shape[0]
    rews = rews.expand_as(next_vals)
    c = (gamma * (1 - dones)).expand_as(next_vals)
    if kind == "nstep":
        y = rews + c * next_vals
        for _ in range(min(p, T) - 1):
            y = th.cat([rews[:-1] + c[:-1] * y[1:], y[-1:]])
        return y
    G = rews[T - 1] + c[T - 1] * next_vals[T - 1]
    ys = [G]
    for t in range(T - 2, -1, -1):
        G = rews[t] + c[t] * ((1 - p) * next_vals[t] + p * G)
        ys.append(G)
    return th.stack(ys[::-1])


class _TdSelect(th.autograd.Function):
    """learner.py:134-143 in one pass over the two Q tensors; the backward writes all of d_agent_out (no zeros + scatter)."""

    @staticmethod
    def forward(ctx, agent_out, target_out, acts, double_q):
        L.require_gpu(agent_out, target_out, acts)
        agent_out, target_out = L.f32c(agent_out), L.f32c(target_out)
        T1, N, A = agent_out.shape
        T = T1 - 1
        if tuple(target_out.shape) != (T, N, A) or acts.dtype != th.int64 or acts.numel() != T * N:
            raise L.UavGnnError(f"td_select: agent_out {tuple(agent_out.shape)}, target_out {tuple(target_out.shape)}, acts "
                                f"{tuple(acts.shape)} {acts.dtype} do not fit [T+1, N, A] / [T, N, A] / [T, N] int64")
        acts = acts if acts.is_contiguous() else acts.contiguous()
        qvals = th.empty((T, N), dtype=th.float32, device=agent_out.device)
        next_vals, next_acts = th.empty_like(qvals), th.empty((T, N), dtype=th.int32, device=agent_out.device)
        with KERNEL_TIMER.span("td_select_fwd", (T, N, A)):
            rc = L.lib().uavgnn_td_select_fwd(agent_out.data_ptr(), target_out.data_ptr(), acts.data_ptr(), T, N, A, int(bool(double_q)),
                                              qvals.data_ptr(), next_vals.data_ptr(), next_acts.data_ptr(), L.stream())
        L.check(rc, "uavgnn_td_select_fwd")
        ctx.save_for_backward(acts)
        ctx.dims = (T, N, A)
        ctx.mark_non_differentiable(next_vals, next_acts)
        return qvals, next_vals, next_acts

    @staticmethod
    def backward(ctx, d_qvals, _d_next, _d_acts):
        acts, = ctx.saved_tensors
        T, N, A = ctx.dims
        d_qvals = L.f32c(d_qvals)
        d_agent_out = th.empty((T + 1, N, A), dtype=th.float32, device=d_qvals.device)
        with KERNEL_TIMER.span("td_select_bwd", (T, N, A)):
            rc = L.lib().uavgnn_td_select_bwd(d_qvals.data_ptr(), acts.data_ptr(), None, T, N, A, d_agent_out.data_ptr(), L.stream())
        L.check(rc, "uavgnn_td_select_bwd")
        return d_agent_out, None, None, None


def td_select(agent_out, target_out, acts, double_q, return_acts=False):
    """agent_out [T+1, N, A], target_out [T, N, A], acts [T, N] or [T, N, 1] int64 -> (qvals [T, N], next_vals [T, N]): Q(s_t, a_t), and
    the bootstrap value target_out[t] at the double-Q choice argmax_a agent_out[t+1] (``double_q``) or its row maximum.  Only qvals
    carries a gradient.  return_acts: also the chosen next actions [T, N] (int32 on the GPU).  CUDA tensors run csrc/td_return.hip, CPU
    tensors the torch chain of ``learner._td_loss``."""
    if agent_out.is_cuda:
        qvals, next_vals, next_acts = _TdSelect.apply(agent_out, target_out, acts, double_q)
    else:
        T, N = target_out.shape[0], target_out.shape[1]
        qvals = agent_out[:-1].gather(2, acts.reshape(T, N, 1)).view(T, N)
        next_acts = (agent_out[1:] if double_q else target_out).detach().argmax(2, keepdim=True)
        next_vals = target_out.detach().gather(2, next_acts).view(T, N)
        next_acts = next_acts.view(T, N)
    return (qvals, next_vals, next_acts) if return_acts else (qvals, next_vals)


class _TdReturnLoss(th.autograd.Function):
    """Targets, TD errors, loss and g = d loss / d qvals in one call (csrc/td_return.hip); the backward is g * grad_output."""

    @staticmethod
    def forward(ctx, qvals, next_vals, rews, dones, weights, gamma, returns, td, workspace):
        L.require_gpu(qvals, next_vals, rews, dones, weights, td)
        qvals, next_vals, rews, dones = L.f32c(qvals), L.f32c(next_vals), L.f32c(rews), L.f32c(dones)
        T, B, C = qvals.shape
        Cr = rews.shape[-1]
        if tuple(next_vals.shape) != (T, B, C) or tuple(rews.shape) != (T, B, Cr) or dones.numel() != T * B:
            raise L.UavGnnError(f"td_return_loss: qvals {tuple(qvals.shape)}, next_vals {tuple(next_vals.shape)}, rews {tuple(rews.shape)}, "
                                f"dones {tuple(dones.shape)} do not fit [T, B, C] / [T, B, C] / [T, B, 1 or C] / [T, B, 1]")
        if weights is not None:
            weights = L.f32c(weights)
            if weights.numel() != B:
                raise L.UavGnnError(f"td_return_loss: {weights.numel()} weights for {B} sequences")
        dev = qvals.device
        if tuple(td.shape) != (T, B, C) or td.dtype != th.float32 or not td.is_contiguous():
            raise L.UavGnnError(f"td_return_loss: td_out must be a contiguous float32 [{T}, {B}, {C}], got {tuple(td.shape)} {td.dtype}")
        lib = L.lib()
        G = lib.uavgnn_td_return_partials(B, C)
        if G < 1:
            L.check(G, "uavgnn_td_return_partials")
        if workspace is None:
            partials = th.empty(G, dtype=th.float32, device=dev)
        else:       # the caller's store (the learner's): one buffer per shape, handed to every call
            partials = workspace.get((G, dev))
            if partials is None:
                partials = workspace[(G, dev)] = th.empty(G, dtype=th.float32, device=dev)
        g = th.empty((T, B, C), dtype=th.float32, device=dev)
        loss = th.empty((), dtype=th.float32, device=dev)
        kind, p = returns
        mode, n_step, lam = (L.UAVGNN_TD_NSTEP, p, 0.0) if kind == "nstep" else (L.UAVGNN_TD_LAMBDA, 0, p)
        with KERNEL_TIMER.span("td_return_fwd", (T, B, C)):
            rc = lib.uavgnn_td_return_fwd(qvals.data_ptr(), next_vals.data_ptr(), rews.data_ptr(), Cr, dones.data_ptr(), L.ptr(weights), T, B,
                                          C, float(gamma), mode, n_step, lam, td.data_ptr(), g.data_ptr(), loss.data_ptr(),
                                          partials.data_ptr(), G, L.stream())
        L.check(rc, "uavgnn_td_return_fwd")
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        g, = ctx.saved_tensors
        return g * d_loss, None, None, None, None, None, None, None, None


def td_return_loss(qvals, next_vals, rews, dones, weights, gamma, returns, td_out=None, workspace=None):
    """(loss, td) of the multi-step TD target ``returns`` = ('nstep', n) / ('lambda', lam) (definitions: ``td_targets_torch``, DESIGN):
    qvals, next_vals [T, B, C]; rews [T, B, C] or [T, B, 1]; dones [T, B, 1]; weights [B] or None (= 1).  td [T, B, C] = qvals - y (no
    gradient; written straight into ``td_out`` when one is given - the fixed-address buffer of a captured update), loss =
    sum_b w_b td^2 / (T B C) with gradient (2 w_b / (T B C)) td towards qvals only: the targets carry none.  ('nstep', 1) and
    ('lambda', 0) give the TD errors of the one-step target bit for bit on finite inputs.  workspace: a dict that keeps the per-workgroup
    partial sums of the loss between calls (None: a fresh buffer per call).  The only cut of a sequence is its stored ``done``; a
    hand-built ring whose sequences straddle an environment reset without one is the caller's business.  CUDA tensors run
    csrc/td_return.hip; CPU tensors run ``td_targets_torch``."""
    returns = normalize_returns(returns)
    if returns is None:
        raise ValueError("td_return_loss: returns is ('nstep', n) or ('lambda', lam); the one-step default is learner._td_loss's own chain")
    if qvals.is_cuda:
        # td is a plain buffer the kernel fills (the caller's fixed-address one, or a fresh one): it never enters the autograd graph
        td = td_out if td_out is not None else th.empty(tuple(qvals.shape), dtype=th.float32, device=qvals.device)
        return _TdReturnLoss.apply(qvals, next_vals, rews, dones, weights, gamma, returns, td, workspace), td
    d = qvals - td_targets_torch(next_vals.detach(), rews, dones, gamma, returns)
    x = d.square() if weights is None else d.square() * weights.view(1, -1, 1)
    td = d.detach()
    if td_out is not None:
        td = td_out.copy_(td)
    return x.sum() / max(d.numel(), 1), td


# ---------------------------------------------------------------------------------------------------------------------
# Distributional Q, quantile-regression form (include/uavgnn_qr.h, csrc/qr/quantile.hip; DESIGN "Distributional Q")
# ---------------------------------------------------------------------------------------------------------------------
QR_K = (8, 16, 32, 64)     # the quantile counts of uavgnn_qr_supported (1 <= A <= 64)


def _qr_device(*tensors) -> bool:
    """The kernels take CUDA float32; CPU and float64 tensors take the torch arms."""
    return all(t.is_cuda and t.dtype == th.float32 for t in tensors)


def quantile_mean_fold_torch(weight, bias, A, K):
    H = weight.shape[1]
    return weight.view(A, K, H).sum(1) * (1.0 / K), bias.view(A, K).sum(1) * (1.0 / K)


def quantile_mean_fold(weight, bias, A, K):
    """(W_bar [A, H], b_bar [A]) of a quantile head's weight [A*K, H] / bias [A*K]: the mean over the K quantiles of every action, so
    that q = h W_bar^T + b_bar is the mean of theta = h W^T + b.  ONE launch on the GPU, no autograd (``QuantileLinear`` uses it where
    no gradient is asked for); CPU / float64 tensors, or a call under grad, take ``quantile_mean_fold_torch``."""
    if tuple(weight.shape[:1]) != (A * K,) or tuple(bias.shape) != (A * K,):
        raise L.UavGnnError(f"quantile_mean_fold: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} do not fit [A*K = {A * K}, H] / [A*K]")
    needs_grad = th.is_grad_enabled() and (weight.requires_grad or bias.requires_grad)
    if needs_grad or not _qr_device(weight, bias):
        return quantile_mean_fold_torch(weight, bias, A, K)
    H = weight.shape[1]
    weight = weight.detach()
    weight = weight if weight.stride(1) == 1 else weight.contiguous()
    bias = bias.detach().contiguous()
    W_bar = th.empty((A, H), dtype=th.float32, device=weight.device)
    b_bar = th.empty((A,), dtype=th.float32, device=weight.device)
    with KERNEL_TIMER.span("qr_mean_fold", (A, K, H)):
        rc = L.qr().uavgnn_qr_mean_fold(weight.data_ptr(), weight.stride(0), bias.data_ptr(), A, K, H, W_bar.data_ptr(), b_bar.data_ptr(),
                                        L.stream())
    L.check(rc, "uavgnn_qr_mean_fold")
    return W_bar, b_bar


def qr_select_torch(theta_pol, theta_tgt, acts, double_q):
    """The select of the quantile TD tail in torch ops (differentiable towards theta_pol through theta_a only):
    theta_pol [T+1, N, A, K], theta_tgt [T, N, A, K], acts [T, N] (or [T, N, 1]) int64 ->
    (theta_a [T, N, K], theta_next [T, N, K], next_acts [T, N] int64, q_pol [T+1, N, A])."""
    T, N, A, K = theta_tgt.shape
    idx = acts.reshape(T, N, 1, 1).expand(T, N, 1, K)
    theta_a = theta_pol[:-1].gather(2, idx).view(T, N, K)
    q_pol = theta_pol.detach().sum(-1) * (1.0 / K)
    pick = theta_pol[1:].detach().sum(-1) if double_q else theta_tgt.detach().sum(-1)
    next_acts = pick.argmax(2)
    theta_next = theta_tgt.detach().gather(2, next_acts.view(T, N, 1, 1).expand(T, N, 1, K)).view(T, N, K)
    return theta_a, theta_next, next_acts, q_pol


class _QrSelect(th.autograd.Function):
    """The select on quantile rows in one pass (csrc/qr/quantile.hip); the backward writes all of d_theta_pol."""

    @staticmethod
    def forward(ctx, theta_pol, theta_tgt, acts, double_q):
        L.require_gpu(theta_pol, theta_tgt, acts)
        theta_pol, theta_tgt = L.f32c(theta_pol), L.f32c(theta_tgt)
        T1, N, A, K = theta_pol.shape
        T = T1 - 1
        if tuple(theta_tgt.shape) != (T, N, A, K) or acts.dtype != th.int64 or acts.numel() != T * N:
            raise L.UavGnnError(f"qr_select: theta_pol {tuple(theta_pol.shape)}, theta_tgt {tuple(theta_tgt.shape)}, acts "
                                f"{tuple(acts.shape)} {acts.dtype} do not fit [T+1, N, A, K] / [T, N, A, K] / [T, N] int64")
        acts = acts if acts.is_contiguous() else acts.contiguous()
        dev = theta_pol.device
        theta_a = th.empty((T, N, K), dtype=th.float32, device=dev)
        theta_next = th.empty_like(theta_a)
        next_acts = th.empty((T, N), dtype=th.int32, device=dev)
        q_pol = th.empty((T1, N, A), dtype=th.float32, device=dev)
        with KERNEL_TIMER.span("qr_select_fwd", (T, N, A, K)):
            rc = L.qr().uavgnn_qr_select_fwd(theta_pol.data_ptr(), theta_tgt.data_ptr(), acts.data_ptr(), T, N, A, K, int(bool(double_q)),
                                             theta_a.data_ptr(), theta_next.data_ptr(), next_acts.data_ptr(), q_pol.data_ptr(), L.stream())
        L.check(rc, "uavgnn_qr_select_fwd")
        ctx.save_for_backward(acts)
        ctx.dims = (T, N, A, K)
        ctx.mark_non_differentiable(theta_next, next_acts, q_pol)
        return theta_a, theta_next, next_acts, q_pol

    @staticmethod
    def backward(ctx, d_theta_a, _d_next, _d_acts, _d_q):
        acts, = ctx.saved_tensors
        T, N, A, K = ctx.dims
        d_theta_a = L.f32c(d_theta_a)
        d_theta_pol = th.empty((T + 1, N, A, K), dtype=th.float32, device=d_theta_a.device)
        with KERNEL_TIMER.span("qr_select_bwd", (T, N, A, K)):
            rc = L.qr().uavgnn_qr_select_bwd(d_theta_a.data_ptr(), acts.data_ptr(), T, N, A, K, d_theta_pol.data_ptr(), L.stream())
        L.check(rc, "uavgnn_qr_select_bwd")
        return d_theta_pol, None, None, None


def qr_select(theta_pol, theta_tgt, acts, double_q):
    """theta_pol [T+1, N, A, K], theta_tgt [T, N, A, K], acts [T, N] or [T, N, 1] int64 -> (theta_a [T, N, K], theta_next [T, N, K],
    next_acts [T, N], q_pol [T+1, N, A]): the quantiles of Q(s_t, a_t), those of the target network at the action whose quantile MEAN is
    largest - on theta_pol[t+1] (``double_q``) or on theta_tgt[t] itself -, that action (int32 on the GPU) and the policy's per-action
    means.  Only theta_a carries a gradient.  CUDA float32 tensors run csrc/qr/quantile.hip, all others ``qr_select_torch``."""
    if _qr_device(theta_pol, theta_tgt):
        return _QrSelect.apply(theta_pol, theta_tgt, acts, double_q)
    return qr_select_torch(theta_pol, theta_tgt, acts, double_q)


def qr_loss_torch(theta_a, theta_next, rews, dones, weights, gamma, n_step=1, kappa=1.0):
    """(loss, td) of the quantile-Huber loss (QR-DQN eq. 10; include/uavgnn_qr.h) in torch ops, differentiable towards theta_a:
    theta_a, theta_next [T, B, C, K]; rews [T, B, C] or [T, B, 1]; dones [T, B, 1]; weights [B] or None.  The n-step targets are
    ``td_targets_torch`` per quantile; they carry no gradient.  Materialises [T, B, C, K, K]."""
    T, B, C, K = theta_a.shape
    y = td_targets_torch(theta_next.detach(), rews.reshape(T, B, -1, 1), dones.reshape(T, B, 1, 1), gamma, ("nstep", int(n_step)))
    tau = (2 * th.arange(K, device=theta_a.device, dtype=theta_a.dtype) + 1) / (2 * K)
    u = y.unsqueeze(-2) - theta_a.unsqueeze(-1)                       # [T, B, C, i, j]
    au = u.abs()
    huber = th.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa))
    wt = (tau.view(K, 1) - (u.detach() < 0).to(u.dtype)).abs()
    rows = (wt * huber).sum(-1).sum(-1) * (1.0 / K) / kappa          # [T, B, C]
    if weights is not None:
        rows = rows * weights.view(1, B, 1)
    td = (theta_a.detach().mean(-1) - y.mean(-1))
    return rows.sum() / (T * B * C), td


class _QrLoss(th.autograd.Function):
    """Targets, the K x K pairs, loss, td and g = d loss / d theta_a in one call (csrc/qr/quantile.hip); the backward is g * grad_output."""

    @staticmethod
    def forward(ctx, theta_a, theta_next, rews, dones, weights, gamma, n_step, kappa, td, workspace):
        L.require_gpu(theta_a, theta_next, rews, dones, weights, td)
        theta_a, theta_next, rews, dones = L.f32c(theta_a), L.f32c(theta_next), L.f32c(rews), L.f32c(dones)
        T, B, C, K = theta_a.shape
        Cr = rews.shape[-1]
        if tuple(theta_next.shape) != (T, B, C, K) or tuple(rews.shape) != (T, B, Cr) or dones.numel() != T * B:
            raise L.UavGnnError(f"qr_loss: theta_a {tuple(theta_a.shape)}, theta_next {tuple(theta_next.shape)}, rews {tuple(rews.shape)}, "
                                f"dones {tuple(dones.shape)} do not fit [T, B, C, K] / [T, B, C, K] / [T, B, 1 or C] / [T, B, 1]")
        if weights is not None:
            weights = L.f32c(weights)
            if weights.numel() != B:
                raise L.UavGnnError(f"qr_loss: {weights.numel()} weights for {B} sequences")
        dev = theta_a.device
        if tuple(td.shape) != (T, B, C) or td.dtype != th.float32 or not td.is_contiguous():
            raise L.UavGnnError(f"qr_loss: td_out must be a contiguous float32 [{T}, {B}, {C}], got {tuple(td.shape)} {td.dtype}")
        lib = L.qr()
        G = lib.uavgnn_qr_loss_partials(T, B, C, K)
        if G < 1:
            L.check(G, "uavgnn_qr_loss_partials")
        if workspace is None:
            partials = th.empty(G, dtype=th.float32, device=dev)
        else:       # the caller's store (the learner's): one buffer per shape, handed to every call
            partials = workspace.get(("qr", G, dev))
            if partials is None:
                partials = workspace[("qr", G, dev)] = th.empty(G, dtype=th.float32, device=dev)
        g = th.empty((T, B, C, K), dtype=th.float32, device=dev)
        loss = th.empty((), dtype=th.float32, device=dev)
        with KERNEL_TIMER.span("qr_loss_fwd", (T, B, C, K)):
            rc = lib.uavgnn_qr_loss_fwd(theta_a.data_ptr(), theta_next.data_ptr(), rews.data_ptr(), Cr, dones.data_ptr(), L.ptr(weights), T, B,
                                        C, K, float(gamma), int(n_step), float(kappa), td.data_ptr(), g.data_ptr(), loss.data_ptr(),
                                        partials.data_ptr(), G, L.stream())
        L.check(rc, "uavgnn_qr_loss_fwd")
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        g, = ctx.saved_tensors
        return g * d_loss, None, None, None, None, None, None, None, None, None


def qr_loss(theta_a, theta_next, rews, dones, weights, gamma, n_step=1, kappa=1.0, td_out=None, workspace=None):
    """(loss, td) of the quantile-regression TD loss: theta_a, theta_next [T, B, C, K] (``qr_select``'s, viewed per environment); rews
    [T, B, C] or [T, B, 1]; dones [T, B, 1]; weights [B] or None (= 1); n-step targets per quantile (n_step = 1: the one-step target).
    loss = sum_b w_b l / (T B C) with l the quantile-Huber row loss at threshold kappa; its gradient reaches theta_a only.  td [T, B, C] =
    mean_i theta_i - mean_j y_j (no gradient; written straight into ``td_out`` when one is given).  workspace: a dict that keeps the
    per-workgroup partial sums between calls.  CUDA float32 tensors run csrc/qr/quantile.hip, all others ``qr_loss_torch``."""
    if isinstance(n_step, bool) or int(n_step) != n_step or n_step < 1:
        raise ValueError(f"qr_loss: n_step must be an integer >= 1, got {n_step!r}")
    if not kappa > 0:
        raise ValueError(f"qr_loss: kappa must be positive, got {kappa!r}")
    if _qr_device(theta_a, theta_next):
        td = td_out if td_out is not None else th.empty(tuple(theta_a.shape[:3]), dtype=th.float32, device=theta_a.device)
        return _QrLoss.apply(theta_a, theta_next, rews, dones, weights, gamma, int(n_step), float(kappa), td, workspace), td
    loss, td = qr_loss_torch(theta_a, theta_next, rews, dones, weights, gamma, n_step, kappa)
    if td_out is not None:
        td = td_out.copy_(td)
    return loss, td


RELU_BWD_FUSED =os.environ.get("UAVGNN_RELU_BWD_FUSED", "1") != "0"   # ReLU mask + bias gradient in one pass (A/B switch)


class _LinearReLU(th.autograd.Function):
    """relu(x W^T + b) with the bias + ReLU applied in the GEMM epilogue (hipBLASLt, via ``torch._addmm_activation``):
    the separate elementwise pass over [N_a, H] (and over [(T+1) N_a, H] in the time-batched encoder) disappears from
    the forward.  Backward masks dy with (y > 0) and reuses the split-K weight-gradient path."""

    @staticmethod
    def forward(ctx, x, W, b, rm_a=None, rm_b=None, train=True):
        ctx.x_rowmax = None
        ctx.n_extra = 0 if rm_a is None else 3
        n_out = W.shape[0]
        rm = None if rm_a is None else (rm_a, rm_b)
        if (rm is not None and b is not None and b.is_contiguous() and W.stride(1) == 1 and gemm_h2_supported(x, n_out, W.shape[1])):
            # the producer (the time-batched K1 launch) left the maxima of the two halves of every row: the layer on the f16x2 kernel
            y = gemm_h2(x, W, rm[0], False, bias=b, relu=True, rowmax2=rm[1])
            if ctx.needs_input_grad[1] and train:      # (needs_input_grad stays True for parameters under no_grad - `train` is the grad mode
                ctx.x_rowmax = th.maximum(rm[0], rm[1])    # at the call site: a rollout step does not pay for the weight gradient's bound)
            ctx.save_for_backward(x, W, y)
            return y
        if (ctx.needs_input_grad[1] and n_out % 4 == 0 and gemm_x3_supported(x, n_out, W.shape[1]) and W.stride(1) == 1 and b is not None
                and b.is_contiguous() and _gemm_tn_h2_shape(x.shape[0], n_out, x.shape[1])):
            # time-batched training forward: the layer's weight gradient will run on the f16x2 kernel - the bound of its X operand (this
            # x) is a by-product of this GEMM's staging
            ctx.x_rowmax = th.empty(x.shape[0], dtype=th.float32, device=x.device)
            y = gemm_x3(x, W, False, bias=b, relu=True, rowmax_out=ctx.x_rowmax)
        else:
            y = _mm_nt(x, W, b, relu=True)
        ctx.save_for_backward(x, W, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W, y = ctx.saved_tensors
        n, C = dy.shape
        if (RELU_BWD_FUSED and ctx.needs_input_grad[2] and dy.is_cuda and dy.dtype == th.float32 and y.dtype == th.float32 and n > 0
                and C % 4 == 0 and _mc_operand(dy) and _mc_operand(y)
                and dy.stride(0) >= C and y.stride(0) >= C):      # a row-broadcast gradient (stride 0) takes the torch path below
            # the mask and the bias gradient in ONE pass over the gradient (csrc/colsum.hip): autograd's threshold_backward + sum
            # are two (5.1 + 1.7 GB per C3 update on the time-batched encoder)
            S = _row_blocks(n)
            dym = th.empty((n, C), dtype=th.float32, device=dy.device)
            part = th.zeros((S, C), dtype=th.float32, device=dy.device)
            rowmax = None
            if C == 256 and ctx.needs_input_grad[0] and gemm_h2_supported(dym, W.shape[1], C) and W.stride(1) == 1:
                # the masked gradient's row maxima on the way: d x = dym W runs on the f16x2 kernel (csrc/gemm_h2.hip)
                rowmax = th.empty(n, dtype=th.float32, device=dy.device)
                L.check(L.lib().uavgnn_relu_bwd_colsum_rowmax(dy.data_ptr(), dy.stride(0), y.data_ptr(), y.stride(0), dym.data_ptr(), C, n,
                                                              C, part.data_ptr(), S, rowmax.data_ptr(), L.stream()),
                        "uavgnn_relu_bwd_colsum_rowmax")
            else:
                L.check(L.lib().uavgnn_relu_bwd_colsum(dy.data_ptr(), dy.stride(0), y.data_ptr(), y.stride(0), dym.data_ptr(), C, n, C,
                                                       part.data_ptr(), S, L.stream()), "uavgnn_relu_bwd_colsum")
            dx, dW, _ = _LinearSplitK._grads(ctx, x, W, dym, False, rowmax=rowmax, x_rowmax=ctx.x_rowmax)
            return (dx, dW, part.sum(0)) + (None,) * ctx.n_extra
        dy = th.ops.aten.threshold_backward(dy, y, 0.0)     # dy where y > 0 else 0, one pass (compare + where were two)
        return tuple(_LinearSplitK._grads(ctx, x, W, dy, True)) + (None,) * ctx.n_extra


def linear_relu(x, W, b):
    rm = getattr(x, "_uavgnn_rowmax", None)      # left by hetero_gatv2 on a time-batched launch
    if rm is not None and rm[2] == _version_of(x):   # (only while x is unchanged: a stale bound overflows f16 or drops bits)
        return _LinearReLU.apply(x, W, b, rm[0], rm[1], th.is_grad_enabled())
    return _LinearReLU.apply(x, W, b)


# ---------------------------------------------------------------------------------------------------------------------
# First encoder layer of the flattened-observation agents, read straight from the padded observations (csrc/flat_obs.hip)
# "1": the fused kernels wherever the shape is supported; "0": th.cat of the pieces + linear_relu; "auto" (default): the path that
# measured faster (profiles/flat_obs_probe.txt, tools/flat_obs_probe.py) - the fused forward for no-grad calls (the rollout) of at most
# FLAT_OBS_AUTO_MAX_ROWS rows and F <= FLAT_OBS_AUTO_MAX_F (16 384 rows, F = 31: 0.035 vs 0.042 ms), th.cat + linear_relu for everything
# else (the time-batched training layer and 8 x 80: the FMA kernels run at 2-7x the vendor GEMM's time there)
FLAT_OBS_FUSED = os.environ.get("UAVGNN_FLAT_OBS_FUSED", "auto")
FLAT_OBS_AUTO_MAX_ROWS = 1 << 15
FLAT_OBS_AUTO_MAX_F = 64


def flat_obs_supported(parts, W, needs_grad=False) -> bool:
    """parts: the (agent, gt, ubs) row views [rows, .] of a flattened-observation batch (graph.FlatObsBatch.parts).  Every piece needs
    unit column stride and rows that do not overlap (an expanded or overlapping view takes the th.cat path).  needs_grad: the call
    will be differentiated (the "auto" mode keeps those on th.cat + linear_relu)."""
    F = sum(p.shape[1] for p in parts)
    rows = parts[0].shape[0]
    mode = str(FLAT_OBS_FUSED)
    if mode == "0" or (mode != "1" and (needs_grad or rows > FLAT_OBS_AUTO_MAX_ROWS or F > FLAT_OBS_AUTO_MAX_F)):
        return False
    return bool(W.is_cuda and W.dtype == th.float32 and W.is_contiguous() and W.shape[1] == F
                and all(p.is_cuda and p.dtype == th.float32 and p.dim() == 2 and p.shape[0] == rows
                        and (p.stride(1) == 1 or p.shape[1] <= 1) and (rows <= 1 or p.stride(0) >= p.shape[1]) for p in parts)
                and rows < 2 ** 31 and L.lib().uavgnn_flat_obs_supported(W.shape[0], F))


def _flat_src(parts):
    """(ptr, row stride, width) per piece, as the C ABI takes them (an empty piece passes NULL)."""
    out = []
    for p in parts:
        out += [p.data_ptr() if p.shape[1] else None, p.stride(0) if p.shape[0] > 1 else p.shape[1], p.shape[1]]
    return out


class _FlatLinearReLU(th.autograd.Function):
    """relu(flat(obs) W^T + b) where flat(obs) = [agent || gt || ubs] (graph.FLAT_OBS_ORDER) is never materialised: the forward
    and the weight gradient read the three padded pieces through their row strides.  The observations carry no gradient; the
    ReLU mask and the bias gradient come from the fused pass of csrc/colsum.hip, the weight gradient from row-chunk partials
    [S, H_out, F] summed in a fixed order (deterministic)."""

    @staticmethod
    def forward(ctx, W, b, agent, gt, ubs):
        parts = (agent, gt, ubs)
        rows, H = agent.shape[0], W.shape[0]
        y = th.empty((rows, H), dtype=th.float32, device=W.device)
        with KERNEL_TIMER.span("flat_obs_fwd", (rows, H, W.shape[1])):
            rc = L.lib().uavgnn_flat_obs_fwd(*_flat_src(parts), rows, W.data_ptr(), L.ptr(b), H, y.data_ptr(), y.stride(0), L.stream())
        L.check(rc, "uavgnn_flat_obs_fwd")
        ctx.has_bias = b is not None
        ctx.save_for_backward(y, agent, gt, ubs)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, agent, gt, ubs = ctx.saved_tensors
        parts = (agent, gt, ubs)
        n, H = dy.shape
        F = sum(p.shape[1] for p in parts)
        lib = L.lib()
        if dy.stride(1) != 1 or dy.stride(0) < H or dy.stride(0) % 4 or dy.data_ptr() % 16:
            dy = dy.contiguous()
        S = _row_blocks(n)
        dym = th.empty((n, H), dtype=th.float32, device=dy.device)
        db_part = th.zeros((S, H), dtype=th.float32, device=dy.device)
        L.check(lib.uavgnn_relu_bwd_colsum(dy.data_ptr(), dy.stride(0), y.data_ptr(), y.stride(0), dym.data_ptr(), H, n, H,
                                           db_part.data_ptr(), S, L.stream()), "uavgnn_relu_bwd_colsum")
        dW = None
        if ctx.needs_input_grad[0]:
            Sw = lib.uavgnn_flat_obs_wgrad_chunks(n, H, F)
            part = th.empty((Sw, H, F), dtype=th.float32, device=dy.device)
            with KERNEL_TIMER.span("flat_obs_wgrad", (n, H, F)):
                rc = lib.uavgnn_flat_obs_wgrad(dym.data_ptr(), dym.stride(0), H, *_flat_src(parts), n, part.data_ptr(), Sw, 0, L.stream())
            L.check(rc, "uavgnn_flat_obs_wgrad")
            dW = part.sum(0)
        db = db_part.sum(0) if ctx.has_bias and ctx.needs_input_grad[1] else None
        return dW, db, None, None, None


def flat_linear_relu(parts, W, b):
    """ReLU(Linear(W, b)) of the flattened observations whose pieces are ``parts`` (agent, gt, ubs row views): the fused kernel
    where ``flat_obs_supported`` (FLAT_OBS_FUSED), else ``th.cat`` of the pieces + ``linear_relu``."""
    needs_grad = th.is_grad_enabled() and (W.requires_grad or (b is not None and b.requires_grad))
    if flat_obs_supported(parts, W, needs_grad):
        return _FlatLinearReLU.apply(W, b, *parts)
    return linear_relu(th.cat(parts, 1), W, b)


# ---------------------------------------------------------------------------------------------------------------------
# Fused recurrent step of the TarMAC agent: ONE autograd node per time step.

class WeightGradSink:
    """In-place accumulator for the weight / bias gradients of the recurrent step across the T+1 steps of a BPTT
    backward.  Every step adds its contribution INSIDE the weight-gradient GEMM (beta = 1, row chunks batched as in
    ``_LinearSplitK``), so the per-step ``sum`` over chunks, the per-step bias reduction result and autograd's
    per-parameter ``AccumulateGrad`` adds (12 parameters x 51 steps small kernels) disappear; ``flush()`` folds the
    accumulators into ``param.grad`` once, in a fixed order (deterministic)."""

    def __init__(self):
        self.seq = None      # time-batched staging of the sequence in flight (begin_sequence)
        self._seq_bufs = None
        self.slots = {}      # (key, chunk count) -> (buffer, flush_fn)
        # d h buffer the fused step's backward handed to autograd LAST (private), keyed by its address.  The entry holds a
        # strong reference: while it is alive the allocator cannot hand that address to another tensor, so an incoming
        # gradient with this data_ptr IS this storage (a bare set of addresses could match a recycled block).  At most
        # one entry: whatever the very next step does not consume is dropped.
        self.owned = {}

    @staticmethod
    def _chunks(n):
        """row chunks of >= 2048: S = 16 at N_a = 32768 (measured best or within 10 % on every layer shape)"""
        S = 1
        while S < 64 and n % (2 * S) == 0 and n // (2 * S) >= 2048:
            S *= 2
        return S

    def weight(self, key, dy, x, flush_fn, allow_tn=True, bounds=None):
        """buffer[S, out, in] += chunked dy^T x (``_wgrad_partials``; bounds: the f16x2 kernel - the caller checked
        gemm_tn_h2_supported).  One slot per arithmetic and chunk count: a change of N mid-accumulation never drops a partial sum."""
        def slot(tag, shape):
            k = (key, shape[0]) if tag is None else (key, tag, shape[0])
            have = self.slots.get(k)
            if have is not None:
                return have[0], True
            # the vendor product and the bf16x3 kernel add to zeros; the f16x2 kernel's first launch writes an uninitialised buffer
            first = tag == "tnh2"
            self.slots[k] = ((th.empty if first else th.zeros)(shape, dtype=th.float32, device=x.device), flush_fn)
            return self.slots[k][0], not first
        _wgrad_partials(dy, x, bounds, allow_tn, slot)

    def weight_h2(self, key, dy, x, bound_y, bound_x, flush_fn):
        """``weight`` on the f16x2 kernel, as the probes call it (tools/h2_pmc_run.py)."""
        self.weight(key, dy, x, flush_fn, bounds=(bound_y, bound_x))

    def bias(self, key, dy, flush_fn):
        """buffer[S, out] += row-blocked column sums of dy: one streaming HIP pass per matrix (csrc/colsum.hip), in
        place (torch: a reduction into a temporary plus an add per step; a transposed GEMV was 20x slower still)"""
        n, C = dy.shape
        S = _row_blocks(n)
        key = (key, S)
        slot = self.slots.get(key)
        if slot is None:
            self.slots[key] = slot = (th.zeros((S, C), dtype=th.float32, device=dy.device), flush_fn)
        if dy.dtype != th.float32 or dy.stride(1) != 1:
            dy = dy.float().contiguous()
        L.check(L.lib().uavgnn_colsum_acc(dy.data_ptr(), dy.stride(0), n, C, slot[0].data_ptr(), S, L.stream()),
                "uavgnn_colsum_acc")

    # ---- time-batched staging of ONE BPTT sequence -------------------------------------------------------------------
    # None of the weight / bias gradient reductions of the recurrent step depends on the recurrence: they are sums over
    # (time step, agent).  Inside begin_sequence() ... end_sequence() the fused step therefore does not reduce anything per
    # step: its forward writes [x || c] and h' into slots of [T1, N, .] buffers, its backward writes d_gi, d_gh, d_proj (and
    # copies dq) into slots of the same shape - the kernels that produce them write there directly, no extra traffic - and
    # end_sequence() issues ONE dy^T x per weight over T1 * N rows (1.67 M at C3: the shape class where csrc/gemm_tn_x3.hip
    # beats the vendor's split-K GEMM) and ONE column sum per bias: 5 + 4 launches per sequence instead of (5 + 4) * T1
    # (autograd of gnn_agents.py:243-246,:56 under learner.py:157).
    def begin_sequence(self, T1, N, x_all):
        """x_all: the time-major [T1 * N, H] input of the T1 recurrent steps (the time-batched encoder's output)."""
        self.seq = _SequenceStage(T1, N, x_all.detach(), self._seq_bufs)
        self._seq_bufs = self.seq.bufs          # the buffers are reused by the next sequence (chunks of one accumulate)

    def end_sequence(self):
        seq, self.seq = self.seq, None
        if seq is None or not seq.bwd_steps:
            return
        T1, N, H = seq.T1, seq.N, seq.H
        full = sorted(seq.bwd_steps) == list(range(T1)) and seq.t_fwd == T1
        if full and len({seq.steps[t].packed for t in range(T1)}) > 1:
            full = False         # packed and plain gate-gradient slots in one sequence (never from one caller): reduce per step
        spans = [(0, T1)] if full else [(t, t + 1) for t in sorted(seq.bwd_steps)]
        for (t0, t1) in spans:
            rows = lambda name, lo=0: seq.bufs[name][t0 + lo:t1 + lo].reshape((t1 - t0) * N, -1)   # noqa: E731
            recs = [seq.steps[t] for t in range(t0, t1)]
            packed = recs[0].packed
            if packed:      # G = [dn_h | dr | dz | dn_i]: d_gi is a view; d_gh comes with its column blocks in the order n, r, z
                d_gi, d_gh = rows("g4")[:, H:], rows("g4")[:, :3 * H]
            else:
                d_gi, d_gh = rows("d_gi"), rows("d_gh")
            bounds = gsum = None
            if full and all(r.rowmax and r.rm_g for r in recs):
                # the row maxima the message kernel (max over [x || c || h] per agent), the gate kernel (d_gi / d_gh) and the d x product
                # (d_proj) left for the f16x2 cell / input-gradient products of every step
                bounds = (seq.bufs["rowmax"][:T1], seq.bufs["rm_g"][:T1], seq.bufs["rm_p"][:T1] if all(r.rm_p for r in recs) else None)
            if all(r.gsum for r in recs):
                # the gate kernels of these steps left per-workgroup column sums d_r | d_z | d_n (input) | d_n (hidden): [., 4H]
                gsum = seq.bufs["gsum"][t0:t1]
                gsum = gsum.reshape(gsum.shape[0] * gsum.shape[1], 4 * H)
            # allow_tn=False: the vendor's batched split-K fp32 GEMM (64 row chunks): at these shapes - 768-, 96- and 9-row outputs over
            # 1.67 M rows - it runs at 135-141 TFLOP/s against 85-107 for csrc/gemm_tn_x3.hip (tools/gemm_tn_big_probe.py),
            # and 25-30 % above its own per-step rate (32 768 rows per call)
            self.step_grads(seq.split, seq.ids, H, seq.x_all[t0 * N:t1 * N], rows("h"), rows("h", 1), rows("inp"), rows("d_proj"), d_gi, d_gh,
                            seq.dq_rows(t0, t1), packed=packed, gsum=gsum, bounds=bounds, allow_tn=False)

    def step_grads(self, split, ids, H, x, h, h2, inp, d_proj, d_gi, d_gh, dq, packed=False, gsum=None, bounds=None, allow_tn=True):
        """The nine parameter gradients of the recurrent step - Wp (its x and h halves), bp, W_ih, b_ih, W_hh, b_hh (n block), W_out,
        b_out - over the rows handed in: the tensors of ONE step, or slot views over a span of steps of a staged sequence.
        split: the step's flush target; ids: {"Wp", "W_ih", "W_hh", "W_out"} -> identity of the parameter (the slot keys).
        packed: d_gi / d_gh are views of G = [dn_h | dr | dz | dn_i] - d_gh has its column blocks in the order n, r, z.
        gsum [., 4H]: the gate kernels' column-sum partials d_r | d_z | d_n (input) | d_n (hidden), instead of passes over d_gi / d_gh.
        bounds = (row maxima of [x || c || h], of d_gi / d_gh, of d_proj or None) of every row handed in: the weight gradients on the
        f16x2 kernel (csrc/gemm_tn_h2.hip) where it covers the shape."""
        if packed:
            # dW_hh is accumulated with its row blocks in the order n, r, z (a slot of its own) and put back in order once, at flush
            whh_key, whh_flush = "W_hh_nrz", lambda g: split("W_hh", th.cat((g[H:], g[:H]), 0), 0)
        else:
            whh_key, whh_flush = "W_hh", lambda g: split("W_hh", g, 0)
        rm_x, rm_g, rm_p = bounds if bounds is not None else (None, None, None)
        if rm_p is not None and gemm_tn_h2_supported(x, d_proj, 96) and gemm_tn_h2_supported(h, d_proj, 96):
            # dWp on the f16x2 kernel with the operands swapped - x^T d_proj = (dWp_x)^T, [H x 96]: one 256 x 128 tile three quarters full
            # (d_proj^T x would fill three eighths of two: slower than the vendor) - 0.93 -> 0.5 ms each against the vendor's 0.74;
            # column bounds: the message kernel's row maxima bound x and h, the per-step row maxima of d_proj (taken for the d x
            # product of the step) bound d_proj
            b_wp = (_max_two_stage(rm_x), _max_two_stage(rm_p))
            self.weight(("Wp_x", ids["Wp"]), x, d_proj, lambda g: split("Wp", g.t(), 0), bounds=b_wp)
            self.weight(("Wp_h", ids["Wp"]), h, d_proj, lambda g: split("Wp", g.t(), H), bounds=b_wp)
        else:
            self.weight(("Wp_x", ids["Wp"]), d_proj, x, lambda g: split("Wp", g, 0), allow_tn)
            self.weight(("Wp_h", ids["Wp"]), d_proj, h, lambda g: split("Wp", g, H), allow_tn)
        self.bias(("bp", ids["Wp"]), d_proj, lambda g: split("bp", g, 0))
        b_gates = None
        if bounds is not None and gemm_tn_h2_supported(d_gi, inp) and gemm_tn_h2_supported(d_gh, h):
            # dW_ih / dW_hh on the f16x2 kernel (177-187 TFLOP/s against the vendor's 131-143 at C3): the column scales of the split
            # come for free - the global maxima of the row maxima bound every column; a column far below the global maximum is held with
            # fewer bits (absolute error <= 2^-39 of the bound per element, averaged down over 10^6 rows: DESIGN.md section 5)
            b_gates = (_max_two_stage(rm_g), _max_two_stage(rm_x))
        self.weight(("W_ih", ids["W_ih"]), d_gi, inp, lambda g: split("W_ih", g, 0), allow_tn, b_gates)
        self.weight((whh_key, ids["W_hh"]), d_gh, h, whh_flush, allow_tn, b_gates)
        if gsum is not None:
            self.bias(("b_ih", ids["W_ih"]), gsum[:, :3 * H], lambda g: split("b_ih", g, 0))
            self.bias(("b_hh_n", ids["W_hh"]), gsum[:, 3 * H:], lambda g: split("b_hh", g, 2 * H))
        else:
            # d_gh == d_gi on the r and z columns: only the n block of b_hh needs its own pass over d_gh
            self.bias(("b_ih", ids["W_ih"]), d_gi, lambda g: split("b_ih", g, 0))
            self.bias(("b_hh_n", ids["W_hh"]), d_gh[:, :H] if packed else d_gh[:, 2 * H:], lambda g: split("b_hh", g, 2 * H))
        self.weight(("W_out", ids["W_out"]), dq, h2, lambda g: split("W_out", g, 0), allow_tn)
        self.bias(("b_out", ids["W_out"]), dq, lambda g: split("b_out", g, 0))

    def flush(self):
        self.end_sequence()
        for key, (buf, fn) in self.slots.items():
            if fn is not None:
                fn(buf.sum(0))
        self.slots = {}
        self.owned.clear()
        self._seq_bufs = None


class _StepRecord:
    """What ONE step of a staged sequence left in its slots: `rowmax` by the forward's message kernel (row maxima of [x || c || h]);
    by the backward's gate kernel `gsum` (its column-sum partials), `rm_g` (row maxima of d_gi / d_gh) and `packed` (ONE [N, 4H] "g4"
    slot instead of "d_gi" / "d_gh"); `rm_p` (row maxima of d_proj) by the d x product; `dq`: the gradient of the step's Q values as
    autograd handed it over."""
    __slots__ = ("rowmax", "gsum", "rm_g", "packed", "rm_p", "dq")

    def __init__(self):
        self.rowmax = self.gsum = self.rm_g = self.packed = self.rm_p = False
        self.dq = None


class _SequenceStage:
    """Slots of the time-batched buffers of one BPTT sequence (WeightGradSink.begin_sequence)."""

    def __init__(self, T1, N, x_all, bufs=None):
        self.T1, self.N, self.x_all = T1, N, x_all
        self.bufs = bufs if bufs is not None else {}
        self.t_fwd = 0
        self.steps = {}                  # step -> _StepRecord: what its forward and backward left in the slots
        self.bwd_steps = []              # steps whose backward ran staged, in that order
        self.split = self.ids = self.H = None

    def dq_rows(self, t0, t1):
        """[(t1 - t0) N, A] gradient of the Q values of steps t0 .. t1 - 1.  The per-step gradients autograd hands to the recurrent step are
        normally consecutive [N, A] slices of ONE buffer (the backward of the learner's stack of the per-step Q values): then the rows are
        a view of it - rounds 4-5 copied every step into a staging slot (51 launches of 4.7 us per update); anything else is gathered by
        one torch.cat."""
        parts = [self.steps[t].dq for t in range(t0, t1)]
        if len(parts) == 1:
            return parts[0] if parts[0].is_contiguous() else parts[0].contiguous()
        first, (N, A) = parts[0], parts[0].shape
        if all(p.is_contiguous() and p.shape == (N, A) and p.dtype == first.dtype and
               p.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() and
               p.storage_offset() == first.storage_offset() + i * N * A for i, p in enumerate(parts)):
            return first.as_strided(((t1 - t0) * N, A), (A, 1), first.storage_offset())
        return th.cat(parts, 0)

    def slot(self, name, t, cols, extra=0, rows=None):
        """[N, cols] slot t of the [T1 + extra, N, cols] buffer `name` (``rows``: another row count than N per step)."""
        n = self.N if rows is None else rows
        b = self.bufs.get(name)
        if b is None or b.shape != (self.T1 + extra, n, cols) or b.device != self.x_all.device:
            b = self.bufs[name] = th.empty((self.T1 + extra, n, cols), dtype=th.float32, device=self.x_all.device)
        return b[t]


GRAD_SINK = None   # set by the learner around loss.backward(); None -> gradients are returned to autograd as usual
SEQ_STAGING = os.environ.get("UAVGNN_SEQ_STAGING", "1") != "0"   # weight / bias gradients of a BPTT sequence reduced once (A/B switch)


def _add_grad(p, g):
    if p.grad is None:
        p.grad = g.clone()
    else:
        p.grad.add_(g)


def _add_grad_cols(p, g, start):
    if p.grad is None:
        p.grad = th.zeros_like(p)
    p.grad[start:start + g.shape[0]].add_(g)


class _TimeSplit(th.autograd.Function):
    """x_all [T1 * N, H] -> T1 per-step views, with a gradient buffer the steps' backward passes write INTO.

    ``unbind`` would make autograd stack the T1 step gradients at the end (1.7 GB of copies for C3, T = 50); here the
    [T1, N, H] buffer is allocated up front, ``slots[t]`` (its t-th slice) is handed to the consumer of x_t (the fused
    recurrent step writes d x_t with ``out=``) and the backward of the split returns the buffer as it is when every
    incoming gradient is its own slice - otherwise it falls back to copying the strays in."""

    @staticmethod
    def forward(ctx, x_all, T1, holder):
        N = x_all.shape[0] // T1
        buf = th.empty((T1, N, x_all.shape[1]), dtype=x_all.dtype, device=x_all.device)
        holder.append(buf)
        ctx.buf = buf
        return tuple(x_all.detach().view(T1, N, -1).unbind(0))

    @staticmethod
    def backward(ctx, *grads):
        buf = ctx.buf
        for t, g in enumerate(grads):
            if g is None:
                buf[t].zero_()
            elif g.data_ptr() != buf[t].data_ptr() or g.stride() != buf[t].stride():
                buf[t].copy_(g)
        return buf.view(-1, buf.shape[2]), None, None


def time_split(x_all, T1):
    """(xs, slots): per-step views of the time-batched encoder output and the slices of its gradient buffer."""
    if not (th.is_grad_enabled() and x_all.requires_grad):
        return x_all.view(T1, x_all.shape[0] // T1, -1).unbind(0), [None] * T1
    holder = []
    xs = _TimeSplit.apply(x_all, T1, holder)
    return xs, list(holder[0].unbind(0))


MSG_FUSED = os.environ.get("UAVGNN_MSG_FUSED", "1") != "0"   # K3a + K3b in one launch (csrc/tarmac_msg.hip); A/B switch


def _tarmac_msg_plan(x, h, Wp, bp, M, K, env, N, H):
    """(weight tiles, agents per graph) when the fused K3a + K3b launch covers this call, else None: graphs with a uniform number
    of agents (every graph <= n_max and N == B n_max), aligned row-major operands, a contiguous stacked projection weight."""
    if not MSG_FUSED or env is None or N == 0:
        return None
    _, B, n_ag = env
    if N != B * n_ag or (H + M) % 4 or not L.lib().uavgnn_tarmac_msg_supported(H, M, K, n_ag):
        return None
    if (Wp.shape != (M + 2 * K, 2 * H) or not Wp.is_contiguous() or Wp.data_ptr() % 16 or not bp.is_contiguous()
            or x.data_ptr() % 16 or h.data_ptr() % 16 or x.dtype != th.float32 or Wp.dtype != th.float32):
        return None
    lib = L.lib()
    tiles = _weight_planes("msgw", (Wp,), (H, M, K), lib.uavgnn_tarmac_msg_weight_bytes(H, M, K),
                           lambda buf: L.check(lib.uavgnn_tarmac_msg_prepare(Wp.data_ptr(), Wp.stride(0), H, M, K, buf.data_ptr(),
                                                                            L.stream()), "uavgnn_tarmac_msg_prepare"))
    return tiles, n_ag


def _launch_tarmac_msg(msg, x, h, bp, M, K, talk_off, talk_src, N, H, c_ptr, ld_c, a_save, proj, ld_p, x_copy, ld_xc, rowmax=None):
    """rowmax [N] (optional): receives max(|x_row|, |c_row|, |h_row|) - the row scales of the f16x2 GRU cell behind this launch (the
    _rowmax entry: the same argument list + that pointer)."""
    tiles, n_ag = msg
    entry, outs = ("uavgnn_tarmac_msg_fwd", ()) if rowmax is None else ("uavgnn_tarmac_msg_fwd_rowmax", (rowmax.data_ptr(),))
    with KERNEL_TIMER.span("tarmac_msg_fwd", (N, H, M, K, int(proj is not None), int(x_copy is not None))):
        rc = getattr(L.lib(), entry)(x.data_ptr(), x.stride(0), h.data_ptr(), h.stride(0), N, H, n_ag, tiles.data_ptr(), bp.data_ptr(), M, K,
                                     L.ptr(talk_off), L.ptr(talk_src), 1.0 / K, c_ptr, ld_c, a_save, proj, ld_p, x_copy, ld_xc, *outs,
                                     L.stream())
    L.check(rc, entry)


DUEL_FUSED = True   # the dueling head on csrc/head.hip and inside the fused TarMAC step; False: the torch formulation (A/B, tools/dueling_probe.py)


def dueling_params(layer):
    """(W_adv [A, H], b_adv [A], w_v [1, H], b_v [1]) of a DuelingLayer (agents/heads.py; dueling.py:10-11)."""
    return layer.adv_head.weight, layer.adv_head.bias, layer.v_head.weight, layer.v_head.bias


def dueling_fold(W_adv, b_adv, w_v, b_v):
    """The dueling combine q = v + (adv - mean_a adv) (dueling.py:16) is linear in the two heads' outputs: q = h W_eff^T + b_eff with
    W_eff = C W_adv + 1 w_v, b_eff = C b_adv + b_v, C = I - 1 1^T / A.  C X = X - the column means of X."""
    return W_adv - W_adv.mean(0, keepdim=True) + w_v, b_adv - b_adv.mean() + b_v


def dueling_split(G, g):
    """The transpose of ``dueling_fold``: (d W_adv, d b_adv, d w_v, d b_v) from G = d W_eff = dq^T h [A, H] and g = d b_eff = colsum(dq) [A]:
    C G, C g, 1^T G, 1^T g (C is symmetric).  Either input may be None (its two results are None then)."""
    dWa, dwv = (None, None) if G is None else (G - G.mean(0, keepdim=True), G.sum(0, keepdim=True))
    dba, dbv = (None, None) if g is None else (g - g.mean(), g.sum().reshape(1))
    return dWa, dba, dwv, dbv


def dueling_supported(h, W_adv, b_adv, w_v, b_v) -> bool:
    """csrc/head.hip has the dueling form for this call: CUDA fp32, H in {64, 128, 256}, n_actions <= 15, DUEL_FUSED."""
    return bool(DUEL_FUSED and h.is_cuda and h.dtype == th.float32 and h.dim() == 2 and h.shape[0] > 0 and _mc_operand(h)
                and all(t.is_cuda and t.dtype == th.float32 and t.is_contiguous() for t in (W_adv, b_adv, w_v, b_v))
                and W_adv.data_ptr() % 16 == 0 and w_v.data_ptr() % 16 == 0
                and L.lib().uavgnn_head_duel_supported(h.shape[1], W_adv.shape[0]))


def _duel_weff(W_adv, w_v):
    """W_eff [A, H] of ``dueling_fold`` (contiguous, 16-byte aligned, no autograd history) for the backward's input gradient
    d h = dq W_eff: three small torch launches, once per ``frozen_weights`` scope and (storage of the two weights) - per call outside."""
    A, H = W_adv.shape
    Wa, wv = W_adv.detach(), w_v.detach()

    def build(planes):
        out = planes.view(th.float32).view(A, H)
        th.sub(Wa, Wa.mean(0, keepdim=True), out=out)
        out.add_(wv)
    return _weight_planes("duel", (W_adv, w_v), (A, H), 4 * A * H, build).view(th.float32).view(A, H)


# ---------------------------------------------------------------------------------------------------------------------
# Noisy-net Q head (csrc/ext/noisy_head.hip, include/uavgnn_ext.h): W = W_mu + W_sigma (.) (f_out f_in^T), b = b_mu + b_sigma (.) f_out
# ---------------------------------------------------------------------------------------------------------------------
def noisy_f(z):
    """f(z) = sign(z) sqrt|z| of the factorised noise."""
    return z.sign() * z.abs().sqrt()


def noisy_supported(h, W_mu, W_sigma, b_mu, b_sigma) -> bool:
    """csrc/ext/noisy_head.hip has the per-row launch for this call: CUDA fp32, H in {64, 128, 256}, n_actions <= 16."""
    return bool(h.is_cuda and h.dtype == th.float32 and h.dim() == 2 and h.shape[0] > 0 and _mc_operand(h)
                and all(t.is_cuda and t.dtype == th.float32 for t in (W_mu, W_sigma, b_mu, b_sigma))
                and _mc_operand(W_mu) and _mc_operand(W_sigma) and W_mu.stride(0) == W_sigma.stride(0)
                and b_mu.is_contiguous() and b_sigma.is_contiguous()
                and L.ext().uavgnn_noisy_head_supported(h.shape[1], W_mu.shape[0]))


def noisy_noise(rng, N, H, A):
    """(f_in [N, H], f_out [N, A]): the values f(xi) of the stream at the device pair `rng`, as the kernels use them (tests, probes)."""
    L.require_gpu(rng)
    f_in = th.empty((N, H), dtype=th.float32, device=rng.device)
    f_out = th.empty((N, A), dtype=th.float32, device=rng.device)
    L.check(L.ext().uavgnn_noisy_noise(rng.data_ptr(), N, H, A, f_in.data_ptr(), f_out.data_ptr(), L.stream()), "uavgnn_noisy_noise")
    return f_in, f_out


def _noisy_head_torch(h, W_mu, b_mu, W_sigma, b_sigma, f_in, f_out):
    """The per-row draw in torch, in the kernel's order: (h W_mu^T + b_mu) + f_out (.) ((h (.) f_in) W_sigma^T + b_sigma)."""
    return th.addmm(b_mu, h, W_mu.t()) + f_out * th.addmm(b_sigma, h * f_in, W_sigma.t())


def noisy_fold_torch(W_mu, W_sigma, b_mu, b_sigma, f_in, f_out):
    """(W_eff, b_eff) of one shared draw f_in [H], f_out [A], in the kernel's order (differentiable torch)."""
    return W_mu + W_sigma * (f_out[:, None] * f_in[None, :]), b_mu + b_sigma * f_out


class _NoisyFold(th.autograd.Function):
    """(W_eff, b_eff, f_in, f_out) of ONE draw - row 0 of the stream at the pair `rng` - in one launch (uavgnn_noisy_fold); the backward
    is one launch too (uavgnn_noisy_fold_bwd): the means' gradients are the incoming ones, the sigmas' are those times the noise."""

    @staticmethod
    def forward(ctx, W_mu, W_sigma, b_mu, b_sigma, rng):
        L.require_gpu(W_mu, W_sigma, b_mu, b_sigma, rng)
        A, H = W_mu.shape
        W_mu, W_sigma, b_mu, b_sigma = L.f32c(W_mu), L.f32c(W_sigma), L.f32c(b_mu), L.f32c(b_sigma)
        W_eff = th.empty((A, H), dtype=th.float32, device=W_mu.device)
        b_eff, f_out = th.empty_like(b_mu), th.empty_like(b_mu)
        f_in = th.empty((H,), dtype=th.float32, device=W_mu.device)
        with KERNEL_TIMER.span("noisy_fold", (A, H)):
            rc = L.ext().uavgnn_noisy_fold(W_mu.data_ptr(), W_sigma.data_ptr(), H, b_mu.data_ptr(), b_sigma.data_ptr(), A, H, rng.data_ptr(),
                                           W_eff.data_ptr(), b_eff.data_ptr(), f_in.data_ptr(), f_out.data_ptr(), L.stream())
        L.check(rc, "uavgnn_noisy_fold")
        ctx.save_for_backward(f_in, f_out)
        ctx.mark_non_differentiable(f_in, f_out)
        return W_eff, b_eff, f_in, f_out

    @staticmethod
    def backward(ctx, dW, db, _d_in, _d_out):
        f_in, f_out = ctx.saved_tensors
        dWs, dbs = noisy_fold_bwd(dW, db, f_in, f_out)
        return dW, dWs, db, dbs, None


def noisy_fold_bwd(dW_eff, db_eff, f_in, f_out):
    """(d W_sigma, d b_sigma) = (d W_eff (.) (f_out f_in^T), d b_eff (.) f_out); either gradient may be None (zeros then)."""
    A, H = f_out.shape[0], f_in.shape[0]
    if dW_eff is None:
        dW_eff = th.zeros((A, H), dtype=f_in.dtype, device=f_in.device)
    if db_eff is None:
        db_eff = th.zeros((A,), dtype=f_in.dtype, device=f_in.device)
    if not (f_in.is_cuda and f_in.dtype == th.float32):
        return dW_eff * (f_out[:, None] * f_in[None, :]), db_eff * f_out
    dW_eff = dW_eff if dW_eff.stride(1) == 1 and dW_eff.dtype == th.float32 else L.f32c(dW_eff.float())
    db_eff = L.f32c(db_eff)
    dWs, dbs = th.empty((A, H), dtype=th.float32, device=f_in.device), th.empty((A,), dtype=th.float32, device=f_in.device)
    with KERNEL_TIMER.span("noisy_fold_bwd", (A, H)):
        rc = L.ext().uavgnn_noisy_fold_bwd(dW_eff.data_ptr(), dW_eff.stride(0), db_eff.data_ptr(), f_in.data_ptr(), f_out.data_ptr(), A, H,
                                           dWs.data_ptr(), dbs.data_ptr(), L.stream())
    L.check(rc, "uavgnn_noisy_fold_bwd")
    return dWs, dbs


def noisy_fold(W_mu, W_sigma, b_mu, b_sigma, rng=None, noise=None):
    """Mode "shared" of the noisy head: (W_eff, b_eff, f_in, f_out) of one draw, with autograd into the four parameters.
    CUDA fp32 with a device pair `rng` and no injected noise: uavgnn_noisy_fold / uavgnn_noisy_fold_bwd (the step is NOT advanced here).
    Elsewhere - CPU, float64, ``noise`` = (f_in [H], f_out [A]) injected (tests) - the same formula in torch, the draw from
    ``torch.randn`` when none is given."""
    A, H = W_mu.shape
    if noise is None and rng is not None and W_mu.is_cuda and W_mu.dtype == th.float32:
        return _NoisyFold.apply(W_mu, W_sigma, b_mu, b_sigma, rng)
    if noise is None:
        noise = (noisy_f(th.randn(H, dtype=W_mu.dtype, device=W_mu.device)), noisy_f(th.randn(A, dtype=W_mu.dtype, device=W_mu.device)))
    f_in, f_out = noise
    return (*noisy_fold_torch(W_mu, W_sigma, b_mu, b_sigma, f_in, f_out), f_in, f_out)


def head_fwd(h, W_out, b_out, duel=None, noisy=None):
    """q = h W_out^T + b_out (gnn_agents.py:56), no autograd: csrc/head.hip for n_actions <= 16, else the vendor GEMM.
    duel = (W_adv, b_adv, w_v, b_v): the dueling head (dueling.py:13-16) instead - W_out / b_out are not read -, csrc/head.hip for
    n_actions <= 15, else the torch formulation.
    noisy = (W_sigma, b_sigma, rng): the noisy head with one draw PER ROW (W_out / b_out are the means) - rng a device int64 pair
    {seed, step}: ONE launch of csrc/ext/noisy_head.hip where it has the shape (the step is not advanced here: the caller does); rng a
    tuple (f_in [N, H], f_out [N, A]) of injected noise, another shape, the CPU or float64: the torch formulation, its draw from
    ``torch.randn`` unless injected."""
    N, H = h.shape
    if noisy is not None:
        Ws, bs, rng = noisy
        A = W_out.shape[0]
        if isinstance(rng, th.Tensor) and noisy_supported(h, W_out, Ws, b_out, bs):
            q = th.empty((N, A), dtype=th.float32, device=h.device)
            with KERNEL_TIMER.span("noisy_head_fwd", (N, H, A)):
                rc = L.ext().uavgnn_noisy_head_fwd(h.data_ptr(), h.stride(0), N, H, W_out.data_ptr(), Ws.data_ptr(), W_out.stride(0),
                                                   b_out.data_ptr(), bs.data_ptr(), A, rng.data_ptr(), q.data_ptr(), A, L.stream())
            L.check(rc, "uavgnn_noisy_head_fwd")
            return q
        if isinstance(rng, tuple):
            f_in, f_out = rng
        elif isinstance(rng, th.Tensor) and rng.is_cuda and h.is_cuda:       # the stream's own values (other shapes on the GPU)
            f_in, f_out = (t.to(h.dtype) for t in noisy_noise(rng, N, H, A))
        else:
            f_in, f_out = noisy_f(th.randn(N, H, dtype=h.dtype, device=h.device)), noisy_f(th.randn(N, A, dtype=h.dtype, device=h.device))
        return _noisy_head_torch(h, W_out, b_out, Ws, bs, f_in, f_out)
    if duel is not None:
        Wa, ba, wv, bv = duel
        A = Wa.shape[0]
        if dueling_supported(h, Wa, ba, wv, bv):
            q = th.empty((N, A), dtype=th.float32, device=h.device)
            with KERNEL_TIMER.span("head_fwd_duel", (N, H, A)):
                rc = L.lib().uavgnn_head_fwd_duel(h.data_ptr(), h.stride(0), N, H, Wa.data_ptr(), Wa.stride(0), wv.data_ptr(), ba.data_ptr(),
                                                  bv.data_ptr(), A, q.data_ptr(), A, L.stream())
            L.check(rc, "uavgnn_head_fwd_duel")
            return q
        out = th.addmm(th.cat((ba, bv), 0), h, th.cat((Wa, wv), 0).t())
        adv, val = out[:, :A], out[:, A:]
        return val + adv - adv.mean(-1, keepdim=True)
    A = W_out.shape[0]
    if (h.is_cuda and h.dtype == th.float32 and N > 0 and _mc_operand(h) and _mc_operand(W_out)
            and b_out.is_contiguous() and L.lib().uavgnn_head_supported(H, A)):
        q = th.empty((N, A), dtype=th.float32, device=h.device)
        with KERNEL_TIMER.span("head_fwd", (N, H, A)):
            rc = L.lib().uavgnn_head_fwd(h.data_ptr(), h.stride(0), N, H, W_out.data_ptr(), W_out.stride(0), b_out.data_ptr(), A,
                                         q.data_ptr(), A, L.stream())
        L.check(rc, "uavgnn_head_fwd")
        return q
    return th.addmm(b_out, h, W_out.t())


class _DuelingHead(th.autograd.Function):
    """q = v + (adv - mean_a adv) of a DuelingLayer outside the fused TarMAC step (gnn_agents._head: the agents without a communication
    block, the other comm blocks, RnnAgent).  Forward: ONE launch of csrc/head.hip on the live parameters.  Backward: the combine is
    linear, so d h = dq W_eff (``_duel_weff``) and the four parameter gradients are the split (``dueling_split``) of ONE product
    G = dq^T h and one column sum - nothing per row beyond what ``ops.linear`` does for a plain head."""

    @staticmethod
    def forward(ctx, h, W_adv, b_adv, w_v, b_v):
        ctx.save_for_backward(h, W_adv, w_v)
        return head_fwd(h, None, None, (W_adv, b_adv, w_v, b_v))

    @staticmethod
    def backward(ctx, dq):
        h, W_adv, w_v = ctx.saved_tensors
        dq = L.f32c(dq)
        dh = dWa = dba = dwv = dbv = None
        if ctx.needs_input_grad[0]:
            dh = _mm_nn(dq, _duel_weff(W_adv, w_v))
        if any(ctx.needs_input_grad[1:]):
            dWa, dba, dwv, dbv = dueling_split(_wgrad(dq, h), _colsum(dq))
        return dh, dWa, dba, dwv, dbv


def dueling_head(h, layer):
    """The Q values of a DuelingLayer on csrc/head.hip, with autograd.  Caller checks ``dueling_supported``."""
    return _DuelingHead.apply(h, *dueling_params(layer))


class _TarmacStep(th.autograd.Function):
    """q, h' = head(GRU([x || c], h)), c = targeted attention over `talk` of the projections of [x || stopgrad(h)]
    (gnn_agents.py:248-271 with n_rounds = 1, then :56).  Forward: 5 vendor GEMMs + K3b + K4, the projection of the two
    halves accumulated in place, c written by K3b straight into the GRU input buffer (no cat, no add kernels).
    Backward: hand-written; weight gradients go to ``GRAD_SINK`` when one is active."""

    @staticmethod
    def forward(ctx, x, h, Wp, bp, W_ih, b_ih, W_hh, b_hh, W_out, b_out, M, K, talk_off, talk_src, t_off, t_dst, t_pos,
                split, env=None, dx_out=None, train=True, duel=None, noisy=None):
        # duel = (W_adv, b_adv, w_v, b_v, identity): the dueling head (dueling.py:13-16) - the forward reads the four parameters in
        # csrc/head.hip; W_out / b_out are then the fold W_eff / b_eff (``dueling_fold``), which is all the backward needs
        # noisy: the noisy head (agents/heads.py NoisyLinear) - ("shared", identity): W_out / b_out are the fold of this update's draw
        # (``noisy_fold``), a plain head to forward and backward, its gradient sunk under the module's identity; ("rows", W_sigma,
        # b_sigma, rng): a no-grad rollout step, W_out / b_out the means, one draw per row inside the head launch
        L.require_gpu(x, h, Wp, W_ih, talk_off)
        N, H = x.shape
        x, h = L.f32c(x), L.f32c(h)
        # K3a + K3b as ONE launch (csrc/tarmac_msg.hip) when the batch is made of graphs with a uniform number of agents: the
        # projections stay on the chip on no-grad calls (two vendor GEMMs + K3b: 52 us per C3 step; traffic floor ~13 us)
        msg = _tarmac_msg_plan(x, h, Wp, bp, M, K, env, N, H)
        if msg is not None:
            proj = None
        elif gemm_x3_supported(x, Wp.shape[0], H) and gemm_x3_supported(h, Wp.shape[0], H) and bp.is_contiguous():
            proj = gemm_x3(x, Wp[:, :H], bias=bp)
            gemm_x3(h, Wp[:, H:], out=proj, accumulate=True)
        else:
            proj = th.addmm(bp, x, Wp[:, :H].t())
            proj.addmm_(h, Wp[:, H:].t())                                 # [N, M + 2K]: value | signature | query
        E = talk_src.shape[0]
        a_save = th.empty(max(E, 1), dtype=th.float32, device=x.device)
        ld = M + 2 * K
        ctx.seq = ctx.seq_t = None
        aligned = all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (W_ih, W_hh))
        # the f16x2 cell needs the row maxima of [x || c || h]: the fused message launch writes them on its way
        rowmax = None
        if (msg is not None and aligned and GRU_FUSED and gru_cell_h2_supported(H + M, H, N, max(x.stride(0), H + M))
                and H % 32 == 0 and M % 32 == 0 and L.lib().uavgnn_tarmac_msg_rowmax_supported(H, M, K, msg[1])):
            rowmax = th.empty(N, dtype=th.float32, device=x.device)
        c_only = None
        if not train and aligned and h.shape[0] >= GRU_FUSED_MIN_ROWS and GRU_FUSED:
            c_only = th.empty((N, M), dtype=th.float32, device=x.device)
            if not gru_cell_two_piece_supported(x, c_only, h):
                c_only = None
        if c_only is not None:
            # no-grad call (rollout, target network): nothing keeps [x || c] for a backward, so K3b writes c alone and the cell
            # reads its input from the two buffers - the 2 x 4 H bytes per agent of the concatenating copy disappear
            if msg is not None:
                _launch_tarmac_msg(msg, x, h, bp, M, K, talk_off, talk_src, N, H, c_only.data_ptr(), M, None, None, 0, None, 0,
                                   rowmax=rowmax)
            else:
                _launch_talk_fwd(env, proj.data_ptr() + 4 * M, ld, proj.data_ptr() + 4 * (M + K), ld, proj.data_ptr(), ld, K, M,
                                 talk_off, talk_src, N, 1.0 / K, c_only.data_ptr(), M, a_save.data_ptr(), None, 0, 0)
            h2, _ = _gru_cell_launch(x, h, W_ih, b_ih, W_hh, b_hh, save=False, inp2=c_only, rowmax=rowmax)
            inp, fused = c_only, True
            gi = gh = h2                                           # placeholders keep save_for_backward's arity
        else:
            # inside a staged BPTT sequence (WeightGradSink.begin_sequence) [x || c] and h' are written into the slots of
            # step t of the time-batched buffers the weight gradients are reduced from at the end of the sequence
            seq = GRAD_SINK.seq if (train and GRAD_SINK is not None) else None
            if seq is not None and (seq.t_fwd >= seq.T1 or N != seq.N or seq.x_all.shape[1] != H or
                                    x.data_ptr() != seq.x_all.data_ptr() + 4 * H * N * seq.t_fwd):
                seq = None           # not a step of the sequence that was announced (or more steps than announced)
            if seq is not None and seq.t_fwd > 0 and h.data_ptr() != seq.slot("h", seq.t_fwd, H, extra=1).data_ptr():
                # end_sequence() reduces W_hh / Wp_h / W_out from the h SLOTS: a caller that masks or copies h between two steps
                # hands over another tensor than the slot the previous step wrote - this step (and, through the x check above,
                # every later one) reduces per step instead
                seq = None
            if seq is not None:
                seq_t = seq.t_fwd
                seq.t_fwd += 1
                seq.steps[seq_t] = _StepRecord()
                inp = seq.slot("inp", seq_t, H + M)
                if seq_t == 0:
                    seq.slot("h", 0, H, extra=1).copy_(h)
            else:
                inp = th.empty((N, H + M), dtype=th.float32, device=x.device)     # [x || c], both halves filled by K3b
            if seq is not None and rowmax is not None:       # kept for the sequence: its maximum scales the weight-gradient products
                rowmax = seq.slot("rowmax", seq_t, 1).view(N)
                seq.steps[seq_t].rowmax = True
            if msg is not None:     # proj, the attention weights and the x half of [x || c] are the launch's training outputs
                proj = th.empty((N, ld), dtype=th.float32, device=x.device)
                _launch_tarmac_msg(msg, x, h, bp, M, K, talk_off, talk_src, N, H, inp.data_ptr() + 4 * H, H + M, a_save.data_ptr(),
                                   proj.data_ptr(), ld, inp.data_ptr(), H + M, rowmax=rowmax)
            else:
                _launch_talk_fwd(env, proj.data_ptr() + 4 * M, ld, proj.data_ptr() + 4 * (M + K), ld, proj.data_ptr(), ld, K, M,
                                 talk_off, talk_src, N, 1.0 / K, inp.data_ptr() + 4 * H, H + M, a_save.data_ptr(), x.data_ptr(),
                                 x.stride(0), H)
            fused = gru_cell_supported(inp, h) and aligned
            if fused:      # K4 in one launch: gi / gh never reach HBM; training forwards keep the [N, 4H] pre-activation sets
                h2, pre = _gru_cell_launch(inp, h, W_ih, b_ih, W_hh, b_hh, save=bool(train),
                                           h2_out=None if seq is None else seq.slot("h", seq_t + 1, H, extra=1), rowmax=rowmax)
                if seq is not None and pre is not None:
                    ctx.seq, ctx.seq_t = seq, seq_t
                gi = gh = pre if pre is not None else h2           # placeholders keep save_for_backward's arity
            else:
                gi = th.addmm(b_ih, inp, W_ih.t())
                gh = th.addmm(b_hh, h, W_hh.t())
                h2 = th.empty_like(h)
                with KERNEL_TIMER.span("gru_gates_fwd"):
                    rc = L.lib().uavgnn_gru_gates_fwd(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), N, H, h2.data_ptr(), L.stream())
                L.check(rc, "uavgnn_gru_gates_fwd")
            # (an accepted step that ran unfused wrote h' into a tensor of its own, not into slot t + 1: the next step's h then
            # fails the slot check above and reduces per step, like this one - ctx.seq stays None)
        rows = noisy is not None and noisy[0] == "rows"
        q = head_fwd(h2, W_out, b_out, None if duel is None else duel[:4], noisy[1:] if rows else None)
        ctx.out_id = None if duel is None else duel[4]
        if noisy is not None and not rows:
            ctx.out_id = noisy[1]
        if proj is None:
            proj = h2                                              # no-grad call through the fused message launch: placeholder
        ctx.dims = (M, K)
        ctx.split, ctx.env, ctx.dx_out, ctx.fused_gru = split, env, dx_out, fused
        ctx.have_pre = bool(train) or not fused
        ctx.save_for_backward(x, h, proj, inp, gi, gh, h2, a_save, Wp, W_ih, W_hh, W_out, talk_off, talk_src, t_off,
                              t_dst, t_pos)
        return q, h2

    @staticmethod
    def backward(ctx, dq, dh2):
        (x, h, proj, inp, gi, gh, h2, a_save, Wp, W_ih, W_hh, W_out, talk_off, talk_src, t_off, t_dst,
         t_pos) = ctx.saved_tensors
        N, H = x.shape
        if not ctx.have_pre:    # gi would be the [N, H] placeholder: reading 4H floats per row from it is out of bounds
            raise L.UavGnnError("tarmac_step: backward through a forward that saved no pre-activations (train=False)")
        sink = GRAD_SINK
        dq = L.f32c(dq) if dq is not None else th.zeros((N, W_out.shape[0]), dtype=th.float32, device=x.device)
        seq = ctx.seq if (sink is not None and ctx.seq is not None and sink.seq is ctx.seq) else None
        head, dh2_tot = _step_dh2(ctx.fused_gru, sink, dq, dh2, W_out, N, H)
        d_gi, d_gh, dh, rm_g, g4 = _step_gate_grads(seq, ctx.seq_t, ctx.fused_gru, gi, gh, h, dh2_tot, head, W_hh)
        dx, d_proj = _step_input_grads(seq, ctx.seq_t, sink, ctx.dims, ctx.env, ctx.dx_out, proj, a_save, Wp, W_ih, W_hh,
                                       (talk_off, talk_src, (t_off, t_dst, t_pos)), d_gi, d_gh, dh, rm_g, g4)
        gWp = gbp = gWih = gbih = gWhh = gbhh = gWo = gbo = None
        ids = {"Wp": id(Wp), "W_ih": id(W_ih), "W_hh": id(W_hh), "W_out": id(W_out) if ctx.out_id is None else ctx.out_id}
        if seq is not None:      # reduced once per sequence (WeightGradSink.end_sequence)
            seq.steps[ctx.seq_t].dq = dq      # (a reference, no copy: see _SequenceStage.dq_rows)
            seq.bwd_steps.append(ctx.seq_t)
            seq.split, seq.H, seq.ids = ctx.split, H, ids
        elif sink is not None:
            sink.step_grads(ctx.split, ids, H, x, h, h2, inp, d_proj, d_gi, d_gh, dq)
        else:
            gWp = th.cat((_wgrad(d_proj, x), _wgrad(d_proj, h)), 1)
            gbp = _colsum(d_proj)
            gWih, gbih = _wgrad(d_gi, inp), _colsum(d_gi)
            gWhh, gbhh = _wgrad(d_gh, h), th.cat((gbih[:2 * H], _colsum(d_gh[:, 2 * H:])))
            gWo, gbo = _wgrad(dq, h2), _colsum(dq)
        return (dx, dh, gWp, gbp, gWih, gbih, gWhh, gbhh, gWo, gbo) + (None,) * 13


def _step_dh2(fused_gru, sink, dq, dh2, W_out, N, H):
    """Backward of the recurrent step, stage 1: the gradient of h', d_hout + dq W_out -> (head, dh2_tot).  head = (dq, W_out): the sum
    is formed INSIDE the gate kernel (the cell ran fused: its pre-activation sets are what that kernel reads) and dh2_tot is the
    incoming d_hout alone (None = 0); head = None: dh2_tot is the whole gradient, from a vendor GEMM."""
    if (fused_gru and H % 4 == 0 and W_out.shape[0] <= 64 and W_out.is_contiguous()
            and W_out.dtype == th.float32 and W_out.data_ptr() % 16 == 0
            and (dh2 is None or (dh2.is_contiguous() and dh2.dtype == th.float32 and dh2.shape == (N, H)))):
        if sink is not None:
            sink.owned.clear()
        return (dq, W_out.detach()), dh2
    if dh2 is None:
        return None, th.mm(dq, W_out)
    if (sink is not None and dh2.is_contiguous() and dh2.dtype == th.float32 and dh2.shape == (N, H)
            and sink.owned.get(dh2.data_ptr()) is not None):
        # inside the learner's BPTT the incoming d h' is the buffer the NEXT step's backward of this very op
        # allocated and returned (registered in sink.owned and kept alive there): nobody else holds it, so accumulate
        # in place instead of copying 33 MB into a fresh output first.  Any other gradient tensor (a hook's,
        # retain_grad's, one autograd summed from several consumers) lives at another address and is left untouched.
        sink.owned.clear()
        return None, dh2.addmm_(dq, W_out)
    return None, th.addmm(dh2, dq, W_out)


def _step_gate_grads(seq, t, fused_gru, gi, gh, h, dh2_tot, head, W_hh):
    """Stage 2: the gate gradients -> (d_gi, d_gh, dh, rm_g, g4).  seq / t: the staged sequence and the step's slot (None: a step of its
    own); gi: the saved [N, 4H] pre-activation sets when the cell ran fused, else gi / gh are the two [N, 3H] blocks.  rm_g [N]: the row
    maxima of d_gi / d_gh where the f16x2 products behind take them (else None); g4 [N, 4H]: the packed buffer [dn_h | dr | dz | dn_i]
    when the step stores its gate gradients once - d_gi is then its view g4[:, H:] and d_gh is None."""
    N, H = h.shape
    rm_g = g4 = None
    if seq is not None:      # staged sequence: the gate gradients go straight into the time-batched buffers
        rec = seq.steps[t]
        G = L.lib().uavgnn_gru_gates_bwd_sum_rows(N, H)
        # the step's share of db_ih / db_hh comes out of the gate kernel: end_sequence() sums [T1 G, 4H] partials instead of
        # streaming the [T1 N, 3H] gate gradients twice more
        sums = seq.slot("gsum", t, 4 * H, rows=G) if G else None
        if sums is not None and H == 256 and W_hh.stride(1) == 1:
            if G4 and gemm_h2_supported(seq.slot("g4", t, 4 * H)[:, H:], H, 3 * H):
                g4 = seq.slot("g4", t, 4 * H)          # ONE buffer [dn_h | dr | dz | dn_i]: the r / z columns are stored once
            if g4 is not None or gemm_h2_supported(seq.slot("d_gh", t, 3 * H), H, 3 * H):
                rm_g = seq.slot("rm_g", t, 1).view(N)  # row maxima of d_gi / d_gh for the f16x2 products of stage 3 (and, over the
                #                                        whole sequence, for the weight gradients)
        rec.gsum, rec.packed, rec.rm_g = sums is not None, g4 is not None, rm_g is not None
        if g4 is not None:
            # packed mode of the gate entry: d_gi == d_gh + H.  d_gi = G[:, H:] in its natural order; `d_gh` is NOT the plain
            # operand (its column blocks come in the order n, r, z): d h in stage 3 takes it as two sources
            d_gi, _, dh = _gru_gates_bwd_from_pre(gi, h, dh2_tot, g4[:, H:], g4[:, :3 * H], head=head, sums=sums, rowmax=rm_g)
            return d_gi, None, dh, rm_g, g4
        d_gi, d_gh, dh = _gru_gates_bwd_from_pre(gi, h, dh2_tot, seq.slot("d_gi", t, 3 * H), seq.slot("d_gh", t, 3 * H),
                                                 head=head, sums=sums, rowmax=rm_g)
    elif fused_gru:
        d_gi, d_gh, dh = _gru_gates_bwd_from_pre(gi, h, dh2_tot, head=head)      # gi holds the saved pre-activation sets
    else:
        d_gi, d_gh, dh = th.empty_like(gi), th.empty_like(gh), th.empty_like(h)
        with KERNEL_TIMER.span("gru_gates_bwd"):
            rc = L.lib().uavgnn_gru_gates_bwd(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), dh2_tot.data_ptr(), N, H,
                                              d_gi.data_ptr(), d_gh.data_ptr(), dh.data_ptr(), L.stream())
        L.check(rc, "uavgnn_gru_gates_bwd")
    return d_gi, d_gh, dh, rm_g, g4


def _step_input_grads(seq, t, sink, dims, env, dx_out, proj, a_save, Wp, W_ih, W_hh, talk, d_gi, d_gh, dh, rm_g, g4):
    """Stage 3: the input gradients -> (dx, d_proj); d h += d_gh W_hh is accumulated into `dh` in place.  d c = d_gi W_ih[:, H:], the
    attention backward (d c -> d_proj) and d x = d_gi W_ih[:, :H] + d_proj Wp[:, :H].  dx_out: where the caller wants d x (the slice of
    the time-split gradient buffer) or None; talk = (talk_off, talk_src, transpose); rm_g / g4: stage 2's."""
    M, K = dims
    N, H = dh.shape
    # d_inp = d_gi W_ih is [N, H + M]: d x | d c.  When the bf16x3 GEMM has the H-column shape, the two halves are separate
    # products: d x lands where the caller wants it (the slice of the time-split gradient buffer) and the projection term is
    # accumulated into it in place - no [N, H] copy in front of the addmm, and 256 of the 320 columns leave the vendor's
    # 64 x 32-tile solution (134 us) for the matrix-core kernel
    split_dinp = (M > 0 and W_ih.stride(1) == 1 and gemm_x3_supported(d_gi, H, W_ih.shape[0])
                  and (dx_out is None or (dx_out.stride(1) == 1 and dx_out.dtype == th.float32)))
    ld = M + 2 * K
    d_proj = th.empty((N, ld), dtype=th.float32, device=dh.device) if seq is None else seq.slot("d_proj", t, ld)
    dx_cat = False
    if split_dinp:
        dx = dx_out if dx_out is not None else th.empty((N, H), dtype=th.float32, device=dh.device)
        # d x = d_gi W_ih[:, :H] + d_proj Wp[:, :H]: ONE product over [d_gi || d_proj] once d_proj exists (behind the attention
        # backward) instead of a product + an accumulating vendor GEMM that re-reads and re-writes d x (31 us per step)
        dx_cat = Wp.stride(1) == 1 and gemm_x3_cat_supported(d_gi, d_proj, H)
        if not dx_cat:
            _mm_nn(d_gi, W_ih[:, :H], out=dx)
        if rm_g is not None and M == 64 and gemm_h2_n64_supported(d_gi, M, 3 * H):
            d_c = gemm_h2_n64(d_gi, W_ih[:, H:], rm_g)                 # [N, M], f16x2 on 128 x 64 tiles
        else:
            d_c = th.mm(d_gi, W_ih[:, H:])                             # [N, M]
        d_c_ptr, d_c_ld = d_c.data_ptr(), M
    else:
        d_inp = _mm_nn(d_gi, W_ih)
        d_c_ptr, d_c_ld = d_inp.data_ptr() + 4 * H, H + M
    if g4 is not None:
        # d h += d_gh W_hh over K in the order r, z, n as ever: [G[:, H:3H] || G[:, :H]] [W_hh[:2H]; W_hh[2H:]] (the stacked weight IS
        # W_hh: the same planes and scales)
        gemm_h2(g4[:, H:3 * H], W_hh[:2 * H], rm_g, True, out=dh, accumulate=True, a2=g4[:, :H], W2=W_hh[2 * H:])
    else:
        _mm_nn(d_gh, W_hh, out=dh, accumulate=True, rowmax=rm_g)
    if sink is not None:
        sink.owned.clear()
        sink.owned[dh.data_ptr()] = dh
    talk_off, talk_src, transpose = talk
    _launch_talk_bwd(env, proj.data_ptr() + 4 * M, ld, proj.data_ptr() + 4 * (M + K), ld, proj.data_ptr(), ld,
                     K, M, talk_off, talk_src, transpose, N, 1.0 / K, a_save, d_c_ptr,
                     d_c_ld, d_proj.data_ptr() + 4 * M, ld, d_proj.data_ptr() + 4 * (M + K), ld, d_proj.data_ptr(),
                     ld)
    if dx_cat and rm_g is not None and gemm_h2_supported(d_gi, H, d_gi.shape[1] + d_proj.shape[1]):
        # f16x2: the row scale of [d_gi || d_proj] is the larger of the gate kernel's bound and d_proj's own, which the launch takes
        # itself (96 columns per row, read once more by its workgroups: a microsecond against a 7.8-us pass of uavgnn_row_absmax)
        if seq is not None:      # kept for the sequence: the column bound of d_proj in the weight gradient dWp (end_sequence)
            rm_p = seq.slot("rm_p", t, 1).view(N)
            seq.steps[t].rm_p = True
        else:
            rm_p = th.empty(N, dtype=th.float32, device=d_gi.device)
        gemm_h2(d_gi, W_ih[:, :H], rm_g, True, out=dx, a2=d_proj, W2=Wp[:, :H], rowmax2_out=rm_p)
    elif dx_cat:
        gemm_x3_cat(d_gi, d_proj, W_ih[:, :H], Wp[:, :H], dx)
    elif split_dinp:
        dx.addmm_(d_proj, Wp[:, :H])                                   # h enters the projections stop-gradded
    elif dx_out is not None:                                           # slice of the time-split gradient buffer
        dx = th.addmm(d_inp[:, :H], d_proj, Wp[:, :H], out=dx_out)
    else:
        dx = th.addmm(d_inp[:, :H], d_proj, Wp[:, :H])
    return dx, d_proj


def tarmac_step(x, h, g, comm, f_out, stacked=None, dx_out=None):
    """comm: the TarMAC module (f_val / f_sign / f_que / f_udt), f_out: nn.Linear head, a DuelingLayer (the caller checks
    ``dueling_supported``) or a NoisyLinear in any of its modes (agents/heads.py: "off" is the plain head on its means).  Returns (q, h').
    ``stacked`` = (Wp, bp) built WITH autograd history when no GRAD_SINK will collect the weight gradients."""
    M, K = comm._msg_size, comm._key_size
    Wp, bp = stacked if stacked is not None else comm.fused_projection()
    off, src = g.talk_csc()
    cell = comm.f_udt
    dueling = hasattr(f_out, "adv_head")
    head_params = dueling_params(f_out) if dueling else (f_out.weight, f_out.bias)
    noisy_mode = getattr(f_out, "noisy_mode", "off")
    fold = f_out.fold() if noisy_mode == "shared" else None     # this update's draw: (W_eff, b_eff) stand in for the plain head's pair
    env = _talk_env(g, M, K)
    t_off, t_dst, t_pos = ((None, None, None) if env is not None else
                           _talk_transpose_if_needed(g, x, h, Wp, cell.weight_ih, head_params[0]))
    H = cell.weight_hh.shape[1]
    params = {"W_ih": cell.weight_ih, "b_ih": cell.bias_ih, "W_hh": cell.weight_hh, "b_hh": cell.bias_hh}
    if not dueling:
        params["W_out"], params["b_out"] = head_params

    def split(name, grad, col0):
        """flush target of the sink: distribute an accumulated gradient to the module's parameters."""
        if name == "Wp":        # rows: f_val | f_sign | f_que ; columns col0 .. col0 + grad.shape[1]
            r = 0
            for lin in (comm.f_val, comm.f_sign, comm.f_que):
                rows = lin.weight.shape[0]
                if lin.weight.grad is None:
                    lin.weight.grad = th.zeros_like(lin.weight)
                lin.weight.grad[:, col0:col0 + grad.shape[1]].add_(grad[r:r + rows])
                r += rows
        elif name == "bp":
            r = 0
            for lin in (comm.f_val, comm.f_sign, comm.f_que):
                rows = lin.bias.shape[0]
                _add_grad(lin.bias, grad[r:r + rows])
                r += rows
        elif name == "b_ih":    # its r and z columns are b_hh's too (see _TarmacStep.backward)
            _add_grad(params["b_ih"], grad)
            _add_grad_cols(params["b_hh"], grad[:2 * H], 0)
        elif name == "b_hh":    # the n block
            _add_grad_cols(params["b_hh"], grad, col0)
        elif dueling and name in ("W_out", "b_out"):     # they hold d W_eff = dq^T h' / d b_eff = colsum(dq): C G | 1^T G, C g | 1^T g
            Wa, ba, wv, bv = head_params
            if name == "W_out":
                dWa, _, dwv, _ = dueling_split(grad, None)
                _add_grad(Wa, dWa)
                _add_grad(wv, dwv)
            else:
                _, dba, _, dbv = dueling_split(None, grad)
                _add_grad(ba, dba)
                _add_grad(bv, dbv)
        elif fold is not None and name in ("W_out", "b_out"):
            # d W_eff / d b_eff of THIS fold (the slot is keyed by it): the means' gradients as they are; the sigmas' are those times the
            # fold's noise - one launch once both halves are in
            _add_grad(params[name], grad)
            if fold.done:
                dWs, dbs = noisy_fold_bwd(grad if name == "W_out" else None, grad if name == "b_out" else None, fold.f_in, fold.f_out)
            else:
                fold.pending[name] = grad if name not in fold.pending else fold.pending[name] + grad
                if len(fold.pending) < 2:
                    return
                dWs, dbs = noisy_fold_bwd(fold.pending.pop("W_out"), fold.pending.pop("b_out"), fold.f_in, fold.f_out)
                fold.done = True
            _add_grad(f_out.weight_sigma, dWs)
            _add_grad(f_out.bias_sigma, dbs)
        else:
            _add_grad(params[name], grad)

    # ANY differentiable input (a trainable Q head over a frozen encoder / GRU included) makes autograd run the backward,
    # which reads the saved pre-activation sets
    train = th.is_grad_enabled() and any(t.requires_grad for t in (x, h, Wp, bp, cell.weight_ih, cell.bias_ih,
                                                                   cell.weight_hh, cell.bias_hh) + tuple(head_params))
    duel = noisy = None
    if noisy_mode == "rows":
        if train:
            raise L.UavGnnError("tarmac_step: the noisy head's mode 'rows' is the no-grad rollout form; an update runs in mode 'shared'")
        W_out, b_out = head_params
        noisy = ("rows", f_out.weight_sigma.detach(), f_out.bias_sigma.detach(), f_out.rng())
    elif fold is not None:
        if stacked is not None:     # no sink: autograd carries the gradients of the fold back to the four parameters
            W_out, b_out = fold.W, fold.b
        else:
            W_out, b_out = fold.W.detach(), fold.b.detach()
            noisy = ("shared", id(fold))
    elif not dueling:
        W_out, b_out = head_params
    else:
        Wa, ba, wv, bv = head_params
        duel = (Wa.detach(), ba.detach(), wv.detach(), bv.detach(), id(Wa))
        if stacked is not None:     # no sink: autograd splits the gradients of the fold back to the four parameters
            W_out, b_out = dueling_fold(Wa, ba, wv, bv)
        else:                       # (a no-grad call has no backward: nothing reads W_out then)
            W_out, b_out = (_duel_weff(Wa, wv) if train else duel[0]), duel[1]
    out = _TarmacStep.apply(x, h, Wp, bp, cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, W_out, b_out, M, K, off, src, t_off,
                            t_dst, t_pos, split, env, dx_out, train, duel, noisy)
    if noisy_mode == "rows":
        noisy[3][1:].add_(1)        # one launch consumed one step
    return out


class _DiscComm(th.autograd.Function):
    """K5.  Hard Gumbel-softmax messages (straight-through) + OR (max) aggregation of DiscreteComm."""

    @staticmethod
    def forward(ctx, logits, gumbel, talk_off, talk_src, t_off, t_dst, t_pos, inv_tau, rng=None):
        L.require_gpu(logits, gumbel, talk_off, talk_src, rng)
        logits = L.f32c(logits)
        N, M2 = logits.shape
        M = M2 // 2
        E = talk_src.shape[0]
        if gumbel is not None:
            gumbel = L.f32c(gumbel)
            if gumbel.numel() != E * M2:
                raise L.UavGnnError(f"disc_comm: gumbel noise must be [E={E}, msg={M}, 2]")
        elif rng is None or rng.dtype != th.int64 or rng.numel() != 2:
            raise L.UavGnnError("disc_comm: either the Gumbel noise or a device int64 {seed, step} pair is required")
        c = th.empty((N, M2), dtype=th.float32, device=logits.device)
        y0 = th.empty((max(E, 1), M), dtype=th.float32, device=logits.device)
        sel = th.empty((N, M2), dtype=th.int32, device=logits.device)
        with KERNEL_TIMER.span("disc_comm_fwd"):
            rc = L.lib().uavgnn_disc_comm_fwd(logits.data_ptr(), M2, L.ptr(gumbel), L.ptr(rng), M, L.ptr(talk_off),
                                              L.ptr(talk_src), N, float(inv_tau), c.data_ptr(), M2, y0.data_ptr(),
                                              sel.data_ptr(), L.stream())
        L.check(rc, "uavgnn_disc_comm_fwd")
        ctx.inv_tau, ctx.M = float(inv_tau), M
        ctx.save_for_backward(y0, sel, t_off, t_dst, t_pos)
        return c

    @staticmethod
    def backward(ctx, d_c):
        y0, sel, t_off, t_dst, t_pos = ctx.saved_tensors
        d_c = L.f32c(d_c)
        N = d_c.shape[0]
        d_logits = th.empty_like(d_c)
        with KERNEL_TIMER.span("disc_comm_bwd"):
            rc = L.lib().uavgnn_disc_comm_bwd(d_c.data_ptr(), d_c.stride(0), y0.data_ptr(), sel.data_ptr(), ctx.M,
                                              L.ptr(t_off), L.ptr(t_dst), L.ptr(t_pos), N, ctx.inv_tau,
                                              d_logits.data_ptr(), d_logits.stride(0), L.stream())
        L.check(rc, "uavgnn_disc_comm_bwd")
        return d_logits, None, None, None, None, None, None, None, None


def disc_comm_aggregate(logits, gumbel, g, tau=0.5, rng=None):
    """Hard Gumbel-softmax messages + OR aggregation of DiscreteComm (gnn_agents.py:166-178).  logits [N, 2*msg] per
    source node; gumbel [E, msg, 2] in CSC order, or None with rng = device int64 {seed, step}: the noise is drawn inside
    the kernel (counter-based Philox keyed by the seed, counter = (CSC position, channel, step))."""
    off, src = g.talk_csc()
    t_off, t_dst, t_pos = _talk_transpose_if_needed(g, logits)
    return _DiscComm.apply(logits, gumbel, off, src, t_off, t_dst, t_pos, 1.0 / tau, rng)


def gumbel_noise(rng, E, msg):
    """The [E, msg, 2] noise tensor the in-kernel generator of K5 draws for rng = {seed, step} (tests)."""
    out = th.empty((E, msg, 2), dtype=th.float32, device=rng.device)
    L.check(L.lib().uavgnn_gumbel_noise(rng.data_ptr(), E, msg, out.data_ptr(), L.stream()), "uavgnn_gumbel_noise")
    return out

/*
 * uavgnn.h - C ABI of the MI355X-native hetero-GNN hot path (libuavgnn.so, gfx950 only).
 *
 * Drop-in boundary for the graph arithmetic that zhangxiaochen95/uav_bs_ctrl's MADRQN agent runs through DGL 0.9.0
 * (reference: algos/madrqn/agents/gnn_agents.py).  Every entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - All functions return 0 on success, a negative UAVGNN_E* code on argument errors, or the NEGATED hipError_t of a
 *     failed launch.  Nothing is thrown across this boundary.
 *   - All pointers are DEVICE pointers owned by the caller (PyTorch allocates every tensor incl. workspaces; the
 *     library allocates nothing and keeps no mutable global state; calls on distinct streams are independent).
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Launches are asynchronous and capturable
 *     into a hipGraph.
 *   - Matrices are row-major fp32; `ld*` is the leading dimension in elements; offsets/indices are int32.
 *   - Relation layout (the layout the reference's graph builder emits, algos/madrqn/utils/env_wrappers.py:69-89):
 *     edges of `seen`/`near` are grouped by destination and src id == edge id, so a relation is x_src[E,F] plus
 *     seg_off[N+1].  `talk` is given twice: CSC (in-edges per destination) and its transpose (out-edges per source,
 *     with the CSC position of each edge) so that the backward is a pure gather (deterministic, no float atomics).
 */
#ifndef UAVGNN_H
#define UAVGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVGNN_VERSION 101 /* 0.1.1 */

#define UAVGNN_EINVAL (-1000)      /* null pointer / non-positive size */
#define UAVGNN_EUNSUPPORTED (-1001) /* shape outside the compiled instantiations */
#define UAVGNN_EWORKSPACE (-1002)   /* workspace too small */

typedef void* uavgnn_stream_t;

int uavgnn_version(void);

/* Human-readable text for a return code of this library (static storage). */
const char* uavgnn_strerror(int code);

/* ------------------------------------------------------------------------------------------------------------------
 * K1  GATv2 relation, forward.
 * Replaces dglnn.GATv2Conv((F_src,F_dst), D, nh, residual=True, allow_zero_in_degree=True, activation=ReLU).forward
 * as constructed at gnn_agents.py:93-96 and called at :103-104 (and drqn/agents/gnn_agents.py:17-18,:27).
 *   el = W_s x_u + b_s ; er = W_d x_v + b_d ; e = attn . lrelu_slope(el+er) per head ; a = softmax over in-edges ;
 *   out[v] = ReLU( sum_u a el[u] + W_r x_v + b_r )            
 * x_src[E,F_src] (E = seg_off[N], also used to pick the schedule for sparse batches), x_dst[N,F_dst], seg_off[N+1]; W_s[H,F_src] b_s[H] W_d[H,F_dst] b_d[H] attn[H] W_r[H,F_dst]
 * b_r[H] (b_r may be NULL = zeros), H = nh*D.  out is written at out[v*ld_out + 0..H) (so two relations can share one
 * [N,2H] buffer = the th.cat of gnn_agents.py:106).  attn_save[E,nh] (may be NULL) receives the softmax weights for
 * the backward.  dst_order[N] (may be NULL = identity) is the order in which destinations are handed to the persistent
 * wavefronts; passing the destinations sorted by decreasing degree balances ragged batches (longest-first).  It only
 * affects scheduling, never results.  Supported: F_src in {2,4}, F_dst == 2, H <= 256, D in {8,16,32,64}.
 */
int uavgnn_gatv2_fwd(const float* x_src, int E, int F_src, const float* x_dst, int F_dst, const int32_t* seg_off,
                     const int32_t* dst_order, int N, const float* W_s, const float* b_s, const float* W_d, const float* b_d, const float* attn,
                     const float* W_r, const float* b_r, int nh, int D, float slope, float* out, int ld_out,
                     float* attn_save, uavgnn_stream_t stream);

/* uavgnn_gatv2_fwd picks the kernel: nh == 4, D in {16,32,64}: the low-degree kernel for two-feature relations whose
 * mean in-degree is <= 8 (`near`), else the fp32-MFMA row-tile kernel; any other (nh, D): the plain-VALU kernel.
 * Same contract, fixed kernel, exported as in-library A/B references: _valu = always the VALU kernel,
 * _mfma = the MFMA kernel whenever it is instantiated (never the low-degree kernel). */
int uavgnn_gatv2_fwd_valu(const float* x_src, int E, int F_src, const float* x_dst, int F_dst, const int32_t* seg_off,
                          const int32_t* dst_order, int N, const float* W_s, const float* b_s, const float* W_d, const float* b_d, const float* attn,
                          const float* W_r, const float* b_r, int nh, int D, float slope, float* out, int ld_out,
                          float* attn_save, uavgnn_stream_t stream);
int uavgnn_gatv2_fwd_mfma(const float* x_src, int E, int F_src, const float* x_dst, int F_dst, const int32_t* seg_off,
                          const int32_t* dst_order, int N, const float* W_s, const float* b_s, const float* W_d, const float* b_d, const float* attn,
                          const float* W_r, const float* b_r, int nh, int D, float slope, float* out, int ld_out,
                          float* attn_save, uavgnn_stream_t stream);

/* K1 forward, BOTH relations of GraphObservationEncoder.forward in ONE launch (reference: the two GATv2Conv calls and the
 * th.cat of algos/madrqn/agents/gnn_agents.py:103-106).  `seen` (x_gt [E_seen,4], seen_off, optional hand-out order
 * seen_order) fills out[:, 0:H), `near` (x_ubs [E_near,2], near_off) fills out[:, H:2H); ld_out >= 2H, 16-byte aligned.
 * seen_params / near_params: HOST arrays of 7 device pointers each, in DGL's GATv2Conv layout
 * {fc_src.weight, fc_src.bias, fc_dst.weight, fc_dst.bias, attn, res_fc.weight, res_fc.bias (may be NULL)}, 16-byte
 * aligned.  attn_save_* as in uavgnn_gatv2_fwd (NULL for inference).  `seen` runs on 16-edge MFMA row tiles per
 * destination, `near` packs two destinations per row tile with [x_u ; x_v] in the K = 4 contraction (any in-degree is
 * correct; <= 8 is one pass).  uavgnn_gatv2_hetero_supported: 1 when (F_seen, F_near, F_dst, nh, D) = (4, 2, 2, 4, 64),
 * else callers use uavgnn_gatv2_fwd per relation (same results up to summation order). */
int uavgnn_gatv2_hetero_supported(int F_seen, int F_near, int F_dst, int nh, int D);
int uavgnn_gatv2_hetero_fwd(const float* x_gt, int E_seen, const int32_t* seen_off, const int32_t* seen_order,
                            const float* x_ubs, int E_near, const int32_t* near_off, const float* x_dst, int N,
                            const float* const* seen_params, const float* const* near_params, int nh, int D, float slope,
                            float* out, int ld_out, float* attn_save_seen, float* attn_save_near,
                            uavgnn_stream_t stream);
/* Same contract with only some phases of the kernel executed (bit 0: `seen` row tiles of the non-isolated destinations,
 * bit 1: `near` + residual-only `seen` rows); phases = 3 is uavgnn_gatv2_hetero_fwd.  In-library ablation reference for
 * benchmarks - output rows of the skipped phase are left untouched.  Bit 8 (256): the score GEMM of both phases on fp32 MFMA
 * (csrc/gatv2_hetero_f32.hip) instead of the bf16 matrix cores with exact three-way operand splits - same results to fp32
 * rounding; the A/B reference and the strict-fp32 leg of bench.py. */
int uavgnn_gatv2_hetero_fwd_phases(const float* x_gt, int E_seen, const int32_t* seen_off, const int32_t* seen_order,
                                   const float* x_ubs, int E_near, const int32_t* near_off, const float* x_dst, int N,
                                   const float* const* seen_params, const float* const* near_params, int nh, int D,
                                   float slope, float* out, int ld_out, float* attn_save_seen, float* attn_save_near,
                                   int phases, uavgnn_stream_t stream);
/* Prepared parameters.  Every workgroup of the forward kernel first turns the parameters of the two modules into the image its
 * LDS holds (bf16 three-way splits of the weight tiles, scaled attention vectors, attn x W_s sums: one memory round trip + ~200
 * VALU instructions per wavefront = 2.9 us of a 20-us rollout launch).  A caller whose parameters stay put over many launches - a
 * rollout between two optimiser steps, the target network between two syncs - builds the image ONCE (uavgnn_gatv2_hetero_prepare,
 * one workgroup) into a buffer of uavgnn_gatv2_hetero_image_bytes() bytes (16-byte aligned) and launches with
 * uavgnn_gatv2_hetero_fwd_image, whose workgroups only copy it.  Results are bit-identical to uavgnn_gatv2_hetero_fwd_phases
 * with the same `phases`.  The image is a function of the parameter VALUES and `slope`: the caller must rebuild it after any
 * parameter change (the library cannot tell).  seen_params / near_params are still required (argument checks, fp32-MFMA route). */
size_t uavgnn_gatv2_hetero_image_bytes(void);
int uavgnn_gatv2_hetero_prepare(const float* const* seen_params, const float* const* near_params, int nh, int D, float slope,
                                void* image, uavgnn_stream_t stream);
int uavgnn_gatv2_hetero_fwd_image(const float* x_gt, int E_seen, const int32_t* seen_off, const int32_t* seen_order,
                                  const float* x_ubs, int E_near, const int32_t* near_off, const float* x_dst, int N,
                                  const float* const* seen_params, const float* const* near_params, int nh, int D,
                                  float slope, const void* image, float* out, int ld_out, float* attn_save_seen,
                                  float* attn_save_near, int phases, uavgnn_stream_t stream);
/* uavgnn_gatv2_hetero_fwd_image (image may be NULL: the in-kernel prologue) that ALSO writes rowmax_near / rowmax_seen [N]: the maximum
 * over the `near` / the `seen` half of every output row (rows are >= 0 behind the ReLU; every element has exactly one writer:
 * deterministic) - the two row bounds uavgnn_gemm_nt_h2 takes for the f_aggr product behind a TIME-BATCHED launch (gnn_agents.py:106).
 * Costs +9 % on a time-batched launch and +1.9 us on a 20-us rollout launch (why the rollout does not use it).  Not with the fp32-MFMA
 * build (phases bit 8): UAVGNN_EUNSUPPORTED. */
int uavgnn_gatv2_hetero_fwd_rowmax(const float* x_gt, int E_seen, const int32_t* seen_off, const int32_t* seen_order,
                                   const float* x_ubs, int E_near, const int32_t* near_off, const float* x_dst, int N,
                                   const float* const* seen_params, const float* const* near_params, int nh, int D, float slope,
                                   const void* image, float* out, int ld_out, float* attn_save_seen, float* attn_save_near,
                                   float* rowmax_near, float* rowmax_seen, int phases, uavgnn_stream_t stream);

/* K1 backward: parameter gradients only (observations are leaves: the reference never needs d/dx, Appendix A.4).
 * out / d_out are the forward output and its gradient (same ld).  Gradients are OVERWRITTEN.  Deterministic: per
 * workgroup partials in `workspace` are combined in a fixed order by a second launch (no float atomics).
 * workspace >= uavgnn_gatv2_bwd_workspace_bytes(F_src, nh*D). */
size_t uavgnn_gatv2_bwd_workspace_bytes(int F_src, int H);
int uavgnn_gatv2_bwd(const float* x_src, int E, int F_src, const float* x_dst, int F_dst, const int32_t* seg_off,
                     const int32_t* dst_order, int N, const float* W_s, const float* b_s, const float* W_d, const float* b_d, const float* attn,
                     int nh, int D, float slope, const float* out, const float* d_out, int ld_out,
                     const float* attn_save, float* dW_s, float* db_s, float* dW_d, float* db_d, float* dattn,
                     float* dW_r, float* db_r, void* workspace, size_t workspace_bytes, uavgnn_stream_t stream);
/* Same contract, generic kernel only (one destination per wavefront).  uavgnn_gatv2_bwd itself picks the
 * pair-of-destinations kernel for two-feature relations with mean in-degree <= 8 (`near`): in-library A/B reference. */
int uavgnn_gatv2_bwd_generic(const float* x_src, int E, int F_src, const float* x_dst, int F_dst, const int32_t* seg_off,
                     const int32_t* dst_order, int N, const float* W_s, const float* b_s, const float* W_d, const float* b_d, const float* attn,
                     int nh, int D, float slope, const float* out, const float* d_out, int ld_out,
                     const float* attn_save, float* dW_s, float* db_s, float* dW_d, float* db_d, float* dattn,
                     float* dW_r, float* db_r, void* workspace, size_t workspace_bytes, uavgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K3b  Targeted attention over the talk relation, forward.
 * Replaces g.apply_edges(fn.u_dot_v('s','q','e')); e/key_size; edge_softmax; update_all(u_mul_e('v','a'), sum)
 * (gnn_agents.py:261-267).   e_uv = <s_u, q_v> * scale ; a = softmax over in-edges of v ; c_v = sum_u a_uv v_u.
 * s,q: [N,K] rows with leading dims ld_s/ld_q, v: [N,M] ld_v (they may be column slices of one projection buffer).
 * talk_off[N+1], talk_src[E] = CSC.  c[N,M] (ld_c) is overwritten (zero for nodes without in-edges);
 * a_save[E] receives the attention weights in CSC order.  K <= 64, M <= 256.
 * With s == q == NULL the attention is uniform: c = mean of in-neighbour rows (the UDF reduce `mailbox.mean(1)` of
 * BaseComm/CommNet, gnn_agents.py:130-133,:214-216).
 * x_copy (may be NULL): when given, row d of x_copy[N, n_copy] (ld_x) is also copied to the n_copy floats IN FRONT of
 * c[d, :] (i.e. c - n_copy + d*ld_c), so that one pass leaves the GRU input [x || c] of gnn_agents.py:270 in place
 * of a separate th.cat.
 */
int uavgnn_talk_attn_fwd(const float* s, int ld_s, const float* q, int ld_q, const float* v, int ld_v, int K, int M,
                         const int32_t* talk_off, const int32_t* talk_src, int N, float scale, float* c, int ld_c,
                         float* a_save, const float* x_copy, int ld_x, int n_copy, uavgnn_stream_t stream);

/* K3b backward.  d_c[N,M] -> d_s, d_q [N,K], d_v [N,M] (overwritten; any of d_s/d_q may be NULL in uniform mode).
 * t_off[N+1], t_dst[E], t_pos[E]: transpose of the CSC (out-edges of each source, destination of each, and the CSC
 * position of the edge).  de_tmp[E] is scratch. */
int uavgnn_talk_attn_bwd(const float* s, int ld_s, const float* q, int ld_q, const float* v, int ld_v, int K, int M,
                         const int32_t* talk_off, const int32_t* talk_src, const int32_t* t_off, const int32_t* t_dst,
                         const int32_t* t_pos, int N, float scale, const float* a_save, const float* d_c, int ld_dc,
                         float* d_s, int ld_ds, float* d_q, int ld_dq, float* d_v, int ld_dv, float* de_tmp,
                         uavgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K4  GRU cell gate math (the pointwise half of nn.GRUCell: gnn_agents.py:29,:123,:164,:208,:246,:282).
 * gi = W_ih i + b_ih, gh = W_hh h + b_hh are [N,3H] (gate order r,z,n);  h' = (1-z) n + z h.
 */
int uavgnn_gru_gates_fwd(const float* gi, const float* gh, const float* h, int N, int H, float* h_out,
                         uavgnn_stream_t stream);
int uavgnn_gru_gates_bwd(const float* gi, const float* gh, const float* h, const float* d_hout, int N, int H,
                         float* d_gi, float* d_gh, float* d_h, uavgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K5  DiscreteComm message passing (gnn_agents.py:166-178,:189): per edge F.gumbel_softmax(logits[src].view(msg,2),
 * tau, hard=True), per destination the element-wise max over in-edges.  The Gumbel noise is either given explicitly
 * (gumbel [E, msg, 2], CSC order: fixtures carrying the reference's own draws) or, with gumbel == NULL, drawn inside the
 * kernel: Philox4x32-10 keyed by the 64-bit seed rng[0], counter (CSC position, channel, step rng[1]), g = -log(-log(u));
 * rng is a DEVICE array {seed, step} (a captured graph replays with the current step; the caller advances it).
 * uavgnn_gumbel_noise writes that same stream as an [E, msg, 2] tensor (tests).  logits[N, 2*msg] (ld) are the
 * per-SOURCE-node encoder outputs.  c[N, 2*msg] is overwritten (zeros for nodes without in-edges); y0_save[E, msg] and
 * sel[N, 2*msg] (CSC position that owns each channel's gradient: the first in-edge whose hard bit is set, else the first
 * in-edge) feed the backward.
 */
int uavgnn_disc_comm_fwd(const float* logits, int ld, const float* gumbel, const long long* rng, int msg,
                         const int32_t* talk_off, const int32_t* talk_src, int N, float inv_tau, float* c, int ld_c,
                         float* y0_save, int32_t* sel, uavgnn_stream_t stream);
int uavgnn_gumbel_noise(const long long* rng, long long E, int msg, float* out, uavgnn_stream_t stream);
/* d_c[N, 2*msg] -> d_logits[N, 2*msg] (overwritten), straight-through estimator; gather over the transposed CSC. */
int uavgnn_disc_comm_bwd(const float* d_c, int ld_dc, const float* y0_save, const int32_t* sel, int msg,
                         const int32_t* t_off, const int32_t* t_dst, const int32_t* t_pos, int N, float inv_tau,
                         float* d_logits, int ld_dl, uavgnn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * f1  Device-side observation -> graph construction for a batch of environments (replaces the Python loops of
 * env_wrappers.py:65-89 build_obs_graph, :139-154 build_comm_graph and dgl.batch/merge :67,:137).
 * Padded observations: gt[N, M, 1+Fg], ubs[N, U, 1+Fu] with column 0 the visibility flag (mubs_cov.py:215-242),
 * N = B*n agent rows; d_u2u[B, n, n] pairwise UBS distances.  Two passes with a prefix sum (caller) in between:
 *   uavgnn_obs_degrees  -> deg_seen[N], deg_near[N]                         (counts of kept rows)
 *   uavgnn_obs_compact  -> x_gt[E_seen, Fg], x_ubs[E_near, Fu] given seen_off / near_off = exclusive scans
 *   uavgnn_talk_degrees -> deg_in[N] (in-degree of every agent), env_edges[B] (edges per environment)
 *   uavgnn_talk_compact -> talk_src[E], talk_eid[E] (CSC; eid = the edge id the reference's i-major loop assigns)
 *                          given talk_off = scan(deg_in) and env_base = scan(env_edges).
 * Kept rows keep the reference's order (ascending m / ascending source i).  Fg == 4, Fu == 2, n <= 64.
 */
int uavgnn_obs_degrees(const float* gt, int M, int Fg, const float* ubs, int U, int Fu, int N, int32_t* deg_seen,
                       int32_t* deg_near, uavgnn_stream_t stream);
int uavgnn_obs_compact(const float* gt, int M, int Fg, const float* ubs, int U, int Fu, int N, const int32_t* seen_off,
                       const int32_t* near_off, float* x_gt, float* x_ubs, uavgnn_stream_t stream);
int uavgnn_talk_degrees(const float* d_u2u, int n, int B, float r_comm, int32_t* deg_in, int32_t* env_edges,
                        uavgnn_stream_t stream);
int uavgnn_talk_compact(const float* d_u2u, int n, int B, float r_comm, const int32_t* talk_off,
                        const int32_t* env_base, int32_t* talk_src, int32_t* talk_eid, uavgnn_stream_t stream);
/* The prefix sums between the two passes, up to four arrays in one launch: o_k[0] = 0, o_k[i + 1] = d_k[0] + ... + d_k[i]
 * (o_k has n_k + 1 entries; o_k == NULL skips the array).  Replaces torch.cumsum + fills in the device builder. */
int uavgnn_offsets_scan4(const int32_t* d0, int n0, int32_t* o0, const int32_t* d1, int n1, int32_t* o1, const int32_t* d2,
                         int n2, int32_t* o2, const int32_t* d3, int n3, int32_t* o3, uavgnn_stream_t stream);

/* ---- rollout: epsilon-greedy selection --------------------------------------------------------------------------
 * acts[a] = u_team[a / n_agents] <= eps ? min(floor(u_agent[a] * A), A - 1) : argmax_j q[a, j]   (first maximum).
 * MultiAgentQLearner.act, learner.py:73-80: one exploration draw per team of n_agents consecutive agents; u_team
 * [N / n_agents] and u_agent [N] are uniforms in [0, 1) supplied by the caller.  acts: int64 [N].
 */
int uavgnn_eps_greedy(const float* q, int ld_q, int N, int A, int n_agents, const float* u_team, const float* u_agent,
                      float eps, long long* acts, uavgnn_stream_t stream);
/* Same with the exploration rate read from DEVICE memory (*eps_dev) at execution time, so that a hipGraph captured around
 * the rollout step replays with the current epsilon of the schedule (algos/madrqn/run.py:60-61). */
int uavgnn_eps_greedy_dev(const float* q, int ld_q, int N, int A, int n_agents, const float* u_team, const float* u_agent,
                          const float* eps_dev, long long* acts, uavgnn_stream_t stream);
/* The schedule itself on the device (run.py:61): *eps = (float) max(eps_end, eps_start - (eps_start - eps_end) / decay_steps * *t),
 * evaluated in double without contraction, then *t += inc.  t: DEVICE int64 counting environment interactions; eps: the word
 * uavgnn_eps_greedy_dev reads.  One thread, no host synchronisation.  decay_steps <= 0: UAVGNN_EINVAL. */
int uavgnn_eps_schedule(long long* t, long long inc, double eps_start, double eps_end, double decay_steps, float* eps,
                        uavgnn_stream_t stream);

/* ---- evaluation episodes and epoch statistics (csrc/eval_stats.hip; reference: algos/madrqn/run.py:63-74, :115-127) ----------------
 * _eps_greedy_philox: the selection rule of uavgnn_eps_greedy - first maximum wins, one exploration draw per team of n_agents
 *   consecutive rows, r = min(floor(u * A), A - 1) with the product formed in float - with the uniforms drawn INSIDE the kernel, so an
 *   evaluation never touches the host's generator and captures into a hipGraph.  rng: DEVICE int64 {seed, step}.
 *     w(index, lane) = first output word of Philox4x32-10 (csrc/common.h) at counter (index, lane, step low word, step high word)
 *                      under the key (seed low word, seed high word) - the keying of uavgnn_replay_sample;
 *     u(index, lane) = (w >> 8) * 2^-24, an exact float in [0, 1);
 *     explore(team)  = u(team, 0) <= eps                       lane 0, index = team: the exploration draw;
 *     acts[a]        = explore(a / n_agents) ? min((int)(u(a, 1) * A), A - 1) : argmax_j q[a, j]     lane 1, index = row: the random action.
 *   eps is *eps_dev (DEVICE, read at execution time) or, when eps_dev == NULL, the host value `eps`.  After the call, in stream order,
 *   rng[1] = step + 1: written by a following one-thread launch, so no thread of the selection observes it.  The result depends on
 *   (seed, step, q, N, A, n_agents, eps) only, never on the launch geometry.  UAVGNN_EINVAL for the argument errors of uavgnn_eps_greedy
 *   (N < 0, A < 1, n_agents < 1, ld_q < A, q or acts NULL with N > 0) or rng == NULL; N == 0 launches no selection and still advances
 *   the step.
 * _stats_push: streaming mean / M2 / min / max of n_keys <= 16 keys in one launch, one workgroup per key.  vals: DEVICE double
 *   [n_keys, ld], the first n values of every row are pushed; acc: DEVICE double [n_keys, 6] = {count, mean, M2, min, max, non-finite
 *   count}, empty state {0, 0, 0, +inf, -inf, 0}.  Non-finite values are left out of the moments and of min / max and counted in
 *   field 5; with n_b finite values of mean mean_b = sum / n_b and M2_b = sum (v - mean_b)^2 (two passes, all in double):
 *     d = mean_b - mean, n' = count + n_b;  mean += d n_b / n';  M2 += M2_b + d^2 count n_b / n';  count = n';  min / max updated.
 *   n_b == 0 (every value non-finite) changes field 5 only.  The reduction order is fixed: the accumulator's bits depend on the
 *   sequence of pushes only.  n == 0: no-op.  n < 0, n_keys outside 1..16, ld < n or a NULL pointer: UAVGNN_EINVAL.  No atomics. */
int uavgnn_eps_greedy_philox(const float* q, int ld_q, int N, int A, int n_agents, long long* rng, const float* eps_dev, float eps,
                             long long* acts, uavgnn_stream_t stream);
int uavgnn_stats_push(const double* vals, int ld, int n, int n_keys, double* acc, uavgnn_stream_t stream);

/* ---- trajectory films of the evaluation simulators (csrc/film.hip; reference: envs/mubs_cov/mubs_cov.py:99-100 reload, :126-127
 * click; envs/subs_cov/subs_cov.py:87-88 reload, :128-131 click; the two recorder.py; read back by algos/madrqn/run.py:73-74 and
 * :132-178 and their algos/drqn twins) ------------------------------------------------------------------------------------------------
 * ONE launch records the current step of all B environments of a simulator into a film of `episodes` episodes of T = episode_limit
 * steps.  Environment b writes slot t[b] of episode e = episode_base + b; t is the simulator's DEVICE step counter (int32: 0 after a
 * reset, k after the k-th step) and episode_base the only host integer, so the call captures into a hipGraph and follows the simulator.
 *   slot 0:       film_pos_ubs[e, 0] <- pos_ubs[b] and film_pos_gts[e] <- pos_gts[b]                  (the recorder's `reload`)
 *   slot k >= 1:  film_pos_ubs[e, k] <- pos_ubs[b] and element k - 1 of every per-step series         (the recorder's `click`)
 * _mubs: film_pos_ubs [episodes, T+1, n, 2] f64; film_fair_idx [episodes, T] f64 <- (double) run_f32[b, 2]; film_reward [episodes, T]
 *   f64 <- (reward[b, 0] + ... + reward[b, n-1]) / n, added in agent order in double (mubs_cov.py:127 reward.mean()); film_pos_gts
 *   [episodes, M, 2] f32.  pos_ubs [B, n, 2] f64, pos_gts [B, M, 2] f32, run_f32 [B, 4], reward [B, n] f64: the simulator's buffers.
 * _subs: film_pos_ubs [episodes, T+1, 2] f64; film_total_throughput / film_fair_idx / film_global_utility [episodes, T] f64 <-
 *   run_f64[b, 0] / [b, 2] / [b, 3]; film_reward [episodes, T] f64 <- reward[b]; film_rate_per_gt [episodes, T, M] f32 <- rate_per_gt[b];
 *   film_velocity [episodes, T] f64 <- hypot(avail_moves[actions[b]]) / dt in double (subs_cov.py:131); film_pos_gts [episodes, M, 2]
 *   f32.  actions [B] int64: the actions of the step just taken; NULL for the call after a reset.  avail_moves [A, 2] f64.
 * status: DEVICE int32 error bits, OR-ed in and never cleared by a kernel.  Bit 0: an environment whose t[b] is outside 0 .. T or
 *   whose episode is outside 0 .. episodes - 1 - and, for _subs, a step slot recorded with actions == NULL or with an action outside
 *   0 .. A - 1 - wrote NOTHING.  No store leaves the film.  Plain vector stores; the OR into status is the only atomic.
 * UAVGNN_EINVAL before any launch: a NULL pointer (actions excepted; the GT and rate pointers only when M > 0), B < 0, n < 1, M < 0,
 *   T < 1, A < 1, dt <= 0, episodes < 0, episode_base < 0.  B == 0: no launch. */
int uavgnn_film_click_mubs(int B, int n, int M, int T, int episodes, int episode_base, const int32_t* t, const double* pos_ubs,
                           const float* pos_gts, const float* run_f32, const double* reward, double* film_pos_ubs,
                           double* film_fair_idx, double* film_reward, float* film_pos_gts, int32_t* status, uavgnn_stream_t stream);
int uavgnn_film_click_subs(int B, int M, int T, int A, double dt, int episodes, int episode_base, const int32_t* t,
                           const long long* actions, const double* avail_moves, const double* pos_ubs, const float* pos_gts,
                           const double* run_f64, const double* reward, const float* rate_per_gt, double* film_pos_ubs,
                           double* film_total_throughput, double* film_fair_idx, double* film_global_utility, double* film_reward,
                           float* film_rate_per_gt, double* film_velocity, float* film_pos_gts, int32_t* status,
                           uavgnn_stream_t stream);

/* ---- device-resident replay state (csrc/replay.hip; reference: algos/madrqn/buffer.py:18-39) ------------------------
 * state: DEVICE int64 {head, size}; rng: DEVICE int64 {seed, draws}; status: DEVICE int32 error bits, OR-ed in and never cleared by a
 * kernel (bit 0: a sample asked for more sequences than the ring holds).  Every entry takes the stream, allocates nothing and
 * never synchronises with the host, so all of them capture into a hipGraph and replay with the CURRENT counters.
 *
 * _commit: the E sequences under construction go to ring slots (head + e) % capacity, every field in one launch; a second
 *   one-thread launch then sets head = (head + E) % capacity and size = min(size + E, capacity).  fields: HOST int64
 *   [n_fields, 3] = {source base, destination base, bytes per sequence}; 16-byte accesses where the bytes and both bases are
 *   multiples of 16, else 4-byte (no multiple of 4: UAVGNN_EINVAL).  E > capacity: UAVGNN_EINVAL before any launch.  At most 16 fields.
 * _sample: idx [B] int64 = B distinct slots of [0, size), uniform without replacement, in ascending order, then draws += 1.
 *   Slot s is keyed by the first word of Philox4x32-10 at counter (s, 0, draws) and key seed; the B smallest (key, slot) pairs
 *   are taken (the rule is spelled out in csrc/replay.hip).  The result depends on (seed, draws, size, B) only.  size < B:
 *   status |= 1 and idx[i] = i % max(size, 1).  capacity <= 65536, else UAVGNN_EUNSUPPORTED.
 * _sample_wide (csrc/replay_wide.hip): the same draw - the same rule, so the same bits as _sample wherever both apply - for every
 *   capacity in [1, 2^30] (above: UAVGNN_EUNSUPPORTED; null pointers, negative sizes, a workspace that is not 16-byte aligned:
 *   UAVGNN_EINVAL).  One workgroup per _slots_per_workgroup() slots of the CAPACITY; seven launches (zero, four key-byte histograms,
 *   count, write) whose number and grids depend on capacity and B alone, never on the device-side size, ordered by the stream; integer
 *   arithmetic and 32-bit integer atomics only, so the result is the same bits run to run.  Workgroups whose chunk lies beyond size do
 *   nothing.  workspace: DEVICE memory of _workspace_bytes(capacity) bytes (<= 0: capacity < 1 or above the limit; 8.2 KB + 8 B per
 *   workgroup), owned by the caller at a fixed address; the call does not depend on its contents at entry (its first launch writes what
 *   the later ones read) and carries nothing to the next draw.  rng[1] is advanced once, by one thread of the last launch; status is
 *   only OR-ed; idx[0 .. B) is written and nothing else.  B == 0: draws += 1, nothing written.
 * _gather: one launch moves every field of the B sampled sequences into time-major buffers: slab_bytes bytes at
 *   src + idx[b] src_seq_stride + t slab_bytes -> dst + t dst_step_stride + b slab_bytes for t < steps.  fields: HOST int64
 *   [n_fields, 7] = {source base, destination base, slab_bytes, steps, src_seq_stride, dst_step_stride, sequences in the ring};
 *   idx may hold repeats and is clamped into the ring.  Same two access widths as _commit.  At most 16 fields, B <= 65535. */
int uavgnn_replay_commit(const long long* fields, int n_fields, int E, int capacity, long long* state, uavgnn_stream_t stream);
int uavgnn_replay_sample(const long long* state, long long* rng, int capacity, int B, long long* idx, int32_t* status,
                         uavgnn_stream_t stream);
long long uavgnn_replay_sample_wide_workspace_bytes(int capacity);   /* host only */
int uavgnn_replay_sample_wide_slots_per_workgroup(void);             /* host only */
int uavgnn_replay_sample_wide(const long long* state, long long* rng, int capacity, int B, long long* idx, int32_t* status,
                              void* workspace, uavgnn_stream_t stream);
int uavgnn_replay_gather(const long long* fields, int n_fields, const long long* idx, int B, uavgnn_stream_t stream);

/* ---- prioritised sequence replay (csrc/replay_prio.hip; Schaul et al. ICLR'16, proportional variant, over sequences) ----------------
 * prio: DEVICE uint32 [capacity], one FIXED-POINT priority per ring slot, 2^20 = 1.0; prio_max: DEVICE uint32 [1], the running maximum,
 * initialised by the caller to 2^20.  state / rng / status as above; status bit 1: a priority update was skipped.  Every entry takes
 * the stream, allocates nothing and never synchronises with the host; the number and grids of its launches depend on (capacity, B, T,
 * C) only, never on the device-side size, so all of them capture into a hipGraph and replay with the CURRENT counters.  capacity <=
 * 2^30 and B <= 65535, else UAVGNN_EUNSUPPORTED; null pointers, non-positive extents, NaN parameters: UAVGNN_EINVAL.
 *
 * _prio_commit: prio[(head + e) % capacity] = *prio_max for e < E.  Call it BEFORE uavgnn_replay_commit, which advances head.
 * _prio_sample: stratified proportional sampling with replacement, integer arithmetic only in every decision.  THE RULE:
 *   S = sum of prio[s] over s < size (64 bits; slots at or beyond size are never read into a decision).  With S = qB B + rB, stratum k
 *   is [lo_k, hi_k), lo_k = k qB + (k rB) / B, hi_k = lo_{k+1}.  r_k = words 0 and 1 (low word first) of Philox4x32-10 at counter
 *   (k, 1, draws_lo, draws_hi) under key (seed_lo, seed_hi); target_k = lo_k + (hi_k > lo_k ? r_k mod (hi_k - lo_k) : 0); idx[k] = the
 *   slot s with prefix[s] <= target_k < prefix[s] + prio[s], prefix the exclusive prefix sum over s < size - ascending, repeats
 *   possible.  weights[k] = (float) (w_k / max_j w_j) with w_k = pow((double) size * prio[idx[k]] / (double) S, -beta) in double.
 *   Then draws += 1.  size == 0 (or S == 0): status |= 1, idx[k] = 0, weights[k] = 1, draws += 1.  1 <= B; 0 <= beta <= 16 (every
 *   power stays finite in double), else UAVGNN_EINVAL.  Four launches (chunk sums
 *   over one workgroup per 4096 slots of the CAPACITY, scan and targets, one wavefront per sample, weights).
 *   workspace: DEVICE memory of _prio_workspace_bytes(capacity, B) bytes (0: an argument out of range), 16-byte aligned, owned by the
 *   caller at a fixed address; the call does not depend on its contents at entry and carries nothing to the next call.
 * _prio_update: td [T, B, C] float32 contiguous, idx [B] int64 ascending (a draw of _prio_sample).  For every b, in double:
 *   a = eta max|td[:, b, :]| + (1 - eta) mean|td[:, b, :]|,  q = clamp(llrint(pow(a + eps, alpha) 2^20), 1, 2^32 - 1)  (alpha == 1:
 *   a + eps itself), prio[idx[b]] = q, *prio_max = max(*prio_max, q).  Of a run of equal indices only the LAST row stores its q (every
 *   valid row enters the maximum).  A non-finite a or an index outside [0, capacity) writes nothing and ORs status bit 1.  One launch;
 *   B == 0: none. */
long long uavgnn_replay_prio_workspace_bytes(int capacity, int B);   /* host only */
int uavgnn_replay_prio_commit(const long long* state, int E, int capacity, uint32_t* prio, const uint32_t* prio_max,
                              uavgnn_stream_t stream);
int uavgnn_replay_prio_sample(const long long* state, long long* rng, int capacity, int B, const uint32_t* prio, double beta,
                              long long* idx, float* weights, int32_t* status, void* workspace, uavgnn_stream_t stream);
int uavgnn_replay_prio_update(const float* td, int T, int B, int C, const long long* idx, int capacity, double alpha, double eta,
                              double eps, uint32_t* prio, uint32_t* prio_max, int32_t* status, uavgnn_stream_t stream);

/* ---- compact replay ring: observations rebuilt from simulator state (csrc/replay_rebuild.hip) -----------------------
 * The padded observations and the global state of B sampled sequences, written TIME-MAJOR as the update's buffers hold them, from
 * the four arrays the multi-UBS simulator computes them from (reference: envs/mubs_cov/mubs_cov.py:212-297 get_obs / get_state; the
 * batch of algos/madrqn/learner.py:99-116): ring fields pos_ubs [n_seq, steps, n, 2] f64, rate / avg [n_seq, steps, M] f32
 * (rate_per_gt and avg_rate AFTER the step's update), pos_gts [n_seq, M, 2] f32 (constant within a sequence).  For step t < steps
 * and row b < B, with s = idx[b] clamped into [0, n_seq) as uavgnn_replay_gather clamps:
 *   obs_gt [steps, B, n, M, Sg], obs_ubs [steps, B, n, n-1, 3], obs_agent [steps, B, n, 2], d_u2u [steps, B, n, n] (may be NULL),
 *   state [steps, B, uavgnn_env_state_dim] (may be NULL)
 * hold the BITS uavgnn_env_step wrote for that state: the same operations in the same types (float64 norms rounded to float32,
 * visibility by d <= float(r_sns) / float(r_comm), float64 divisions).  int_consts / f64_consts: the HOST arrays of uavgnn_env_step.
 * Sg: the last extent of obs_gt, 5 with fair_service and 4 without - anything else, a null argument (obs_ubs may be NULL when
 * n == 1), n_seq < 1, steps < 1 or B < 0: UAVGNN_EINVAL.  n <= 16, M <= 1024, else UAVGNN_EUNSUPPORTED.  One launch, no host
 * synchronisation, nothing allocated: it captures into a hipGraph.  Stores are 16 bytes wide where a field's floats per (step, row)
 * are a multiple of four and its base is 16-byte aligned, else 4 bytes.  B == 0: no launch. */
int uavgnn_replay_rebuild_obs(const int32_t* int_consts, const double* f64_consts, const double* pos_ubs, const float* rate,
                              const float* avg, const float* pos_gts, int n_seq, int steps, const long long* idx, int B,
                              float* obs_gt, int Sg, float* obs_ubs, float* obs_agent, float* d_u2u, float* state,
                              uavgnn_stream_t stream);

/* ---- bias gradients ---------------------------------------------------------------------------------------------
 * acc[s, :] += column sums of the rows [s*R, (s+1)*R) of x[N, C] (row stride ld, unit column stride), R = ceil(N / S).
 * The db = dY.sum(0) of the Linear / GRUCell backward (gnn_agents.py:43-46,:237-246 under learner.py:157), accumulated
 * across the BPTT steps in the caller's acc[S, C]; the caller folds the S partials once per update.  Deterministic.
 */
int uavgnn_colsum_acc(const float* x, long long ld, int N, int C, float* acc, int S, uavgnn_stream_t stream);
/* ---- QMIX mixing tail (csrc/qmix.hip; reference: algos/madrqn/agents/mixers.py:31-45 under learner.py:145-148) ------------------
 * proj [rows, (n+3) e] (row stride ld_proj floats) is the stacked hyper-network projection of agents/qmix.py with the column blocks
 * w1 [n e, agent-major] | w_final [e] | b1 [e] | v_hid [e]; qs [rows, n] contiguous; v2w [e], v2b [1]: the weight and bias of V[2].
 *   pre_j = sum_i qs_i |w1_ij| + b1_j,  hid_j = elu(pre_j),  q_tot = sum_j hid_j |wf_j| + sum_j relu(vh_j) v2w_j + v2b
 * fp32 VALU, dword accesses only (no alignment asked of any operand), deterministic, no atomics.  1 <= n <= 16 and 1 <= e <= 128, else
 * UAVGNN_EUNSUPPORTED; a NULL operand is UAVGNN_EINVAL; rows == 0 returns 0 without a launch.
 * _fwd (mixers.py:31-45): q_tot [rows]; nothing else is written or saved.
 * _bwd (mixers.py:31-45 under loss.backward()): recomputes pre / hid and writes d_proj [rows, (n+3) e] (row stride ld_dproj; every
 *   element of the four blocks, with sign(0) = 0 for the two abs and [vh > 0] for the ReLU), d_qs [rows, n] and partials [G, e+1]:
 *   row g of it holds workgroup g's sums over its rows of d_qtot relu(vh_j) (columns 0..e-1: d v2w) and of d_qtot (column e: d v2b);
 *   the caller sums the G rows in a fixed order.  G must be what _bwd_partials returns for (rows, e), else UAVGNN_EINVAL.
 * _bwd_partials (mixers.py:31-45): G, a function of the shape only (never of the device), at least 1. */
int uavgnn_qmix_mix_fwd(const float* proj, long long ld_proj, const float* qs, const float* v2w, const float* v2b, int rows, int n, int e,
                        float* q_tot, uavgnn_stream_t stream);
int uavgnn_qmix_mix_bwd(const float* proj, long long ld_proj, const float* qs, const float* d_qtot, const float* v2w, int rows, int n,
                        int e, float* d_proj, long long ld_dproj, float* d_qs, float* partials, int G, uavgnn_stream_t stream);
int uavgnn_qmix_mix_bwd_partials(int rows, int e);
/* ---- TD tail behind the Q head (csrc/td_return.hip; reference: algos/madrqn/learner.py:134-154) ----------------------------------
 * Action select, multi-step targets, TD errors, loss and its gradient (DESIGN: "Multi-step TD targets").  All operands are contiguous
 * fp32 unless said otherwise; plain dword accesses, no atomics, deterministic; arguments only (no environment is read).  T, N, A, B, C
 * below 1, a NULL required operand or a size that does not match is UAVGNN_EINVAL, and nothing is launched.
 * _td_select_fwd (learner.py:134-143): agent_out [T+1, N, A], target_out [T, N, A], acts [T, N] int64 ->
 *   qvals [T, N] = agent_out[t, n, acts[t, n]] (NaN for an index outside [0, A): nothing is read there),
 *   next_acts [T, N] int32 (may be NULL) = argmax_a agent_out[t+1, n, a] if double_q, else argmax_a target_out[t, n, a],
 *   next_vals [T, N] = target_out[t, n, next_acts[t, n]].  The first maximum wins and a NaN counts as the maximum (torch.argmax / max).
 * _td_select_bwd (learner.py:134 under loss.backward(), :157): d_agent_out [T+1, N, A], EVERY element written (so the caller hands in
 *   uninitialised memory): d_qvals[t, n] (times *scale, a device scalar, when scale is not NULL) at (t, n, acts[t, n]), exact zeros
 *   elsewhere and in all of row T.
 * _td_return_fwd (learner.py:145-154, extended): qvals, next_vals [T, B, C]; rews [T, B, Cr], Cr = 1 (broadcast) or C; dones [T, B, 1];
 *   weights [B] or NULL (= 1); c_t = gamma (1 - done_t).  mode UAVGNN_TD_NSTEP with n_step >= 1 (lam is not read):
 *     y_t = sum_{k<m} (prod_{j<k} c_{t+j}) r_{t+k} + (prod_{j<m} c_{t+j}) V_{t+m-1},  m = min(n_step, T - t);
 *   mode UAVGNN_TD_LAMBDA with 0 <= lam <= 1 (n_step is not read):
 *     G_{T-1} = r_{T-1} + c_{T-1} V_{T-1},  G_t = r_t + c_t ((1 - lam) V_t + lam G_{t+1}),  y_t = G_t.
 *   Outputs: td [T, B, C] = q - y, g [T, B, C] = (2 w_b / (T B C)) td, loss [1] = sum w_b td^2 / (T B C), summed in two stages in a fixed
 *   order through workspace [G] floats, G = uavgnn_td_return_partials(B, C) (anything else: UAVGNN_EINVAL).  Every operation of a target
 *   is rounded once, in the order r + ((gamma (1 - done)) V): n_step = 1 and lam = 0 give learner.py:150's TD errors bit for bit.
 * _td_return_partials (learner.py:154): G, a function of (B, C) only. */
#define UAVGNN_TD_NSTEP 0
#define UAVGNN_TD_LAMBDA 1
int uavgnn_td_select_fwd(const float* agent_out, const float* target_out, const long long* acts, int T, long long N, int A, int double_q,
                         float* qvals, float* next_vals, int* next_acts, uavgnn_stream_t stream);
int uavgnn_td_select_bwd(const float* d_qvals, const long long* acts, const float* scale, int T, long long N, int A, float* d_agent_out,
                         uavgnn_stream_t stream);
int uavgnn_td_return_fwd(const float* qvals, const float* next_vals, const float* rews, int Cr, const float* dones, const float* weights,
                         int T, int B, int C, float gamma, int mode, int n_step, float lam, float* td, float* g, float* loss,
                         float* workspace, int G, uavgnn_stream_t stream);
int uavgnn_td_return_partials(int B, int C);
/* ---- dense layers on the f16 matrix cores, exactly scaled two-term splits (csrc/gemm_h2.hip, round 6) -----------------------------
 * Y = [X (K1 columns) || X2 (K - K1 columns; NULL: one source, K1 = K)] B^T (+ bias) (+ Y) (ReLU): the products of
 * uavgnn_gemm_nt_x3 / _cat with THREE f16 x f16 MFMA products per fp32 product instead of six bf16 ones (arithmetic, error and
 * non-finite behaviour: uavgnn_gru_cell_fwd_h2 above).  Replaces the input-gradient halves of the recurrent step and of f_aggr under
 * loss.backward() (learner.py:157 through gnn_agents.py:246, :99).
 *   rowmax / rowmax2  per row of the activation operand an upper bound of max |.| over the row (rowmax2 may be NULL; the larger of
 *                     the two is used), tight to within its power of two, from the kernels that produced the operand:
 *                     uavgnn_gru_gates_bwd_fused_sums_rowmax (d_gi / d_gh), uavgnn_relu_bwd_colsum_rowmax (masked gradient),
 *                     uavgnn_row_absmax (anything, as a pass of its own);
 *   planes            uavgnn_split_h2(W [R, C], transpose): f16 planes [2][n_out][K] + 2^-e per output row (uavgnn_split_h2_bytes(n_out,
 *                     K) bytes, 16-byte aligned), n_out / K = R / C (transpose = 0: y = x W^T) or C / R (transpose = 1: dx = dy W);
 *   epilogue          UAVGNN_GEMM_ACCUMULATE, UAVGNN_GEMM_RELU, UAVGNN_GEMM_STAGING_INTERLEAVED (the 256 x 128-tile kernel only:
 *                     UAVGNN_GEMM_TILE_* are UAVGNN_EUNSUPPORTED). */
int uavgnn_gemm_h2_supported(int M, int N, int K);
long long uavgnn_split_h2_bytes(int n_out, int K);
int uavgnn_split_h2(const float* W, int ld, int R, int C, int transpose, void* planes, uavgnn_stream_t stream);
int uavgnn_gemm_nt_h2(const float* X, int ldx, int K1, const float* X2, int ldx2, int M, int K, const float* rowmax, const float* rowmax2,
                      const void* planes, int N, const float* bias, float* Y, int ldy, int epilogue, uavgnn_stream_t stream);
/* uavgnn_gemm_nt_h2 for a second source WITHOUT a producer that bounds its rows (d_proj of the recurrent step: three kernels write its 96
 * columns): the launch takes the row maxima of X2 [M, K - K1] itself - every workgroup reads its 256 rows of X2 once more in front of its
 * first slice - uses max(rowmax, that) as the row's bound and writes the maxima to rowmax2_out [M] (Inf for a row that holds Inf / NaN:
 * what uavgnn_row_absmax(X2) returns, bit for bit; a maximum is order-independent).  X2 must not be NULL. */
int uavgnn_gemm_nt_h2_rm2(const float* X, int ldx, int K1, const float* X2, int ldx2, int M, int K, const float* rowmax, float* rowmax2_out,
                          const void* planes, int N, const float* bias, float* Y, int ldy, int epilogue, uavgnn_stream_t stream);
/* uavgnn_gemm_nt_h2 on 128 x 64 output tiles, for products with few output columns (d c = d_gi W_ih[:, H:] of the recurrent step:
 * [N, 768] x [768, 64], which the 256 x 128-tile kernel would run with half of every tile empty and the vendor's fp32 GEMM ran before):
 * Y [M, N] = X [M, K] B^T.  One source, no bias / accumulate / ReLU; N % 64 == 0, K % 64 == 0, ldx % 4 == 0, ldy % 4 == 0, X / planes / Y 16-byte
 * aligned (UAVGNN_EUNSUPPORTED otherwise).  rowmax and planes as for uavgnn_gemm_nt_h2; same arithmetic and accumulation order over K. */
int uavgnn_gemm_nt_h2_n64(const float* X, int ldx, int M, int K, const float* rowmax, const void* planes, int N, float* Y, int ldy,
                          uavgnn_stream_t stream);
/* uavgnn_gru_gates_bwd_fused_sums / uavgnn_relu_bwd_colsum that ALSO write row_absmax [N] = max |.| over the rows of d_gi and d_gh /
 * of `out` (H = 256 / C = 256 only - one wavefront owns a row -, UAVGNN_EUNSUPPORTED otherwise; the second not in place).
 * Packed mode of the gate entry: the r and z columns of d_gi and d_gh hold the same numbers, so a caller that passes
 * d_gi == d_gh + H (in floats) gets ONE [N, 4H] buffer G = [dn_h | dr | dz | dn_i] based at d_gh (16-byte aligned), every gate
 * gradient stored once: d_gi is the strided view G[:, H:4H] and d_gh, with its column blocks in the order n, r, z, the view G[:, :3H]
 * (row stride 4H).  Under the plain meaning that pointer relation makes the two [N, 3H] outputs overlap, so no valid plain call has
 * it.  col_sums, row_absmax and d_h are what the plain call writes, bit for bit. */
int uavgnn_gru_gates_bwd_fused_sums_rowmax(const float* pre, const float* h, const float* d_hout, const float* dq, int n_out,
                                           const float* W_out, int N, int H, float* d_gi, float* d_gh, float* d_h, float* col_sums,
                                           float* row_absmax, uavgnn_stream_t stream);
int uavgnn_relu_bwd_colsum_rowmax(const float* dy, long long ld, const float* y, long long ldy, float* out, long long ldo, int N, int C,
                                  float* acc, int S, float* row_absmax, uavgnn_stream_t stream);
/* The ReLU backward fused with the bias gradient of the Linear in front of it (reference: f_aggr = Sequential(Linear, ReLU),
 * gnn_agents.py:99-102, under learner.py:157): out [N, C] = dy where y > 0 else 0, acc[S, C] += row-blocked column sums of out
 * (as uavgnn_colsum_acc).  One pass over the gradient instead of autograd's threshold_backward + sum.  C % 4 == 0, strides % 4 == 0,
 * 16-byte aligned operands; `out` may be `dy` itself (same pointer and row stride: in place); any other
 * overlap of `out` with `dy` or `y` is UAVGNN_EINVAL. */
int uavgnn_relu_bwd_colsum(const float* dy, long long ld, const float* y, long long ldy, float* out, long long ldo, int N, int C,
                           float* acc, int S, uavgnn_stream_t stream);

/* ---- first encoder layer on flattened observations (csrc/flat_obs.hip) ---------------------------------------------
 * Linear(F, H_out) + ReLU of the o = 'mlp' agents (rnn_agents.py:15-18, gnn_agents.py:62-77) read straight from the padded
 * observation tensors: row r of the flattened observation is [agent[r] (F_a) || gt[r] (K_g = M Sg) || ubs[r] (K_u = (n-1) 3)]
 * (gym 0.21's sorted Dict keys), the three pieces at agent + r ld_a, gt + r ld_g, ubs + r ld_u (floats;
 * unit column stride); F = F_a + K_g + K_u.  The [rows, F] concatenation is never written.  fp32 FMA in a fixed order.
 *   _supported     1 when H_out is 64, 128 or 256 and 1 <= F <= 1024 (else the entries return UAVGNN_EUNSUPPORTED)
 *   _fwd           y [rows, H_out] (row stride ld_y) = ReLU(x W^T + b); W [H_out, F] contiguous, b [H_out] or NULL
 *   _wgrad_chunks  the row-chunk count S the caller should use for _wgrad
 *   _wgrad         partials [S, H_out, F] (+)= per row chunk sum of dy[r]^T x[r] (dy: the ReLU-masked gradient, row stride ld_dy;
 *                  uavgnn_relu_bwd_colsum gives it and the bias gradient).  The caller sums over S in a fixed order: deterministic. */
int uavgnn_flat_obs_supported(int H_out, int F);
int uavgnn_flat_obs_fwd(const float* agent, long long ld_a, int F_a, const float* gt, long long ld_g, int K_g, const float* ubs,
                        long long ld_u, int K_u, int rows, const float* W, const float* b, int H_out, float* y, long long ld_y,
                        uavgnn_stream_t stream);
int uavgnn_flat_obs_wgrad_chunks(long long rows, int H_out, int F);
int uavgnn_flat_obs_wgrad(const float* dy, long long ld_dy, int H_out, const float* agent, long long ld_a, int F_a, const float* gt,
                          long long ld_g, int K_g, const float* ubs, long long ld_u, int K_u, int rows, float* partials, int S,
                          int accumulate, uavgnn_stream_t stream);

/* ---- K3b, per-graph formulation ---------------------------------------------------------------------------------
 * Same contract and arithmetic as uavgnn_talk_attn_fwd / _bwd for a batch of B SMALL graphs (what dgl.batch of
 * per-environment graphs gives: common.py:45, env_wrappers.py:139-154): graph_off[B+1] = agent-node boundaries, every
 * graph has at most n_max <= 16 agents and at most n_max^2 talk edges, all of them inside the graph.  One wavefront
 * per graph, projections staged in LDS; the backward needs neither the transposed CSC nor a scratch array.  A graph
 * that violates the bounds gets NaN outputs.  uavgnn_talk_attn_env_supported(n_max, M, K) -> 1 when the shape fits
 * (K = 0 for uniform mode); otherwise use the per-destination entry points.
 */
int uavgnn_talk_attn_env_supported(int n_max, int M, int K);
int uavgnn_talk_attn_env_fwd(const float* s, int ld_s, const float* q, int ld_q, const float* v, int ld_v, int K, int M,
                             const int32_t* talk_off, const int32_t* talk_src, const int32_t* graph_off, int B,
                             int n_max, float scale, float* c, int ld_c, float* a_save, const float* x_copy, int ld_x,
                             int n_copy, uavgnn_stream_t stream);
int uavgnn_talk_attn_env_bwd(const float* s, int ld_s, const float* q, int ld_q, const float* v, int ld_v, int K, int M,
                             const int32_t* talk_off, const int32_t* talk_src, const int32_t* graph_off, int B,
                             int n_max, float scale, const float* a_save, const float* d_c, int ld_dc, float* d_s,
                             int ld_ds, float* d_q, int ld_dq, float* d_v, int ld_dv, uavgnn_stream_t stream);

/* ---- K3a + K3b in one launch (csrc/tarmac_msg.hip) ----------------------------------------------------------------
 * The TarMAC message of a batch of small graphs with a UNIFORM number of agents (gnn_agents.py:254-267):
 *   proj = [x || h] Wp^T + bp   (Wp = [f_val; f_sign; f_que].weight stacked: M value, K signature, K query columns),
 *   c_v = sum_{u -> v} softmax_u(<sign_u, query_v> * scale) value_u over `talk`.
 * Replaces the two projection GEMMs (ATen addmm behind gnn_agents.py:258-260) + uavgnn_talk_attn_env_fwd; the projections never
 * reach HBM on no-grad calls.  fp32 in / out; the projection GEMM runs on the bf16 matrix cores as six exact bf16 products per
 * fp32 product (csrc/bf16x3.h).
 *   uavgnn_tarmac_msg_supported  H % 32 == 0, M + 2K <= 128, K <= 64, n_ag in {1, 2, 4, 8, 16};
 *   uavgnn_tarmac_msg_prepare    the stacked weight [M + 2K, 2H] (row stride ld) -> bf16 plane tiles
 *                                (uavgnn_tarmac_msg_weight_bytes(H, M, K) bytes, 16-byte aligned); once per weight version;
 *   uavgnn_tarmac_msg_fwd        c_out [N, M] (row stride ld_c) always; training outputs, each optional (NULL): a_save [E]
 *                                attention weight per CSC position, proj_out [N, M + 2K], x_copy [N, H] (the x half of the GRU
 *                                input [x || c]).  M + 2K <= 96 runs the wavefront-pair kernel, wider projections the
 *                                one-wavefront-per-row-tile kernel.
 * Preconditions: every graph has exactly n_ag agents (rows i n_ag .. (i + 1) n_ag - 1; N % n_ag == 0; 16 % n_ag == 0: no graph
 * straddles two 16-row tiles, the unit a wavefront works on); the rows of a tile have at most 256 in-edges, all from rows of the
 * same tile - a violating tile gets NaN messages, never a silent fallback. */
int uavgnn_tarmac_msg_supported(int H, int M, int K, int n_ag);
long long uavgnn_tarmac_msg_weight_bytes(int H, int M, int K);
int uavgnn_tarmac_msg_prepare(const float* Wp, int ld, int H, int M, int K, void* tiles, uavgnn_stream_t stream);
int uavgnn_tarmac_msg_fwd(const float* x, int ld_x, const float* h, int ld_h, int N, int H, int n_ag, const void* tiles,
                          const float* bias, int M, int K, const int32_t* talk_off, const int32_t* talk_src, float scale,
                          float* c_out, int ld_c, float* a_save, float* proj_out, int ld_p, float* x_copy, int ld_xc,
                          uavgnn_stream_t stream);
/* ... that also writes row_absmax [N] = max(|x_row|, |c_row|, |h_row|) per agent - the row scales of uavgnn_gru_cell_fwd_h2 behind it
 * (every element of x and h passes through this kernel anyway; a maximum is order-independent: deterministic).  Wavefront-pair
 * kernel only: M + 2K <= 96 (uavgnn_tarmac_msg_rowmax_supported), UAVGNN_EUNSUPPORTED otherwise. */
int uavgnn_tarmac_msg_rowmax_supported(int H, int M, int K, int n_ag);
int uavgnn_tarmac_msg_fwd_rowmax(const float* x, int ld_x, const float* h, int ld_h, int N, int H, int n_ag, const void* tiles,
                                 const float* bias, int M, int K, const int32_t* talk_off, const int32_t* talk_src, float scale,
                                 float* c_out, int ld_c, float* a_save, float* proj_out, int ld_p, float* x_copy, int ld_xc,
                                 float* row_absmax, uavgnn_stream_t stream);

/* ---- derived indexes of a batch --------------------------------------------------------------------------------
 * What the reference gets from DGL's lazy format materialisation (CSR/CSC created inside the first message-passing
 * call on every new graph - reached from gnn_agents.py:103-104, :264-267) is explicit here and deterministic.
 *
 * uavgnn_degree_order: order[N] = destinations of a segment relation sorted by decreasing in-degree
 *   (stable; degrees >= 255 share one bucket).  A scheduling hint for uavgnn_gatv2_fwd / _bwd (dst_order), never
 *   needed for correctness.  workspace: uavgnn_degree_order_workspace_bytes(N).
 * uavgnn_csc_transpose: out-edge lists of the talk CSC: t_off[N+1]; for slot k of source u, t_dst[k] = destination
 *   and t_pos[k] = position of that edge in the CSC, ascending within each source.  Consumed by
 *   uavgnn_talk_attn_bwd / uavgnn_disc_comm_bwd.  talk_src values must lie in [0, N).  Out-lists are sorted by one
 *   lane each (insertion sort): meant for the short lists of this domain (<= n_agents - 1 per source).
 *   workspace: uavgnn_csc_transpose_workspace_bytes(N).
 * uavgnn_csc_transpose_env: the same result for a batch of B small graphs (graph_off[B+1] = agent-node boundaries,
 *   graph_off[0] == 0, graph_off[B] == N) whose talk edges stay inside their graph - what dgl.batch of per-env
 *   graphs produces (common.py:45, env_wrappers.py:67).  One wavefront per graph, one launch, no workspace; cost per
 *   graph ~ ceil(agents / 64) x its edge count, so it is meant for graphs of up to a few hundred agents.
 */
size_t uavgnn_degree_order_workspace_bytes(int N);
int uavgnn_degree_order(const int32_t* seg_off, int N, int32_t* order, void* workspace, size_t workspace_bytes,
                        uavgnn_stream_t stream);
size_t uavgnn_csc_transpose_workspace_bytes(int N);
int uavgnn_csc_transpose(const int32_t* talk_off, const int32_t* talk_src, int N, int E, int32_t* t_off,
                         int32_t* t_dst, int32_t* t_pos, void* workspace, size_t workspace_bytes,
                         uavgnn_stream_t stream);
int uavgnn_csc_transpose_env(const int32_t* talk_off, const int32_t* talk_src, const int32_t* graph_off, int B, int N,
                             int32_t* t_off, int32_t* t_dst, int32_t* t_pos, uavgnn_stream_t stream);

/* Tail of the learner's update in one launch over FLAT fp32 buffers of n elements (reference:
 * algos/madrqn/learner.py:157-166): g[i] clamped to [-clip, clip] for i < n_clip (clip_grad_value_ on the policy network
 * only; clip <= 0: none; the clamped gradient is written back), torch.optim.AdamW step on (p, exp_avg, exp_avg_sq) with
 * decoupled weight decay, then p_targ <- polyak p_targ + (1 - polyak) p (p_targ may be NULL).  hyper: DEVICE array
 * {lr, t} (t = 1-based count of this step) so that a captured graph replays with current values.  The betas are
 * doubles and the bias corrections are formed in double, as torch.optim.AdamW does on the host.  16-byte aligned
 * buffers. */
int uavgnn_adamw_polyak(float* p, float* g, float* exp_avg, float* exp_avg_sq, float* p_targ, long long n,
                        long long n_clip, const float* hyper, double beta1, double beta2, float eps, float weight_decay,
                        float clip, float polyak, uavgnn_stream_t stream);

/* Batched simulator step of the multi-UBS coverage environment, B independent environments per launch (reference:
 * envs/mubs_cov/mubs_cov.py:104-129 step, :131-210 _transmit_data, :212-242 get_obs, :278-296 get_state, :324-341
 * _get_reward; envs/common.py:19-25 Jain index, :49-59 air-to-ground channel gain).  actions [B, n] int64 or NULL (the
 * reset-time transmission: no move, t stays as it is).  In/out per environment: pos_ubs [B,n,2] f64, prior [B,M] (GT
 * priorities used by this step -> priorities for the next one), avg_rate [B,M], t [B], run_f32 [B,4] = {total throughput,
 * average global utility, Jain index, global utility}, n_colls [B].  Outputs: d_u2g [B,n,M], d_u2u [B,n,n], gt_ubs /
 * gt_rb [B,M] (serving UBS / resource block per GT, -1 = unserved), rate_per_gt [B,M], rate_per_ubs [B,n] f64,
 * mask_collision [B,n], reward [B,n] f64, done [B], padded observations obs_gt [B,n,M,5|4], obs_ubs [B,n,n-1,3] (holds
 * nothing and may be NULL when n == 1), obs_agent [B,n,2] (column 0 = visibility flag: the input format of uavgnn_obs_degrees / _compact) and the global state
 * [B, uavgnn_env_state_dim] (may be NULL).  int_consts / f64_consts: HOST arrays,
 *   int_consts [7]:  {n_ubs, n_gts, n_rbs, n_actions, episode_limit, fair_service, avoid_collision}
 *   f64_consts [18]: {range_pos, r_cov, r_sns, r_comm, dt, h_ubs, p_tx, n0, bw, fc, a, b, eta_los, eta_nlos, safe_dist, penalty,
 *                     reward_scale_rate, max_rate}
 * (the indices have names in csrc/env_math.h, which decodes them for this entry and for uavgnn_replay_rebuild_obs). */
int uavgnn_env_state_dim(int n_ubs, int n_gts, int fair_service);
int uavgnn_env_step(const int32_t* int_consts, const double* f64_consts, int B, const long long* actions,
                    const double* avail_moves, double* pos_ubs, const float* pos_gts, int32_t* prior, float* avg_rate,
                    int32_t* t, float* run_f32, double* n_colls, float* d_u2g, float* d_u2u, int32_t* gt_ubs,
                    int32_t* gt_rb, float* rate_per_gt, double* rate_per_ubs, int32_t* mask_collision, double* reward,
                    float* done, float* obs_gt, float* obs_ubs, float* obs_agent, float* state, uavgnn_stream_t stream);

/* Reset-time placements of the simulator, B environments per launch: initial UBS positions pos_ubs [B,n,2] f64, GT
 * positions pos_gts [B,M,2] f32 and the initial GT priority permutation prior [B,M] - what uavgnn_env_step(actions = NULL)
 * consumes - drawn as the reference's maps draw them (envs/mubs_cov/maps.py set_positions of Map, Debug, HotSpot,
 * DenseHotSpot, DenseHotSpotV2; np.random.permutation at mubs_cov.py:96): UBSs on distinct lattice points, GTs on distinct
 * lattice points / in a hotspot block / in groups around distinct cells of a hotspot block, GT rows shuffled.  Counter-based
 * Philox4x32-10: key = seed rng[0], counter = (environment, draw slot, rng[1]); rng is a DEVICE array {seed, resets} (a
 * captured graph replays with the current counter; the caller advances it), so environment b's placement depends on
 * (seed, resets, b) only.  fixed_ubs [n,2] f64 / fixed_gts [M,2] f32: the placement of kind `fixed` (NULL otherwise).
 * n <= 16, M <= 1024, else UAVGNN_EUNSUPPORTED.  int_consts / f64_consts: HOST arrays; their layout, the draw slots and the
 * sampling rules are in csrc/map_sample.hip. */
int uavgnn_map_sample(const int32_t* int_consts, const double* f64_consts, int B, const long long* rng,
                      const double* fixed_ubs, const float* fixed_gts, double* pos_ubs, float* pos_gts, int32_t* prior,
                      uavgnn_stream_t stream);

/* Batched simulator step of the single-UBS coverage environment of experiment 1, B independent environments per launch
 * (reference: envs/subs_cov/subs_cov.py:113-133 step, :135-157 _transmit_data, :159-171 get_obs, :186-191 reward and
 * termination; envs/common.py:19-25 Jain index, :49-59 air-to-ground channel gain).  actions [B] int64 or NULL (the reset-time
 * transmission: no move, t stays as it is).  In/out per environment: pos_ubs [B,2] f64, prior [B,M] (GT priorities used by
 * this step -> the stable argsort of the new averages), avg_rate [B,M], t [B], run_f64 [B,4] = {total throughput, average
 * global utility, Jain index, global utility}.  In: pos_gts [B,M,2], avail_moves [A,2] f64.  Outputs: d_u2g [B,M], sched [B,M]
 * (1 = served), rate_per_gt [B,M], reward [B] f64, done [B], observations obs_gt [B,M,4], obs_agent [B,2] and obs_flat
 * [B, 2 + 4 M] = agent || gt row-major (gym's flatten of the key-sorted Dict space).  M <= 1024, else UAVGNN_EUNSUPPORTED.
 * No host synchronisation, no allocation.  int_consts / f64_consts: HOST arrays, layout in csrc/subs_env.hip. */
int uavgnn_subs_env_step(const int32_t* int_consts, const double* f64_consts, int B, const long long* actions,
                         const double* avail_moves, double* pos_ubs, const float* pos_gts, int32_t* prior, float* avg_rate,
                         int32_t* t, double* run_f64, float* d_u2g, int32_t* sched, float* rate_per_gt, double* reward,
                         float* done, float* obs_gt, float* obs_agent, float* obs_flat, uavgnn_stream_t stream);

/* Reset-time placements of the single-UBS environment, B environments per launch (reference: subs_cov.py:92-111
 * _set_position, np.random.permutation at :84): the UBS at the centre, pos_ubs [B,2] f64; n_grps groups at angles
 * (u + g / n_grps) 2 pi and radii uniform in [0.2, 0.3] range_pos; GTs at 0.25 r_cov N(0,1) per coordinate around their group,
 * clipped to [0, range_pos], rows shuffled, pos_gts [B,M,2] f32; prior [B,M] a uniform permutation.  Counter-based
 * Philox4x32-10 keyed as uavgnn_map_sample keys it: rng is a DEVICE array {seed, resets}, environment b's placement depends on
 * (seed, resets, b) only.  Normals by Box-Muller, evaluated in double and rounded to float32 once.  M = n_grps gts_per_grp <=
 * 1024, else UAVGNN_EUNSUPPORTED.  int_consts / f64_consts: HOST arrays; their layout, the draw slots and the rules are in
 * csrc/subs_env.hip. */
int uavgnn_subs_env_sample(const int32_t* int_consts, const double* f64_consts, int B, const long long* rng, double* pos_ubs,
                           float* pos_gts, int32_t* prior, uavgnn_stream_t stream);

/* The four construction passes above + the three prefix sums in ONE launch for small batches (B n <=
 * uavgnn_build_graph_small_max_agents() = 4096 agents; reference: env_wrappers.py:65-89,:122-154 for B environments): seen_off /
 * near_off / talk_off [B n + 1], graph_off [B + 1] and the compacted x_gt / x_ubs / talk_src / talk_eid (allocated by the
 * caller at capacity B n M / B n U / B n n rows; the first E rows are written).  d_u2u NULL: no talk relation (talk_off, when
 * given, is zero-filled).  Bit-identical to the multi-launch path. */
int uavgnn_build_graph_small_max_agents(void);
int uavgnn_build_graph_small(const float* gt, int M, int Fg, const float* ubs, int U, int Fu, const float* d_u2u, int n, int B,
                             float r_comm, int32_t* seen_off, int32_t* near_off, int32_t* talk_off, float* x_gt, float* x_ubs,
                             int32_t* talk_src, int32_t* talk_eid, int32_t* graph_off, uavgnn_stream_t stream);

/* K4, the whole GRU cell in one launch (reference: nn.GRUCell at algos/madrqn/agents/gnn_agents.py:29,:123,:164,:208,
 * :246,:282; SURVEY 2.2 "gru_cell_fused"): h_out = GRUCell(inp [N, K_in] (leading dimension ld_inp), h [N, H]) with PyTorch's
 * parameter layout W_ih [3H, K_in], W_hh [3H, H], b_ih / b_hh [3H] (gate order r, z, n).  Both GEMMs run on fp32 MFMA into
 * shared r / z accumulators and separate gi_n / gh_n accumulators, gates in the epilogue: the [N, 3H] pre-activations never
 * reach HBM.  pre_save (may be NULL): [N, 4H] = r_pre | z_pre | gi_n | gh_n (biases included) for
 * uavgnn_gru_gates_bwd_fused, which produces the same d_gi / d_gh [N, 3H] and d_h [N, H] as uavgnn_gru_gates_bwd.
 * uavgnn_gru_cell_supported: K_in and H multiples of 32 (else: vendor GEMMs + uavgnn_gru_gates_fwd). */
int uavgnn_gru_cell_supported(int K_in, int H);
int uavgnn_gru_cell_fwd(const float* inp, int ld_inp, int K_in, const float* h, int N, int H, const float* W_ih,
                        const float* b_ih, const float* W_hh, const float* b_hh, float* h_out, float* pre_save,
                        uavgnn_stream_t stream);
/* The same cell on the bf16 matrix cores (csrc/gru_x3.hip, csrc/bf16x3.h): every fp32 operand is split exactly into three
 * bf16 terms and each fp32 product is accumulated as six bf16 x bf16 MFMA products in fp32 (error below an fp32 GEMM's,
 * profiles/r02_ubench_gemm_bf16x3.txt; fp32 MFMA issues at 1/16 of the bf16 MFMA rate on gfx950).
 * uavgnn_gru_split_weights writes the bf16 planes of W_ih then W_hh ([3][3H][K_in] | [3][3H][H], ..._workspace_bytes bytes,
 * 16-byte aligned) - call it whenever the weights may have changed; uavgnn_gru_cell_fwd_x3 has the contract of
 * uavgnn_gru_cell_fwd with `planes` in place of the two weight matrices; 4 N max(ld_inp, H) must stay below 2^32 (32-bit byte
 * offsets inside the kernel: 3.3 M rows at K_in = 320), UAVGNN_EUNSUPPORTED otherwise. */
int uavgnn_gru_cell_x3_supported(int K_in, int H);   /* K_in % 32 == 0 and H % 64 == 0 */
long long uavgnn_gru_cell_x3_workspace_bytes(int K_in, int H);
int uavgnn_gru_split_weights(const float* W_ih, int K_in, const float* W_hh, int H, void* planes, uavgnn_stream_t stream);
int uavgnn_gru_cell_fwd_x3(const float* inp, int ld_inp, int K_in, const float* h, int N, int H, const void* planes,
                           const float* b_ih, const float* b_hh, float* h_out, float* pre_save, uavgnn_stream_t stream);
/* The same call with the cell's input given as TWO pieces [inp (K1 columns) || inp2 (K2 columns)] - the TarMAC step's
 * th.cat([x, c]) (gnn_agents.py:268-270) without the concatenated copy; K1, K2 multiples of 32 (K2 = 0: one piece), `planes`
 * built for K_in = K1 + K2. */
int uavgnn_gru_cell_fwd_x3_cat(const float* inp, int ld_inp, int K1, const float* inp2, int ld_inp2, int K2, const float* h,
                               int N, int H, const void* planes, const float* b_ih, const float* b_hh, float* h_out,
                               float* pre_save, uavgnn_stream_t stream);
/* ... with a per-call variant word (0 = uavgnn_gru_cell_fwd_x3_cat).  UAVGNN_GRU_STAGING_BLOCKS: the staging of a K slice as a
 * block in front of / behind its first MFMA group (the round-2 schedule; the A/B reference of tools/gru_probe.py) instead of
 * interleaved with it - bit-identical results.  A call argument, not process state: the library keeps no mutable globals. */
#define UAVGNN_GRU_STAGING_BLOCKS 1
int uavgnn_gru_cell_fwd_x3_opts(const float* inp, int ld_inp, int K1, const float* inp2, int ld_inp2, int K2, const float* h,
                                int N, int H, const void* planes, const float* b_ih, const float* b_hh, float* h_out,
                                float* pre_save, int flags, uavgnn_stream_t stream);
/* The same cell with HALF the matrix-core work (csrc/gru_h2.hip, round 6): "f16x2" - every row of the activation operand
 * [inp || inp2 || h] and every output unit's row of [W_ih | W_hh] is scaled by a power of two that puts its largest magnitude into
 * [2^14, 2^15) (exact), the scaled value is split as hi = rn_f16(v), lo = rn_f16(v - hi) (hi + lo = v to <= 2^-23 |v|), and an fp32
 * product is the fp32-accumulated sum of THREE f16 x f16 MFMA products (hi lo + lo hi + hi hi; the dropped lo lo <= 2^-22 |a b|),
 * un-scaled exactly in the epilogue.  fp32 in / out / accumulate; measured error against float64 at or below the vendor fp32 GEMM's
 * and the bf16x3 cell's (profiles/r06_h2_error_tables.txt).  Replaces nn.GRUCell at gnn_agents.py:246 exactly like
 * uavgnn_gru_cell_fwd_x3_cat.
 *   row_absmax [N]   an upper bound of max |.| over every row of [inp || inp2 || h], tight to within its power of two:
 *                    uavgnn_tarmac_msg_fwd_rowmax writes it on its way (the producer of `c`), uavgnn_row_absmax computes it in a pass
 *                    of its own.  A bound that is too SMALL overflows f16: the row's outputs are NaN, never a plausible number;
 *   planes           uavgnn_gru_split_weights_h2: f16 planes [2][3H][K_in] | [2][3H][H] | 2^-e per weight row (float [3H]),
 *                    uavgnn_gru_cell_h2_workspace_bytes bytes, 16-byte aligned; rebuilt whenever the weights may have changed.
 * Non-finite operands follow the bf16x3 kernels' contract (a row that holds Inf / NaN yields NaN outputs); rows whose largest
 * magnitude is below 2^-112 lose relative precision (the scale exponent is clamped to 126).  Same shape limits as the x3 cell. */
int uavgnn_gru_cell_h2_supported(int K_in, int H);   /* K_in % 32 == 0 and H % 64 == 0 */
long long uavgnn_gru_cell_h2_workspace_bytes(int K_in, int H);
int uavgnn_gru_split_weights_h2(const float* W_ih, int K_in, const float* W_hh, int H, void* planes, uavgnn_stream_t stream);
int uavgnn_gru_cell_fwd_h2(const float* inp, int ld_inp, int K1, const float* inp2, int ld_inp2, int K2, const float* h, int N, int H,
                           const float* row_absmax, const void* planes, const float* b_ih, const float* b_hh, float* h_out,
                           float* pre_save, uavgnn_stream_t stream);
/* out [N] = max |.| per row over up to three row-major pieces (a2 / a3 may be NULL); Inf when the row holds Inf or NaN. */
int uavgnn_row_absmax(const float* a1, int ld1, int K1, const float* a2, int ld2, int K2, const float* a3, int ld3, int K3, int N,
                      float* out, uavgnn_stream_t stream);
/* The Q head for n_actions <= 16 (csrc/head.hip; reference: nn.Linear(H, n_actions) at algos/madrqn/agents/gnn_agents.py:43-46,:56):
 * q [N, A] (row stride ld_q) = h [N, H] (row stride ld_h) W [A, H]^T (row stride ld_w) + b [A].  fp32 in / out, exact fp32 products
 * on the matrix cores (v_mfma_f32_16x16x4_f32), one pass over h.  H in {64, 128, 256}, A <= 16, ld_h % 4 == 0, ld_w % 4 == 0, h and W
 * 16-byte aligned (UAVGNN_EUNSUPPORTED otherwise). */
int uavgnn_head_supported(int H, int A);
int uavgnn_head_fwd(const float* h, int ld_h, int N, int H, const float* W, int ld_w, const float* b, int A, float* q, int ld_q,
                    uavgnn_stream_t stream);
/* The dueling Q head for n_actions <= 15 (csrc/head.hip; reference: DuelingLayer.forward at algos/madrqn/agents/dueling.py:13-16, built
 * at algos/madrqn/agents/gnn_agents.py:43-46 and called at :56): q [N, A] (row stride ld_q) = v + (adv - mean over the A columns of adv),
 * adv = h W_adv^T + b_adv (W_adv [A, H], row stride ld_w), v = h w_v^T + b_v (w_v [H], b_v [1]).  The four parameters are read through
 * their own pointers on every launch: no stacked copy.  Same schedule as uavgnn_head_fwd (value = column A of the 16-column tile), the
 * combine in registers (fixed order, bit-reproducible).  H in {64, 128, 256}, 1 <= A <= 15, ld_h % 4 == 0, ld_w % 4 == 0, h, W_adv and
 * w_v 16-byte aligned (UAVGNN_EUNSUPPORTED otherwise); a NULL pointer or a row stride below the row length: UAVGNN_EINVAL; N == 0: 0. */
int uavgnn_head_duel_supported(int H, int A);
int uavgnn_head_fwd_duel(const float* h, int ld_h, int N, int H, const float* W_adv, int ld_w, const float* w_v, const float* b_adv,
                         const float* b_v, int A, float* q, int ld_q, uavgnn_stream_t stream);
/* The recurrent half of nn.GRUCell for FEW rows (csrc/gru_rec.hip; reference: the GRU cells of the agents without a communication
 * block - algos/drqn/agents/gnn_agents.py:25-29, algos/madrqn/agents/rnn_agents.py:22-26, gnn_agents.py:29 - at 32 sequences x 1 or 8
 * agents): the input projection gi = x W_ih^T + b_ih does not depend on h, so the caller forms it for all steps of a sequence in one
 * GEMM and only this half walks the sequence.  Parallel over (16-row tile) x (16 hidden columns); exact fp32 products, fp32
 * accumulation on v_mfma_f32_16x16x4_f32 in a fixed order; bit-reproducible.  uavgnn_gru_rec_supported: H % 16 == 0, 16 <= H <= 256.
 *   fwd  gi [N, 3H] (row stride ld_gi; b_ih included; gate order r | z | n), h [N, H] (ld_h), W_hh [3H, H], b_hh [3H] ->
 *        h_out [N, H] (ld_ho) = (1 - z) n + z h; pre_save (may be NULL): [N, 4H] = r_pre | z_pre | gi_n | gh_n, the set
 *        uavgnn_gru_cell_fwd saves.
 *   bwd  pre [N, 4H], h [N, H] (ld_h), d_hout / d_carry (each may be NULL; contiguous [N, H]; their sum is the gradient of h') ->
 *        d_gi, d_gh [N, 3H] as uavgnn_gru_gates_bwd_fused writes them and dh_prev [N, H] = dh z + d_gh W_hh.
 * Rows >= N are never written.  Leading dimensions are multiples of 4 floats and every base is 16-byte aligned
 * (UAVGNN_EUNSUPPORTED otherwise).  Workgroups read whole rows of h (d_hout / d_carry) while others write column blocks of h_out
 * (dh_prev): an h_out whose ADDRESS RANGE [base, base + 4 ((N - 1) ld + H)) intersects h's, or a dh_prev whose range intersects
 * d_hout's / d_carry's, is UAVGNN_EINVAL before any launch - the ranges are compared, not the elements, so two disjoint column views of
 * one wider buffer (h = buf[:, :H], h_out = buf[:, H:]) are refused as well. */
int uavgnn_gru_rec_supported(int H);
int uavgnn_gru_rec_fwd(const float* gi, int ld_gi, const float* h, int ld_h, int N, int H, const float* W_hh, const float* b_hh,
                       float* h_out, int ld_ho, float* pre_save, uavgnn_stream_t stream);
int uavgnn_gru_rec_bwd(const float* pre, const float* h, int ld_h, const float* d_hout, const float* d_carry, int N, int H,
                       const float* W_hh, float* d_gi, float* d_gh, float* dh_prev, uavgnn_stream_t stream);
/* Dense layers on the bf16 matrix cores (csrc/gemm_x3.hip; reference: the nn.Linear layers of
 * algos/madrqn/agents/gnn_agents.py - f_aggr :101-102, :106, TarMAC projections :227-236 - and the input-gradient GEMMs of
 * loss.backward(), learner.py:157): Y[M, N] = X[M, K] B[N, K]^T (+ bias[N]) (+ Y) (then ReLU), fp32 in / out, each fp32 product
 * as six exact bf16 products (bf16x3.h).  uavgnn_split_bf16x3 turns a weight matrix W [R, C] (row stride ld) into the bf16
 * planes the GEMM reads: [3][R][C] (transpose = 0: forward, B = W) or [3][C][R] (transpose = 1: input gradient, B = W^T);
 * 6 R C bytes, 16-byte aligned.  K % 32 == 0, ldx % 4 == 0, X 16-byte aligned; M, N arbitrary. */
#define UAVGNN_GEMM_ACCUMULATE 1
#define UAVGNN_GEMM_RELU 2
/* kernel variants, selected per call by further bits of `epilogue` (A/B references of tools/gemm_x3_probe.py; the two eight-wave
 * variants agree bit for bit, so do the two four-wave ones - the pairs differ in accumulation order, inside the same error
 * bound): default = 256 x 128 tiles, eight waves, double-buffered LDS, staging of a slice as a block;
 * STAGING_INTERLEAVED = the same with the staging interleaved with the MFMAs (faster per launch, not per power-limited cycle);
 * TILE_128 = 128 x 128 tiles, four waves; TILE_64 = 64 x 128 tiles, four waves (batches of a few thousand rows: twice the workgroups) */
#define UAVGNN_GEMM_STAGING_INTERLEAVED 4
#define UAVGNN_GEMM_TILE_128 8
#define UAVGNN_GEMM_TILE_64 16
int uavgnn_gemm_x3_supported(int M, int N, int K);
int uavgnn_split_bf16x3(const float* W, int ld, int R, int C, int transpose, void* planes, uavgnn_stream_t stream);
int uavgnn_gemm_nt_x3(const float* X, int ldx, int M, int K, const void* planes, int N, const float* bias, float* Y, int ldy,
                      int epilogue, uavgnn_stream_t stream);
/* ... with the contraction over TWO buffers, [X (K1 columns) || X2 (K - K1 columns)], without a concatenated copy (K1 % 32 == 0,
 * ldx2 % 4 == 0, X2 16-byte aligned; default tiles only - UAVGNN_EUNSUPPORTED with TILE_128 / TILE_64): the GRU backward's
 * d x = d_gi W_ih[:, :H] + d_proj Wp[:, :H] (learner.py:157 through gnn_agents.py:246,:258-260) as one product over K = 3H + M + 2K;
 * `planes` = uavgnn_split_bf16x3 of the stacked weight. */
int uavgnn_gemm_nt_x3_cat(const float* X, int ldx, int K1, const float* X2, int ldx2, int M, int K, const void* planes, int N,
                          const float* bias, float* Y, int ldy, int epilogue, uavgnn_stream_t stream);
/* uavgnn_gemm_nt_x3 (the 256 x 128-tile kernel only: UAVGNN_GEMM_TILE_* are UAVGNN_EUNSUPPORTED) that ALSO writes rowmax_out [M] = max |.|
 * over every row of X, a by-product of its staging: the bound of an f16x2 product that reads the same operand later (the layer's weight
 * gradient, uavgnn_gemm_tn_h2) at no extra traffic. */
int uavgnn_gemm_nt_x3_rowmax(const float* X, int ldx, int M, int K, const void* planes, int N, const float* bias, float* Y, int ldy,
                             int epilogue, float* rowmax_out, uavgnn_stream_t stream);

/* Weight gradient of a dense layer on the bf16x3 arithmetic (csrc/gemm_tn_x3.hip): partials[s][Mo, Ko] (+)= dY[rows_s, :Mo]^T
 * X[rows_s, :Ko] for the S contiguous row chunks rows_s of the n_rows rows (chunk = ceil(n_rows / S) rounded up to 32 rows);
 * the caller sums the S partial products in a fixed order.  dY [n_rows, >= Mo] (row stride ldy), X [n_rows, >= Ko] (row
 * stride ldx), fp32, unit inner stride, any 4-byte alignment; partials [S, Mo, Ko] fp32, fully overwritten unless
 * `accumulate`.  Replaces autograd's dW = dy^T x of nn.Linear / nn.GRUCell (gnn_agents.py:99, :243-246, :43-46 under
 * learner.py:157).  uavgnn_gemm_tn_x3_chunks: the S this library would pick (output tiles x S fills the chip). */
int uavgnn_gemm_tn_x3_chunks(long long n_rows, int Mo, int Ko);
int uavgnn_gemm_tn_x3(const float* dY, int ldy, int Mo, const float* X, int ldx, int Ko, long long n_rows, float* partials,
                      int S, int accumulate, uavgnn_stream_t stream);
/* The same weight gradient on the f16x2 arithmetic (csrc/gemm_tn_h2.hip, round 6; arithmetic and error: uavgnn_gru_cell_fwd_h2): the
 * contraction runs over the ROWS of both operands, so the power-of-two scales of the two-term split are per COLUMN.
 *   colmax_y [Mo] / colmax_x [Ko]  upper bounds of max |.| over every column of dY / X, tight to within their power of two:
 *                                  uavgnn_col_absmax (one pass over the operand; Inf for a column that holds Inf / NaN -> NaN outputs);
 *   partials [S][Mo][Ko]           one partial product per row chunk (the caller sums them in a fixed order), `accumulate` adds in place.
 * n_rows % 32 == 0, Mo % 4 == 0, Ko % 4 == 0, 16-byte aligned rows (uavgnn_gemm_tn_h2_supported; UAVGNN_EUNSUPPORTED otherwise).
 * Replaces the vendor's fp32 split-K GEMM for dW_ih / dW_hh of nn.GRUCell (gnn_agents.py:246) and csrc/gemm_tn_x3.hip for f_aggr
 * (gnn_agents.py:99) under loss.backward() (learner.py:157) over the time-batched rows of a BPTT sequence. */
int uavgnn_col_absmax(const float* x, long long ld, long long n, int C, float* out, uavgnn_stream_t stream);
int uavgnn_gemm_tn_h2_supported(long long n_rows, int Mo, int Ko);
int uavgnn_gemm_tn_h2_chunks(long long n_rows, int Mo, int Ko);
int uavgnn_gemm_tn_h2(const float* dY, long long ldy, int Mo, const float* X, long long ldx, int Ko, long long n_rows,
                      const float* colmax_y, const float* colmax_x, float* partials, int S, int accumulate, uavgnn_stream_t stream);
/* Output tiles are 256 rows by tj columns, tj = uavgnn_gemm_tn_h2_width(Ko): 160 where 160 divides Ko and 128 does not (dW_ih, Ko = 320),
 * else 96 where 96 divides Ko and neither 128 nor 160 does (dWp^T, Ko = 96), else 128 - no column tile of MFMAs is padding where such a
 * width exists.  uavgnn_gemm_tn_h2_chunks counts tiles at that width.  The _tj forms take the width as an argument (96, 128 or 160; 0 = the
 * rule; anything else UAVGNN_EINVAL / 0 chunks): every width takes every Ko, and a partial product P[s] does not depend on the width, bit
 * for bit - only the default chunk count S does (and with it where the fixed-order sum over the rows is cut). */
int uavgnn_gemm_tn_h2_width(int Ko);
int uavgnn_gemm_tn_h2_chunks_tj(long long n_rows, int Mo, int Ko, int tj);
int uavgnn_gemm_tn_h2_tj(const float* dY, long long ldy, int Mo, const float* X, long long ldx, int Ko, long long n_rows,
                         const float* colmax_y, const float* colmax_x, float* partials, int S, int accumulate, int tj,
                         uavgnn_stream_t stream);
int uavgnn_gru_gates_bwd_fused(const float* pre, const float* h, const float* d_hout, int N, int H, float* d_gi, float* d_gh,
                               float* d_h, uavgnn_stream_t stream);
/* The same with the Q head's input gradient folded in: the gradient of h' is d_hout (NULL = 0) + dq W_out, dq [N, n_out] the
 * gradient of q = h' W_out^T + b_out (reference: algos/madrqn/agents/gnn_agents.py:56 `self.f_out(h)` on the GRU output), W_out
 * [n_out, H] row-major and 16-byte aligned, n_out <= 64.  Replaces `d_hout + dq @ W_out` followed by the call above: the [N, H]
 * sum never reaches HBM.  UAVGNN_EUNSUPPORTED for H % 4 != 0, n_out > 64 or an unaligned W_out. */
int uavgnn_gru_gates_bwd_fused_head(const float* pre, const float* h, const float* d_hout, const float* dq, int n_out,
                                    const float* W_out, int N, int H, float* d_gi, float* d_gh, float* d_h,
                                    uavgnn_stream_t stream);
/* ... which also writes the launch's share of the cell's BIAS gradients: col_sums [uavgnn_gru_gates_bwd_sum_rows(N, H)][4 H] (16-byte
 * aligned) holds per-workgroup column sums d_r | d_z | d_n (input side) | d_n (hidden side); db_ih = the sum over its rows of columns
 * [0 : 3H], db_hh = of columns [0 : 2H] and [3H : 4H] (fixed summation order: deterministic).  dq / W_out may both be NULL (no head
 * term; d_hout is then required).  Replaces autograd's db = sum over rows of d_gi / d_gh (nn.GRUCell under learner.py:157), i.e. a
 * second pass over the [N, 3H] gate gradients.  uavgnn_gru_gates_bwd_sum_rows returns 0 when H / 4 does not divide 256. */
int uavgnn_gru_gates_bwd_sum_rows(int N, int H);
int uavgnn_gru_gates_bwd_fused_sums(const float* pre, const float* h, const float* d_hout, const float* dq, int n_out,
                                    const float* W_out, int N, int H, float* d_gi, float* d_gh, float* d_h, float* col_sums,
                                    uavgnn_stream_t stream);

/* Backward of the fused GRU cell as ONE call (csrc/gru_bwd.hip; reference: autograd of nn.GRUCell at gnn_agents.py:246,:270
 * under learner.py:157): gate gradients from the pre-activation sets saved by the forward (pre [N, 4H]), d_inp [N, K_in]
 * (leading dimension ld_dinp) = d_gi W_ih, d_h [N, H] = d_hout * z + d_gh W_hh, both GEMMs on the bf16x3 arithmetic.
 * d_gi / d_gh [N, 3H] are OUTPUTS kept for the caller: the weight / bias gradients (dW_ih = d_gi^T inp, dW_hh = d_gh^T h, db_ih =
 * colsum d_gi, db_hh = [colsum d_gi[:, :2H] | colsum d_gh[:, 2H:]]) are sums over agents AND time steps, which a BPTT caller
 * forms once per sequence (uavgnn_gemm_tn_x3 / uavgnn_colsum_acc over the stacked operands).  planes_bwd: bf16 planes of
 * W_ih^T then W_hh^T written by uavgnn_gru_split_weights_bwd (uavgnn_gru_cell_bwd_workspace_bytes bytes, 16-byte aligned);
 * 3H % 32 == 0, pre / d_gi / d_gh / d_inp 16-byte aligned, ld_dinp % 4 == 0. */
long long uavgnn_gru_cell_bwd_workspace_bytes(int K_in, int H);
int uavgnn_gru_split_weights_bwd(const float* W_ih, int K_in, const float* W_hh, int H, void* planes, uavgnn_stream_t stream);
int uavgnn_gru_cell_bwd(const float* pre, const float* h, const float* d_hout, int N, int K_in, int H, const void* planes_bwd,
                        float* d_gi, float* d_gh, float* d_inp, int ld_dinp, float* d_h, uavgnn_stream_t stream);

/* ONE query for every caller-provided scratch / plane buffer (bytes; 0 = unknown kind or bad sizes).  Arguments per kind:
 *   GATV2_BWD (F_src, H)            partial rows of uavgnn_gatv2_bwd          DEGREE_ORDER (N)   CSC_TRANSPOSE (N)
 *   GRU_PLANES (K_in, H)            uavgnn_gru_split_weights                  GRU_BWD_PLANES (K_in, H)  uavgnn_gru_split_weights_bwd
 *   GEMM_PLANES (R, C)              uavgnn_split_bf16x3                       GEMM_TN_PARTIALS (n_rows, Mo, Ko)  uavgnn_gemm_tn_x3
 *   K1_IMAGE ()                     uavgnn_gatv2_hetero_prepare */
#define UAVGNN_WS_GATV2_BWD 1
#define UAVGNN_WS_DEGREE_ORDER 2
#define UAVGNN_WS_CSC_TRANSPOSE 3
#define UAVGNN_WS_GRU_PLANES 4
#define UAVGNN_WS_GRU_BWD_PLANES 5
#define UAVGNN_WS_GEMM_PLANES 6
#define UAVGNN_WS_GEMM_TN_PARTIALS 7
#define UAVGNN_WS_K1_IMAGE 8
long long uavgnn_workspace_bytes(int kind, long long a, long long b, long long c);

#ifdef __cplusplus
}
#endif
#endif /* UAVGNN_H */

// Compact replay ring: the padded observations and the global state of sampled sequences REBUILT from the simulator state the ring
// stores - pos_ubs [n,2] f64, rate_per_gt [M] and avg_rate [M] per step, pos_gts [M,2] per sequence - instead of copied from stored
// observations (reference: envs/mubs_cov/mubs_cov.py:212-297 get_obs / get_state; algos/madrqn/learner.py:99-116, the batch an update
// reads).  Every value is what env_step_kernel (csrc/env_sim.hip, "observations" and "global state") wrote when the step was
// simulated, operation by operation and dtype by dtype:
//   d_u2g / d_u2u  float64 norm of (float32 GT - float64 UBS) / (float64 UBS - float64 UBS), rounded to float32
//   visibility     d <= float(r_sns) / d <= float(r_comm)
//   offsets        float64 difference / float64 min(range_pos, r_sns | r_comm), rounded to float32
//   rates          float64(rate) / max_rate and float64(avg) / max_rate * M / (n R), rounded to float32
//   state row      agent positions / range_pos in float64, GT positions / float(range_pos) in float32, the two rates as above
// Both kernels call the SAME functions for these elements (csrc/env_math.h; same contraction, no fast-math), so the bits are the same;
// the two rate columns depend on the GT alone and are evaluated once per GT instead of once per (UBS, GT) pair - the same operations on
// the same operands.
//
// One workgroup per (step t, sampled row b), grid-strided: it reads 16 n + 16 M bytes, keeps positions, the per-GT columns, the
// visibility flags, the two offset columns of every (UBS, GT) pair and the UBS-UBS distances in LDS (9 n M + 16 M + ... bytes, at
// most 64 KB), and writes n M Sg floats of obs_gt (plus the small fields).  The stores dominate, so every destination is written by FLATTENED element: consecutive lanes hold consecutive addresses, four elements per
// lane as one 16-byte store where the field's floats per item are a multiple of four and its base is 16-byte aligned, else one float.
#include "common.h"
#include "env_math.h"

namespace uavgnn {
namespace {

// One wavefront per workgroup: an item is a chain of dependent round trips (idx, then the state, then the stores) with little work
// in between, so what hides the latency is the number of INDEPENDENT items in flight per CU - 32 one-wave workgroups against 8 of
// four waves that wait for one another at every barrier (profiles/compact_replay_probe.txt).
constexpr int kThreads = 64;
constexpr int kMaxGrid = 16384;      // 256 CUs x 32 resident wavefronts x 2; the rest is grid-strided

struct RebuildArgs {
  int n, M, R, fair_service, state_dim;                  // copied from the EnvConsts of uavgnn_env_step
  double range_pos, r_sns, r_comm, max_rate;
  const double* pos_ubs;             // [n_seq, T1, n, 2]
  const float* rate;                 // [n_seq, T1, M]
  const float* avg;                  // [n_seq, T1, M]
  const float* pos_gts;              // [n_seq, M, 2]
  const long long* idx;              // [B]
  long long n_seq;
  int T1, B;
  float *obs_gt, *obs_ubs, *obs_agent, *d_u2u, *state;   // time-major [T1, B, ...]; d_u2u / state may be null
  int vec_gt, vec_ubs, vec_agent, vec_duu, vec_state;    // 1: 16-byte stores
};

template <class F>
__device__ __forceinline__ void write_flat(float* __restrict__ dst, int count, int vec, F elem) {
  if (vec) {
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
    for (int q = threadIdx.x; q < count / 4; q += kThreads) {
      float4 v;
      v.x = elem(4 * q);
      v.y = elem(4 * q + 1);
      v.z = elem(4 * q + 2);
      v.w = elem(4 * q + 3);
      d4[q] = v;
    }
  } else {
    for (int e = threadIdx.x; e < count; e += kThreads) dst[e] = elem(e);
  }
}

template <bool FAIR>
__global__ __launch_bounds__(kThreads) void replay_rebuild_kernel(RebuildArgs c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = c.n, M = c.M, R = c.R;
  constexpr int Sg = FAIR ? 5 : 4, Ss = FAIR ? 4 : 3;
  const int tid = threadIdx.x;
  double* PU = reinterpret_cast<double*>(smem);            // [n][2]
  float* PG = reinterpret_cast<float*>(PU + 2 * n);        // [M][2]
  float* RN = PG + 2 * M;                                  // [M] float(float64(rate) / max_rate)
  float* AN = RN + M;                                      // [M] float(float64(avg) / max_rate * M / (n R))
  float* DUU = AN + M;                                     // [n][n]
  float* AG = DUU + n * n;                                 // [n][2] float(float64 position / range_pos)
  float* OX = AG + 2 * n;                                  // [n][M] columns 1 and 2 of obs_gt: the offsets of a visible GT, else 0
  float* OY = OX + n * M;
  unsigned char* VIS = reinterpret_cast<unsigned char*>(OY + n * M);   // [n][M] d_u2g <= float(r_sns)
  const double norm_s = fmin(c.range_pos, c.r_sns), norm_c = fmin(c.range_pos, c.r_comm);
  const long long items = static_cast<long long>(c.T1) * c.B;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int t = static_cast<int>(item / c.B), b = static_cast<int>(item - static_cast<long long>(t) * c.B);
    long long s = c.idx[b];
    s = s < 0 ? 0 : (s >= c.n_seq ? c.n_seq - 1 : s);
    const size_t step = static_cast<size_t>(s) * c.T1 + t;
    const double* __restrict__ pu = c.pos_ubs + step * n * 2;
    const float* __restrict__ pg = c.pos_gts + static_cast<size_t>(s) * M * 2;
    const float* __restrict__ rate = c.rate + step * M;
    const float* __restrict__ avg = c.avg + step * M;
    for (int k = tid; k < 2 * n; k += kThreads) PU[k] = pu[k];
    for (int k = tid; k < 2 * M; k += kThreads) PG[k] = pg[k];
    for (int m = tid; m < M; m += kThreads) {
      RN[m] = obs_rate(rate[m], c.max_rate);
      if (FAIR) AN[m] = obs_avg_rate(avg[m], c.max_rate, M, n, R);
    }
    __syncthreads();
    // distances as env_step_kernel's step 1: float64 norm of (float32 GT position - float64 UBS position), float32
    for (int k = tid; k < n * M; k += kThreads) {
      const int i = k / M, m = k - i * M;
      const double dx = static_cast<double>(PG[2 * m]) - PU[2 * i], dy = static_cast<double>(PG[2 * m + 1]) - PU[2 * i + 1];
      const float d = dist_f32(dx, dy);
      const bool vis = d <= static_cast<float>(c.r_sns);
      VIS[k] = vis;
      // dx, dy ARE (float64(GT) - UBS): the two float64 divisions per pair run here, on full wavefronts, not once per stored element
      OX[k] = vis ? obs_offset(dx, norm_s) : 0.f;
      OY[k] = vis ? obs_offset(dy, norm_s) : 0.f;
    }
    for (int k = tid; k < n * n; k += kThreads) {
      const int i = k / n, jx = k - i * n;
      const double dx = PU[2 * jx] - PU[2 * i], dy = PU[2 * jx + 1] - PU[2 * i + 1];
      DUU[k] = dist_f32(dx, dy);
    }
    for (int k = tid; k < 2 * n; k += kThreads) AG[k] = obs_pos(PU[k], c.range_pos);
    __syncthreads();
    // ---- observations (mubs_cov.py:215-242) ---------------------------------------------------------------------------------------
    write_flat(c.obs_gt + static_cast<size_t>(item) * n * M * Sg, n * M * Sg, c.vec_gt, [&](int e) -> float {
      const int k = e / Sg, col = e - k * Sg;
      const bool vis = VIS[k];
      if (col == 0) return vis ? 1.f : 0.f;
      if (col == 1) return OX[k];
      if (col == 2) return OY[k];
      const int m = k % M;
      if (col == 3) return vis ? RN[m] : 0.f;
      return vis ? AN[m] : 0.f;
    });
    if (n > 1)
      write_flat(c.obs_ubs + static_cast<size_t>(item) * n * (n - 1) * 3, n * (n - 1) * 3, c.vec_ubs, [&](int e) -> float {
        const int k = e / 3, col = e - k * 3;
        const int i = k / (n - 1), jj = k - i * (n - 1);
        const int other = jj < i ? jj : jj + 1;
        const bool vis = DUU[i * n + other] <= static_cast<float>(c.r_comm);
        if (col == 0) return vis ? 1.f : 0.f;
        const int a = col - 1;
        return vis ? obs_offset(PU[2 * other + a] - PU[2 * i + a], norm_c) : 0.f;
      });
    write_flat(c.obs_agent + static_cast<size_t>(item) * n * 2, 2 * n, c.vec_agent, [&](int e) -> float { return AG[e]; });
    if (c.d_u2u != nullptr)
      write_flat(c.d_u2u + static_cast<size_t>(item) * n * n, n * n, c.vec_duu, [&](int e) -> float { return DUU[e]; });
    // ---- global state (mubs_cov.py:278-296) ------------------------------------------------------------------------------------------
    if (c.state != nullptr)
      write_flat(c.state + static_cast<size_t>(item) * c.state_dim, c.state_dim, c.vec_state, [&](int e) -> float {
        if (e < 2 * n) return AG[e];
        const int q = e - 2 * n;
        const int m = q / Ss, col = q - m * Ss;
        if (col <= 1) return state_gt_pos(PG[2 * m + col], c.range_pos);
        if (col == 2) return RN[m];
        return AN[m];
      });
    __syncthreads();      // the next item overwrites the LDS this one's stores read
  }
}

inline size_t rebuild_lds_bytes(int n, int M) {
  const size_t f = 4 * static_cast<size_t>(M) + static_cast<size_t>(n) * n + 2 * static_cast<size_t>(n) +
                   2 * static_cast<size_t>(n) * M;   // floats
  return 16 * static_cast<size_t>(n) + 4 * f + static_cast<size_t>(n) * M + 16;
}

inline int vec_ok(const float* p, long long floats_per_item) {
  return p != nullptr && floats_per_item > 0 && floats_per_item % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

// int_consts / f64_consts: the arrays of uavgnn_env_step (layout: include/uavgnn.h)
extern "C" int uavgnn_replay_rebuild_obs(const int32_t* int_consts, const double* f64_consts, const double* pos_ubs,
                                         const float* rate, const float* avg, const float* pos_gts, int n_seq, int steps,
                                         const long long* idx, int B, float* obs_gt, int Sg, float* obs_ubs, float* obs_agent,
                                         float* d_u2u, float* state, uavgnn_stream_t stream) {
  if (!int_consts || !f64_consts || !pos_ubs || !rate || !avg || !pos_gts || n_seq < 1 || steps < 1 || B < 0 ||
      (B > 0 && !idx) || !obs_gt || !obs_agent)
    return UAVGNN_EINVAL;
  const EnvConsts ec = env_consts(int_consts, f64_consts);
  RebuildArgs c;
  c.n = ec.n; c.M = ec.M; c.R = ec.R; c.fair_service = ec.fair_service; c.state_dim = ec.state_dim;
  c.range_pos = ec.range_pos; c.r_sns = ec.r_sns; c.r_comm = ec.r_comm; c.max_rate = ec.max_rate;
  if (Sg != (c.fair_service ? 5 : 4)) return UAVGNN_EINVAL;
  if (c.n < 1 || c.n > 16 || c.M < 1 || c.M > 1024 || c.R < 1 || c.R > 16) return UAVGNN_EUNSUPPORTED;
  if (c.n > 1 && !obs_ubs) return UAVGNN_EINVAL;
  c.pos_ubs = pos_ubs; c.rate = rate; c.avg = avg; c.pos_gts = pos_gts; c.idx = idx;
  c.n_seq = n_seq; c.T1 = steps; c.B = B;
  c.obs_gt = obs_gt; c.obs_ubs = obs_ubs; c.obs_agent = obs_agent; c.d_u2u = d_u2u; c.state = state;
  c.vec_gt = vec_ok(obs_gt, static_cast<long long>(c.n) * c.M * Sg);
  c.vec_ubs = vec_ok(obs_ubs, static_cast<long long>(c.n) * (c.n - 1) * 3);
  c.vec_agent = vec_ok(obs_agent, 2ll * c.n);
  c.vec_duu = vec_ok(d_u2u, static_cast<long long>(c.n) * c.n);
  c.vec_state = vec_ok(state, c.state_dim);
  const long long items = static_cast<long long>(steps) * B;
  if (items == 0) return 0;
  const int grid = capped_grid(items, 1, kMaxGrid);
  const size_t lds = rebuild_lds_bytes(c.n, c.M);
  if (lds > 64 * 1024) return UAVGNN_EUNSUPPORTED;        // n M above ~7000; uavgnn_env_step refuses such a map sooner (n M 16 B of LDS)
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (c.fair_service) hipLaunchKernelGGL(replay_rebuild_kernel<true>, dim3(grid), dim3(kThreads), lds, st, c);
  else hipLaunchKernelGGL(replay_rebuild_kernel<false>, dim3(grid), dim3(kThreads), lds, st, c);
  return launch_status();
}

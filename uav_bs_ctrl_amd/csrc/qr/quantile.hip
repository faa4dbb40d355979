// Distributional Q-learning, quantile-regression form (QR-DQN; Dabney et al., AAAI 2018): the mean fold of the quantile head, the
// action select on quantile rows and the pairwise quantile-Huber loss with its n-step targets.  include/uavgnn_qr.h has the
// definitions; DESIGN "Distributional Q: quantile regression" the reasons.
//
// Mapping.  A row of K quantiles (K in {8, 16, 32, 64}) lives in a group of K adjacent lanes, 64 / K rows per wavefront, four
// wavefronts per workgroup; a capped grid strides over the rows.  In the loss, lane i holds theta_i and the target y_i; the loop over j
// broadcasts y_j inside the group (a shuffle of width K), so the K x K pairs exist in registers only: lane i's own accumulators give
// g_i, a butterfly over the group the row loss.  The n-step coefficients are recomputed per row from rews / dones (at most n_step
// steps), innermost first, the order of csrc/td_return.hip.
//
// Arithmetic: every product and sum is a single rounded fp32 operation (no contraction: the pragma below and -ffp-contract=off in
// build.py).  A sum over k or j of one lane runs in ascending index; a sum over the K lanes of a group is the butterfly at lane
// distances K/2, ..., 1 (every lane ends with the same bits: fp32 addition commutes).  The loss is a two-stage sum: each workgroup
// leaves the sum of its rows' terms in the caller's workspace (per group in ascending row order, the groups of a wavefront by the
// 64-lane butterfly, the four wavefronts in ascending order), one workgroup adds those in the order of td_return.hip's second stage.
// The geometry is a function of the shapes alone, so the bits are too.  Non-finite values propagate as IEEE arithmetic has it; argmax
// takes the first maximum and counts a NaN as the maximum (torch.argmax); an action outside [0, A) reads nothing and gives NaN.
#include <math.h>

#include "common.h"
#include "uavgnn_qr.h"

#pragma clang fp contract(off)

namespace uavgnn {
namespace {

constexpr int kThreads = 256;    // four wavefronts: 256 / K rows per workgroup trip
constexpr int kGridCap = 2048;   // workgroups of a row-streaming launch (capped_grid's default: 256 CUs x 8)
constexpr int kSumThreads = 256;
constexpr int kNoAction = 0x7fffffff;

template <int K>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = K / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// torch.argmax / torch.max: first maximum, a NaN counts as the maximum (the first one wins)
__device__ __forceinline__ bool takes_over(float v, float best) { return v > best || (v != v && best == best); }

// the same rule between two candidates of different lanes: a total order, so both lanes of a butterfly step agree
__device__ __forceinline__ bool beats(float v2, int i2, float v1, int i1) {
  if (i2 == kNoAction) return false;
  if (i1 == kNoAction) return true;
  const bool n2 = v2 != v2, n1 = v1 != v1;
  if (n2 || n1) return n2 && (!n1 || i2 < i1);
  return v2 > v1 || (v2 == v1 && i2 < i1);
}

template <int K>
__device__ __forceinline__ float quantile_sum(const float* __restrict__ p) {
  float s = p[0];
#pragma unroll
  for (int k = 1; k < K; ++k) s += p[k];
  return s;
}

// lane i of a group takes the actions i, i + K, ...: their quantile sums in ascending k; the group's argmax by the butterfly
template <int K>
__device__ __forceinline__ int group_argmax(const float* __restrict__ row, int A, int i, float* __restrict__ means) {
  constexpr float inv_k = 1.f / K;
  float bv = 0.f;
  int bi = kNoAction;
  for (int a = i; a < A; a += K) {
    const float s = quantile_sum<K>(row + static_cast<long long>(a) * K);
    if (means != nullptr) means[a] = s * inv_k;
    if (bi == kNoAction || takes_over(s, bv)) {
      bv = s;
      bi = a;
    }
  }
#pragma unroll
  for (int o = K / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (beats(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  return bi;
}

template <int K>
__global__ __launch_bounds__(kThreads) void qr_select_fwd_kernel(const float* __restrict__ theta_pol, const float* __restrict__ theta_tgt,
                                                                 const long long* __restrict__ acts, long long rows, long long N, int A,
                                                                 int double_q, float* __restrict__ theta_a, float* __restrict__ theta_next,
                                                                 int* __restrict__ next_acts, float* __restrict__ q_pol) {
  constexpr int kRows = kThreads / K;
  const int i = threadIdx.x & (K - 1), grp = threadIdx.x / K;
  const long long rows1 = rows + N, step = static_cast<long long>(gridDim.x) * kRows, AK = static_cast<long long>(A) * K;
  // group r walks the policy's row r = (t', n) of [T+1, N]: its means, the taken action's quantiles (t' < T) and the output row whose
  // choice is made on it - (t' - 1, n) under double-Q, (t', n) on the target network's own row otherwise
  for (long long r = static_cast<long long>(blockIdx.x) * kRows + grp; r < rows1; r += step) {
    const float* __restrict__ pol = theta_pol + r * AK;
    int best = kNoAction;
    long long o = -1;
    if (double_q) {
      if (r >= N || q_pol != nullptr) best = group_argmax<K>(pol, A, i, q_pol != nullptr ? q_pol + r * A : nullptr);
      if (r >= N) o = r - N;
    } else {
      if (q_pol != nullptr) group_argmax<K>(pol, A, i, q_pol + r * A);
      if (r < rows) {
        o = r;
        best = group_argmax<K>(theta_tgt + o * AK, A, i, nullptr);
      }
    }
    if (o >= 0) {
      theta_next[o * K + i] = theta_tgt[o * AK + static_cast<long long>(best) * K + i];
      if (next_acts != nullptr && i == 0) next_acts[o] = best;
    }
    if (r < rows) {
      const long long a = acts[r];
      theta_a[r * K + i] = (a >= 0 && a < A) ? pol[a * K + i] : nanf("");
    }
  }
}

__global__ __launch_bounds__(kThreads) void qr_select_bwd_kernel(const float* __restrict__ d_theta_a, const long long* __restrict__ acts,
                                                                 long long rows, long long total, int A, int K,
                                                                 float* __restrict__ d_theta_pol) {
  const long long step = static_cast<long long>(gridDim.x) * kThreads;
  for (long long e = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; e < total; e += step) {
    const long long ra = e / K, row = ra / A;       // K is a power of two: a shift
    const int k = static_cast<int>(e - ra * K), a = static_cast<int>(ra - row * A);
    float v = 0.f;
    if (row < rows && acts[row] == a) v = d_theta_a[row * K + k];
    d_theta_pol[e] = v;     // rows [T N, (T + 1) N): the last step's quantiles are nobody's chosen action
  }
}

__global__ __launch_bounds__(kThreads) void qr_mean_fold_kernel(const float* __restrict__ W, int ld_w, const float* __restrict__ b, int A,
                                                                int K, int H, float* __restrict__ W_bar, float* __restrict__ b_bar) {
  const long long AH = static_cast<long long>(A) * H, total = AH + A, step = static_cast<long long>(gridDim.x) * kThreads;
  const float inv_k = 1.f / static_cast<float>(K);
  for (long long e = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; e < total; e += step) {
    if (e < AH) {
      const long long a = e / H, h = e - a * H;
      const float* __restrict__ p = W + a * K * ld_w + h;
      float s = p[0];
      for (int k = 1; k < K; ++k) s += p[static_cast<long long>(k) * ld_w];
      W_bar[e] = s * inv_k;
    } else {
      const long long a = e - AH;
      float s = b[a * K];
      for (int k = 1; k < K; ++k) s += b[a * K + k];
      b_bar[a] = s * inv_k;
    }
  }
}

template <int K>
__global__ __launch_bounds__(kThreads) void qr_loss_fwd_kernel(const float* __restrict__ theta_a, const float* __restrict__ theta_next,
                                                               const float* __restrict__ rews, int rew_per_agent,
                                                               const float* __restrict__ dones, const float* __restrict__ weights,
                                                               int T, int B, int C, long long rows, float gamma, int n_step, float kappa,
                                                               float count, float* __restrict__ td, float* __restrict__ g,
                                                               float* __restrict__ partials) {
  constexpr int kRows = kThreads / K;
  constexpr float inv_k = 1.f / K;
  __shared__ float part[kThreads / kWave];
  const int i = threadIdx.x & (K - 1), grp = threadIdx.x / K;
  const float tau = static_cast<float>(2 * i + 1) * (0.5f * inv_k), one_m_tau = 1.f - tau;     // both exact
  const float half_kappa = 0.5f * kappa;
  const long long M = static_cast<long long>(B) * C, step = static_cast<long long>(gridDim.x) * kRows;
  float acc = 0.f;      // lane 0 of a group: the sum of w_b l over its rows
  for (long long row = static_cast<long long>(blockIdx.x) * kRows + grp; row < rows; row += step) {
    // rows < 2^31 (checked by the entry point): 32-bit divisions
    const uint32_t t = static_cast<uint32_t>(row) / static_cast<uint32_t>(M);
    const uint32_t j = static_cast<uint32_t>(row) - t * static_cast<uint32_t>(M);
    const uint32_t b = j / static_cast<uint32_t>(C);
    const float w = weights != nullptr ? weights[b] : 1.f;
    const long long last = (static_cast<long long>(t) + n_step < T ? static_cast<long long>(t) + n_step : T) - 1;     // t + m - 1
    float y = theta_next[(last * M + j) * K + i];
    for (long long u = last; u >= static_cast<long long>(t); --u) {
      const float r = rew_per_agent ? rews[u * M + j] : rews[u * B + b];
      y = r + (gamma * (1.f - dones[u * B + b])) * y;
    }
    const float th = theta_a[row * K + i];
    float la = 0.f, ga = 0.f;
#pragma unroll 8
    for (int jj = 0; jj < K; ++jj) {
      const float u = __shfl(y, jj, K) - th;
      const float au = fabsf(u);
      const float wt = u < 0.f ? one_m_tau : tau;                                   // |tau_i - [u < 0]|
      const float hub = au <= kappa ? (0.5f * u) * u : kappa * (au - half_kappa);
      const float cl = u > kappa ? kappa : (u < -kappa ? -kappa : u);               // a NaN stays a NaN
      la += wt * hub;
      ga += wt * cl;
    }
    const float l = (group_sum<K>(la) * inv_k) / kappa;
    const float mean_th = group_sum<K>(th) * inv_k, mean_y = group_sum<K>(y) * inv_k;
    g[row * K + i] = -(((w / count) * inv_k) * (ga / kappa));
    if (i == 0) {
      td[row] = mean_th - mean_y;
      acc += w * l;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = part[0];
#pragma unroll
    for (int k = 1; k < kThreads / kWave; ++k) tot += part[k];
    partials[blockIdx.x] = tot;
  }
}

__global__ __launch_bounds__(kSumThreads) void qr_loss_sum_kernel(const float* __restrict__ partials, int G, float count,
                                                                  float* __restrict__ loss) {
  __shared__ float part[kSumThreads / kWave];
  float acc = 0.f;
  for (int i = threadIdx.x; i < G; i += kSumThreads) acc += partials[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = part[0];
#pragma unroll
    for (int k = 1; k < kSumThreads / kWave; ++k) tot += part[k];
    loss[0] = tot / count;
  }
}

inline bool k_supported(int K) { return K == 8 || K == 16 || K == 32 || K == 64; }

// rows * A * K elements addressed with 64-bit indices: refuse what would overflow them
inline bool fits(int T, long long N, int A, int K) { return N <= 0x7fffffffffffLL / (static_cast<long long>(T) + 1) / A / K; }

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_qr_supported(int A, int K) { return (A >= 1 && A <= 64 && k_supported(K)) ? 1 : 0; }

extern "C" int uavgnn_qr_mean_fold(const float* W, int ld_w, const float* b, int A, int K, int H, float* W_bar, float* b_bar,
                                   uavgnn_stream_t stream) {
  if (!W || !b || !W_bar || !b_bar || A < 1 || K < 1 || H < 1 || ld_w < H) return UAVGNN_EINVAL;
  if (!uavgnn_qr_supported(A, K)) return UAVGNN_EUNSUPPORTED;
  const long long total = static_cast<long long>(A) * H + A;
  hipLaunchKernelGGL(qr_mean_fold_kernel, dim3(capped_grid(total, kThreads, kGridCap)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     W, ld_w, b, A, K, H, W_bar, b_bar);
  return launch_status();
}

extern "C" int uavgnn_qr_select_fwd(const float* theta_pol, const float* theta_tgt, const long long* acts, int T, long long N, int A, int K,
                                    int double_q, float* theta_a, float* theta_next, int* next_acts, float* q_pol,
                                    uavgnn_stream_t stream) {
  if (!theta_pol || !theta_tgt || !acts || !theta_a || !theta_next || T < 1 || N < 1 || A < 1 || K < 1) return UAVGNN_EINVAL;
  if (!uavgnn_qr_supported(A, K)) return UAVGNN_EUNSUPPORTED;
  if (!fits(T, N, A, K)) return UAVGNN_EINVAL;
  const long long rows = static_cast<long long>(T) * N;
  const dim3 grid(capped_grid(rows + N, kThreads / K, kGridCap)), block(kThreads);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int dq = double_q != 0 ? 1 : 0;
#define UAVGNN_QR_SELECT(KK)                                                                                                         \
  hipLaunchKernelGGL(qr_select_fwd_kernel<KK>, grid, block, 0, st, theta_pol, theta_tgt, acts, rows, N, A, dq, theta_a, theta_next, \
                     next_acts, q_pol)
  switch (K) {
    case 8: UAVGNN_QR_SELECT(8); break;
    case 16: UAVGNN_QR_SELECT(16); break;
    case 32: UAVGNN_QR_SELECT(32); break;
    default: UAVGNN_QR_SELECT(64); break;
  }
#undef UAVGNN_QR_SELECT
  return launch_status();
}

extern "C" int uavgnn_qr_select_bwd(const float* d_theta_a, const long long* acts, int T, long long N, int A, int K, float* d_theta_pol,
                                    uavgnn_stream_t stream) {
  if (!d_theta_a || !acts || !d_theta_pol || T < 1 || N < 1 || A < 1 || K < 1) return UAVGNN_EINVAL;
  if (!uavgnn_qr_supported(A, K)) return UAVGNN_EUNSUPPORTED;
  if (!fits(T, N, A, K)) return UAVGNN_EINVAL;
  const long long rows = static_cast<long long>(T) * N, total = (rows + N) * A * K;
  hipLaunchKernelGGL(qr_select_bwd_kernel, dim3(capped_grid(total, kThreads, kGridCap)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     d_theta_a, acts, rows, total, A, K, d_theta_pol);
  return launch_status();
}

extern "C" int uavgnn_qr_loss_partials(int T, int B, int C, int K) {
  if (T < 1 || B < 1 || C < 1 || K < 1) return UAVGNN_EINVAL;
  if (!k_supported(K)) return UAVGNN_EUNSUPPORTED;
  if (static_cast<long long>(T) * B > 0x7fffffffLL / C) return UAVGNN_EINVAL;      // rows are indexed in 32 bits
  return capped_grid(static_cast<long long>(T) * B * C, kThreads / K, kGridCap);
}

extern "C" int uavgnn_qr_loss_fwd(const float* theta_a, const float* theta_next, const float* rews, int Cr, const float* dones,
                                  const float* weights, int T, int B, int C, int K, float gamma, int n_step, float kappa, float* td, float* g,
                                  float* loss, float* workspace, int G, uavgnn_stream_t stream) {
  if (!theta_a || !theta_next || !rews || !dones || !td || !g || !loss || !workspace || T < 1 || B < 1 || C < 1 || K < 1)
    return UAVGNN_EINVAL;
  if ((Cr != 1 && Cr != C) || n_step < 1 || !(kappa > 0.f)) return UAVGNN_EINVAL;
  const int want = uavgnn_qr_loss_partials(T, B, C, K);
  if (want < 0) return want;
  if (G != want) return UAVGNN_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long rows = static_cast<long long>(T) * B * C;
  const float count = static_cast<float>(static_cast<double>(T) * B * C);
  const int per_agent = (Cr == C && C > 1) ? 1 : 0;
  const dim3 grid(G), block(kThreads);
#define UAVGNN_QR_LOSS(KK)                                                                                                            \
  hipLaunchKernelGGL(qr_loss_fwd_kernel<KK>, grid, block, 0, st, theta_a, theta_next, rews, per_agent, dones, weights, T, B, C, rows, \
                     gamma, n_step, kappa, count, td, g, workspace)
  switch (K) {
    case 8: UAVGNN_QR_LOSS(8); break;
    case 16: UAVGNN_QR_LOSS(16); break;
    case 32: UAVGNN_QR_LOSS(32); break;
    default: UAVGNN_QR_LOSS(64); break;
  }
#undef UAVGNN_QR_LOSS
  int rc = launch_status();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(qr_loss_sum_kernel, dim3(1), dim3(kSumThreads), 0, st, workspace, G, count, loss);
  return launch_status();
}

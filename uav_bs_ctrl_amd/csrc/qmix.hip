// QMIX mixing tail: everything of the monotonic mixer behind its one hyper-network GEMM, forward and backward.
//
// Reference: algos/madrqn/agents/mixers.py:31-45 (w1 = |hyper_w_1(s)|, hidden = elu(bmm(qs, w1) + b1),
// w_final = |hyper_w_final(s)|, v = V(s), y = bmm(hidden, w_final) + v) reached from learner.py:145-148.  The package runs the four
// state-conditioned projections as ONE GEMM (agents/qmix.py); its output proj [rows, (n+3) e] holds the column blocks
//     w1 [n e, agent-major] | w_final [e] | b1 [e] | v_hid [e]
// and this file does the rest per row (rows = T B):
//     pre_j = sum_i qs_i |w1_ij| + b1_j        hid_j = elu(pre_j)
//     q_tot = sum_j hid_j |wf_j| + sum_j relu(vh_j) v2w_j + v2b
// The forward saves nothing; the backward recomputes pre / hid from proj and qs, so an update moves proj twice and d_proj once
// instead of a [rows, n e] intermediate per elementwise op of the torch formulation.
//
// Layout: lane <-> embed column, EP = next power of two >= e (at most 64) lanes per row and 64 / EP rows per wavefront, so every column
// block of a row is read as e contiguous floats; e > 64 gives each lane two columns (col, col + 64).  Row sums are xor-shuffles inside
// the row's lane group.  All loads and stores are dwords: the row stride (n+3) e floats has no alignment to offer (n = 3, e = 5).
// fp32 VALU, expf / expm1f.  No atomics: the sums over rows (d v2w, d v2b) leave as per-workgroup partials in a fixed order.
#include <type_traits>

#include "common.h"

namespace uavgnn {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxAgents = 16;    // the simulator's own limit
constexpr int kMaxEmbed = 128;
constexpr int kGridCap = 2048;    // 256 CUs x 8 workgroups; grid-stride beyond

inline int lane_group(int e) {
  int ep = 1;
  while (ep < e && ep < kWave) ep <<= 1;
  return ep;
}

// workgroups of both kernels: a function of the shape only, so the partials and their summation order do not depend on the device
inline int mix_grid(long long rows, int e) {
  return capped_grid(rows, kWaves * (kWave / lane_group(e)), kGridCap);
}

template <int EP>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = EP >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float sign0(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }   // sign(0) = 0: torch's abs backward

template <int EP, int CPL>
__global__ __launch_bounds__(kThreads) void qmix_mix_fwd_kernel(const float* __restrict__ proj, long long ld,
                                                                const float* __restrict__ qs, const float* __restrict__ v2w,
                                                                const float* __restrict__ v2b, int rows, int n, int e,
                                                                float* __restrict__ q_tot) {
  constexpr int RPW = kWave / EP;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int j = lane & (EP - 1), sub = lane / EP;
  float vw[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) vw[c] = (j + c * EP < e) ? v2w[j + c * EP] : 0.f;
  const float vb = v2b[0];
  const long long step = static_cast<long long>(gridDim.x) * (kWaves * RPW);
  for (long long r0 = static_cast<long long>(blockIdx.x) * (kWaves * RPW); r0 < rows; r0 += step) {
    const long long row = r0 + wave * RPW + sub;
    float t = 0.f;
    if (row < rows) {
      const float* __restrict__ p = proj + static_cast<size_t>(row) * static_cast<size_t>(ld);
      const float* __restrict__ q = qs + static_cast<size_t>(row) * n;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int col = j + c * EP;
        if (col < e) {
          const float wf = p[n * e + col], b1 = p[(n + 1) * e + col], vh = p[(n + 2) * e + col];
          float pre = 0.f;
#pragma unroll 4
          for (int i = 0; i < n; ++i) pre = fmaf(q[i], fabsf(p[i * e + col]), pre);
          pre += b1;
          const float hid = pre > 0.f ? pre : expm1f(pre);
          t += hid * fabsf(wf) + fmaxf(vh, 0.f) * vw[c];
        }
      }
    }
    t = group_sum<EP>(t);
    if (j == 0 && row < rows) q_tot[row] = t + vb;
  }
}

template <int EP, int CPL>
__global__ __launch_bounds__(kThreads) void qmix_mix_bwd_kernel(const float* __restrict__ proj, long long ld,
                                                                const float* __restrict__ qs, const float* __restrict__ d_qtot,
                                                                const float* __restrict__ v2w, int rows, int n, int e,
                                                                float* __restrict__ d_proj, long long ldd, float* __restrict__ d_qs,
                                                                float* __restrict__ partials) {
  constexpr int RPW = kWave / EP;
  __shared__ float part[kWaves][kWave * CPL + 1];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int j = lane & (EP - 1), sub = lane / EP;
  float vw[CPL], acc_w[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    vw[c] = (j + c * EP < e) ? v2w[j + c * EP] : 0.f;
    acc_w[c] = 0.f;
  }
  float acc_b = 0.f;
  const long long step = static_cast<long long>(gridDim.x) * (kWaves * RPW);
  for (long long r0 = static_cast<long long>(blockIdx.x) * (kWaves * RPW); r0 < rows; r0 += step) {
    const long long row = r0 + wave * RPW + sub;
    const bool live = row < rows;
    float w[CPL][kMaxAgents], dpre[CPL], qv[kMaxAgents];
    float g = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) dpre[c] = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxAgents; ++i) {
      qv[i] = 0.f;
#pragma unroll
      for (int c = 0; c < CPL; ++c) w[c][i] = 0.f;
    }
    if (live) {
      const float* __restrict__ p = proj + static_cast<size_t>(row) * static_cast<size_t>(ld);
      float* __restrict__ dp = d_proj + static_cast<size_t>(row) * static_cast<size_t>(ldd);
      const float* __restrict__ q = qs + static_cast<size_t>(row) * n;
      g = d_qtot[row];
#pragma unroll
      for (int i = 0; i < kMaxAgents; ++i)
        if (i < n) qv[i] = q[i];
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int col = j + c * EP;
        if (col < e) {
          const float wf = p[n * e + col], b1 = p[(n + 1) * e + col], vh = p[(n + 2) * e + col];
#pragma unroll
          for (int i = 0; i < kMaxAgents; ++i)
            if (i < n) w[c][i] = p[i * e + col];
          float pre = 0.f;
#pragma unroll
          for (int i = 0; i < kMaxAgents; ++i)
            if (i < n) pre = fmaf(qv[i], fabsf(w[c][i]), pre);
          pre += b1;
          const float ex = pre > 0.f ? 0.f : expf(pre);
          const float hid = pre > 0.f ? pre : expm1f(pre);
          const float dq = g * fabsf(wf) * (pre > 0.f ? 1.f : ex);
          dpre[c] = dq;
          dp[n * e + col] = g * hid * sign0(wf);
          dp[(n + 1) * e + col] = dq;
          dp[(n + 2) * e + col] = vh > 0.f ? g * vw[c] : 0.f;
#pragma unroll
          for (int i = 0; i < kMaxAgents; ++i)
            if (i < n) dp[i * e + col] = dq * qv[i] * sign0(w[c][i]);
          acc_w[c] += g * fmaxf(vh, 0.f);
        }
      }
      acc_b += g;
    }
    // d_qs[i] = sum_j d pre_j |w1_ij|: one reduction per agent inside the row's lane group (dead lanes carry zeros)
    float mine = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxAgents; ++i) {
      if (i < n) {       // uniform
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CPL; ++c) s = fmaf(dpre[c], fabsf(w[c][i]), s);
        s = group_sum<EP>(s);
        if constexpr (EP >= kMaxAgents) {
          mine = (j == i) ? s : mine;
        } else {
          if (j == 0 && live) d_qs[static_cast<size_t>(row) * n + i] = s;
        }
      }
    }
    if constexpr (EP >= kMaxAgents) {
      if (j < n && live) d_qs[static_cast<size_t>(row) * n + j] = mine;
    }
  }
  // partials[block, 0..e) = sum over the block's rows of g relu(vh_j), partials[block, e] = sum of g: lane groups of a wave in
  // ascending xor order, then the waves in ascending order
  float sb = (j == 0) ? acc_b : 0.f;
#pragma unroll
  for (int o = kWave >> 1; o > 0; o >>= 1) sb += __shfl_xor(sb, o);
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
#pragma unroll
    for (int o = EP; o < kWave; o <<= 1) acc_w[c] += __shfl_xor(acc_w[c], o);
    if (sub == 0) part[wave][j + c * EP] = acc_w[c];
  }
  if (lane == 0) part[wave][kWave * CPL] = sb;
  __syncthreads();
  float* __restrict__ out = partials + static_cast<size_t>(blockIdx.x) * (e + 1);
  for (int col = threadIdx.x; col <= e; col += kThreads) {
    const int k = col < e ? col : kWave * CPL;
    float tot = part[0][k];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) tot += part[wv][k];
    out[col] = tot;
  }
}

template <typename F>
inline bool dispatch(int e, F&& f) {
  switch (lane_group(e)) {
    case 1: f(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}, std::integral_constant<int, 1>{}); return true;
    case 16: f(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{}); return true;
    case 32: f(std::integral_constant<int, 32>{}, std::integral_constant<int, 1>{}); return true;
    case 64:
      if (e <= kWave) f(std::integral_constant<int, 64>{}, std::integral_constant<int, 1>{});
      else f(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
      return true;
  }
  return false;
}

inline bool shape_ok(int n, int e) { return n >= 1 && n <= kMaxAgents && e >= 1 && e <= kMaxEmbed; }

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_qmix_mix_bwd_partials(int rows, int e) {
  if (rows < 0 || e < 1 || e > kMaxEmbed) return UAVGNN_EUNSUPPORTED;
  return mix_grid(rows, e);
}

extern "C" int uavgnn_qmix_mix_fwd(const float* proj, long long ld_proj, const float* qs, const float* v2w, const float* v2b, int rows,
                                   int n, int e, float* q_tot, uavgnn_stream_t stream) {
  if (!proj || !qs || !v2w || !v2b || !q_tot || rows < 0) return UAVGNN_EINVAL;
  if (!shape_ok(n, e)) return UAVGNN_EUNSUPPORTED;
  if (ld_proj < static_cast<long long>(n + 3) * e) return UAVGNN_EINVAL;
  if (rows == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int G = mix_grid(rows, e);
  dispatch(e, [&](auto ep, auto cpl) {
    hipLaunchKernelGGL((qmix_mix_fwd_kernel<decltype(ep)::value, decltype(cpl)::value>), dim3(G), dim3(kThreads), 0, st, proj, ld_proj,
                       qs, v2w, v2b, rows, n, e, q_tot);
  });
  return launch_status();
}

extern "C" int uavgnn_qmix_mix_bwd(const float* proj, long long ld_proj, const float* qs, const float* d_qtot, const float* v2w, int rows,
                                   int n, int e, float* d_proj, long long ld_dproj, float* d_qs, float* partials, int G,
                                   uavgnn_stream_t stream) {
  if (!proj || !qs || !d_qtot || !v2w || !d_proj || !d_qs || !partials || rows < 0) return UAVGNN_EINVAL;
  if (!shape_ok(n, e)) return UAVGNN_EUNSUPPORTED;
  if (ld_proj < static_cast<long long>(n + 3) * e || ld_dproj < static_cast<long long>(n + 3) * e || G != mix_grid(rows, e))
    return UAVGNN_EINVAL;
  if (rows == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch(e, [&](auto ep, auto cpl) {
    hipLaunchKernelGGL((qmix_mix_bwd_kernel<decltype(ep)::value, decltype(cpl)::value>), dim3(G), dim3(kThreads), 0, st, proj, ld_proj,
                       qs, d_qtot, v2w, rows, n, e, d_proj, ld_dproj, d_qs, partials);
  });
  return launch_status();
}

// The TD tail behind the Q head: action select, multi-step targets (n-step / lambda returns), TD errors, loss and its gradient.
//
// Reference: algos/madrqn/learner.py:134-154 (gather of Q(s,a), double-Q target, one-step target, MSE over [T, B, n]); the multi-step
// targets are this package's extension of that one-step target (DESIGN: "Multi-step TD targets").  With c_t = gamma (1 - done_t):
//     n-step   y_t = sum_{k<m} (prod_{j<k} c_{t+j}) r_{t+k} + (prod_{j<m} c_{t+j}) V_{t+m-1},   m = min(n, T - t)
//     lambda   G_{T-1} = r_{T-1} + c_{T-1} V_{T-1},   G_t = r_t + c_t ((1 - lambda) V_t + lambda G_{t+1}),   y_t = G_t
//     td = q - y,   loss = sum w_b td^2 / (T B C),   g = (2 w_b / (T B C)) td
// The torch formulation is a Python loop over T with three or four elementwise launches per step; here the select is one pass over the two
// Q tensors, the recursion one thread per (b, c) walking t backwards, the select's backward one pass that writes all of d_agent_out.
//
// Arithmetic: every product and sum of a target is a single rounded fp32 operation (contraction into FMAs is switched off for this file:
// the pragma below and -ffp-contract=off in build.py; HIP's __fmul_rn / __fadd_rn are plain operators the compiler may still fuse), in
// the order r + ((gamma (1 - done)) V) for n = 1 and lambda = 0 - the order of the torch chain, so the TD errors are its bits on finite
// inputs.  The n-step sum is evaluated innermost first, y = r_t + c_t (r_{t+1} + c_{t+1} (... + c_{t+m-1} V_{t+m-1})): two roundings per
// term; n >= T is that same chain carried from step to step (y_t = r_t + c_t y_{t+1}).  Non-finite values propagate as IEEE arithmetic
// has it (a NaN in Q reaches td, g and the loss; argmax / max take the FIRST NaN of a row as torch does), with one exception that
// follows torch.where-free code: lambda = 0 and lambda = 1 skip the vanishing term instead of multiplying it by zero, so an infinite V
// or G under a zero coefficient does not make a NaN.  An action index outside [0, A) reads nothing and gives NaN (torch asserts).
//
// The loss is a two-stage sum in a fixed order (the rule of learner._mse: no semaphore reduction, no atomically accumulated scalar):
// each wavefront-sized workgroup leaves the sum of its lanes' terms in the caller's workspace, one workgroup adds those.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace uavgnn {
namespace {

constexpr int kSelThreads = 256;
constexpr int kRetThreads = kWave;      // one wavefront per workgroup: B C / 64 of them spread the T-long dependent chains over the CUs
constexpr int kSumThreads = 256;

// torch.argmax / torch.max: first maximum, a NaN counts as the maximum (the first one wins)
__device__ __forceinline__ bool takes_over(float v, float best) { return v > best || (v != v && best == best); }

__global__ __launch_bounds__(kSelThreads) void td_select_fwd_kernel(const float* __restrict__ agent_out, const float* __restrict__ target_out,
                                                                    const long long* __restrict__ acts, long long rows, long long N, int A,
                                                                    int double_q, float* __restrict__ qvals, float* __restrict__ next_vals,
                                                                    int* __restrict__ next_acts) {
  const long long step = static_cast<long long>(gridDim.x) * kSelThreads;
  for (long long i = static_cast<long long>(blockIdx.x) * kSelThreads + threadIdx.x; i < rows; i += step) {
    const float* __restrict__ cur = agent_out + i * A;           // agent_out[t, n]
    const float* __restrict__ tgt = target_out + i * A;          // target_out[t, n]
    const float* __restrict__ pick = double_q ? cur + N * A : tgt;   // agent_out[t + 1, n]: the row the double-Q choice is made on
    const long long a = acts[i];
    int best = 0;
    float bv = pick[0];
    for (int j = 1; j < A; ++j) {
      const float v = pick[j];
      if (takes_over(v, bv)) {
        bv = v;
        best = j;
      }
    }
    qvals[i] = (a >= 0 && a < A) ? cur[a] : nanf("");
    next_vals[i] = double_q ? tgt[best] : bv;
    if (next_acts != nullptr) next_acts[i] = best;
  }
}

__global__ __launch_bounds__(kSelThreads) void td_select_bwd_kernel(const float* __restrict__ d_qvals, const long long* __restrict__ acts,
                                                                    const float* __restrict__ scale, long long rows, long long total,
                                                                    int A, float* __restrict__ d_agent_out) {
  const float s = scale != nullptr ? *scale : 1.f;
  const long long step = static_cast<long long>(gridDim.x) * kSelThreads;
  for (long long e = static_cast<long long>(blockIdx.x) * kSelThreads + threadIdx.x; e < total; e += step) {
    // 32-bit division wherever the tensor allows it (the 64-bit one is some forty instructions per element)
    const long long row = total <= 0x7fffffffLL ? static_cast<long long>(static_cast<uint32_t>(e) / static_cast<uint32_t>(A)) : e / A;
    const int col = static_cast<int>(e - row * A);
    float v = 0.f;
    if (row < rows && acts[row] == col) v = scale != nullptr ? __fmul_rn(d_qvals[row], s) : d_qvals[row];
    d_agent_out[e] = v;     // rows [T N, (T + 1) N): the last step's Q values are nobody's chosen action
  }
}

struct Step {
  float q, v, r, d;
};

__device__ __forceinline__ Step load_step(const float* __restrict__ qvals, const float* __restrict__ next_vals, const float* __restrict__ rews,
                                          const float* __restrict__ dones, long long t, long long M, long long B, long long j, long long b,
                                          int rew_per_agent) {
  Step s;
  s.q = qvals[t * M + j];
  s.v = next_vals[t * M + j];
  s.r = rew_per_agent ? rews[t * M + j] : rews[t * B + b];
  s.d = dones[t * B + b];
  return s;
}

// MODE 0: the carried recursion (lambda returns; n-step with n >= T runs it at lambda = 1).  MODE 1: n-step, n < T, innermost first.
template <int MODE>
__global__ __launch_bounds__(kRetThreads) void td_return_fwd_kernel(const float* __restrict__ qvals, const float* __restrict__ next_vals,
                                                                    const float* __restrict__ rews, int rew_per_agent,
                                                                    const float* __restrict__ dones, const float* __restrict__ weights,
                                                                    int T, int B, int C, float gamma, int n_step, float lam,
                                                                    float* __restrict__ td, float* __restrict__ g,
                                                                    float* __restrict__ partials) {
  const long long M = static_cast<long long>(B) * C;
  const long long j = static_cast<long long>(blockIdx.x) * kRetThreads + threadIdx.x;
  float acc = 0.f;
  if (j < M) {
    const long long b = M <= 0x7fffffffLL ? static_cast<long long>(static_cast<uint32_t>(j) / static_cast<uint32_t>(C)) : j / C;
    const float w = weights != nullptr ? weights[b] : 1.f;
    const float coef = (2.f * w) / static_cast<float>(static_cast<double>(T) * static_cast<double>(M));
    const float keep = __fsub_rn(1.f, lam);
    float carried = 0.f;      // G_{t+1}
    Step nxt = load_step(qvals, next_vals, rews, dones, T - 1, M, B, j, b, rew_per_agent);
    for (long long t = T - 1; t >= 0; --t) {
      const Step s = nxt;
      if (t > 0) nxt = load_step(qvals, next_vals, rews, dones, t - 1, M, B, j, b, rew_per_agent);   // in flight under step t's arithmetic
      float y;
      if (MODE == 0) {
        float boot = s.v;
        if (t < T - 1 && lam != 0.f)
          boot = lam == 1.f ? carried : __fadd_rn(__fmul_rn(keep, s.v), __fmul_rn(lam, carried));
        y = __fadd_rn(s.r, __fmul_rn(__fmul_rn(gamma, __fsub_rn(1.f, s.d)), boot));
        carried = y;
      } else {
        const long long last = (t + n_step < T ? t + n_step : T) - 1;      // t + m - 1
        y = next_vals[last * M + j];
        for (long long u = last; u > t; --u) {
          const float r = rew_per_agent ? rews[u * M + j] : rews[u * B + b];
          y = __fadd_rn(r, __fmul_rn(__fmul_rn(gamma, __fsub_rn(1.f, dones[u * B + b])), y));
        }
        y = __fadd_rn(s.r, __fmul_rn(__fmul_rn(gamma, __fsub_rn(1.f, s.d)), y));
      }
      const float e = __fsub_rn(s.q, y);
      td[t * M + j] = e;
      g[t * M + j] = coef * e;
      acc = fmaf(w * e, e, acc);
    }
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kSumThreads) void td_loss_sum_kernel(const float* __restrict__ partials, int G, float count,
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

inline long long return_grid(long long B, long long C) { return (B * C + kRetThreads - 1) / kRetThreads; }

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_td_return_partials(int B, int C) {
  if (B < 1 || C < 1 || return_grid(B, C) > 0x7fffffffLL) return UAVGNN_EINVAL;
  return static_cast<int>(return_grid(B, C));
}

extern "C" int uavgnn_td_select_fwd(const float* agent_out, const float* target_out, const long long* acts, int T, long long N, int A,
                                    int double_q, float* qvals, float* next_vals, int* next_acts, uavgnn_stream_t stream) {
  if (!agent_out || !target_out || !acts || !qvals || !next_vals || T < 1 || N < 1 || A < 1) return UAVGNN_EINVAL;
  if (N > 0x7fffffffffffLL / (static_cast<long long>(T) + 1) / A) return UAVGNN_EINVAL;
  const long long rows = static_cast<long long>(T) * N;
  hipLaunchKernelGGL(td_select_fwd_kernel, dim3(capped_grid(rows, kSelThreads)), dim3(kSelThreads), 0, static_cast<hipStream_t>(stream),
                     agent_out, target_out, acts, rows, N, A, double_q != 0 ? 1 : 0, qvals, next_vals, next_acts);
  return launch_status();
}

extern "C" int uavgnn_td_select_bwd(const float* d_qvals, const long long* acts, const float* scale, int T, long long N, int A,
                                    float* d_agent_out, uavgnn_stream_t stream) {
  if (!d_qvals || !acts || !d_agent_out || T < 1 || N < 1 || A < 1) return UAVGNN_EINVAL;
  if (N > 0x7fffffffffffLL / (static_cast<long long>(T) + 1) / A) return UAVGNN_EINVAL;
  const long long rows = static_cast<long long>(T) * N, total = (rows + N) * A;
  hipLaunchKernelGGL(td_select_bwd_kernel, dim3(capped_grid(total, kSelThreads)), dim3(kSelThreads), 0, static_cast<hipStream_t>(stream),
                     d_qvals, acts, scale, rows, total, A, d_agent_out);
  return launch_status();
}

extern "C" int uavgnn_td_return_fwd(const float* qvals, const float* next_vals, const float* rews, int Cr, const float* dones,
                                    const float* weights, int T, int B, int C, float gamma, int mode, int n_step, float lam, float* td,
                                    float* g, float* loss, float* workspace, int G, uavgnn_stream_t stream) {
  if (!qvals || !next_vals || !rews || !dones || !td || !g || !loss || !workspace || T < 1 || B < 1 || C < 1) return UAVGNN_EINVAL;
  if (Cr != 1 && Cr != C) return UAVGNN_EINVAL;
  if (mode == UAVGNN_TD_NSTEP ? n_step < 1 : (mode != UAVGNN_TD_LAMBDA || !(lam >= 0.f && lam <= 1.f))) return UAVGNN_EINVAL;
  if (return_grid(B, C) > 0x7fffffffLL || G != static_cast<int>(return_grid(B, C))) return UAVGNN_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float count = static_cast<float>(static_cast<double>(T) * B * C);
  const int per_agent = (Cr == C && C > 1) ? 1 : 0;
  if (mode == UAVGNN_TD_NSTEP && n_step < T) {
    hipLaunchKernelGGL(td_return_fwd_kernel<1>, dim3(G), dim3(kRetThreads), 0, st, qvals, next_vals, rews, per_agent, dones, weights, T, B, C,
                       gamma, n_step, 0.f, td, g, workspace);
  } else {
    hipLaunchKernelGGL(td_return_fwd_kernel<0>, dim3(G), dim3(kRetThreads), 0, st, qvals, next_vals, rews, per_agent, dones, weights, T, B, C,
                       gamma, 0, mode == UAVGNN_TD_NSTEP ? 1.f : lam, td, g, workspace);
  }
  int rc = launch_status();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(td_loss_sum_kernel, dim3(1), dim3(kSumThreads), 0, st, workspace, G, count, loss);
  return launch_status();
}

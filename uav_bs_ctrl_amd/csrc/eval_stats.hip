// Evaluation episodes and epoch statistics of the device loop: the two launches `test_agent()` and the epoch logger need so that
// neither draws from the host's generator nor copies a value to the host (reference: algos/madrqn/run.py:63-74 test_agent, :115-127
// the logger's mean / std / min / max per key through utils/mpi_tools.py:78-98).
//
// uavgnn_eps_greedy_philox.  The selection rule of uavgnn_eps_greedy (csrc/act_select.hip) with the uniforms drawn INSIDE the kernel:
//   w(index, lane) = philox4x32_10(counter = (index, lane, step_lo, step_hi), key = (seed_lo, seed_hi))[0]
//   u(index, lane) = (w >> 8) * 2^-24                                        an exact float in [0, 1)
//   explore(team)  = u(team, 0) <= eps                                       one draw per team of n_agents consecutive rows
//   acts[a]        = explore(a / n_agents) ? min((int)(u(a, 1) * (float) A), A - 1) : argmax_j q[a, j]      (first maximum)
// {seed, step} are read from DEVICE memory by every thread of the selection launch; a SECOND one-thread launch on the same stream then
// writes step + 1, so no thread of the selection can see a half-advanced counter (the pattern of uavgnn_replay_commit).  A row is a
// pure function of (seed, step, its Q values, A, n_agents, eps): the grid-stride loop may hand it to any thread.
//
// uavgnn_stats_push.  ONE workgroup of 256 threads per key.  Thread t holds the values t, t + 256, ... of the key's row; non-finite
// values only count into field 5.  Pass 1: finite count n_b, sum, min, max -> mean_b = sum / n_b.  Pass 2: M2_b = sum (v - mean_b)^2.
// Every workgroup sum is per-thread partials in index order, a butterfly over the 64 lanes of a wavefront (both partners of an
// exchange add the same two numbers, so all lanes agree) and the four wavefront totals added in wavefront order by EVERY thread (the
// second pass needs mean_b everywhere): a fixed order, no atomics.  Thread 0 then merges (Chan et al.'s pairwise update):
//   d = mean_b - mean;  n' = count + n_b;  mean += d n_b / n';  M2 += M2_b + d^2 count n_b / n';  count = n'
// All in double.  The accumulator is written with plain vector stores by that one thread.
#include "common.h"

#include <math.h>

namespace uavgnn {
namespace {

constexpr int kStatThreads = 256;
constexpr int kStatWaves = kStatThreads / kWave;
constexpr int kMaxKeys = 16;

__device__ __forceinline__ float philox_unit(uint32_t index, uint32_t lane, uint32_t s0, uint32_t s1, uint32_t k0, uint32_t k1) {
  uint32_t c[4] = {index, lane, s0, s1};
  philox4x32_10(c, k0, k1);
  return static_cast<float>(c[0] >> 8) * 0x1p-24f;
}

__global__ void eps_greedy_philox_kernel(const float* __restrict__ q, int ld_q, int N, int A, int n_agents,
                                         const long long* __restrict__ rng, const float* __restrict__ eps_dev, float eps,
                                         long long* __restrict__ acts) {
  if (eps_dev != nullptr) eps = *eps_dev;
  const unsigned long long seed = static_cast<unsigned long long>(rng[0]), step = static_cast<unsigned long long>(rng[1]);
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  const uint32_t s0 = static_cast<uint32_t>(step), s1 = static_cast<uint32_t>(step >> 32);
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long a = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; a < N; a += stride) {
    const float* __restrict__ row = q + static_cast<size_t>(a) * ld_q;
    int best = 0;
    float bv = row[0];
    for (int j = 1; j < A; ++j) {
      const float v = row[j];
      if (v > bv) {     // first maximum wins, NaN never wins (as uavgnn_eps_greedy)
        bv = v;
        best = j;
      }
    }
    const bool explore = philox_unit(static_cast<uint32_t>(a / n_agents), 0u, s0, s1, k0, k1) <= eps;
    int r = static_cast<int>(philox_unit(static_cast<uint32_t>(a), 1u, s0, s1, k0, k1) * static_cast<float>(A));
    r = r < A ? r : A - 1;
    acts[a] = explore ? r : best;
  }
}

__global__ void rng_advance_kernel(long long* __restrict__ rng) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  rng[1] = static_cast<long long>(static_cast<unsigned long long>(rng[1]) + 1ull);
}

struct OpSum {
  __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
};
struct OpMin {
  __device__ __forceinline__ double operator()(double a, double b) const { return a < b ? a : b; }
};
struct OpMax {
  __device__ __forceinline__ double operator()(double a, double b) const { return a > b ? a : b; }
};

// workgroup reduction in a fixed order; every thread returns the result.  `part` is LDS of kStatWaves doubles.
template <class Op>
__device__ __forceinline__ double block_reduce(double v, double* part, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  __syncthreads();                       // the previous reduction's readers are done with `part`
  if (lane == 0) part[wave] = v;
  __syncthreads();
  double r = part[0];
#pragma unroll
  for (int w = 1; w < kStatWaves; ++w) r = op(r, part[w]);
  return r;
}

__global__ __launch_bounds__(kStatThreads) void stats_push_kernel(const double* __restrict__ vals, int ld, int n,
                                                                  double* __restrict__ acc) {
  __shared__ double part[kStatWaves];
  const double* __restrict__ row = vals + static_cast<size_t>(blockIdx.x) * ld;
  double* __restrict__ a = acc + static_cast<size_t>(blockIdx.x) * 6;
  const int tid = threadIdx.x;
  double sum = 0.0, cnt = 0.0, bad = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < n; i += kStatThreads) {
    const double v = row[i];
    if (isfinite(v)) {
      sum += v;
      cnt += 1.0;
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    } else {
      bad += 1.0;
    }
  }
  sum = block_reduce(sum, part, OpSum());
  cnt = block_reduce(cnt, part, OpSum());         // counts below 2^31: exact in double
  bad = block_reduce(bad, part, OpSum());
  lo = block_reduce(lo, part, OpMin());
  hi = block_reduce(hi, part, OpMax());
  const double mean_b = cnt > 0.0 ? sum / cnt : 0.0;
  double m2 = 0.0;
  for (int i = tid; i < n; i += kStatThreads) {
    const double v = row[i];
    if (isfinite(v)) {
      const double d = v - mean_b;
      m2 += d * d;
    }
  }
  m2 = block_reduce(m2, part, OpSum());
  if (tid != 0) return;
  if (cnt > 0.0) {
    const double count = a[0], mean = a[1];
    const double d = mean_b - mean, n2 = count + cnt;
    a[0] = n2;
    a[1] = mean + d * cnt / n2;
    a[2] = a[2] + (m2 + d * d * count * cnt / n2);
    a[3] = lo < a[3] ? lo : a[3];
    a[4] = hi > a[4] ? hi : a[4];
  }
  if (bad > 0.0) a[5] = a[5] + bad;
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_eps_greedy_philox(const float* q, int ld_q, int N, int A, int n_agents, long long* rng, const float* eps_dev,
                                        float eps, long long* acts, uavgnn_stream_t stream) {
  if (N < 0 || A < 1 || n_agents < 1 || ld_q < A || !rng || (N > 0 && (!q || !acts))) return UAVGNN_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (N > 0)
    hipLaunchKernelGGL(eps_greedy_philox_kernel, dim3(capped_grid(N, 256)), dim3(256), 0, st, q, ld_q, N, A, n_agents, rng, eps_dev,
                       eps, acts);
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  return launch_status();
}

extern "C" int uavgnn_stats_push(const double* vals, int ld, int n, int n_keys, double* acc, uavgnn_stream_t stream) {
  if (n < 0 || n_keys < 1 || n_keys > kMaxKeys || ld < n || !vals || !acc) return UAVGNN_EINVAL;
  if (n == 0) return 0;
  hipLaunchKernelGGL(stats_push_kernel, dim3(n_keys), dim3(kStatThreads), 0, static_cast<hipStream_t>(stream), vals, ld, n, acc);
  return launch_status();
}

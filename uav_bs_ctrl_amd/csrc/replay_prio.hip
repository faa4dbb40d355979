// Proportional prioritised replay over sequences on the device (Schaul et al., "Prioritized experience replay", ICLR'16; the sequence
// form of Kapturowski et al., "Recurrent experience replay in distributed reinforcement learning", ICLR'19): priorities of new
// sequences, the stratified proportional sampler with its importance weights, and the priority update from an update's TD errors.
//
// Priorities are UNSIGNED 32-BIT FIXED POINT: PRIO_ONE = 2^20 stands for 1.0, one word per ring slot (prio [capacity]) and a one-word
// running maximum (prio_max, initially PRIO_ONE).  Which slot is drawn is decided by integer arithmetic alone - no float enters a
// decision - so a draw is the same bits run to run and has an exact restatement (tests/replay_prio_ref.py).  state {head, size}, rng
// {seed, draws} and status are those of csrc/replay.hip; status bit 1: a priority update was skipped.
//
// uavgnn_replay_prio_commit.  prio[(head + e) % capacity] = *prio_max for e < E: a new sequence is drawn at least as readily as any the
// ring holds.  Issued BEFORE uavgnn_replay_commit, whose second launch advances head.  One launch.
//
// uavgnn_replay_prio_sample.  B slots of [0, size), proportional to priority, stratified, WITH replacement.  THE RULE:
//   1  S = sum of prio[s] over s < size, a 64-bit integer.  Slots at or beyond size are never read into a decision.
//   2  S = qB B + rB; stratum k < B is [lo_k, hi_k) with lo_k = k qB + (k rB) / B (integer division), hi_k = lo_{k+1} (hi_{B-1} = S).
//      No product exceeds 64 bits for B <= 65535: k qB <= S < 2^62, k rB < 2^32.
//   3  r_k = words 0 and 1 (word 0 the low half) of philox4x32_10(counter = (k, 1, draws_lo, draws_hi), key = (seed_lo, seed_hi)).
//      The second counter word 1 keeps the stream apart from the uniform sampler's (k, 0, ..).
//   4  target_k = lo_k + (hi_k > lo_k ? r_k mod (hi_k - lo_k) : 0)
//   5  idx[k] = the slot s with prefix[s] <= target_k < prefix[s] + prio[s], prefix the exclusive prefix sum of prio over s < size.
//      Targets ascend with k, so idx comes out in ASCENDING order and may hold repeats (uavgnn_replay_gather and
//      uavgnn_replay_rebuild_obs accept repeats).
//   6  weights[k] = (float) (w_k / max_j w_j),  w_k = pow((double) size * (double) prio[idx_k] / (double) S, -beta), all in double
//      (the product first, then the quotient; the division by the maximum last).
//   7  draws += 1.
//   8  size == 0 (or S == 0: a ring whose priorities below size are all zero, which neither _commit nor _update ever writes):
//      status |= 1, idx[k] = 0, weights[k] = 1, draws += 1 all the same.
// Four launches on the caller's stream, ordered by the stream alone (no flag, no spin-wait, no "last block done" counter); their number
// and grids depend on (capacity, B) only, never on the device-side size, so the call captures into a graph:
//   1  sums      G = ceil(capacity / 4096) workgroups of 256 threads: the 64-bit sum of a chunk of 4096 slots (16 per thread, coalesced,
//                slots >= size count zero) -> chunk[g].  EVERY workgroup writes its word, so nothing of the workspace is read before
//                this call wrote it.
//   2  place     one workgroup: exclusive scan of chunk[] in place (thread t owns a contiguous run of ceil(G / 256) chunks; the 256 run
//                totals are scanned through the wavefronts and LDS), header {size, S}, then target_k for k < B (rule 2-4).
//   3  resolve   one wavefront per sample: binary search of the chunk (the last g with chunk[g] <= target), then up to 64 trips of 64
//                slots - a 64-bit wavefront prefix sum, the first lane whose inclusive sum exceeds the target is the slot - and
//                idx[k], picked[k] = prio[idx[k]].
//   4  tail      one workgroup: the weights (rule 6: two passes over picked[], a workgroup maximum in between; 0 <= beta <= 16
//                keeps every power finite), status, draws += 1.
// Algorithmic bytes per draw: 4 size (the priorities, once) + B x (8 log2 G + <= 16 KB of one chunk, from L2) + 28 B.
//
// workspace (16-byte aligned, caller-owned, uavgnn_replay_prio_workspace_bytes(capacity, B) bytes; holds nothing across calls):
//   uint64 [0, 4)            header {size, S, -, -}
//   uint64 [4, 4 + G)        chunk sums, then their exclusive prefix sums
//   uint64 [4 + G, .. + B)   targets
//   uint32 [B]               picked priorities
//
// uavgnn_replay_prio_update.  td [T, B, C] float32: the TD errors of the update just formed.  For sequence b, in double:
//   a = eta max |td[:, b, :]| + (1 - eta) mean |td[:, b, :]|        (each product rounded on its own: no contraction)
//   q = clamp(llrint(pow(a + eps, alpha) 2^20), 1, 2^32 - 1)        (alpha == 1: a + eps itself, so the value is exact)
//   prio[idx[b]] = q  and  *prio_max = max(*prio_max, q)            (one integer atomic maximum per workgroup)
// idx ascends, so repeats are adjacent: only the LAST row of a run of equal indices stores its q (every valid row enters the maximum).
// A non-finite a, or an index outside [0, capacity), writes nothing and ORs status bit 1.  One launch: a workgroup owns floor(256 / C)
// consecutive sequences (one when C > 256), whose step rows td[t, b0 : b0 + rows, :] are contiguous - thread j keeps maximum and sum of
// column j over the T steps (consecutive lanes, consecutive floats), then one thread per sequence folds its C partials from LDS.
#include "common.h"

namespace uavgnn {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPerThread = 16;
constexpr int kSlots = kThreads * kPerThread;          // the chunk of one workgroup
constexpr int kMaxCapacity = 1 << 30;
constexpr int kMaxBatch = 65535;
constexpr double kMaxBeta = 16.0;                      // size prio / S lies in [2^-62, 2^62]: its power -beta stays finite in double
constexpr int kHead = 4;                               // header words (uint64)
using u64 = unsigned long long;

inline int groups_of(int capacity) { return (capacity + kSlots - 1) / kSlots; }

__device__ __forceinline__ int clamped_size(const long long* __restrict__ state, int capacity) {
  const long long size64 = state[1];
  return size64 < 0 ? 0 : (size64 > capacity ? capacity : static_cast<int>(size64));
}

__device__ __forceinline__ u64 wave_inclusive_scan64(u64 v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const u64 up = __shfl_up(v, o);
    v += lane >= o ? up : 0ull;
  }
  return v;
}

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void replay_prio_commit_kernel(const long long* __restrict__ state, int E, int capacity, uint32_t* __restrict__ prio,
                                          const uint32_t* __restrict__ prio_max) {
  const int e = static_cast<int>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= E) return;
  long long head = state[0];
  if (head < 0 || head >= capacity) head = ((head % capacity) + capacity) % capacity;   // as replay_commit_kernel
  prio[(head + e) % capacity] = *prio_max;
}

__global__ __launch_bounds__(kThreads) void replay_prio_sums_kernel(const long long* __restrict__ state, int capacity,
                                                                    const uint32_t* __restrict__ prio, u64* __restrict__ ws) {
  __shared__ u64 part[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, g = blockIdx.x;
  const int size = clamped_size(state, capacity);
  const int lo = g * kSlots;
  u64 sum = 0ull;
  if (lo < size) {
#pragma unroll 4
    for (int j = 0; j < kPerThread; ++j) {
      const int s = lo + j * kThreads + tid;
      if (s < size) sum += prio[s];
    }
  }
  sum = wave_sum64(sum);
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  if (tid == 0) ws[kHead + g] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(kThreads) void replay_prio_place_kernel(const long long* __restrict__ state,
                                                                     const long long* __restrict__ rng, int capacity, int B, int G,
                                                                     u64* __restrict__ ws) {
  __shared__ u64 wave_tot[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  u64* __restrict__ chunk = ws + kHead;
  const int per = (G + kThreads - 1) / kThreads;
  const int c0 = tid * per < G ? tid * per : G, c1 = c0 + per < G ? c0 + per : G;
  u64 mine = 0ull;
  for (int c = c0; c < c1; ++c) mine += chunk[c];
  const u64 inc = wave_inclusive_scan64(mine, lane);
  if (lane == kWave - 1) wave_tot[wave] = inc;
  __syncthreads();
  u64 before = inc - mine, S = 0ull;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    before += w < wave ? wave_tot[w] : 0ull;
    S += wave_tot[w];
  }
  for (int c = c0; c < c1; ++c) {                      // in place: this thread alone reads and writes its run
    const u64 v = chunk[c];
    chunk[c] = before;
    before += v;
  }
  const int size = clamped_size(state, capacity);
  if (tid == 0) {
    ws[0] = static_cast<u64>(size);
    ws[1] = S;
  }
  if (size == 0 || S == 0ull) return;
  const u64 seed = static_cast<u64>(rng[0]), draws = static_cast<u64>(rng[1]);
  const u64 qB = S / static_cast<u64>(B), rB = S % static_cast<u64>(B);
  u64* __restrict__ target = chunk + G;
  for (int k = tid; k < B; k += kThreads) {
    const u64 lo = static_cast<u64>(k) * qB + static_cast<u64>(k) * rB / static_cast<u64>(B);
    const u64 hi = k + 1 == B ? S : static_cast<u64>(k + 1) * qB + static_cast<u64>(k + 1) * rB / static_cast<u64>(B);
    uint32_t c[4] = {static_cast<uint32_t>(k), 1u, static_cast<uint32_t>(draws), static_cast<uint32_t>(draws >> 32)};
    philox4x32_10(c, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
    const u64 r = (static_cast<u64>(c[1]) << 32) | c[0];
    target[k] = lo + (hi > lo ? r % (hi - lo) : 0ull);
  }
}

__global__ __launch_bounds__(kThreads) void replay_prio_resolve_kernel(const uint32_t* __restrict__ prio, int B, int G,
                                                                       const u64* __restrict__ ws, long long* __restrict__ idx,
                                                                       uint32_t* __restrict__ picked) {
  const int lane = threadIdx.x & (kWave - 1);
  const int k = static_cast<int>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (k >= B) return;                                  // uniform per wavefront
  const int size = static_cast<int>(ws[0]);
  const u64 S = ws[1];
  if (size == 0 || S == 0ull) {
    if (lane == 0) idx[k] = 0;
    return;
  }
  const u64* __restrict__ chunk = ws + kHead;
  const u64 target = chunk[G + k];                     // < S
  int a = 0, b = G - 1;                                // the last g with chunk[g] <= target (chunk[0] = 0): its sum holds the target
  while (a < b) {
    const int m = (a + b + 1) >> 1;
    if (chunk[m] <= target) a = m;
    else b = m - 1;
  }
  u64 base = chunk[a];
  const int lo = a * kSlots;
  int found = size - 1;                                // never kept: target < S puts it inside the chunk
  for (int it = 0; it < kSlots / kWave; ++it) {
    const int s = lo + it * kWave + lane;
    const u64 v = s < size ? prio[s] : 0ull;
    const u64 inc = base + wave_inclusive_scan64(v, lane);
    const u64 hit = __ballot(inc > target);
    if (hit) {
      found = lo + it * kWave + (__ffsll(hit) - 1);
      break;
    }
    base = __shfl(inc, kWave - 1);
  }
  if (lane == 0) {
    idx[k] = found;
    picked[k] = prio[found];
  }
}

__global__ __launch_bounds__(kThreads) void replay_prio_tail_kernel(long long* __restrict__ rng, int B, double beta,
                                                                    const u64* __restrict__ ws, const uint32_t* __restrict__ picked,
                                                                    float* __restrict__ weights, int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double wave_top[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int size = static_cast<int>(ws[0]);
  const u64 S = ws[1];
  if (size == 0 || S == 0ull) {
    for (int k = tid; k < B; k += kThreads) weights[k] = 1.0f;
    if (tid == 0) {
      atomicOr(status, 1);
      rng[1] = rng[1] + 1;
    }
    return;
  }
  const double n = static_cast<double>(size), total = static_cast<double>(S);
  double top = 0.0;                                    // every w is positive: prio[idx] >= 1 on a slot that holds the target
  for (int k = tid; k < B; k += kThreads) top = fmax(top, pow(n * static_cast<double>(picked[k]) / total, -beta));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = fmax(top, __shfl_xor(top, o));
  if (lane == 0) wave_top[wave] = top;
  __syncthreads();
  top = fmax(fmax(wave_top[0], wave_top[1]), fmax(wave_top[2], wave_top[3]));
  for (int k = tid; k < B; k += kThreads)
    weights[k] = static_cast<float>(pow(n * static_cast<double>(picked[k]) / total, -beta) / top);
  if (tid == 0) rng[1] = rng[1] + 1;
}

__global__ __launch_bounds__(kThreads) void replay_prio_update_kernel(const float* __restrict__ td, int T, int B, int C, int nb,
                                                                      const long long* __restrict__ idx, int capacity, double alpha,
                                                                      double eta, double eps, uint32_t* __restrict__ prio,
                                                                      uint32_t* __restrict__ prio_max, int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double part_top[kThreads], part_sum[kThreads];
  __shared__ uint32_t block_top;
  const int tid = threadIdx.x;
  const int b0 = static_cast<int>(blockIdx.x) * nb;
  const int rows = B - b0 < nb ? B - b0 : nb;          // sequences of this workgroup: b0 .. b0 + rows - 1
  const int width = rows * C;                          // td[t, b0 : b0 + rows, :] is `width` contiguous floats (rows == 1 when C > 256)
  if (tid == 0) block_top = 0u;
  double top = 0.0, sum = 0.0;
  for (int e = tid; e < width; e += kThreads) {        // consecutive lanes read consecutive floats of every step
    const float* __restrict__ col = td + static_cast<long long>(b0) * C + e;
    for (int t = 0; t < T; ++t) {
      const double v = fabs(static_cast<double>(col[static_cast<long long>(t) * B * C]));
      top = fmax(top, v);                              // a NaN is dropped here and kept by the sum: a is non-finite either way
      sum += v;
    }
  }
  part_top[tid] = top;
  part_sum[tid] = sum;
  __syncthreads();
  if (tid < rows) {
    const int first = nb == 1 ? 0 : tid * C, last = nb == 1 ? kThreads : first + C;
    top = 0.0;
    sum = 0.0;
    for (int k = first; k < last; ++k) {
      top = fmax(top, part_top[k]);
      sum += part_sum[k];
    }
    const int b = b0 + tid;
    const double mean = sum / (static_cast<double>(T) * static_cast<double>(C));
    const double lead = eta * top, rest = (1.0 - eta) * mean;
    const double a = lead + rest;
    const long long s = idx[b];
    if (!(fabs(a) <= 1.79769313486231570815e308) || s < 0 || s >= capacity) {
      atomicOr(status, 2);
    } else {
      const double x = a + eps;
      const double v = (alpha == 1.0 ? x : pow(x, alpha)) * 1048576.0;
      const uint32_t q = !(v >= 1.0) ? 1u : (v >= 4294967295.0 ? 0xFFFFFFFFu : static_cast<uint32_t>(llrint(v)));
      if (b + 1 == B || idx[b + 1] != s) prio[s] = q;
      atomicMax(&block_top, q);
    }
  }
  __syncthreads();
  if (tid == 0 && block_top != 0u) atomicMax(prio_max, block_top);
}

inline bool aligned(const void* p, long long a) { return reinterpret_cast<uintptr_t>(p) % static_cast<uintptr_t>(a) == 0; }

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" long long uavgnn_replay_prio_workspace_bytes(int capacity, int B) {
  if (capacity < 1 || capacity > kMaxCapacity || B < 1 || B > kMaxBatch) return 0;
  const long long bytes = 8ll * (kHead + groups_of(capacity) + B) + 4ll * B;
  return (bytes + 15) / 16 * 16;
}

extern "C" int uavgnn_replay_prio_commit(const long long* state, int E, int capacity, uint32_t* prio, const uint32_t* prio_max,
                                         uavgnn_stream_t stream) {
  if (!state || E < 0 || capacity < 1 || E > capacity || !prio || !prio_max) return UAVGNN_EINVAL;
  if (!aligned(prio, 4) || !aligned(prio_max, 4)) return UAVGNN_EINVAL;
  if (capacity > kMaxCapacity || E > 65535) return UAVGNN_EUNSUPPORTED;
  if (E == 0) return 0;
  hipLaunchKernelGGL(replay_prio_commit_kernel, dim3((E + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), state, E, capacity, prio, prio_max);
  return launch_status();
}

extern "C" int uavgnn_replay_prio_sample(const long long* state, long long* rng, int capacity, int B, const uint32_t* prio, double beta,
                                         long long* idx, float* weights, int32_t* status, void* workspace, uavgnn_stream_t stream) {
  if (!state || !rng || capacity < 1 || B < 1 || !prio || !idx || !weights || !status || !workspace) return UAVGNN_EINVAL;
  if (!aligned(workspace, 16) || !aligned(prio, 4) || !(beta >= 0.0 && beta <= kMaxBeta)) return UAVGNN_EINVAL;
  if (capacity > kMaxCapacity || B > kMaxBatch) return UAVGNN_EUNSUPPORTED;
  const int G = groups_of(capacity);
  u64* ws = static_cast<u64*>(workspace);
  uint32_t* picked = reinterpret_cast<uint32_t*>(ws + kHead + G + B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(replay_prio_sums_kernel, dim3(G), dim3(kThreads), 0, st, state, capacity, prio, ws);
  hipLaunchKernelGGL(replay_prio_place_kernel, dim3(1), dim3(kThreads), 0, st, state, rng, capacity, B, G, ws);
  hipLaunchKernelGGL(replay_prio_resolve_kernel, dim3((B + kWaves - 1) / kWaves), dim3(kThreads), 0, st, prio, B, G, ws, idx, picked);
  hipLaunchKernelGGL(replay_prio_tail_kernel, dim3(1), dim3(kThreads), 0, st, rng, B, beta, ws, picked, weights, status);
  return launch_status();
}

extern "C" int uavgnn_replay_prio_update(const float* td, int T, int B, int C, const long long* idx, int capacity, double alpha, double eta,
                                         double eps, uint32_t* prio, uint32_t* prio_max, int32_t* status, uavgnn_stream_t stream) {
  if (T < 1 || B < 0 || C < 1 || capacity < 1 || !prio || !prio_max || !status || (B > 0 && (!td || !idx))) return UAVGNN_EINVAL;
  if (!(alpha == alpha) || !(eta == eta) || !(eps == eps) || !aligned(prio, 4) || !aligned(prio_max, 4)) return UAVGNN_EINVAL;
  if (capacity > kMaxCapacity || B > kMaxBatch || static_cast<long long>(T) * C > 0x7fffffffll) return UAVGNN_EUNSUPPORTED;
  if (B == 0) return 0;
  const int nb = C <= kThreads ? kThreads / C : 1;     // sequences per workgroup: their step rows are contiguous in td
  hipLaunchKernelGGL(replay_prio_update_kernel, dim3((B + nb - 1) / nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream), td, T, B, C,
                     nb, idx, capacity, alpha, eta, eps, prio, prio_max, status);
  return launch_status();
}

// The replay sampler for rings of up to 2^30 sequences: uavgnn_replay_sample under THE RULE of csrc/replay.hip - same keys, same
// B smallest (key, slot) pairs, ties at the threshold key by slot, ascending slot order, draws += 1, the same wrap at size < B - on as
// many workgroups as the ring needs.  Same bits as the one-workgroup kernel wherever both apply; capacity in [1, 2^30].
//
// One workgroup of 256 threads owns a contiguous chunk of kSlots = 4096 slots (16 per thread); G = ceil(capacity / 4096) workgroups per
// launch, a grid the HOST knows - never the device-side size, so the call captures into a graph.  A workgroup whose chunk begins at or
// beyond size returns at once.  Seven launches on the caller's stream, ordered by the stream alone (no spin-wait, no "last block done"
// counter, no floating point; what crosses workgroups is atomicAdd on 32-bit integers, commutative, so the same bits run to run):
//   1  zero      one workgroup: zeroes the four 256-bin histograms and the super-group totals, and SNAPSHOTS {size clamped into
//                [0, capacity], seed, draws} into the workspace: the launches below read the snapshot, so the one thread that advances
//                rng[1] in the last launch races with no reader of it
//   2-5 hist p   key byte p, most significant first.  Every wavefront first locates the bins of the bytes before p from the global
//                histograms (1 KB each; redundant and identical in every wavefront - no one-workgroup "locate" launch, no LDS), then
//                the workgroup histograms byte p of its keys that match the prefix in LDS and adds its non-zero bins to the global one
//   6  count     the threshold key and k (how many slots holding exactly that key are taken) are known: per workgroup the numbers of
//                keys below / at the threshold -> wg_lt / wg_eq [G], and added to the totals of its super-group of 512 workgroups
//   7  write     exclusive offsets of a workgroup = super-group totals before its super-group + workgroup counts before it inside the
//                super-group (<= 511 + 511 words, summed by the 256 threads: the scan is O(1024) per workgroup at any G); thread t
//                compacts its 16 contiguous slots from the workgroup prefix sum, taking the first k threshold-key slots globally.
//                size < B: status |= 1 and the wrapped indices, grid-strided over all workgroups.  Workgroup 0, thread 0: draws += 1.
// Keys are RECOMPUTED in every launch (6 Philox calls per slot and draw, about 100 integer operations each, 16 per thread and launch)
// instead of stored once: the workspace stays O(G) words (8.2 KB + 8 B per workgroup: 2.1 MB at 2^30 slots against 4 GB of keys), and
// a draw is bound by its seven launches up to 2^20 slots (profiles/replay_sampler_wide_probe.txt), not by the keys.
//
// workspace (uint32 words, 16-byte aligned, caller-owned, nothing read before this call wrote it):
//   [0, 8)          snapshot {size, seed_lo, seed_hi, draws_lo, draws_hi, -, -, -}
//   [8, 1032)       hist[4][256]
//   [1032, 2056)    super_lt[512], super_eq[512]
//   [2056, 2056+2G) wg_lt[G], wg_eq[G]     (written by the count launch for every workgroup the write launch reads: never zeroed)
#include "common.h"
#include "replay_sample.h"

namespace uavgnn {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPerThread = 16;
constexpr int kSlots = kThreads * kPerThread;          // the chunk of one workgroup
constexpr int kMaxCapacity = 1 << 30;
constexpr int kSuper = 512;                            // workgroups per super-group
constexpr int kMaxSupers = kMaxCapacity / kSlots / kSuper;
constexpr int kHeadWords = 8, kHistWords = 4 * 256;
constexpr int kHistAt = kHeadWords, kSuperAt = kHistAt + kHistWords, kGroupAt = kSuperAt + 2 * kMaxSupers;
static_assert(kMaxSupers == 512 && 2 * kThreads >= kSuper && 2 * kThreads >= kMaxSupers, "the write launch sums two words per thread");

inline int groups_of(int capacity) { return (capacity + kSlots - 1) / kSlots; }

struct Snapshot {
  int size;
  SampleKey key;
  unsigned long long draws;
};

__device__ __forceinline__ Snapshot snapshot_of(const uint32_t* __restrict__ ws) {
  Snapshot s;
  s.size = static_cast<int>(ws[0]);
  s.key = SampleKey{ws[3], ws[4], ws[1], ws[2]};
  s.draws = (static_cast<unsigned long long>(ws[4]) << 32) | ws[3];
  return s;
}

// The radix select so far: from the global histograms of the first `passes` key bytes, the key prefix of the B-th smallest pair and how
// many of the pairs at / below it are still to be taken.  Every lane of the calling wavefront returns the same values; lane l owns bins
// 4 l .. 4 l + 3.  1 <= B <= number of keys, so exactly one bin answers per pass.
__device__ __forceinline__ void locate(const uint32_t* __restrict__ hist, int passes, int B, int lane, uint32_t& prefix, int& k) {
  prefix = 0u;
  k = B;
  for (int p = 0; p < passes; ++p) {
    const uint4 hv = reinterpret_cast<const uint4*>(hist + 256 * p)[lane];
    const int h[4] = {static_cast<int>(hv.x), static_cast<int>(hv.y), static_cast<int>(hv.z), static_cast<int>(hv.w)};
    const int tot = h[0] + h[1] + h[2] + h[3];
    int below = wave_inclusive_scan(tot, lane) - tot;
    int bin = -1, rem = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (below < k && k <= below + h[j]) {
        bin = 4 * lane + j;
        rem = k - below;
      }
      below += h[j];
    }
    const unsigned long long owners = __ballot(bin >= 0);
    const int src = owners ? __ffsll(owners) - 1 : 0;
    bin = __shfl(bin, src);
    rem = __shfl(rem, src);
    prefix |= static_cast<uint32_t>(bin & 255) << (24 - 8 * p);
    k = rem;
  }
}

__global__ __launch_bounds__(kThreads) void replay_wide_zero_kernel(const long long* __restrict__ state,
                                                                    const long long* __restrict__ rng, int capacity,
                                                                    uint32_t* __restrict__ ws) {
  const int tid = threadIdx.x;
  for (int i = kHistAt + tid; i < kGroupAt; i += kThreads) ws[i] = 0u;
  if (tid == 0) {
    const long long size64 = state[1];
    const unsigned long long seed = static_cast<unsigned long long>(rng[0]), draws = static_cast<unsigned long long>(rng[1]);
    ws[0] = static_cast<uint32_t>(size64 < 0 ? 0 : (size64 > capacity ? capacity : static_cast<int>(size64)));
    ws[1] = static_cast<uint32_t>(seed);
    ws[2] = static_cast<uint32_t>(seed >> 32);
    ws[3] = static_cast<uint32_t>(draws);
    ws[4] = static_cast<uint32_t>(draws >> 32);
  }
}

__global__ __launch_bounds__(kThreads) void replay_wide_hist_kernel(uint32_t* __restrict__ ws, int B, int pass) {
  __shared__ uint32_t hist[256];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const Snapshot sn = snapshot_of(ws);
  const int lo = static_cast<int>(blockIdx.x) * kSlots;
  if (sn.size < B || lo >= sn.size) return;            // uniform: the whole workgroup leaves
  uint32_t prefix;
  int k;
  locate(ws + kHistAt, pass, B, lane, prefix, k);
  const uint32_t mask = pass == 0 ? 0u : ~0u << (32 - 8 * pass);
  const int shift = 24 - 8 * pass;
  hist[tid] = 0u;
  __syncthreads();
#pragma unroll 4
  for (int j = 0; j < kPerThread; ++j) {
    const int s = lo + j * kThreads + tid;
    if (s < sn.size) {
      const uint32_t ks = sn.key(static_cast<uint32_t>(s));
      if ((ks & mask) == prefix) atomicAdd(&hist[(ks >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  const uint32_t mine = hist[tid];
  if (mine != 0u) atomicAdd(&ws[kHistAt + 256 * pass + tid], mine);
}

__global__ __launch_bounds__(kThreads) void replay_wide_count_kernel(uint32_t* __restrict__ ws, int B, int G) {
  __shared__ int wave_lt[kWaves], wave_eq[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, g = blockIdx.x;
  const Snapshot sn = snapshot_of(ws);
  const int lo = g * kSlots;
  if (sn.size < B || lo >= sn.size) return;
  uint32_t thr;
  int k;
  locate(ws + kHistAt, 4, B, lane, thr, k);
  int n_lt = 0, n_eq = 0;                              // of the wavefront: the same in every lane
#pragma unroll 4
  for (int j = 0; j < kPerThread; ++j) {
    const int s = lo + j * kThreads + tid;
    const uint32_t ks = sn.key(static_cast<uint32_t>(s));
    const bool in = s < sn.size;
    n_lt += __popcll(__ballot(in && ks < thr));
    n_eq += __popcll(__ballot(in && ks == thr));
  }
  if (lane == 0) {
    wave_lt[wave] = n_lt;
    wave_eq[wave] = n_eq;
  }
  __syncthreads();
  if (tid == 0) {
    int lt = 0, eq = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      lt += wave_lt[w];
      eq += wave_eq[w];
    }
    ws[kGroupAt + g] = static_cast<uint32_t>(lt);
    ws[kGroupAt + G + g] = static_cast<uint32_t>(eq);
    if (lt != 0) atomicAdd(&ws[kSuperAt + g / kSuper], static_cast<uint32_t>(lt));
    if (eq != 0) atomicAdd(&ws[kSuperAt + kMaxSupers + g / kSuper], static_cast<uint32_t>(eq));
  }
}

__global__ __launch_bounds__(kThreads) void replay_wide_write_kernel(const uint32_t* __restrict__ ws, long long* __restrict__ rng, int B,
                                                                     int G, long long* __restrict__ idx, int* __restrict__ status) {
  __shared__ int wave_lt[kWaves], wave_eq[kWaves], part_lt[kWaves], part_eq[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, g = blockIdx.x;
  const Snapshot sn = snapshot_of(ws);
  const bool advances = g == 0 && tid == 0;            // the one thread that writes rng[1]; nothing of this call reads it any more
  if (sn.size < B) {
    const int m = sn.size > 1 ? sn.size : 1;
    for (long long i = static_cast<long long>(g) * kThreads + tid; i < B; i += static_cast<long long>(gridDim.x) * kThreads)
      idx[i] = i % m;
    if (advances) {
      atomicOr(status, 1);
      rng[1] = static_cast<long long>(sn.draws + 1);
    }
    return;
  }
  if (B == 0) {                                        // nothing to select (the host launches one workgroup)
    if (advances) rng[1] = static_cast<long long>(sn.draws + 1);
    return;
  }
  const int lo = g * kSlots;
  if (lo >= sn.size) return;                           // never workgroup 0: size >= B >= 1
  uint32_t thr;
  int k;
  locate(ws + kHistAt, 4, B, lane, thr, k);
  // ---- pairs below / at the threshold in the workgroups before this one -------------------------------------------------------------
  const int sg = g / kSuper, first = sg * kSuper;
  int p_lt = 0, p_eq = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = tid + h * kThreads;
    if (i < sg) {
      p_lt += static_cast<int>(ws[kSuperAt + i]);
      p_eq += static_cast<int>(ws[kSuperAt + kMaxSupers + i]);
    }
    if (first + i < g) {
      p_lt += static_cast<int>(ws[kGroupAt + first + i]);
      p_eq += static_cast<int>(ws[kGroupAt + G + first + i]);
    }
  }
  p_lt = wave_inclusive_scan(p_lt, lane);
  p_eq = wave_inclusive_scan(p_eq, lane);
  // ---- this thread's 16 contiguous slots ------------------------------------------------------------------------------------------------
  const int t_lo = lo + tid * kPerThread;
  uint32_t lt_mask = 0u, eq_mask = 0u;
#pragma unroll 4
  for (int j = 0; j < kPerThread; ++j) {
    const int s = t_lo + j;
    const uint32_t ks = sn.key(static_cast<uint32_t>(s));
    const bool in = s < sn.size;
    lt_mask |= static_cast<uint32_t>(in && ks < thr) << j;
    eq_mask |= static_cast<uint32_t>(in && ks == thr) << j;
  }
  const int n_lt = __popc(lt_mask), n_eq = __popc(eq_mask);
  const int inc_lt = wave_inclusive_scan(n_lt, lane), inc_eq = wave_inclusive_scan(n_eq, lane);
  if (lane == kWave - 1) {
    wave_lt[wave] = inc_lt;
    wave_eq[wave] = inc_eq;
    part_lt[wave] = p_lt;
    part_eq[wave] = p_eq;
  }
  __syncthreads();
  int lt_before = inc_lt - n_lt, eq_before = inc_eq - n_eq;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    lt_before += part_lt[w] + (w < wave ? wave_lt[w] : 0);
    eq_before += part_eq[w] + (w < wave ? wave_eq[w] : 0);
  }
  int out = lt_before + (eq_before < k ? eq_before : k);
#pragma unroll 4
  for (int j = 0; j < kPerThread; ++j) {
    const bool lt = (lt_mask >> j) & 1u, eq = (eq_mask >> j) & 1u;
    const bool take = lt || (eq && eq_before < k);
    eq_before += eq;
    if (take && out < B) idx[out] = t_lo + j;
    out += take;
  }
  if (advances) rng[1] = static_cast<long long>(sn.draws + 1);
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" long long uavgnn_replay_sample_wide_workspace_bytes(int capacity) {
  if (capacity < 1 || capacity > kMaxCapacity) return 0;
  return 4ll * (kGroupAt + 2ll * groups_of(capacity));
}

extern "C" int uavgnn_replay_sample_wide_slots_per_workgroup(void) { return kSlots; }

extern "C" int uavgnn_replay_sample_wide(const long long* state, long long* rng, int capacity, int B, long long* idx, int32_t* status,
                                         void* workspace, uavgnn_stream_t stream) {
  if (!state || !rng || capacity < 1 || B < 0 || (B > 0 && !idx) || !status || !workspace) return UAVGNN_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return UAVGNN_EINVAL;
  if (capacity > kMaxCapacity) return UAVGNN_EUNSUPPORTED;
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int G = groups_of(capacity);
  hipLaunchKernelGGL(replay_wide_zero_kernel, dim3(1), dim3(kThreads), 0, st, state, rng, capacity, ws);
  if (B > 0) {
    for (int pass = 0; pass < 4; ++pass) hipLaunchKernelGGL(replay_wide_hist_kernel, dim3(G), dim3(kThreads), 0, st, ws, B, pass);
    hipLaunchKernelGGL(replay_wide_count_kernel, dim3(G), dim3(kThreads), 0, st, ws, B, G);
  }
  hipLaunchKernelGGL(replay_wide_write_kernel, dim3(B > 0 ? G : 1), dim3(kThreads), 0, st, ws, rng, B, G, idx, status);
  return launch_status();
}

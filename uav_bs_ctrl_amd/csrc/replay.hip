// Device-resident replay state: ring commit, batch sampler, batch gather and the exploration schedule - the four pieces a
// captured training episode needs so that nothing of the replay lives on the host (reference: algos/madrqn/buffer.py:18-39
// push / sample, algos/madrqn/run.py:60-61 the epsilon schedule; the DRQN's algos/drqn/buffer.py is the same ring).
//
// Shared device state (written by ONE thread, in plain C++, after the work that reads it):
//   state  int64[2] {head, size}   next ring slot, number of committed sequences
//   rng    int64[2] {seed, draws}  the sampler's key and its draw counter
//   status int32[1]                error bits, OR-ed in, never cleared by a kernel.  bit 0: a sample asked for more sequences
//                                  than the ring holds
//
// uavgnn_replay_commit.  The E sequences under construction go to ring slots (head + e) % capacity, every field in one launch:
// field f is `bytes` contiguous bytes per sequence at src + e bytes -> dst + slot bytes.  A SECOND one-thread launch on the same
// stream then sets head = (head + E) % capacity, size = min(size + E, capacity): the copy launch only reads the counters, so no
// workgroup can see a half-advanced state.  A field is moved with 16-byte accesses when its bytes per sequence and both bases
// are multiples of 16, otherwise with 4-byte accesses (anything that is no multiple of 4 is UAVGNN_EINVAL).
//
// uavgnn_replay_sample.  B distinct slots of [0, size), uniform without replacement, then draws += 1.  THE RULE:
//   key(s) = philox4x32_10(counter = (s, 0, draws_lo, draws_hi), key = (seed_lo, seed_hi))[0]      for every slot s in [0, size)
//   (lo / hi: the low / high 32 bits of the int64; Philox4x32-10 as in csrc/common.h; [0]: the first output word)
//   the B smallest pairs (key(s), s) - ordered by key, ties by slot - are selected and written in ASCENDING SLOT ORDER.
// Independent keys make every B-subset equally likely (up to the 2^-32 granularity of the keys, ties broken by slot), so the
// draw is the reference's random.sample(memory, B) as a SET.  The ORDER differs - random.sample returns a random order, this
// one is sorted - and does not matter: the loss is a mean over the batch, every sequence of the batch enters
// it symmetrically.  The result depends on (seed, draws, size, B) only, never on the launch geometry: ONE workgroup; the
// threshold pair is found by a 4-pass radix select over the key bytes (256-bin LDS histogram of the keys that match the prefix
// found so far), keys at the threshold are taken in slot order, and the selected slots are compacted by a workgroup prefix sum
// over contiguous slot chunks.  Keys are recomputed per pass (64 Philox calls per thread and pass at 65 536 slots) instead of
// held: 65 536 keys do not fit the LDS of one workgroup.  capacity <= 65536, else UAVGNN_EUNSUPPORTED.
//   size < B: status |= 1 and idx[i] = i % max(size, 1) - nothing downstream can read outside the ring; draws += 1 all the same.
// Which entry point serves which ring: uavgnn_replay_sample (here) every capacity <= 65 536 - the rings of every run so far, which keep
// their one launch; uavgnn_replay_sample_wide (csrc/replay_wide.hip) every capacity in [1, 2^30] under the SAME RULE, so the same bits
// wherever both apply, in seven launches over one workgroup per 4096 slots; replay.py picks by capacity (> 65 536: the wide one).
//
// uavgnn_replay_gather.  One launch moves every field of the B sampled sequences from the ring into the TIME-MAJOR fixed-address
// buffers of a captured update: for field f, sampled row b and step t < steps,
//   slab_bytes bytes at  src + idx[b] src_seq_stride + t slab_bytes   ->   dst + t dst_step_stride + b slab_bytes.
// gt / ubs / agent / d_u2u / state [T+1, B, ...], act / rew / done [T, B, ...] are fields of T+1 / T steps; h0 / h1 are one-step
// fields whose source bases are h[:, 0] / h[:, 1].  idx may hold repeats; an index outside [0, n_seq) is clamped into it (the
// sampler never writes one).  16-byte accesses when slab_bytes, both strides and both bases are multiples of 16, else 4-byte.
// A pure copy: its roof is HBM bandwidth over 2 x the bytes moved.  Consecutive lanes read consecutive 16-byte (4-byte) words of
// one sequence and write consecutive words of one step slab, so both sides coalesce wherever a slab spans a wavefront's reach.
//
// uavgnn_eps_schedule.  One thread: eps = (float) max(eps_end, eps_start - (eps_start - eps_end) / decay_steps * t) evaluated in
// double WITHOUT contraction (each of the division, the product and the difference rounded on its own - run.py:61's
// -(eps_start - eps_end) / decay_steps * t + eps_start gives the same bits, negation being exact), then t += inc.
#include "common.h"
#include "replay_sample.h"

namespace uavgnn {
namespace {

constexpr int kMaxFields = 16;
constexpr int kCopyThreads = 256;
constexpr int kUnitsPerThread = 8;        // 16-byte (4-byte) words a thread moves before another workgroup is worth its launch
constexpr int kMaxBlocksPerRow = 64;
constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / kWave;
constexpr int kMaxCapacity = 65536;       // = 64 slots per thread: the selection masks of a thread's chunk are two 64-bit words

struct CopyField {
  const char* src;
  char* dst;
  long long bytes;         // per sequence
  int vec;                 // 1: 16-byte accesses, 0: 4-byte
  int block0;              // first blockIdx.x of this field
};
struct CopyArgs {
  CopyField f[kMaxFields];
  int n_fields;
};

struct GatherField {
  const char* src;
  char* dst;
  long long src_seq_stride, dst_step_stride, n_seq;
  unsigned slab_units, units;   // per step / per sequence, in 16-byte or 4-byte words
  int vec, block0;
};
struct GatherArgs {
  GatherField f[kMaxFields];
  int n_fields;
};

// the field a workgroup works on: the last one whose first block is not beyond blockIdx.x (uniform: scalar code)
template <class Args>
__device__ __forceinline__ int field_of_block(const Args& a) {
  int f = 0;
  for (int i = 1; i < a.n_fields; ++i) f = static_cast<int>(blockIdx.x) >= a.f[i].block0 ? i : f;
  return f;
}

template <class W>
__device__ __forceinline__ void copy_words(const char* __restrict__ src, char* __restrict__ dst, unsigned n, unsigned first,
                                           unsigned stride) {
  const W* __restrict__ s = reinterpret_cast<const W*>(src);
  W* __restrict__ d = reinterpret_cast<W*>(dst);
  for (unsigned i = first; i < n; i += stride) d[i] = s[i];
}

__global__ __launch_bounds__(kCopyThreads) void replay_commit_kernel(CopyArgs a, int n_blocks_of_last, int capacity,
                                                                     const long long* __restrict__ state) {
  const int fi = field_of_block(a);
  const CopyField f = a.f[fi];
  const int blocks = (fi + 1 < a.n_fields ? a.f[fi + 1].block0 : f.block0 + n_blocks_of_last) - f.block0;
  long long head = state[0];
  if (head < 0 || head >= capacity) head = ((head % capacity) + capacity) % capacity;   // a corrupted counter cannot leave the ring
  const long long slot = (head + blockIdx.y) % capacity;
  const char* src = f.src + static_cast<long long>(blockIdx.y) * f.bytes;
  char* dst = f.dst + slot * f.bytes;
  const unsigned first = (blockIdx.x - f.block0) * kCopyThreads + threadIdx.x, stride = blocks * kCopyThreads;
  if (f.vec) copy_words<uint4>(src, dst, static_cast<unsigned>(f.bytes >> 4), first, stride);
  else copy_words<uint32_t>(src, dst, static_cast<unsigned>(f.bytes >> 2), first, stride);
}

__global__ void replay_advance_kernel(long long* __restrict__ state, int E, int capacity) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  long long head = state[0], size = state[1];
  if (head < 0 || head >= capacity) head = ((head % capacity) + capacity) % capacity;
  size = size < 0 ? 0 : size;
  state[0] = (head + E) % capacity;
  state[1] = size + E < capacity ? size + E : capacity;
}

template <class W>
__device__ __forceinline__ void gather_words(const GatherField& f, const char* __restrict__ src, char* __restrict__ dst,
                                             unsigned first, unsigned stride) {
  const W* __restrict__ s = reinterpret_cast<const W*>(src);
  for (unsigned u = first; u < f.units; u += stride) {
    const unsigned t = u / f.slab_units, r = u - t * f.slab_units;
    reinterpret_cast<W*>(dst + static_cast<long long>(t) * f.dst_step_stride)[r] = s[u];
  }
}

__global__ __launch_bounds__(kCopyThreads) void replay_gather_kernel(GatherArgs a, int n_blocks_of_last,
                                                                     const long long* __restrict__ idx) {
  const int fi = field_of_block(a);
  const GatherField f = a.f[fi];
  const int blocks = (fi + 1 < a.n_fields ? a.f[fi + 1].block0 : f.block0 + n_blocks_of_last) - f.block0;
  long long s = idx[blockIdx.y];
  s = s < 0 ? 0 : (s >= f.n_seq ? f.n_seq - 1 : s);
  const int width = f.vec ? 16 : 4;
  const char* src = f.src + s * f.src_seq_stride;
  char* dst = f.dst + static_cast<long long>(blockIdx.y) * f.slab_units * width;
  const unsigned first = (blockIdx.x - f.block0) * kCopyThreads + threadIdx.x, stride = blocks * kCopyThreads;
  if (f.vec) gather_words<uint4>(f, src, dst, first, stride);
  else gather_words<uint32_t>(f, src, dst, first, stride);
}

// ---- the sampler (SampleKey, wave_inclusive_scan: replay_sample.h) ----------------------------------------------------------
__global__ __launch_bounds__(kSampleThreads) void replay_sample_kernel(const long long* __restrict__ state,
                                                                       long long* __restrict__ rng, int capacity, int B,
                                                                       long long* __restrict__ idx, int* __restrict__ status) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t found[2];                       // {key prefix, how many of the pairs at / below it are still to be taken}
  __shared__ int wave_lt[kSampleWaves], wave_eq[kSampleWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const long long size64 = state[1];
  const int size = size64 < 0 ? 0 : (size64 > capacity ? capacity : static_cast<int>(size64));
  const unsigned long long seed = static_cast<unsigned long long>(rng[0]), draws = static_cast<unsigned long long>(rng[1]);
  __syncthreads();                                    // every thread holds the counter before thread 0 may advance it
  if (size < B) {
    const int m = size > 1 ? size : 1;
    for (int i = tid; i < B; i += kSampleThreads) idx[i] = i % m;
    if (tid == 0) {
      atomicOr(status, 1);
      rng[1] = static_cast<long long>(draws + 1);
    }
    return;
  }
  const SampleKey key{static_cast<uint32_t>(draws), static_cast<uint32_t>(draws >> 32), static_cast<uint32_t>(seed),
                      static_cast<uint32_t>(seed >> 32)};
  // ---- radix select: the key of the B-th smallest (key, slot) pair, most significant byte first -------------------------------
  uint32_t prefix = 0u, mask = 0u;
  int k = B;                                          // pairs still to be taken among the keys that match the prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int s = tid; s < size; s += kSampleThreads) {
      const uint32_t ks = key(static_cast<uint32_t>(s));
      if ((ks & mask) == prefix) atomicAdd(&hist[(ks >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wave == 0) {                                  // lane l owns bins 4 l .. 4 l + 3
      int h[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = static_cast<int>(hist[4 * lane + j]);
        tot += h[j];
      }
      int below = wave_inclusive_scan(tot, lane) - tot;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (below < k && k <= below + h[j]) {         // exactly one bin: 1 <= k <= number of matching keys
          found[0] = prefix | (static_cast<uint32_t>(4 * lane + j) << shift);
          found[1] = static_cast<uint32_t>(k - below);
        }
        below += h[j];
      }
    }
    __syncthreads();
    prefix = found[0];
    k = static_cast<int>(found[1]);
    mask |= 255u << shift;
  }
  // prefix: the threshold key; k >= 1: how many slots holding exactly that key are taken (the lowest ones)
  // ---- compaction in slot order: thread t owns the contiguous chunk [t C, (t+1) C), C <= 64 ---------------------------------------
  const int C = (size + kSampleThreads - 1) / kSampleThreads;
  const int lo = tid * C, hi = lo + C < size ? lo + C : size;
  unsigned long long lt_mask = 0ull, eq_mask = 0ull;
  for (int s = lo; s < hi; ++s) {
    const uint32_t ks = key(static_cast<uint32_t>(s));
    lt_mask |= static_cast<unsigned long long>(ks < prefix) << (s - lo);
    eq_mask |= static_cast<unsigned long long>(ks == prefix) << (s - lo);
  }
  const int n_lt = __popcll(lt_mask), n_eq = __popcll(eq_mask);
  const int inc_lt = wave_inclusive_scan(n_lt, lane), inc_eq = wave_inclusive_scan(n_eq, lane);
  if (lane == kWave - 1) {
    wave_lt[wave] = inc_lt;
    wave_eq[wave] = inc_eq;
  }
  __syncthreads();
  int lt_before = inc_lt - n_lt, eq_before = inc_eq - n_eq;
  for (int w = 0; w < wave; ++w) {
    lt_before += wave_lt[w];
    eq_before += wave_eq[w];
  }
  int out = lt_before + (eq_before < k ? eq_before : k);
  for (int s = lo; s < hi; ++s) {
    const bool lt = (lt_mask >> (s - lo)) & 1ull, eq = (eq_mask >> (s - lo)) & 1ull;
    const bool take = lt || (eq && eq_before < k);
    eq_before += eq;
    if (take && out < B) idx[out] = s;
    out += take;
  }
  if (tid == 0) rng[1] = static_cast<long long>(draws + 1);
}

__global__ void eps_schedule_kernel(long long* __restrict__ t, long long inc, double eps_start, double eps_end,
                                    double decay_steps, float* __restrict__ eps) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long tv = *t;
  const double slope = (eps_start - eps_end) / decay_steps;
  const double drop = slope * static_cast<double>(tv);
  const double v = eps_start - drop;
  *eps = static_cast<float>(eps_end > v ? eps_end : v);
  *t = tv + inc;
}

inline bool aligned(const void* p, long long a) { return reinterpret_cast<uintptr_t>(p) % static_cast<uintptr_t>(a) == 0; }

inline int blocks_for(long long units) {
  long long b = (units + kCopyThreads * kUnitsPerThread - 1) / (kCopyThreads * kUnitsPerThread);
  return static_cast<int>(b < 1 ? 1 : (b > kMaxBlocksPerRow ? kMaxBlocksPerRow : b));
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

// fields: HOST int64 [n_fields, 3] = {source base (the sequences under construction), destination base (the ring), bytes per sequence}
extern "C" int uavgnn_replay_commit(const long long* fields, int n_fields, int E, int capacity, long long* state,
                                    uavgnn_stream_t stream) {
  if (!fields || n_fields < 0 || E < 0 || capacity < 1 || !state || E > capacity) return UAVGNN_EINVAL;
  if (n_fields > kMaxFields || E > 65535) return UAVGNN_EUNSUPPORTED;
  CopyArgs a;
  int n = 0, next_block = 0, last_blocks = 0;
  for (int i = 0; i < n_fields; ++i) {
    const void* src = reinterpret_cast<const void*>(fields[3 * i]);
    void* dst = reinterpret_cast<void*>(fields[3 * i + 1]);
    const long long bytes = fields[3 * i + 2];
    if (bytes < 0 || (bytes > 0 && (!src || !dst))) return UAVGNN_EINVAL;
    if (bytes == 0) continue;
    if (bytes % 4 != 0 || !aligned(src, 4) || !aligned(dst, 4)) return UAVGNN_EINVAL;
    if (bytes > 0x7fffffffll) return UAVGNN_EUNSUPPORTED;
    CopyField& f = a.f[n++];
    f.src = static_cast<const char*>(src);
    f.dst = static_cast<char*>(dst);
    f.bytes = bytes;
    f.vec = bytes % 16 == 0 && aligned(src, 16) && aligned(dst, 16);
    f.block0 = next_block;
    last_blocks = blocks_for(bytes / (f.vec ? 16 : 4));
    next_block += last_blocks;
  }
  a.n_fields = n;
  if (E == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n > 0) hipLaunchKernelGGL(replay_commit_kernel, dim3(next_block, E), dim3(kCopyThreads), 0, st, a, last_blocks, capacity, state);
  hipLaunchKernelGGL(replay_advance_kernel, dim3(1), dim3(1), 0, st, state, E, capacity);
  return launch_status();
}

extern "C" int uavgnn_replay_sample(const long long* state, long long* rng, int capacity, int B, long long* idx, int32_t* status,
                                    uavgnn_stream_t stream) {
  if (!state || !rng || capacity < 1 || B < 0 || (B > 0 && !idx) || !status) return UAVGNN_EINVAL;
  if (capacity > kMaxCapacity) return UAVGNN_EUNSUPPORTED;
  hipLaunchKernelGGL(replay_sample_kernel, dim3(1), dim3(kSampleThreads), 0, static_cast<hipStream_t>(stream), state, rng, capacity,
                     B, idx, status);
  return launch_status();
}

// fields: HOST int64 [n_fields, 7] = {source base (step 0 of ring slot 0), destination base (step 0, row 0), bytes per step slab, steps,
//         source sequence stride in bytes, destination step stride in bytes, sequences in the ring (idx is clamped below it)}
extern "C" int uavgnn_replay_gather(const long long* fields, int n_fields, const long long* idx, int B, uavgnn_stream_t stream) {
  if (!fields || n_fields < 0 || B < 0 || (B > 0 && !idx)) return UAVGNN_EINVAL;
  if (n_fields > kMaxFields || B > 65535) return UAVGNN_EUNSUPPORTED;
  GatherArgs a;
  int n = 0, next_block = 0, last_blocks = 0;
  for (int i = 0; i < n_fields; ++i) {
    const long long* d = fields + 7 * i;
    const void* src = reinterpret_cast<const void*>(d[0]);
    void* dst = reinterpret_cast<void*>(d[1]);
    const long long slab = d[2], steps = d[3], ss = d[4], ds = d[5], n_seq = d[6];
    if (slab < 0 || steps < 0 || n_seq < 1) return UAVGNN_EINVAL;
    if (slab == 0 || steps == 0) continue;
    if (!src || !dst || ss < slab * steps || ds < slab * B) return UAVGNN_EINVAL;     // a sequence inside its stride, B rows inside a step
    if (slab % 4 != 0 || ss % 4 != 0 || ds % 4 != 0 || !aligned(src, 4) || !aligned(dst, 4)) return UAVGNN_EINVAL;
    if (slab * steps > 0x7fffffffll) return UAVGNN_EUNSUPPORTED;
    GatherField& f = a.f[n++];
    f.src = static_cast<const char*>(src);
    f.dst = static_cast<char*>(dst);
    f.src_seq_stride = ss;
    f.dst_step_stride = ds;
    f.n_seq = n_seq;
    f.vec = slab % 16 == 0 && ss % 16 == 0 && ds % 16 == 0 && aligned(src, 16) && aligned(dst, 16);
    const int w = f.vec ? 16 : 4;
    f.slab_units = static_cast<unsigned>(slab / w);
    f.units = static_cast<unsigned>(slab * steps / w);
    f.block0 = next_block;
    last_blocks = blocks_for(f.units);
    next_block += last_blocks;
  }
  a.n_fields = n;
  if (B == 0 || n == 0) return 0;
  hipLaunchKernelGGL(replay_gather_kernel, dim3(next_block, B), dim3(kCopyThreads), 0, static_cast<hipStream_t>(stream), a,
                     last_blocks, idx);
  return launch_status();
}

extern "C" int uavgnn_eps_schedule(long long* t, long long inc, double eps_start, double eps_end, double decay_steps, float* eps,
                                   uavgnn_stream_t stream) {
  if (!t || !eps || !(decay_steps > 0.0)) return UAVGNN_EINVAL;
  hipLaunchKernelGGL(eps_schedule_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), t, inc, eps_start, eps_end,
                     decay_steps, eps);
  return launch_status();
}

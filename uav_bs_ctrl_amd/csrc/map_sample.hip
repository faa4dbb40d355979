// Reset-time placement sampler of the device simulator: initial UBS / GT positions and the initial GT priority
// permutation of B environments in ONE launch (reference: envs/mubs_cov/maps.py `set_positions` of Map :31-35, Debug
// :47-50, HotSpot :64-75, DenseHotSpot :97-113, DenseHotSpotV2 :125-132, and np.random.permutation at
// envs/mubs_cov/mubs_cov.py:96).  One wavefront per environment, several per workgroup, scratch in LDS, lanes over GTs.
// The reference draws from Python's / NumPy's global generators; this kernel draws the same DISTRIBUTIONS from a
// counter-based generator, so environment b of a launch produces the same placement whatever B and the grid are.
//
// Random numbers.  Philox4x32-10 (csrc/common.h), key = the 64-bit seed rng[0] (low word, high word), counter =
// (environment b, draw slot, low word of rng[1], high word of rng[1]); rng is a DEVICE int64 pair {seed, resets} as K5's
// {seed, step} is (a captured graph replays with the current counter; the caller advances rng[1]).  One Philox call per
// slot yields four 32-bit words w0..w3.  Slot numbering:
//   slot k,        k in [0, 16):    UBS pick k                                                        (w0)
//   slot 16:                        hotspot pick                                                      (w0)
//   slot 1024 + k, k in [0, 1024):  GT-lattice pick k: GT k of `uniform_lattice`, the block cell of GT k of `hotspot`,
//                                   the block cell of group k of `dense_hotspot`                      (w0)
//   slot 2048 + m, m in [0, 1024):  GT m in generation order: w0 -> u_x, w1 -> u_y (offset from the centre), w2 -> its
//                                   shuffle key, w3 -> priority key m
// Integer in [0, m) from a word w: __umulhi(w, m) = floor(w m / 2^32) (bias <= m / 2^32).  Uniform in (0, 1) from a word
// w: ((w >> 9) + 1/2) 2^-23, K5's.
//
// Distinct lattice points (the reference's select_from_cube is random.sample over the lattice: an ordered uniform sample
// without replacement).  A lattice of L x L points is the virtual identity array a[p] = p, p = x L + y in
// itertools.product order, C = L^2.  Partial Fisher-Yates with exactly `count` draws: pick k takes
// j = k + umulhi(w_k, C - k), its result is a[j], then a[j] <- a[k].  Only displaced entries are stored (a sparse table of
// at most `count` (position, value) pairs in LDS): the base map's 250 000-point lattice never exists.  No rejection.
//
// Placement (all in double; every product is exact - 200 int, 100 (u - 1/2), 800 (u - 1/2) - and so is every sum, hence
// FMA contraction cannot change a result), clipped to [0, range_pos], UBSs stored f64 and GTs f32:
//   UBS i           = pitch_u (p / L_u, p % L_u),  p = pick i from the L_u x L_u lattice (`fixed`: the given array)
//   uniform_lattice : GT m = pitch_u (p / L_u, p % L_u),  p = GT-lattice pick m from the SAME kind of lattice (own draws)
//   fixed           : GT m = the given array
//   spot kinds      : q = umulhi(w0 of slot 16, L_s^2), spot = pitch_s (o + q / L_s, o + q % L_s)
//                     GT m = spot + pitch_c (c / r, c % r) + spread ((u_x, u_y) - 1/2),  c = GT-lattice pick m / gpg from the
//                     r x r block (c = 0 without picks)
//     hotspot          L_s = (range_pos // 200) // r, r = ceil(sqrt(n_gts)), o = 0, pitch_s = 200 r, gpg = 1, spread = 0
//     dense_hotspot    L_s = (range_pos // 200) // r, r = ceil(sqrt(n_grps)), o = 0, pitch_s = 200 r, spread = r_cov
//     dense_hotspot_v2 L_s = range_pos // 400 - 1, o = 1, pitch_s = 400, no picks, spread = 800
// Shuffle of the GT rows (spot kinds only, np.random.shuffle) and the priority permutation (every kind): the stable
// argsort of the M keys, as a rank count - rank(m) = #{m' : key[m'] < key[m] or (key[m'] == key[m] and m' < m)}.  GT m of
// the generation order lands in output row rank_shuffle(m); prior[rank_priority(m)] = m.
#include "common.h"
#include "env_math.h"   // Draws, unit, clip, stable_rank

namespace uavgnn {
namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kThreads = kWave * kWavesPerBlock;
constexpr int kMaxUbs = 16, kMaxGts = 1024;
constexpr uint32_t kSlotSpot = 16, kSlotPick = 1024, kSlotGt = 2048;
enum Kind { kUniformLattice = 0, kFixed = 1, kHotspot = 2, kDenseHotspot = 3, kDenseHotspotV2 = 4, kNumKinds = 5 };

struct MapConsts {
  int kind, n, M, L_u, L_s, r, n_picks, gpg, origin;
  double range_pos, pitch_u, pitch_s, pitch_c, spread;
};

// Ordered sample of `count` distinct points of [0, C) by the whole wavefront.  pick[k] holds the word of draw k on entry and
// the sampled point on return; key / val: the sparse table (position -> displaced value), at most `count` entries.
__device__ void sample_distinct(uint32_t* pick, int* key, int* val, int count, uint32_t C, int lane) {
  int used = 0;
  for (int k = 0; k < count; ++k) {
    const int j = k + static_cast<int>(__umulhi(pick[k], C - static_cast<uint32_t>(k)));
    int vj = j, vk = k, at_j = -1;
    for (int base = 0; base < used; base += kWave) {
      const int i = base + lane;
      const int ki = i < used ? key[i] : -1;
      const unsigned long long hit_j = __ballot(ki == j), hit_k = __ballot(ki == k);
      if (hit_j) {
        at_j = base + __ffsll(static_cast<long long>(hit_j)) - 1;
        vj = val[at_j];
      }
      if (hit_k) vk = val[base + __ffsll(static_cast<long long>(hit_k)) - 1];
    }
    wave_sync();
    if (lane == 0) {
      pick[k] = static_cast<uint32_t>(vj);
      if (j != k) {
        const int at = at_j >= 0 ? at_j : used;
        key[at] = j;
        val[at] = vk;
      }
    }
    if (j != k && at_j < 0) ++used;
    wave_sync();
  }
}

__global__ __launch_bounds__(kThreads) void map_sample_kernel(MapConsts c, int B, int words_per_wave, int table,
                                                              const long long* __restrict__ rng,
                                                              const double* __restrict__ fixed_ubs,
                                                              const float* __restrict__ fixed_gts,
                                                              double* __restrict__ pos_ubs, float* __restrict__ pos_gts,
                                                              int32_t* __restrict__ prior) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x * kWavesPerBlock + wave;
  if (b >= B) return;                                       // whole wavefronts leave; no workgroup barrier below
  // ---- this wavefront's LDS: pick[table] | val[table] | key[table] aliased with keys[M] (the table is dead by then) ----
  uint32_t* pick = reinterpret_cast<uint32_t*>(smem) + static_cast<size_t>(wave) * words_per_wave;
  int* val = reinterpret_cast<int*>(pick + table);
  int* key = val + table;
  uint32_t* keys = reinterpret_cast<uint32_t*>(key);
  const int n = c.n, M = c.M;
  const unsigned long long seed = static_cast<unsigned long long>(rng[0]), resets = static_cast<unsigned long long>(rng[1]);
  const Draws d{static_cast<uint32_t>(b), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                static_cast<uint32_t>(resets), static_cast<uint32_t>(resets >> 32)};
  double* pu = pos_ubs + static_cast<size_t>(b) * n * 2;
  float* pg = pos_gts + static_cast<size_t>(b) * M * 2;
  const uint32_t L_u = static_cast<uint32_t>(c.L_u);

  // ---- UBSs ------------------------------------------------------------------------------------------------------------
  if (c.kind == kFixed) {
    for (int i = lane; i < 2 * n; i += kWave) pu[i] = clip(fixed_ubs[i], c.range_pos);
    for (int i = lane; i < 2 * M; i += kWave) pg[i] = static_cast<float>(clip(static_cast<double>(fixed_gts[i]), c.range_pos));
  } else {
    if (lane < n) pick[lane] = d.word0(lane);
    wave_sync();
    sample_distinct(pick, key, val, n, L_u * L_u, lane);
    if (lane < n) {
      const uint32_t p = pick[lane];
      pu[2 * lane] = clip(c.pitch_u * static_cast<double>(p / L_u), c.range_pos);
      pu[2 * lane + 1] = clip(c.pitch_u * static_cast<double>(p % L_u), c.range_pos);
    }
    wave_sync();
  }
  // ---- GTs -------------------------------------------------------------------------------------------------------------
  if (c.kind == kUniformLattice) {
    for (int k = lane; k < M; k += kWave) pick[k] = d.word0(kSlotPick + k);
    wave_sync();
    sample_distinct(pick, key, val, M, L_u * L_u, lane);
    for (int m = lane; m < M; m += kWave) {
      const uint32_t p = pick[m];
      pg[2 * m] = static_cast<float>(clip(c.pitch_u * static_cast<double>(p / L_u), c.range_pos));
      pg[2 * m + 1] = static_cast<float>(clip(c.pitch_u * static_cast<double>(p % L_u), c.range_pos));
    }
  } else if (c.kind != kFixed) {
    const uint32_t L_s = static_cast<uint32_t>(c.L_s), r = static_cast<uint32_t>(c.r);
    const uint32_t q = __umulhi(d.word0(kSlotSpot), L_s * L_s);
    const double sx = c.pitch_s * static_cast<double>(c.origin + q / L_s), sy = c.pitch_s * static_cast<double>(c.origin + q % L_s);
    if (c.n_picks > 0) {
      for (int k = lane; k < c.n_picks; k += kWave) pick[k] = d.word0(kSlotPick + k);
      wave_sync();
      sample_distinct(pick, key, val, c.n_picks, r * r, lane);
    }
    for (int m = lane; m < M; m += kWave) {                 // the table is dead: its key array becomes the shuffle keys
      uint32_t w[4];
      d.words(kSlotGt + m, w);
      keys[m] = w[2];
    }
    wave_sync();
    for (int m = lane; m < M; m += kWave) {
      uint32_t w[4];
      d.words(kSlotGt + m, w);
      const uint32_t cell = c.n_picks > 0 ? pick[m / c.gpg] : 0u;
      const double x = sx + c.pitch_c * static_cast<double>(cell / r) + c.spread * (unit(w[0]) - 0.5);
      const double y = sy + c.pitch_c * static_cast<double>(cell % r) + c.spread * (unit(w[1]) - 0.5);
      const int row = stable_rank(keys, M, m);
      pg[2 * row] = static_cast<float>(clip(x, c.range_pos));
      pg[2 * row + 1] = static_cast<float>(clip(y, c.range_pos));
    }
  }
  // ---- initial priorities ------------------------------------------------------------------------------------------------
  wave_sync();
  for (int m = lane; m < M; m += kWave) {
    uint32_t w[4];
    d.words(kSlotGt + m, w);
    keys[m] = w[3];
  }
  wave_sync();
  for (int m = lane; m < M; m += kWave) prior[static_cast<size_t>(b) * M + stable_rank(keys, M, m)] = m;
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

// int_consts: {kind, n_ubs, n_gts, L_u, L_s, r, n_picks, gts_per_pick, origin}   (kind: 0 uniform_lattice, 1 fixed, 2 hotspot,
//             3 dense_hotspot, 4 dense_hotspot_v2; the fields a kind does not use are ignored)
// f64_consts: {range_pos, pitch_u, pitch_s, pitch_c, spread}
extern "C" int uavgnn_map_sample(const int32_t* int_consts, const double* f64_consts, int B, const long long* rng,
                                 const double* fixed_ubs, const float* fixed_gts, double* pos_ubs, float* pos_gts,
                                 int32_t* prior, uavgnn_stream_t stream) {
  if (!int_consts || !f64_consts || B < 0 || !rng || !pos_ubs || !pos_gts || !prior) return UAVGNN_EINVAL;
  MapConsts c;
  c.kind = int_consts[0]; c.n = int_consts[1]; c.M = int_consts[2]; c.L_u = int_consts[3]; c.L_s = int_consts[4];
  c.r = int_consts[5]; c.n_picks = int_consts[6]; c.gpg = int_consts[7]; c.origin = int_consts[8];
  c.range_pos = f64_consts[0]; c.pitch_u = f64_consts[1]; c.pitch_s = f64_consts[2]; c.pitch_c = f64_consts[3];
  c.spread = f64_consts[4];
  if (c.kind < 0 || c.kind >= kNumKinds || c.n < 1 || c.n > kMaxUbs || c.M < 1 || c.M > kMaxGts) return UAVGNN_EUNSUPPORTED;
  if (c.kind == kFixed && (!fixed_ubs || !fixed_gts)) return UAVGNN_EINVAL;
  int table = c.n;                                         // entries of the sparse table = the largest number of picks
  if (c.kind != kFixed) {
    if (c.L_u < 1 || c.L_u > 46340) return UAVGNN_EUNSUPPORTED;                       // L_u^2 stays below 2^31
    const long long C_u = static_cast<long long>(c.L_u) * c.L_u;
    if (c.n > C_u) return UAVGNN_EINVAL;                                              // more picks than lattice points
    if (c.kind == kUniformLattice) {
      if (c.M > C_u) return UAVGNN_EINVAL;
      table = c.M > table ? c.M : table;
    } else {
      if (c.L_s < 1 || c.L_s > 46340 || c.origin < 0) return UAVGNN_EUNSUPPORTED;
      if (c.n_picks < 0 || c.n_picks > kMaxGts) return UAVGNN_EUNSUPPORTED;
      if (c.n_picks > 0) {
        if (c.r < 1 || c.r > 46340 || c.gpg < 1) return UAVGNN_EUNSUPPORTED;
        if (c.n_picks > static_cast<long long>(c.r) * c.r || static_cast<long long>(c.n_picks) * c.gpg != c.M)
          return UAVGNN_EINVAL;
        table = c.n_picks > table ? c.n_picks : table;
      } else {
        c.r = 1;
        c.gpg = 1;
      }
    }
  }
  if (B == 0) return 0;
  const int words_per_wave = 2 * table + (table > c.M ? table : c.M);     // <= 3 x 1024 words: 48 KiB per workgroup
  const size_t lds = static_cast<size_t>(kWavesPerBlock) * words_per_wave * 4;
  hipLaunchKernelGGL(map_sample_kernel, dim3((B + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kThreads), lds,
                     static_cast<hipStream_t>(stream), c, B, words_per_wave, table, rng, fixed_ubs, fixed_gts, pos_ubs,
                     pos_gts, prior);
  return launch_status();
}

// Device simulator of the single-UBS coverage environment (experiment 1; reference: envs/subs_cov/subs_cov.py
// `SingleUbsCoverageEnv`): B independent environments per launch, one wavefront each, several wavefronts per workgroup,
// lanes over GTs.  Two entries:
//
// uavgnn_subs_env_step   - step :113-133 (move, clip), _transmit_data :135-157 (distances, greedy schedule, A2G channel gain -
//   envs/common.py:49-59 -, rates, running averages, Jain index - envs/common.py:19-25 -, utilities, next priorities), get_obs
//   :159-171, reward and termination :186-191.
// uavgnn_subs_env_sample - the placements of _set_position :92-111 and the np.random.permutation of reset :84.
//
// ---- step: constants -------------------------------------------------------------------------------------------------------
//   int_consts (host): {n_gts M, n_rbs, n_actions A, episode_limit, n_grps}
//   f64_consts (host): {range_pos, r_cov, dt, h_ubs, p_tx, n0, bw, fc, a, b, eta_los, eta_nlos, reward_scale_rate, max_rate}
//
// ---- step: arithmetic, operation by operation and dtype by dtype (NumPy 2 promotion rules) -----------------------------------
// The UBS position is float64 from the first move on (float32 + float64 move, :117) and float32 (range_pos / 2) at reset, so
//   moving (actions != NULL): t += 1; position clipped in float64; d[m] = float32(sqrt(dx^2 + dy^2)) with dx, dy the float64
//     differences of the float32 GT position and the float64 UBS position; observation offsets dx / range_pos in float64;
//   reset-time transmission (actions == NULL): t stays; the stored position is read as float32; differences, norm and the
//     observation quotients are float32 operations.
// Covered: d[m] <= float32(r_cov).  The greedy loop of :142-145 walks the GTs in priority order and serves covered ones while
// fewer than n_rbs are served; as a RANK COUNT: GT m = prior[i] is served iff it is covered and fewer than n_rbs covered GTs
// stand at positions < i of prior (a wavefront-wide prefix count, 64 positions per round).
// Channel gain (envs/common.py:49-59): arctan / exp / LoS probability in float32 (float32 distances, Python scalars), direct
// distance and path loss in float64 (np.square(h_ubs) is an int64 scalar: float32 array + int64 -> float64).
// rate[m] = bw log2(1 + p_tx g[m] sched[m] / (bw n0)) 1e-6, avg[m] = (avg[m] t + rate[m]) / (t + 1), the Jain index of
// max(avg, 1e-6), global utility = Jain * mean(rate), total throughput += sum(rate) dt / 1e3, average global utility
// = (old t + utility) / (t + 1), reward = reward_scale_rate * utility / max_rate: all float64 in the reference and here.
// rate_per_gt and avg_rate are STORED as float32 (the state the next step reads is the float32 average); the observation
// columns rate / max_rate and avg / max_rate * n_grps are formed from the float64 values before that rounding.  The sums over
// GTs run per lane over m = lane, lane + 64, ... and then through a fixed butterfly over the 64 lanes: the result does not
// depend on B or on the grid.  run_f64 [B,4] = {total throughput, average global utility, Jain index, global utility}.
// Next priorities (:157): np.argsort is not stable in NumPy; this kernel writes the STABLE ascending order of the stored
// float32 averages (ties -> lower GT index first), as csrc/env_sim.hip does - tests/test_env_sim.py says how fixtures pin it.
// done = [t == episode_limit] (:190-191; BadMask is the same flag, :126).
// Observations: obs_agent [B,2] = position / range_pos; obs_gt [B,M,4] = {dx / range_pos, dy / range_pos, rate / max_rate,
// avg / max_rate * n_grps}; obs_flat [B, 2 + 4 M] = agent || gt row-major, what gym's `flatten` of the (key-sorted) Dict space
// yields - the same float32 values, written twice.
// A prior that is no permutation of 0..M-1 is memory-safe (entries outside [0, M) are skipped), its schedule is unspecified.
//
// ---- sample: constants, draw slots and rules ---------------------------------------------------------------------------------
//   int_consts (host): {n_grps G, gts_per_grp P}      (M = G P)
//   f64_consts (host): {range_pos, r_cov}
// Random numbers: Philox4x32-10 (csrc/common.h) exactly as csrc/map_sample.hip uses it - key = the 64-bit seed rng[0] (low word,
// high word), counter = (environment b, draw slot, low word of rng[1], high word of rng[1]); rng is a DEVICE int64 pair
// {seed, resets}.  One call per slot yields the words w0..w3.  Uniform in (0, 1) from a word w: U(w) = ((w >> 9) + 1/2) 2^-23.
//   slot 0:                         w0 -> u, the common angle offset of the groups
//   slot 1024 + g, g in [0, G):     w0 -> u_g, the radius draw of group g
//   slot 2048 + m, m in [0, M):     GT m in generation order (group g = m / P): w0, w1 -> its Box-Muller pair, w2 -> its shuffle
//                                   key, w3 -> priority key m
// Placement, everything in double:
//   UBS      = (range_pos / 2, range_pos / 2)
//   theta_g  = (U(u) + g / G) * 2 pi,      r_g = 0.2 range_pos + U(u_g) * (0.3 range_pos - 0.2 range_pos)
//   centre_g = UBS + r_g (cos theta_g, sin theta_g)
//   rho      = sqrt(-2 ln U(w0)),  phi = 2 pi U(w1),  (z_x, z_y) = rho (cos phi, sin phi)                  (Box-Muller)
//   GT m     = clip(centre_g + 0.25 r_cov (z_x, z_y), 0, range_pos), rounded to float32 once
// Shuffle of the GT rows (np.random.shuffle) and the priority permutation: the stable argsort of the M keys, as a rank count -
// rank(m) = #{m' : key[m'] < key[m] or (key[m'] == key[m] and m' < m)}.  GT m of the generation order lands in output row
// rank_shuffle(m); prior[rank_priority(m)] = m.
#include "common.h"
#include "env_math.h"

namespace uavgnn {
namespace {

constexpr int kMaxGts = 1024;
constexpr int kMaxWavesPerBlock = 4;
constexpr uint32_t kSlotAngle = 0, kSlotGroup = 1024, kSlotGt = 2048;
constexpr double kTwoPi = 6.283185307179586;

struct SubsConsts {
  int M, R, A, episode_limit, n_grps;
  double range_pos, r_cov, dt, h_ubs, p_tx, n0, bw, fc, a, b, eta_los, eta_nlos, rew_scale, max_rate;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kWave * kMaxWavesPerBlock) void subs_env_step_kernel(
    SubsConsts c, int B, int words_per_wave, const long long* __restrict__ actions, const double* __restrict__ avail_moves,
    double* __restrict__ pos_ubs, const float* __restrict__ pos_gts, int32_t* __restrict__ prior,
    float* __restrict__ avg_rate, int32_t* __restrict__ t_io, double* __restrict__ run_f64, float* __restrict__ d_u2g_out,
    int32_t* __restrict__ sched_out, float* __restrict__ rate_out, double* __restrict__ reward_out,
    float* __restrict__ done_out, float* __restrict__ obs_gt, float* __restrict__ obs_agent, float* __restrict__ obs_flat) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= B) return;                                       // whole wavefronts leave; no workgroup barrier below
  const int M = c.M;
  // ---- this wavefront's LDS: served flags [M] | float32 averages [M] ----------------------------------------------------------
  int* SCH = reinterpret_cast<int*>(smem) + static_cast<size_t>(wave) * words_per_wave;
  float* AVG = reinterpret_cast<float*>(SCH + words_per_wave / 2);
  const size_t bM = static_cast<size_t>(b) * M;
  const float* __restrict__ pg = pos_gts + bM * 2;

  const bool moving = actions != nullptr;
  int t = t_io[b];
  if (moving) t += 1;                                                                        // subs_cov.py:114
  // ---- position (:115-117) -----------------------------------------------------------------------------------------------------
  double px = pos_ubs[2 * static_cast<size_t>(b)], py = pos_ubs[2 * static_cast<size_t>(b) + 1];
  if (moving) {
    long long a = actions[b];
    a = a < 0 ? 0 : (a >= c.A ? c.A - 1 : a);
    px = fmin(fmax(px + avail_moves[2 * a + 0], 0.0), c.range_pos);
    py = fmin(fmax(py + avail_moves[2 * a + 1], 0.0), c.range_pos);
  }
  const float pxf = static_cast<float>(px), pyf = static_cast<float>(py), rngf = static_cast<float>(c.range_pos);
  // ---- distances (:137-139) and coverage -----------------------------------------------------------------------------------------
  for (int m = lane; m < M; m += kWave) {
    float d;
    if (moving) {
      const double dx = static_cast<double>(pg[2 * m]) - px, dy = static_cast<double>(pg[2 * m + 1]) - py;
      d = dist_f32(dx, dy);
    } else {   // reset time: float32 position, float32 arithmetic (not csrc/env_math.h's)
      const float dx = pg[2 * m] - pxf, dy = pg[2 * m + 1] - pyf;
      d = sqrtf(dx * dx + dy * dy);
    }
    d_u2g_out[bM + m] = d;
    AVG[m] = d;                                             // parked here until the averages are formed
    SCH[m] = 0;
  }
  wave_sync();
  // ---- greedy schedule (:142-145) as a prefix count over the priority order ---------------------------------------------------------
  const float r_cov = static_cast<float>(c.r_cov);
  int base = 0;
  for (int i0 = 0; i0 < M; i0 += kWave) {
    const int i = i0 + lane;
    int m = i < M ? prior[bM + i] : -1;
    if (m < 0 || m >= M) m = -1;
    const bool cov = m >= 0 && AVG[m] <= r_cov;
    const unsigned long long bal = __ballot(cov);
    const int before = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (cov && before < c.R) SCH[m] = 1;
    base += __popcll(bal);
  }
  wave_sync();
  // ---- rates, averages, observations (:147-152, :159-171) -----------------------------------------------------------------------------
  const double k_los = a2g_excess_loss(c.eta_los), k_nlos = a2g_excess_loss(c.eta_nlos);
  const double noise = c.bw * c.n0;
  const size_t F = 2 + 4 * static_cast<size_t>(M);
  float* __restrict__ og = obs_gt + bM * 4;
  float* __restrict__ of = obs_flat + static_cast<size_t>(b) * F + 2;
  double s_rate = 0.0, s_x = 0.0, s_xx = 0.0;
  for (int m = lane; m < M; m += kWave) {
    const float d = AVG[m];
    const int served = SCH[m];
    const double p_rx = served ? a2g_rx_power(c, d, k_los, k_nlos) : 0.0;   // A2G channel gain (envs/common.py:49-59)
    const double rate = c.bw * log2(1.0 + p_rx / noise) * 1e-6;
    const double avg = (static_cast<double>(avg_rate[bM + m]) * t + rate) / (t + 1);
    const double x = fmax(avg, 1e-6);                       // np.clip(x, 1e-6, inf) of the Jain index
    s_rate += rate;
    s_x += x;
    s_xx += x * x;
    const float avg_f = static_cast<float>(avg);
    sched_out[bM + m] = served;
    rate_out[bM + m] = static_cast<float>(rate);
    avg_rate[bM + m] = avg_f;
    float ox, oy;
    if (moving) {
      ox = static_cast<float>((static_cast<double>(pg[2 * m]) - px) / c.range_pos);
      oy = static_cast<float>((static_cast<double>(pg[2 * m + 1]) - py) / c.range_pos);
    } else {
      ox = (pg[2 * m] - pxf) / rngf;
      oy = (pg[2 * m + 1] - pyf) / rngf;
    }
    const float o2 = static_cast<float>(rate / c.max_rate), o3 = static_cast<float>(avg / c.max_rate * c.n_grps);
    og[4 * m + 0] = ox; og[4 * m + 1] = oy; og[4 * m + 2] = o2; og[4 * m + 3] = o3;
    of[4 * m + 0] = ox; of[4 * m + 1] = oy; of[4 * m + 2] = o2; of[4 * m + 3] = o3;
    AVG[m] = avg_f;                                         // the distance is consumed: the slot now holds the sort key
  }
  // ---- scalars (:153-156, :186-191): every lane holds the same sums ---------------------------------------------------------------------
  s_rate = wave_sum_f64(s_rate);
  s_x = wave_sum_f64(s_x);
  s_xx = wave_sum_f64(s_xx);
  if (lane == 0) {
    double* rf = run_f64 + static_cast<size_t>(b) * 4;
    const double fair = (s_x * s_x) / (static_cast<double>(M) * s_xx);
    const double gu = fair * (s_rate / static_cast<double>(M));
    rf[0] = rf[0] + s_rate * c.dt / 1e3;
    rf[1] = (rf[1] * t + gu) / (t + 1);
    rf[2] = fair;
    rf[3] = gu;
    reward_out[b] = c.rew_scale * gu / c.max_rate;
    done_out[b] = (t == c.episode_limit) ? 1.f : 0.f;
    t_io[b] = t;
    pos_ubs[2 * static_cast<size_t>(b)] = px;
    pos_ubs[2 * static_cast<size_t>(b) + 1] = py;
    const float ax = moving ? static_cast<float>(px / c.range_pos) : pxf / rngf;
    const float ay = moving ? static_cast<float>(py / c.range_pos) : pyf / rngf;
    obs_agent[2 * static_cast<size_t>(b)] = ax;
    obs_agent[2 * static_cast<size_t>(b) + 1] = ay;
    obs_flat[static_cast<size_t>(b) * F] = ax;
    obs_flat[static_cast<size_t>(b) * F + 1] = ay;
  }
  wave_sync();
  // ---- next priorities (:157): STABLE ascending order of the stored averages ----------------------------------------------------------------
  for (int m = lane; m < M; m += kWave) prior[bM + stable_rank(AVG, M, m)] = m;
}

// ---- reset-time sampler (Draws, unit, clip, stable_rank: csrc/env_math.h) -------------------------------------------------------------
__global__ __launch_bounds__(kWave * kMaxWavesPerBlock) void subs_env_sample_kernel(
    int G, int P, double range_pos, double r_cov, int B, const long long* __restrict__ rng, double* __restrict__ pos_ubs,
    float* __restrict__ pos_gts, int32_t* __restrict__ prior) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= B) return;                                       // whole wavefronts leave; no workgroup barrier below
  const int M = G * P;
  uint32_t* keys = reinterpret_cast<uint32_t*>(smem) + static_cast<size_t>(wave) * M;
  const unsigned long long seed = static_cast<unsigned long long>(rng[0]), resets = static_cast<unsigned long long>(rng[1]);
  const Draws d{static_cast<uint32_t>(b), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                static_cast<uint32_t>(resets), static_cast<uint32_t>(resets >> 32)};
  const double cx = range_pos / 2, cy = range_pos / 2;
  if (lane == 0) {
    pos_ubs[2 * static_cast<size_t>(b)] = cx;
    pos_ubs[2 * static_cast<size_t>(b) + 1] = cy;
  }
  uint32_t w[4];
  d.words(kSlotAngle, w);
  const double u = unit(w[0]);
  const double r_min = 0.2 * range_pos, r_max = 0.3 * range_pos;
  float* pg = pos_gts + static_cast<size_t>(b) * M * 2;
  for (int m = lane; m < M; m += kWave) {
    d.words(kSlotGt + m, w);
    keys[m] = w[2];
  }
  wave_sync();
  for (int m = lane; m < M; m += kWave) {
    const int g = m / P;
    d.words(kSlotGroup + g, w);
    const double theta = (u + static_cast<double>(g) / static_cast<double>(G)) * kTwoPi;
    const double r_g = r_min + unit(w[0]) * (r_max - r_min);
    d.words(kSlotGt + m, w);
    const double rho = sqrt(-2.0 * log(unit(w[0]))), phi = kTwoPi * unit(w[1]);
    const double x = cx + r_g * cos(theta) + 0.25 * r_cov * (rho * cos(phi));
    const double y = cy + r_g * sin(theta) + 0.25 * r_cov * (rho * sin(phi));
    const int row = stable_rank(keys, M, m);
    pg[2 * row] = static_cast<float>(clip(x, range_pos));
    pg[2 * row + 1] = static_cast<float>(clip(y, range_pos));
  }
  wave_sync();
  for (int m = lane; m < M; m += kWave) {
    d.words(kSlotGt + m, w);
    keys[m] = w[3];
  }
  wave_sync();
  for (int m = lane; m < M; m += kWave) prior[static_cast<size_t>(b) * M + stable_rank(keys, M, m)] = m;
}

// wavefronts per workgroup: as many (<= 4) as fit 64 KiB of LDS at `words` 32-bit words each
inline int waves_per_block(int words) {
  int w = static_cast<int>((64 * 1024) / (static_cast<size_t>(words) * 4));
  return w < 1 ? 1 : (w > kMaxWavesPerBlock ? kMaxWavesPerBlock : w);
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_subs_env_step(const int32_t* int_consts, const double* f64_consts, int B, const long long* actions,
                                    const double* avail_moves, double* pos_ubs, const float* pos_gts, int32_t* prior,
                                    float* avg_rate, int32_t* t, double* run_f64, float* d_u2g, int32_t* sched,
                                    float* rate_per_gt, double* reward, float* done, float* obs_gt, float* obs_agent,
                                    float* obs_flat, uavgnn_stream_t stream) {
  if (!int_consts || !f64_consts || B < 0 || !pos_ubs || !pos_gts || !prior || !avg_rate || !t || !run_f64 || !d_u2g || !sched ||
      !rate_per_gt || !reward || !done || !obs_gt || !obs_agent || !obs_flat || (actions && !avail_moves))
    return UAVGNN_EINVAL;
  SubsConsts c;
  c.M = int_consts[0]; c.R = int_consts[1]; c.A = int_consts[2]; c.episode_limit = int_consts[3]; c.n_grps = int_consts[4];
  c.range_pos = f64_consts[0]; c.r_cov = f64_consts[1]; c.dt = f64_consts[2]; c.h_ubs = f64_consts[3]; c.p_tx = f64_consts[4];
  c.n0 = f64_consts[5]; c.bw = f64_consts[6]; c.fc = f64_consts[7]; c.a = f64_consts[8]; c.b = f64_consts[9];
  c.eta_los = f64_consts[10]; c.eta_nlos = f64_consts[11]; c.rew_scale = f64_consts[12]; c.max_rate = f64_consts[13];
  if (c.M < 1 || c.M > kMaxGts || c.A < 1) return UAVGNN_EUNSUPPORTED;
  if (c.R < 0 || c.n_grps < 1) return UAVGNN_EINVAL;
  if (B == 0) return 0;
  const int words_per_wave = 2 * ((c.M + 3) & ~3);          // served flags | averages, each a multiple of 16 bytes
  const int wpb = waves_per_block(words_per_wave);
  hipLaunchKernelGGL(subs_env_step_kernel, dim3((B + wpb - 1) / wpb), dim3(kWave * wpb),
                     static_cast<size_t>(wpb) * words_per_wave * 4, static_cast<hipStream_t>(stream), c, B, words_per_wave, actions,
                     avail_moves, pos_ubs, pos_gts, prior, avg_rate, t, run_f64, d_u2g, sched, rate_per_gt, reward, done, obs_gt,
                     obs_agent, obs_flat);
  return launch_status();
}

extern "C" int uavgnn_subs_env_sample(const int32_t* int_consts, const double* f64_consts, int B, const long long* rng,
                                      double* pos_ubs, float* pos_gts, int32_t* prior, uavgnn_stream_t stream) {
  if (!int_consts || !f64_consts || B < 0 || !rng || !pos_ubs || !pos_gts || !prior) return UAVGNN_EINVAL;
  const int G = int_consts[0], P = int_consts[1];
  if (G < 1 || P < 1) return UAVGNN_EINVAL;
  if (static_cast<long long>(G) * P > kMaxGts) return UAVGNN_EUNSUPPORTED;
  if (B == 0) return 0;
  const int M = G * P;
  const int wpb = waves_per_block(M);
  hipLaunchKernelGGL(subs_env_sample_kernel, dim3((B + wpb - 1) / wpb), dim3(kWave * wpb), static_cast<size_t>(wpb) * M * 4,
                     static_cast<hipStream_t>(stream), G, P, f64_consts[0], f64_consts[1], B, rng, pos_ubs, pos_gts, prior);
  return launch_status();
}

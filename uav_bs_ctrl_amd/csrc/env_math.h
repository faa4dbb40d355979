// What the environment kernels must agree on, ONE text each: the constants of uavgnn_env_step, the elements of an observation
// (csrc/env_sim.hip writes them when a step is simulated, csrc/replay_rebuild.hip rewrites the same bits from the stored simulator
// state), the A2G channel gain (csrc/env_sim.hip, csrc/subs_env.hip), the stable rank behind every argsort and the draw primitives of
// the reset-time samplers (csrc/map_sample.hip, csrc/subs_env.hip).  Every function restates the reference operation by operation
// and dtype by dtype (NumPy 2 promotion rules): operand order, casts and the places where a value is rounded to float32 are part of
// the contract - a caller that needs another arithmetic (the reset-time float32 branch of csrc/subs_env.hip) keeps its own text.
#ifndef UAVGNN_ENV_MATH_H
#define UAVGNN_ENV_MATH_H
#include "common.h"

namespace uavgnn {

// ---- constants of uavgnn_env_step (layout: include/uavgnn.h) ---------------------------------------------------------------------
enum EnvIntConst {
  kEnvNUbs = 0, kEnvNGts, kEnvNRbs, kEnvNActions, kEnvEpisodeLimit, kEnvFairService, kEnvAvoidCollision, kEnvIntConsts
};
enum EnvF64Const {
  kEnvRangePos = 0, kEnvRCov, kEnvRSns, kEnvRComm, kEnvDt, kEnvHUbs, kEnvPTx, kEnvN0, kEnvBw, kEnvFc, kEnvA, kEnvB, kEnvEtaLos,
  kEnvEtaNlos, kEnvSafeDist, kEnvPenalty, kEnvRewScale, kEnvMaxRate, kEnvF64Consts
};

struct EnvConsts {
  int n, M, R, A, episode_limit, fair_service, avoid_collision, state_dim;
  double range_pos, r_cov, r_sns, r_comm, dt, h_ubs, p_tx, n0, bw, fc, a, b, eta_los, eta_nlos, safe_dist, penalty,
      rew_scale, max_rate;
};

inline EnvConsts env_consts(const int32_t* int_consts, const double* f64_consts) {
  EnvConsts c;
  c.n = int_consts[kEnvNUbs]; c.M = int_consts[kEnvNGts]; c.R = int_consts[kEnvNRbs]; c.A = int_consts[kEnvNActions];
  c.episode_limit = int_consts[kEnvEpisodeLimit]; c.fair_service = int_consts[kEnvFairService];
  c.avoid_collision = int_consts[kEnvAvoidCollision];
  c.state_dim = uavgnn_env_state_dim(c.n, c.M, c.fair_service);
  c.range_pos = f64_consts[kEnvRangePos]; c.r_cov = f64_consts[kEnvRCov]; c.r_sns = f64_consts[kEnvRSns];
  c.r_comm = f64_consts[kEnvRComm]; c.dt = f64_consts[kEnvDt]; c.h_ubs = f64_consts[kEnvHUbs]; c.p_tx = f64_consts[kEnvPTx];
  c.n0 = f64_consts[kEnvN0]; c.bw = f64_consts[kEnvBw]; c.fc = f64_consts[kEnvFc]; c.a = f64_consts[kEnvA]; c.b = f64_consts[kEnvB];
  c.eta_los = f64_consts[kEnvEtaLos]; c.eta_nlos = f64_consts[kEnvEtaNlos]; c.safe_dist = f64_consts[kEnvSafeDist];
  c.penalty = f64_consts[kEnvPenalty]; c.rew_scale = f64_consts[kEnvRewScale]; c.max_rate = f64_consts[kEnvMaxRate];
  return c;
}

// ---- observation elements (mubs_cov.py:135-141, :215-242, :278-296) ----------------------------------------------------------------
// distance: float64 norm of float64 differences, stored float32
__device__ __forceinline__ float dist_f32(double dx, double dy) { return static_cast<float>(sqrt(dx * dx + dy * dy)); }
// offset of a visible neighbour: float64 difference / float64 min(range_pos, r_sns | r_comm)
__device__ __forceinline__ float obs_offset(double d, double norm) { return static_cast<float>(d / norm); }
__device__ __forceinline__ float obs_rate(float rate, double max_rate) {
  return static_cast<float>(static_cast<double>(rate) / max_rate);
}
__device__ __forceinline__ float obs_avg_rate(float avg, double max_rate, int M, int n, int R) {
  return static_cast<float>(static_cast<double>(avg) / max_rate * M / (n * R));
}
// agent position (float64) / range_pos
__device__ __forceinline__ float obs_pos(double pos, double range_pos) { return static_cast<float>(pos / range_pos); }
// GT position in the global state: float32 / float32(range_pos)
__device__ __forceinline__ float state_gt_pos(float gt, double range_pos) { return gt / static_cast<float>(range_pos); }

// ---- A2G channel (envs/common.py:49-59) ---------------------------------------------------------------------------------------------
// excess-loss factor of eta_los / eta_nlos, loop-invariant
__device__ __forceinline__ double a2g_excess_loss(double eta) { return pow(10.0, eta / 20.0); }
// p_tx * gain at float32 ground distance d: arctan / exp / LoS probability in float32 (float32 distances, Python scalars), direct
// distance and path loss in float64 (np.square(h_ubs) is a float64).  C: EnvConsts or the single-UBS constants.
template <class C>
__device__ __forceinline__ double a2g_rx_power(const C& c, float d, double k_los, double k_nlos) {
  const float ang = atanf(static_cast<float>(c.h_ubs) / (d + 1e-5f));
  const float p_los = 1.f / (1.f + static_cast<float>(c.a) * expf(-static_cast<float>(c.b) * (ang - static_cast<float>(c.a))));
  const double dd = sqrt(static_cast<double>(d * d) + c.h_ubs * c.h_ubs);
  const double q = 4.0 * 3.141592653589793 * c.fc * dd / 3e8;
  const double fspl = q * q;
  const double pl = static_cast<double>(p_los) * fspl * k_los + static_cast<double>(1.f - p_los) * fspl * k_nlos;
  return c.p_tx * (1.0 / pl);
}

// ---- stable ascending rank of keys[m] among keys[0..M): ties -> lower index first ---------------------------------------------------
template <class T>
__device__ __forceinline__ int stable_rank(const T* keys, int M, int m) {
  const T km = keys[m];
  int rank = 0;
  for (int m2 = 0; m2 < M; ++m2) {
    const T k2 = keys[m2];
    rank += (k2 < km) || (k2 == km && m2 < m);
  }
  return rank;
}

// ---- draws of the reset-time samplers: Philox4x32-10, key = seed, counter = (environment, slot, reset counter) ---------------------
struct Draws {
  uint32_t b, k0, k1, r0, r1;
  __device__ __forceinline__ void words(uint32_t slot, uint32_t w[4]) const {
    w[0] = b; w[1] = slot; w[2] = r0; w[3] = r1;
    philox4x32_10(w, k0, k1);
  }
  __device__ __forceinline__ uint32_t word0(uint32_t slot) const {
    uint32_t w[4];
    words(slot, w);
    return w[0];
  }
};

// uniform in (0, 1) from a word: ((w >> 9) + 1/2) 2^-23
__device__ __forceinline__ double unit(uint32_t w) { return (static_cast<double>(w >> 9) + 0.5) * 1.1920928955078125e-7; }
__device__ __forceinline__ double clip(double v, double hi) { return fmin(fmax(v, 0.0), hi); }

}  // namespace uavgnn
#endif  // UAVGNN_ENV_MATH_H

// Trajectory films of the evaluation simulators: what the reference's recorders keep of an episode, written on the device by ONE
// launch per step (reference: envs/mubs_cov/mubs_cov.py:99-100 reload, :126-127 click; envs/subs_cov/subs_cov.py:87-88 reload,
// :128-131 click; envs/mubs_cov/recorder.py and envs/subs_cov/recorder.py hold the film; algos/madrqn/run.py:73-74 and :132-178 and
// their algos/drqn twins read it back through `replay`).
//
// A film holds `episodes` episodes of T = episode_limit steps.  One launch records the CURRENT step of all B environments:
// environment b writes slot t[b] of episode e = episode_base + b, where t is the simulator's own DEVICE step counter (0 after a
// reset, k after the k-th step).  The slot is never a host value - the only host integer is episode_base, a constant of the round -
// so the same launch serves an eager loop, a captured graph and a caller's own loop, and it cannot drift from the simulator.
//
//   slot 0 (after the reset)     pos_ubs[e, 0] and the GT positions pos_gts[e]
//   slot k >= 1 (after a step)   pos_ubs[e, k] and element k - 1 of every per-step series
//
// uavgnn_film_click_mubs   pos_ubs [episodes, T+1, n, 2] f64   <- pos_ubs [B, n, 2]
//                          fair_idx [episodes, T] f64          <- run_f32[b, 2], widened
//                          reward [episodes, T] f64            <- (reward[b, 0] + ... + reward[b, n-1]) / n, added in agent order, in double
//                          pos_gts [episodes, M, 2] f32        <- pos_gts [B, M, 2]
// uavgnn_film_click_subs   pos_ubs [episodes, T+1, 2] f64      <- pos_ubs [B, 2]
//                          total_throughput / fair_idx / global_utility [episodes, T] f64 <- run_f64[b, 0] / [b, 2] / [b, 3]
//                          reward [episodes, T] f64            <- reward[b]
//                          rate_per_gt [episodes, T, M] f32    <- rate_per_gt [B, M]
//                          velocity [episodes, T] f64          <- hypot(moves[a_b, 0], moves[a_b, 1]) / dt, in double
//                          pos_gts [episodes, M, 2] f32        <- pos_gts [B, M, 2]
//
// Bounds.  An environment whose t[b] is outside 0 .. T or whose episode is outside 0 .. episodes - 1 writes NOTHING and ORs bit 0
// into `status` (device int32, never cleared by a kernel).  The single-UBS entry does the same for a step slot (t >= 1) recorded
// without actions (actions == NULL is the call after a reset) or with an action outside 0 .. A - 1.  No other store can leave the film.
//
// A grid-stride loop over (environment, element): element k of an environment is one value of one field, so every store is a plain
// vector store of 4 or 8 bytes and no two threads write the same address.  The only atomic is the OR into `status`.
#include "common.h"

#include <math.h>

namespace uavgnn {
namespace {

constexpr int kFilmThreads = 256;

__global__ __launch_bounds__(kFilmThreads) void film_click_mubs_kernel(
    int B, int n, int M, int T, int episodes, int episode_base, const int* __restrict__ t, const double* __restrict__ pos_ubs,
    const float* __restrict__ pos_gts, const float* __restrict__ run_f32, const double* __restrict__ reward,
    double* __restrict__ f_pos_ubs, double* __restrict__ f_fair_idx, double* __restrict__ f_reward, float* __restrict__ f_pos_gts,
    int* __restrict__ status) {
  const long long W = 2ll * n + 2 + 2ll * M;          // elements of one environment: positions, two scalars, GT positions
  const long long total = static_cast<long long>(B) * W, stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long b = i / W, k = i - b * W;
    const int slot = t[b];
    const long long e = static_cast<long long>(episode_base) + b;
    if (slot < 0 || slot > T || e >= episodes) {      // e >= 0: episode_base >= 0 is checked on the host
      if (k == 0) atomicOr(status, 1);
      continue;
    }
    if (k < 2ll * n) {
      f_pos_ubs[(e * (T + 1) + slot) * 2 * n + k] = pos_ubs[b * 2 * n + k];
    } else if (k == 2ll * n) {
      if (slot >= 1) f_fair_idx[e * T + slot - 1] = static_cast<double>(run_f32[b * 4 + 2]);
    } else if (k == 2ll * n + 1) {
      if (slot >= 1) {
        double s = 0.0;
        for (int a = 0; a < n; ++a) s += reward[b * n + a];
        f_reward[e * T + slot - 1] = s / static_cast<double>(n);
      }
    } else if (slot == 0) {
      const long long j = k - (2ll * n + 2);
      f_pos_gts[e * 2 * M + j] = pos_gts[b * 2 * M + j];
    }
  }
}

__global__ __launch_bounds__(kFilmThreads) void film_click_subs_kernel(
    int B, int M, int T, int A, double dt, int episodes, int episode_base, const int* __restrict__ t,
    const long long* __restrict__ actions, const double* __restrict__ moves, const double* __restrict__ pos_ubs,
    const float* __restrict__ pos_gts, const double* __restrict__ run_f64, const double* __restrict__ reward,
    const float* __restrict__ rate_per_gt, double* __restrict__ f_pos_ubs, double* __restrict__ f_total_throughput,
    double* __restrict__ f_fair_idx, double* __restrict__ f_global_utility, double* __restrict__ f_reward,
    float* __restrict__ f_rate_per_gt, double* __restrict__ f_velocity, float* __restrict__ f_pos_gts, int* __restrict__ status) {
  const long long W = 7 + 3ll * M;                    // 2 position values, 5 scalars, M rates, 2 M GT position values
  const long long total = static_cast<long long>(B) * W, stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long b = i / W, k = i - b * W;
    const int slot = t[b];
    const long long e = static_cast<long long>(episode_base) + b;
    bool ok = slot >= 0 && slot <= T && e < episodes;
    long long act = 0;
    if (ok && slot >= 1) {
      ok = actions != nullptr;
      if (ok) {
        act = actions[b];
        ok = act >= 0 && act < A;
      }
    }
    if (!ok) {
      if (k == 0) atomicOr(status, 1);
      continue;
    }
    const long long s = e * T + slot - 1;             // element of the per-step series (read only where slot >= 1)
    if (k < 2) {
      f_pos_ubs[(e * (T + 1) + slot) * 2 + k] = pos_ubs[b * 2 + k];
    } else if (k < 7) {
      if (slot >= 1) {
        if (k == 2) f_total_throughput[s] = run_f64[b * 4 + 0];
        else if (k == 3) f_fair_idx[s] = run_f64[b * 4 + 2];
        else if (k == 4) f_global_utility[s] = run_f64[b * 4 + 3];
        else if (k == 5) f_reward[s] = reward[b];
        else f_velocity[s] = hypot(moves[2 * act], moves[2 * act + 1]) / dt;
      }
    } else if (k < 7 + M) {
      if (slot >= 1) f_rate_per_gt[s * M + (k - 7)] = rate_per_gt[b * M + (k - 7)];
    } else if (slot == 0) {
      const long long j = k - (7 + M);
      f_pos_gts[e * 2 * M + j] = pos_gts[b * 2 * M + j];
    }
  }
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_film_click_mubs(int B, int n, int M, int T, int episodes, int episode_base, const int32_t* t,
                                      const double* pos_ubs, const float* pos_gts, const float* run_f32, const double* reward,
                                      double* film_pos_ubs, double* film_fair_idx, double* film_reward, float* film_pos_gts,
                                      int32_t* status, uavgnn_stream_t stream) {
  if (B < 0 || n < 1 || M < 0 || T < 1 || episodes < 0 || episode_base < 0) return UAVGNN_EINVAL;
  if (!t || !pos_ubs || !run_f32 || !reward || !film_pos_ubs || !film_fair_idx || !film_reward || !status) return UAVGNN_EINVAL;
  if (M > 0 && (!pos_gts || !film_pos_gts)) return UAVGNN_EINVAL;
  if (B == 0) return 0;
  const long long work = static_cast<long long>(B) * (2ll * n + 2 + 2ll * M);
  hipLaunchKernelGGL(film_click_mubs_kernel, dim3(capped_grid(work, kFilmThreads)), dim3(kFilmThreads), 0,
                     static_cast<hipStream_t>(stream), B, n, M, T, episodes, episode_base, t, pos_ubs, pos_gts, run_f32, reward,
                     film_pos_ubs, film_fair_idx, film_reward, film_pos_gts, status);
  return launch_status();
}

extern "C" int uavgnn_film_click_subs(int B, int M, int T, int A, double dt, int episodes, int episode_base, const int32_t* t,
                                      const long long* actions, const double* avail_moves, const double* pos_ubs,
                                      const float* pos_gts, const double* run_f64, const double* reward, const float* rate_per_gt,
                                      double* film_pos_ubs, double* film_total_throughput, double* film_fair_idx,
                                      double* film_global_utility, double* film_reward, float* film_rate_per_gt,
                                      double* film_velocity, float* film_pos_gts, int32_t* status, uavgnn_stream_t stream) {
  if (B < 0 || M < 0 || T < 1 || A < 1 || !(dt > 0.0) || episodes < 0 || episode_base < 0) return UAVGNN_EINVAL;
  if (!t || !avail_moves || !pos_ubs || !run_f64 || !reward || !film_pos_ubs || !film_total_throughput || !film_fair_idx ||
      !film_global_utility || !film_reward || !film_velocity || !status)
    return UAVGNN_EINVAL;
  if (M > 0 && (!pos_gts || !rate_per_gt || !film_rate_per_gt || !film_pos_gts)) return UAVGNN_EINVAL;
  if (B == 0) return 0;
  const long long work = static_cast<long long>(B) * (7 + 3ll * M);
  hipLaunchKernelGGL(film_click_subs_kernel, dim3(capped_grid(work, kFilmThreads)), dim3(kFilmThreads), 0,
                     static_cast<hipStream_t>(stream), B, M, T, A, dt, episodes, episode_base, t, actions, avail_moves, pos_ubs,
                     pos_gts, run_f64, reward, rate_per_gt, film_pos_ubs, film_total_throughput, film_fair_idx, film_global_utility,
                     film_reward, film_rate_per_gt, film_velocity, film_pos_gts, status);
  return launch_status();
}

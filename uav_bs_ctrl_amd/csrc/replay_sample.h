// What the two replay samplers share (csrc/replay.hip: one workgroup, capacity <= 65 536; csrc/replay_wide.hip: many workgroups):
// the key of a slot under THE RULE of csrc/replay.hip and the wavefront prefix sum both compactions are built on.
#pragma once
#include "common.h"

namespace uavgnn {

// key(s) = philox4x32_10(counter = (s, 0, draws_lo, draws_hi), key = (seed_lo, seed_hi))[0]
struct SampleKey {
  uint32_t d0, d1, k0, k1;
  __device__ __forceinline__ uint32_t operator()(uint32_t s) const {
    uint32_t c[4] = {s, 0u, d0, d1};
    philox4x32_10(c, k0, k1);
    return c[0];
  }
};

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int up = __shfl_up(v, o);
    v += lane >= o ? up : 0;
  }
  return v;
}

}  // namespace uavgnn

// Wavefront helpers of the K1 forward family (csrc/gatv2_hetero.hip, csrc/gatv2_hetero_f32.hip, csrc/gatv2_mfma.hip,
// csrc/gatv2_small.hip): DPP moves inside a 16-lane row, the all-reduces built on them and the head reduction over the four lane
// groups of the MFMA D layout.  (The K1 backward, csrc/gatv2.hip, has helpers of its own.)
#ifndef UAVGNN_K1_WAVE_H
#define UAVGNN_K1_WAVE_H
#include "common.h"

namespace uavgnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.4426950408889634f;

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), CTRL, 0xf, 0xf, false));
}
constexpr int kRowRor = 0x120;        // DPP control base of row_ror:n
constexpr int kQuadXor1 = 0xB1;       // quad_perm:[1,0,3,2]
constexpr int kQuadXor2 = 0x4E;       // quad_perm:[2,3,0,1]
constexpr int kHalfMirror = 0x141;    // row_half_mirror: lane i <-> 7 - i inside every 8 lanes

// All-reduce over the 16 lanes of a row (lane>>4 fixed) with DPP row rotations: v += ror(v, 8), 4, 2, 1.
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<kRowRor + 8>(v);
  v += dpp_mov<kRowRor + 4>(v);
  v += dpp_mov<kRowRor + 2>(v);
  v += dpp_mov<kRowRor + 1>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_mov<kRowRor + 8>(v));
  v = fmaxf(v, dpp_mov<kRowRor + 4>(v));
  v = fmaxf(v, dpp_mov<kRowRor + 2>(v));
  v = fmaxf(v, dpp_mov<kRowRor + 1>(v));
  return v;
}

// Sum pe[k] over the four 16-lane groups and leave head (lane>>4)'s total in every lane: 3 swaps + 3 adds.
__device__ __forceinline__ float reduce_heads(float pe0, float pe1, float pe2, float pe3) {
  auto s02 = __builtin_amdgcn_permlane32_swap(__float_as_uint(pe0), __float_as_uint(pe2), false, false);
  const float a = __uint_as_float(s02[0]) + __uint_as_float(s02[1]);  // lo half: head 0 over {g,g+2}; hi half: head 2
  auto s13 = __builtin_amdgcn_permlane32_swap(__float_as_uint(pe1), __float_as_uint(pe3), false, false);
  const float b = __uint_as_float(s13[0]) + __uint_as_float(s13[1]);  // lo half: head 1; hi half: head 3
  auto t = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(t[0]) + __uint_as_float(t[1]);
}

// v of lane `lane` (wave-uniform index) in every lane
__device__ __forceinline__ float rl(float v, int lane) {
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), lane));
}

}  // namespace uavgnn
#endif  // UAVGNN_K1_WAVE_H

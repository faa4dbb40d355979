// fp32 GEMM arithmetic on the f16 matrix cores of gfx950 with exactly scaled two-term splits ("f16x2"): shared device helpers.
//
// The arithmetic, its error bound and its non-finite behaviour are described in csrc/gru_h2.hip's header.  Everything that takes
// part in it - the weight-split kernels (uavgnn_split_h2, uavgnn_gru_split_weights_h2) and every consumer (csrc/gru_h2.hip,
// csrc/gemm_h2.hip, csrc/gemm_tn_h2.hip) - takes the scale exponent and the split from HERE: the exactness argument needs them to
// agree bit for bit.  tests/test_f16x2_emulation.py restates these functions in NumPy.
#pragma once
#include <hip/hip_runtime.h>

namespace uavgnn {
namespace h2 {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// 32x32x16 fragments read from 32-wide K slices of four 16-byte chunks per row (the layout and swizzle of bf16x3.h's swz32)
__device__ __forceinline__ int swz32(int row) { return (row >> 2) & 3; }
__device__ __forceinline__ f16x8 as_frag(u32x4 v) { return __builtin_bit_cast(f16x8, v); }
__device__ __forceinline__ f32x16 mfma32(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// scale exponent of a row (column) whose largest magnitude is `amax`: 2^se * amax lies in [2^14, 2^15) (se clamped to the normal range)
__device__ __forceinline__ int scale_exp(float amax) {
  const int e = static_cast<int>((__float_as_uint(amax) >> 23) & 0xffu);      // biased exponent; 255: Inf / NaN, 0: zero / subnormal
  return max(-126, min(126, 14 - (e - 127)));
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float(static_cast<unsigned>(e + 127) << 23); }

struct Split2 {
  unsigned hi, lo;   // two packed f16 each: low half = first element
};
// (x, y) already scaled -> hi + lo (round to nearest even both times; x - hi is exact in fp32)
__device__ __forceinline__ Split2 split_pair(float x, float y) {
  Split2 s;
  const f16x2 h = __builtin_convertvector(f32x2{x, y}, f16x2);
  s.hi = __builtin_bit_cast(unsigned, h);
  const f32x2 r = f32x2{x, y} - __builtin_convertvector(h, f32x2);
  s.lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
  return s;
}
// four consecutive k of one row (one 16-byte global load) scaled by `s` -> one 8-byte group per plane
__device__ __forceinline__ void stage4(unsigned short* p, int plane_stride, float4 v, float s) {
  const Split2 a = split_pair(v.x * s, v.y * s), b = split_pair(v.z * s, v.w * s);
  *reinterpret_cast<u32x2*>(p) = u32x2{a.hi, b.hi};
  *reinterpret_cast<u32x2*>(p + plane_stride) = u32x2{a.lo, b.lo};
}
// four consecutive columns of one row, each with its own column scale -> one 8-byte group per plane
__device__ __forceinline__ void stage4(unsigned short* p, int plane_stride, float4 v, float4 s) {
  const Split2 a = split_pair(v.x * s.x, v.y * s.y), b = split_pair(v.z * s.z, v.w * s.w);
  *reinterpret_cast<u32x2*>(p) = u32x2{a.hi, b.hi};
  *reinterpret_cast<u32x2*>(p + plane_stride) = u32x2{a.lo, b.lo};
}

}  // namespace h2
}  // namespace uavgnn

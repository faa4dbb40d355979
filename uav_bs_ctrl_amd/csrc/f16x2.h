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
// The split of v at the power-of-two scale s: hi = f16(v s), lo = f16(v s - hi), round to nearest even both times, f16 subnormals kept.
// Each term is ONE mixed-precision FMA (fp32 x fp32 + addend -> the f16 low or high half of the destination, v_fma_mixlo_f16 /
// v_fma_mixhi_f16; lo takes hi as its f16 addend): four single-pass instructions per element pair, and no packed fp32 beside the
// MFMAs.  Same bits as a separate multiply, conversion and subtraction: v s is exact (s is a power of two) and v s - hi is exact in
// fp32, so the FMA's single rounding is the conversion's; the -0 addend keeps the sign of a zero product.  (Only a product below the
// fp32 range, |v s| < 2^-150, is treated differently: there a negative one leaves lo = -0 where the rounded product gave +0; hi and
// every dot product are the same.)  The plain C++ form compiles to five to seven VALU per pair - the compiler recomputes hi for the
// second FMA - hence the asm; it is not volatile, so the scheduler still moves it.
//
// (x sx, y sy) -> hi + lo: the weight-split kernels (one pair per thread and trip)
__device__ __forceinline__ Split2 split_pair(float x, float y, float sx, float sy) {
  Split2 s;
  const float nz = -0.f;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "=v"(s.hi) : "v"(x), "v"(sx), "s"(nz));
  asm("v_fma_mixhi_f16 %0, %1, %2, %3" : "+v"(s.hi) : "v"(y), "v"(sy), "s"(nz));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(s.lo) : "v"(x), "v"(sx), "v"(s.hi));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(s.lo) : "v"(y), "v"(sy), "v"(s.hi));
  return s;
}
__device__ __forceinline__ Split2 split_pair(float x, float y, float s) { return split_pair(x, y, s, s); }
// Four values (one 16-byte load) in two steps of four instructions, for the kernels that stage inside their MFMA loops: the hi words
// {(v.x, v.y), (v.z, v.w)}, then the lo words from them.  The two destinations of a step alternate, so no instruction reads the
// register its predecessor wrote half of (the wait state that costs), and a step is one statement: it moves as a whole and a hand
// schedule can place it (the scheduler's instruction groups do not see asm).
__device__ __forceinline__ u32x2 split4_hi(float4 v, float4 s) {
  unsigned a, b;
  const float nz = -0.f;
  asm("v_fma_mixlo_f16 %0, %2, %6, %10\n\t"
      "v_fma_mixlo_f16 %1, %4, %8, %10\n\t"
      "v_fma_mixhi_f16 %0, %3, %7, %10\n\t"
      "v_fma_mixhi_f16 %1, %5, %9, %10"
      : "=&v"(a), "=&v"(b)
      : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w), "v"(s.x), "v"(s.y), "v"(s.z), "v"(s.w), "s"(nz));
  return u32x2{a, b};
}
__device__ __forceinline__ u32x2 split4_lo(float4 v, float4 s, u32x2 hi) {
  unsigned a, b;
  asm("v_fma_mixlo_f16 %0, %2, %6, -%10 op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixlo_f16 %1, %4, %8, -%11 op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %0, %3, %7, -%10 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %1, %5, %9, -%11 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "=&v"(a), "=&v"(b)
      : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w), "v"(s.x), "v"(s.y), "v"(s.z), "v"(s.w), "v"(hi[0]), "v"(hi[1]));
  return u32x2{a, b};
}
__device__ __forceinline__ float4 scale4(float s) { return make_float4(s, s, s, s); }
// four consecutive columns of one row, each at its own column scale -> one 8-byte group per plane
__device__ __forceinline__ void stage4(unsigned short* p, int plane_stride, float4 v, float4 s) {
  const u32x2 hi = split4_hi(v, s);
  *reinterpret_cast<u32x2*>(p) = hi;
  *reinterpret_cast<u32x2*>(p + plane_stride) = split4_lo(v, s, hi);
}
// four consecutive k of one row (one 16-byte global load) at the row's scale `s` -> one 8-byte group per plane
__device__ __forceinline__ void stage4(unsigned short* p, int plane_stride, float4 v, float s) { stage4(p, plane_stride, v, scale4(s)); }

}  // namespace h2
}  // namespace uavgnn

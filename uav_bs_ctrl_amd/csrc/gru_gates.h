// Fast gate non-linearities of the matrix-core GRU cells (csrc/gru_x3.hip, csrc/gru_h2.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace uavgnn {

// on the hardware transcendentals (v_exp_f32, v_rcp_f32: 1 ulp each): absolute error <= 2e-7, far inside the 1e-5 parity
// tolerance; tanh as 1 - 2 / (1 + e^{2x}) saturates correctly at both ends (e^{2x} -> inf / 0).  NOT csrc/gru_fused.hip's
// sigmoidf_ (1 / (1 + expf(-x)), the accurate library calls), which the fp32 cell and the gate-gradient kernels keep.
__device__ __forceinline__ float fast_sigmoid(float x) { return __frcp_rn(1.f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.f - 2.f * __frcp_rn(1.f + __expf(2.f * x)); }

}  // namespace uavgnn

// The Q head of the agent - q = h' W_out^T + b_out, /root/reference/algos/madrqn/agents/gnn_agents.py:43-46,:56 (nn.Linear(H, n_actions)) -
// for n_actions <= 16: [N, 256] x [256, 9] at C3.  The vendor GEMM takes 11.8 us for it (a 16 x 256 macro tile, 82 TFLOP/s: neither
// compute- nor bandwidth-bound); what the layer costs is reading h' once - 33.5 MB, ~7 us.
//
// One wavefront per tile of 16 rows, fp32 products on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 multiply, fp32 accumulate, a
// fixed order): lane (i, g) loads float4 s of row i - columns 16 s + 4 g .. + 3, 64 contiguous bytes per row and instruction - and
// feeds its four components to four MFMAs as the A element of K slot g; lane (j, g) holds the same four columns of row j of W_out
// (zero for j >= n_actions) as the B element.  The contraction order inside a 16-wide slice is therefore permuted (slot g of MFMA
// (s, c) is column 16 s + 4 g + c) - a sum over k does not care, both operands agree.  H / 16 loads per lane are issued before the
// first MFMA: 16 KB per wavefront in flight.  The weights live in registers (H / 4 per lane).
//
// The dueling form - q = V + (A - mean_a A), the reference's algos/madrqn/agents/dueling.py:13-16, the head the agent builds at
// gnn_agents.py:43-46 and calls at :56 when `dueling` is set - for n_actions <= 15 on the same schedule (head_fwd_duel_kernel): lane
// (j, g) holds row j of adv_head.weight for j < A, v_head.weight for j == A, zeros above, each read through its own pointer (no stacked
// copy of the parameters exists, so there is nothing to invalidate after an optimiser step).  The combine stays in registers: in the D
// layout the 16 lanes that share g hold the 16 columns of one output row per r, i.e. one DPP row - the advantage sum and the broadcast of
// the value column are four row rotations each (a fixed tree, every lane ends with the same bits).
#include "common.h"

namespace uavgnn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int NS>   // NS = H / 16 float4 loads per lane and row tile
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ h, int ld_h, int N, const float* __restrict__ W, int ld_w,
                                                       const float* __restrict__ b, int A, float* __restrict__ q, int ld_q, int tiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  float4 w[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    w[s] = j < A ? *reinterpret_cast<const float4*>(W + static_cast<size_t>(j) * ld_w + 16 * s + 4 * g) : float4{0.f, 0.f, 0.f, 0.f};
  const float bj = j < A ? b[j] : 0.f;
  for (int tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
    const int row0 = tile * 16;
    const float* __restrict__ hr = h + static_cast<size_t>(min(row0 + j, N - 1)) * ld_h + 4 * g;
    float4 a[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = *reinterpret_cast<const float4*>(hr + 16 * s);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, w[s].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, w[s].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, w[s].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, w[s].w, acc, 0, 0, 0);
    }
    // D layout: lane (j, g) holds column j of rows 4 g .. 4 g + 3
    if (j < A) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * g + r;
        if (row < N) q[static_cast<size_t>(row) * ld_q + j] = acc[r] + bj;
      }
    }
  }
}

// sum over the 16 lanes of a DPP row, the same bits in every lane: after the rotation by 8 the values have period 8 within the row, then
// 4, 2, 1 (x + y == y + x), so the tree is one and the same for all lanes
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_allsum(float v) {
  constexpr int kRowRorCtl = 0x120;
  v += dpp_f<kRowRorCtl + 8>(v);
  v += dpp_f<kRowRorCtl + 4>(v);
  v += dpp_f<kRowRorCtl + 2>(v);
  v += dpp_f<kRowRorCtl + 1>(v);
  return v;
}

template <int NS>   // NS = H / 16 float4 loads per lane and row tile
__global__ __launch_bounds__(256) void head_fwd_duel_kernel(const float* __restrict__ h, int ld_h, int N, const float* __restrict__ W_adv,
                                                            int ld_w, const float* __restrict__ w_v, const float* __restrict__ b_adv,
                                                            const float* __restrict__ b_v, int A, float* __restrict__ q, int ld_q,
                                                            int tiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  // columns 0 .. A - 1: the advantages, column A: the state value, above: zeros
  const float* __restrict__ wr = j < A ? W_adv + static_cast<size_t>(j) * ld_w : w_v;
  float4 w[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    w[s] = j <= A ? *reinterpret_cast<const float4*>(wr + 16 * s + 4 * g) : float4{0.f, 0.f, 0.f, 0.f};
  const float bj = j < A ? b_adv[j] : (j == A ? b_v[0] : 0.f);
  const float inv_A = 1.f / static_cast<float>(A);
  for (int tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
    const int row0 = tile * 16;
    const float* __restrict__ hr = h + static_cast<size_t>(min(row0 + j, N - 1)) * ld_h + 4 * g;
    float4 a[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = *reinterpret_cast<const float4*>(hr + 16 * s);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, w[s].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, w[s].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, w[s].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, w[s].w, acc, 0, 0, 0);
    }
    // D layout: lane (j, g) holds column j of rows 4 g .. 4 g + 3 - the 16 lanes of a DPP row hold one output row per r.  All 64 lanes
    // take part in the row sums (no branch around them); only the stores are masked
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float y = acc[r] + bj;                                  // bias before the combine, as nn.Linear
      const float adv_sum = row16_allsum(j < A ? y : 0.f);          // columns >= A enter as zeros
      const float val = row16_allsum(j == A ? y : 0.f);             // one non-zero term: the value column itself, in every lane
      const int row = row0 + 4 * g + r;
      if (j < A && row < N) q[static_cast<size_t>(row) * ld_q + j] = val + (y - adv_sum * inv_A);
    }
  }
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_head_supported(int H, int A) { return (H == 64 || H == 128 || H == 256) && A >= 1 && A <= 16; }

// q [N, A] (row stride ld_q) = h [N, H] (row stride ld_h) W [A, H]^T (row stride ld_w) + b [A]; fp32, products exact in fp32
extern "C" int uavgnn_head_fwd(const float* h, int ld_h, int N, int H, const float* W, int ld_w, const float* b, int A, float* q, int ld_q,
                               uavgnn_stream_t stream) {
  if (N < 0 || !h || !W || !b || !q || ld_h < H || ld_w < H || ld_q < A) return UAVGNN_EINVAL;
  if (!uavgnn_head_supported(H, A) || (ld_h & 3) || (ld_w & 3) ||
      ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(W)) & 15))
    return UAVGNN_EUNSUPPORTED;
  if (N == 0) return 0;
  const int tiles = (N + 15) / 16;
  const dim3 grid(capped_grid(tiles, 4, 4096)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define UAVGNN_HEAD(NS_) hipLaunchKernelGGL((head_fwd_kernel<NS_>), grid, block, 0, st, h, ld_h, N, W, ld_w, b, A, q, ld_q, tiles)
  switch (H) {
    case 64: UAVGNN_HEAD(4); break;
    case 128: UAVGNN_HEAD(8); break;
    default: UAVGNN_HEAD(16); break;
  }
#undef UAVGNN_HEAD
  return launch_status();
}

extern "C" int uavgnn_head_duel_supported(int H, int A) { return (H == 64 || H == 128 || H == 256) && A >= 1 && A <= 15; }

// q [N, A] (row stride ld_q) = v + (adv - mean over the A columns of adv), adv = h W_adv^T + b_adv, v = h w_v^T + b_v (dueling.py:13-16)
extern "C" int uavgnn_head_fwd_duel(const float* h, int ld_h, int N, int H, const float* W_adv, int ld_w, const float* w_v,
                                    const float* b_adv, const float* b_v, int A, float* q, int ld_q, uavgnn_stream_t stream) {
  if (N < 0 || !h || !W_adv || !w_v || !b_adv || !b_v || !q || ld_h < H || ld_w < H || ld_q < A) return UAVGNN_EINVAL;
  if (!uavgnn_head_duel_supported(H, A) || (ld_h & 3) || (ld_w & 3) ||
      ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(W_adv) | reinterpret_cast<uintptr_t>(w_v)) & 15))
    return UAVGNN_EUNSUPPORTED;
  if (N == 0) return 0;
  const int tiles = (N + 15) / 16;
  const dim3 grid(capped_grid(tiles, 4, 4096)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define UAVGNN_HEAD_DUEL(NS_)                                                                                                     \
  hipLaunchKernelGGL((head_fwd_duel_kernel<NS_>), grid, block, 0, st, h, ld_h, N, W_adv, ld_w, w_v, b_adv, b_v, A, q, ld_q, tiles)
  switch (H) {
    case 64: UAVGNN_HEAD_DUEL(4); break;
    case 128: UAVGNN_HEAD_DUEL(8); break;
    default: UAVGNN_HEAD_DUEL(16); break;
  }
#undef UAVGNN_HEAD_DUEL
  return launch_status();
}

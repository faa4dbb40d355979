// The noisy-net Q head (include/uavgnn_ext.h; Fortunato et al., ICLR 2018, factorised Gaussian noise): q = h W^T + b with
// W = W_mu + W_sigma (.) (f_out f_in^T), b = b_mu + b_sigma (.) f_out, f(z) = sign(z) sqrt|z|.
//
// Mode "rows" (noisy_head_fwd_kernel): every row has its own draw, so no effective weight exists - but the noise factorises,
//   q[r, j] = (h[r, :] . W_mu[j, :] + b_mu[j]) + f_out[r, j] * ((h[r, :] (.) f_in[r, :]) . W_sigma[j, :] + b_sigma[j]),
// i.e. two products over the same pass of h on the schedule of csrc/head.hip: one wavefront per tile of 16 rows, lane (i, g) loads
// float4 s of row i - columns 16 s + 4 g .. + 3 - and feeds its components to v_mfma_f32_16x16x4_f32 as the A element of K slot g,
// lane (j, g) holds the same columns of row j of BOTH weight matrices as B elements.  The four columns of one load are the four
// normals of ONE Philox block, block(i, 4 s + g): one generator call per load, and the noise never leaves the registers.  f_out is
// needed in the D layout (lane (j, g): column j of rows 4 g .. 4 g + 3): the lanes (i, g < ceil(A / 4)) draw block(i, 0x10000 + g)
// and the tile is transposed by lane permutes (ds_bpermute: no LDS is allocated).
//
// Mode "shared" (noisy_fold_kernel / noisy_fold_bwd_kernel): one draw for a whole update, folded into (W_eff, b_eff) once.
//
// Compiled without packed fp32 and with -ffp-contract=off (build.py): the header fixes the order of single-rounded operations.
#include "common.h"
#include "uavgnn_ext.h"

namespace uavgnn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kOutBlock0 = 0x10000u;   // xi_out's block indices start here; xi_in's end below (H <= 4 * 0x10000)
constexpr int kMaxCols = 4 * 0x10000;

// f(z) = sign(z) sqrt|z|
__device__ __forceinline__ float f_noise(float z) { return copysignf(sqrtf(fabsf(z)), z); }

// f of the four normals of block(row, b) at the pair (seed, step): THE definition every kernel of this file shares
__device__ __forceinline__ float4 f_block(uint32_t row, uint32_t b, uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo,
                                          uint32_t step_hi) {
  uint32_t c[4] = {row, b, step_lo, step_hi};
  philox4x32_10(c, seed_lo, seed_hi);
  constexpr float kScale = 1.f / 8388608.f;   // 2^-23
  const float u0 = (static_cast<float>(c[0] >> 9) + 0.5f) * kScale, u1 = (static_cast<float>(c[1] >> 9) + 0.5f) * kScale;
  const float u2 = (static_cast<float>(c[2] >> 9) + 0.5f) * kScale, u3 = (static_cast<float>(c[3] >> 9) + 0.5f) * kScale;
  const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u2));
  float s0, c0, s1, c1;
  sincospif(2.f * u1, &s0, &c0);   // cos(2 pi u), sin(2 pi u): the reduction of sincospi is exact
  sincospif(2.f * u3, &s1, &c1);
  return float4{f_noise(r0 * c0), f_noise(r0 * s0), f_noise(r1 * c1), f_noise(r1 * s1)};
}

struct Pair {
  uint32_t seed_lo, seed_hi, step_lo, step_hi;
};
__device__ __forceinline__ Pair load_pair(const long long* __restrict__ rng) {
  const unsigned long long seed = static_cast<unsigned long long>(rng[0]), step = static_cast<unsigned long long>(rng[1]);
  return Pair{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(step),
              static_cast<uint32_t>(step >> 32)};
}
__device__ __forceinline__ float4 f_block(uint32_t row, uint32_t b, const Pair& p) {
  return f_block(row, b, p.seed_lo, p.seed_hi, p.step_lo, p.step_hi);
}

__device__ __forceinline__ float component(const float4& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); }

template <int NS>   // NS = H / 16 float4 loads per lane and row tile
__global__ __launch_bounds__(256) void noisy_head_fwd_kernel(const float* __restrict__ h, int ld_h, int N, const float* __restrict__ W_mu,
                                                             const float* __restrict__ W_sigma, int ld_w, const float* __restrict__ b_mu,
                                                             const float* __restrict__ b_sigma, int A,
                                                             const long long* __restrict__ rng, float* __restrict__ q, int ld_q, int tiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const Pair pair = load_pair(rng);
  float4 wm[NS], ws[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const size_t off = static_cast<size_t>(j) * ld_w + 16 * s + 4 * g;
    wm[s] = j < A ? *reinterpret_cast<const float4*>(W_mu + off) : float4{0.f, 0.f, 0.f, 0.f};
    ws[s] = j < A ? *reinterpret_cast<const float4*>(W_sigma + off) : float4{0.f, 0.f, 0.f, 0.f};
  }
  const float bm = j < A ? b_mu[j] : 0.f, bs = j < A ? b_sigma[j] : 0.f;
  const int out_blocks = (A + 3) >> 2;
  for (int tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
    const int row0 = tile * 16;
    const int row_a = min(row0 + j, N - 1);    // rows past N repeat the last one (its noise too): never stored
    const float* __restrict__ hr = h + static_cast<size_t>(row_a) * ld_h + 4 * g;
    float4 a[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = *reinterpret_cast<const float4*>(hr + 16 * s);
    // f_out of row i = row0 + j, columns 4 g .. 4 g + 3, in the lanes with g < ceil(A / 4); drawn while the loads are in flight
    float4 fo = {0.f, 0.f, 0.f, 0.f};
    if (g < out_blocks) fo = f_block(static_cast<uint32_t>(row_a), kOutBlock0 + g, pair);
    f32x4 acc_m = {0.f, 0.f, 0.f, 0.f}, acc_s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float4 fi = f_block(static_cast<uint32_t>(row_a), static_cast<uint32_t>(4 * s + g), pair);
      acc_m = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, wm[s].x, acc_m, 0, 0, 0);
      acc_s = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x * fi.x, ws[s].x, acc_s, 0, 0, 0);
      acc_m = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, wm[s].y, acc_m, 0, 0, 0);
      acc_s = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y * fi.y, ws[s].y, acc_s, 0, 0, 0);
      acc_m = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, wm[s].z, acc_m, 0, 0, 0);
      acc_s = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z * fi.z, ws[s].z, acc_s, 0, 0, 0);
      acc_m = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, wm[s].w, acc_m, 0, 0, 0);
      acc_s = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w * fi.w, ws[s].w, acc_s, 0, 0, 0);
    }
    // D layout: lane (j, g) holds column j of rows 4 g .. 4 g + 3; f_out[row 4 g + r, column j] is component j & 3 of the draw held by
    // lane (i = 4 g + r, g' = j >> 2).  All 64 lanes take part in the permutes (no branch around them); only the stores are masked
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int src = (4 * g + r) + 16 * (j >> 2);
      const float4 t = {__shfl(fo.x, src), __shfl(fo.y, src), __shfl(fo.z, src), __shfl(fo.w, src)};
      const float f = component(t, j & 3);
      const int row = row0 + 4 * g + r;
      if (j < A && row < N) q[static_cast<size_t>(row) * ld_q + j] = (acc_m[r] + bm) + f * (acc_s[r] + bs);
    }
  }
}

// f_in [N, H] and f_out [N, A] of the stream: one work item per Philox block
__global__ __launch_bounds__(256) void noisy_noise_kernel(const long long* __restrict__ rng, int N, int H, int A, float* __restrict__ f_in,
                                                          float* __restrict__ f_out) {
  const Pair pair = load_pair(rng);
  const long long bi = f_in ? (H + 3) >> 2 : 0, bo = f_out ? (A + 3) >> 2 : 0, per_row = bi + bo;
  const long long total = per_row * N;
  for (long long it = blockIdx.x * 256ll + threadIdx.x; it < total; it += gridDim.x * 256ll) {
    const long long row = it / per_row, b = it - row * per_row;
    const bool in = b < bi;
    const uint32_t blk = in ? static_cast<uint32_t>(b) : kOutBlock0 + static_cast<uint32_t>(b - bi);
    const float4 f = f_block(static_cast<uint32_t>(row), blk, pair);
    const int cols = in ? H : A, c0 = 4 * static_cast<int>(in ? b : b - bi);
    float* __restrict__ dst = (in ? f_in : f_out) + row * cols + c0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < cols) dst[k] = component(f, k);
  }
}

// one work item per (output row j, block of four columns)
__global__ __launch_bounds__(256) void noisy_fold_kernel(const float* __restrict__ W_mu, const float* __restrict__ W_sigma, int ld_w,
                                                         const float* __restrict__ b_mu, const float* __restrict__ b_sigma, int A, int H,
                                                         const long long* __restrict__ rng, float* __restrict__ W_eff,
                                                         float* __restrict__ b_eff, float* __restrict__ f_in, float* __restrict__ f_out) {
  const Pair pair = load_pair(rng);
  const long long bi = (H + 3) >> 2, total = bi * A;
  for (long long it = blockIdx.x * 256ll + threadIdx.x; it < total; it += gridDim.x * 256ll) {
    const int j = static_cast<int>(it / bi), b = static_cast<int>(it - static_cast<long long>(j) * bi);
    const float4 fi = f_block(0u, static_cast<uint32_t>(b), pair);
    const float fo = component(f_block(0u, kOutBlock0 + static_cast<uint32_t>(j >> 2), pair), j & 3);
    if (b == 0) {
      f_out[j] = fo;
      b_eff[j] = b_mu[j] + b_sigma[j] * fo;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = 4 * b + k;
      if (col < H) {
        const float fk = component(fi, k);
        if (j == 0) f_in[col] = fk;
        const size_t src = static_cast<size_t>(j) * ld_w + col;
        W_eff[static_cast<size_t>(j) * H + col] = W_mu[src] + W_sigma[src] * (fo * fk);
      }
    }
  }
}

__global__ __launch_bounds__(256) void noisy_fold_bwd_kernel(const float* __restrict__ dW_eff, int ld, const float* __restrict__ db_eff,
                                                             const float* __restrict__ f_in, const float* __restrict__ f_out, int A, int H,
                                                             float* __restrict__ dW_sigma, float* __restrict__ db_sigma) {
  const long long total = static_cast<long long>(A) * H;
  for (long long it = blockIdx.x * 256ll + threadIdx.x; it < total; it += gridDim.x * 256ll) {
    const int j = static_cast<int>(it / H), k = static_cast<int>(it - static_cast<long long>(j) * H);
    const float fo = f_out[j];
    dW_sigma[it] = dW_eff[static_cast<size_t>(j) * ld + k] * (fo * f_in[k]);
    if (k == 0) db_sigma[j] = db_eff[j] * fo;
  }
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_noisy_head_supported(int H, int A) { return (H == 64 || H == 128 || H == 256) && A >= 1 && A <= 16; }

extern "C" int uavgnn_noisy_head_fwd(const float* h, int ld_h, int N, int H, const float* W_mu, const float* W_sigma, int ld_w,
                                     const float* b_mu, const float* b_sigma, int A, const long long* rng, float* q, int ld_q,
                                     uavgnn_stream_t stream) {
  if (N < 0 || !h || !W_mu || !W_sigma || !b_mu || !b_sigma || !rng || !q || ld_h < H || ld_w < H || ld_q < A) return UAVGNN_EINVAL;
  if (!uavgnn_noisy_head_supported(H, A) || (ld_h & 3) || (ld_w & 3) ||
      ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(W_mu) | reinterpret_cast<uintptr_t>(W_sigma)) & 15))
    return UAVGNN_EUNSUPPORTED;
  if (N == 0) return 0;
  const int tiles = (N + 15) / 16;
  const dim3 grid(capped_grid(tiles, 4, 4096)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define UAVGNN_NOISY_HEAD(NS_)                                                                                                       \
  hipLaunchKernelGGL((noisy_head_fwd_kernel<NS_>), grid, block, 0, st, h, ld_h, N, W_mu, W_sigma, ld_w, b_mu, b_sigma, A, rng, q, ld_q, \
                     tiles)
  switch (H) {
    case 64: UAVGNN_NOISY_HEAD(4); break;
    case 128: UAVGNN_NOISY_HEAD(8); break;
    default: UAVGNN_NOISY_HEAD(16); break;
  }
#undef UAVGNN_NOISY_HEAD
  return launch_status();
}

extern "C" int uavgnn_noisy_noise(const long long* rng, int N, int H, int A, float* f_in, float* f_out, uavgnn_stream_t stream) {
  if (!rng || N < 0 || H < 1 || A < 1 || H > kMaxCols || A > kMaxCols) return UAVGNN_EINVAL;
  if (N == 0 || (!f_in && !f_out)) return 0;
  const long long blocks = static_cast<long long>(N) * ((f_in ? (H + 3) / 4 : 0) + (f_out ? (A + 3) / 4 : 0));
  hipLaunchKernelGGL(noisy_noise_kernel, dim3(capped_grid(blocks, 256, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), rng, N, H,
                     A, f_in, f_out);
  return launch_status();
}

extern "C" int uavgnn_noisy_fold(const float* W_mu, const float* W_sigma, int ld_w, const float* b_mu, const float* b_sigma, int A, int H,
                                 const long long* rng, float* W_eff, float* b_eff, float* f_in, float* f_out, uavgnn_stream_t stream) {
  if (!W_mu || !W_sigma || !b_mu || !b_sigma || !rng || !W_eff || !b_eff || !f_in || !f_out || A < 1 || H < 1 || ld_w < H ||
      H > kMaxCols || A > kMaxCols)
    return UAVGNN_EINVAL;
  const long long items = static_cast<long long>(A) * ((H + 3) / 4);
  hipLaunchKernelGGL(noisy_fold_kernel, dim3(capped_grid(items, 256, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), W_mu, W_sigma,
                     ld_w, b_mu, b_sigma, A, H, rng, W_eff, b_eff, f_in, f_out);
  return launch_status();
}

extern "C" int uavgnn_noisy_fold_bwd(const float* dW_eff, int ld, const float* db_eff, const float* f_in, const float* f_out, int A, int H,
                                     float* dW_sigma, float* db_sigma, uavgnn_stream_t stream) {
  if (!dW_eff || !db_eff || !f_in || !f_out || !dW_sigma || !db_sigma || A < 1 || H < 1 || ld < H) return UAVGNN_EINVAL;
  hipLaunchKernelGGL(noisy_fold_bwd_kernel, dim3(capped_grid(static_cast<long long>(A) * H, 256, 4096)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), dW_eff, ld, db_eff, f_in, f_out, A, H, dW_sigma, db_sigma);
  return launch_status();
}

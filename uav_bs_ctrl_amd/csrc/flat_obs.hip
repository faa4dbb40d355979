// First encoder layer of the flattened-observation agents (exp2, o = 'mlp') read straight from the padded observations.
//
// The reference flattens every agent's observation dict with gym's `flatten` (FlattenedObservation, mubs_cov.py:70-74) and
// feeds it to Linear(F, H) + ReLU (rnn_agents.py:15-18, gnn_agents.py:62-77).  gym 0.21's Dict space sorts the keys of a
// plain dict, so the row is [agent (F_a) || gt (K_g = M Sg) || ubs (K_u = (n-1) 3)].  These kernels
// read the three padded tensors through base pointers and row strides; the [rows, F] concatenation is never written.
//
//   forward   y[r, o]  = ReLU(b[o] + sum_k W[o, k] x[r, k])                       one launch, rows x H_out outputs
//   wgrad     part[s, o, k] (+)= sum over the rows r of chunk s of dy[r, o] x[r, k]   the caller sums over s in a fixed order
//
// fp32 FMA throughout (exact products, fp32 accumulation, k / rows in a fixed order): two launches on the same inputs give the
// same bits, and a strided view gives the bits of its contiguous copy.  Rows of x and W are staged through LDS in slices of
// kKs columns, so F is bounded only by kMaxF.  Compiled without packed fp32 (build.py): the broadcast FMAs would otherwise be
// packed with operand selects (tools/isa_audit.py).
#include "common.h"

namespace uavgnn {
namespace {

constexpr int kThreads = 256;
constexpr int kKs = 32;        // K slice staged per step
constexpr int kRt = 32;        // rows per thread (forward) / rows per LDS stage (wgrad)
constexpr int kMaxF = 1024;    // 8 x 80 (F = 423) fits with room
constexpr int kMaxChunks = 512;
constexpr long long kMaxPartialFloats = 8ll << 20;

struct FlatSrc {
  const float* a;
  long long lda;
  int Fa;
  const float* g;
  long long ldg;
  int Kg;
  const float* u;
  long long ldu;
  int Ku;
};

// column k (< Fa + Kg + Ku) of row `row` of the flattened observation
__device__ __forceinline__ float flat_at(const FlatSrc& s, long long row, int k) {
  if (k < s.Fa) return s.a[row * s.lda + k];
  k -= s.Fa;
  if (k < s.Kg) return s.g[row * s.ldg + k];
  return s.u[row * s.ldu + (k - s.Kg)];
}

__device__ __forceinline__ float relu_keep_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

// grid: ceil(rows / (kRt G)), G = 256 / H row groups.  Thread (group, o) owns output column o of kRt consecutive rows.
template <int H>
__global__ __launch_bounds__(kThreads) void flat_obs_fwd_kernel(FlatSrc src, int F, int rows, const float* __restrict__ W,
                                                                const float* __restrict__ b, float* __restrict__ y, long long ldy) {
  constexpr int G = kThreads / H;
  constexpr int TR = kRt * G;
  __shared__ __attribute__((aligned(16))) float xs[kKs][TR + 4];
  __shared__ float ws[kKs][H];
  const int tid = threadIdx.x;
  const int o = tid % H, grp = tid / H;
  const long long r0 = static_cast<long long>(blockIdx.x) * TR;
  float acc[kRt];
#pragma unroll
  for (int j = 0; j < kRt; ++j) acc[j] = 0.f;
  for (int k0 = 0; k0 < F; k0 += kKs) {
    __syncthreads();
    for (int e = tid; e < TR * kKs; e += kThreads) {       // k fastest: a row's columns are consecutive in memory
      const int r = e / kKs, kk = e % kKs, k = k0 + kk;
      const long long row = r0 + r;
      xs[kk][r] = (row < rows && k < F) ? flat_at(src, row, k) : 0.f;
    }
    for (int e = tid; e < H * kKs; e += kThreads) {
      const int oo = e / kKs, kk = e % kKs, k = k0 + kk;
      ws[kk][oo] = k < F ? W[static_cast<long long>(oo) * F + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kKs; ++kk) {       // padded columns (k >= F) add 0 x 0
      const float w = ws[kk][o];
      const float4* xr = reinterpret_cast<const float4*>(&xs[kk][grp * kRt]);
#pragma unroll
      for (int q = 0; q < kRt / 4; ++q) {
        const float4 xv = xr[q];
        acc[4 * q + 0] = fmaf(w, xv.x, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(w, xv.y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(w, xv.z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(w, xv.w, acc[4 * q + 3]);
      }
    }
  }
  const float bo = b ? b[o] : 0.f;
#pragma unroll
  for (int j = 0; j < kRt; ++j) {
    const long long row = r0 + grp * kRt + j;
    if (row < rows) y[row * ldy + o] = relu_keep_nan(acc[j] + bo);
  }
}

// grid (S, ceil(F / kKs)).  Workgroup (s, slice) owns part[s, :, slice]: thread (group, o) holds kKs / G columns of row o of dW.
// The rows of chunk s are walked in kRt-row stages in increasing order (padded rows add 0 x 0).
template <int H>
__global__ __launch_bounds__(kThreads) void flat_obs_wgrad_kernel(FlatSrc src, int F, int rows, int rows_per_chunk,
                                                                  const float* __restrict__ dy, long long ldd,
                                                                  float* __restrict__ part, int accumulate) {
  constexpr int G = kThreads / H;
  constexpr int KT = kKs / G;
  __shared__ __attribute__((aligned(16))) float xs[kRt][kKs];
  __shared__ float ds[kRt][H];
  const int tid = threadIdx.x;
  const int o = tid % H, grp = tid / H;
  const int s = blockIdx.x, k0 = blockIdx.y * kKs;
  const long long lo = static_cast<long long>(s) * rows_per_chunk;
  const long long hi = min(static_cast<long long>(rows), lo + rows_per_chunk);
  float acc[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) acc[j] = 0.f;
  for (long long r0 = lo; r0 < hi; r0 += kRt) {
    __syncthreads();
    for (int e = tid; e < kRt * kKs; e += kThreads) {
      const int r = e / kKs, kk = e % kKs, k = k0 + kk;
      const long long row = r0 + r;
      xs[r][kk] = (row < hi && k < F) ? flat_at(src, row, k) : 0.f;
    }
    for (int e = tid; e < kRt * H; e += kThreads) {
      const int r = e / H, oo = e % H;
      const long long row = r0 + r;
      ds[r][oo] = row < hi ? dy[row * ldd + oo] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < kRt; ++r) {
      const float d = ds[r][o];
      const float4* xr = reinterpret_cast<const float4*>(&xs[r][grp * KT]);
#pragma unroll
      for (int q = 0; q < KT / 4; ++q) {
        const float4 xv = xr[q];
        acc[4 * q + 0] = fmaf(d, xv.x, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(d, xv.y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(d, xv.z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(d, xv.w, acc[4 * q + 3]);
      }
    }
  }
  float* p = part + (static_cast<long long>(s) * H + o) * F;
#pragma unroll
  for (int j = 0; j < KT; ++j) {
    const int k = k0 + grp * KT + j;
    if (k < F) p[k] = accumulate ? p[k] + acc[j] : acc[j];
  }
}

bool shape_ok(int H, int F) { return (H == 64 || H == 128 || H == 256) && F >= 1 && F <= kMaxF; }

int check_src(const FlatSrc& s, int rows) {
  if (s.Fa < 0 || s.Kg < 0 || s.Ku < 0) return UAVGNN_EINVAL;
  if (rows > 0 && ((s.Fa > 0 && (!s.a || s.lda < s.Fa)) || (s.Kg > 0 && (!s.g || s.ldg < s.Kg)) ||
                   (s.Ku > 0 && (!s.u || s.ldu < s.Ku))))
    return UAVGNN_EINVAL;
  return 0;
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_flat_obs_supported(int H_out, int F) { return shape_ok(H_out, F) ? 1 : 0; }

extern "C" int uavgnn_flat_obs_fwd(const float* agent, long long ld_a, int F_a, const float* gt, long long ld_g, int K_g,
                                   const float* ubs, long long ld_u, int K_u, int rows, const float* W, const float* b, int H_out,
                                   float* y, long long ld_y, uavgnn_stream_t stream) {
  const FlatSrc src{agent, ld_a, F_a, gt, ld_g, K_g, ubs, ld_u, K_u};
  const int F = F_a + K_g + K_u;
  if (rows < 0 || check_src(src, rows) || (rows > 0 && (!W || !y)) || ld_y < H_out) return UAVGNN_EINVAL;
  if (!shape_ok(H_out, F)) return UAVGNN_EUNSUPPORTED;
  if (rows == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tr = kRt * (kThreads / H_out);
  const dim3 grid((rows + tr - 1) / tr);
  switch (H_out) {
    case 64: hipLaunchKernelGGL(flat_obs_fwd_kernel<64>, grid, dim3(kThreads), 0, st, src, F, rows, W, b, y, ld_y); break;
    case 128: hipLaunchKernelGGL(flat_obs_fwd_kernel<128>, grid, dim3(kThreads), 0, st, src, F, rows, W, b, y, ld_y); break;
    default: hipLaunchKernelGGL(flat_obs_fwd_kernel<256>, grid, dim3(kThreads), 0, st, src, F, rows, W, b, y, ld_y); break;
  }
  return launch_status();
}

extern "C" int uavgnn_flat_obs_wgrad_chunks(long long rows, int H_out, int F) {
  if (rows < 1 || !shape_ok(H_out, F)) return 1;
  // >= 64 rows per chunk (16 384 rows: 256 chunks, one workgroup per CU per column slice), at most kMaxChunks chunks, and partials
  // [S, H_out, F] of at most kMaxPartialFloats (8 x 80, H_out = 256: 77 chunks x 14 column slices = 1 078 workgroups, 33 MB)
  long long s = (rows + 63) / 64;
  const long long cap = kMaxPartialFloats / (static_cast<long long>(H_out) * F);
  if (s > kMaxChunks) s = kMaxChunks;
  if (s > cap) s = cap;
  return static_cast<int>(s < 1 ? 1 : s);
}

extern "C" int uavgnn_flat_obs_wgrad(const float* dy, long long ld_dy, int H_out, const float* agent, long long ld_a, int F_a,
                                     const float* gt, long long ld_g, int K_g, const float* ubs, long long ld_u, int K_u, int rows,
                                     float* partials, int S, int accumulate, uavgnn_stream_t stream) {
  const FlatSrc src{agent, ld_a, F_a, gt, ld_g, K_g, ubs, ld_u, K_u};
  const int F = F_a + K_g + K_u;
  if (rows < 0 || S < 1 || !partials || check_src(src, rows) || (rows > 0 && !dy) || ld_dy < H_out) return UAVGNN_EINVAL;
  if (!shape_ok(H_out, F)) return UAVGNN_EUNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (rows == 0) {
    if (accumulate) return 0;
    return hipMemsetAsync(partials, 0, sizeof(float) * static_cast<size_t>(S) * H_out * F, st) == hipSuccess ? 0 : UAVGNN_EINVAL;
  }
  const int rpc = (rows + S - 1) / S;       // chunks past the last row write zeros
  const dim3 grid(S, (F + kKs - 1) / kKs);
  switch (H_out) {
    case 64:
      hipLaunchKernelGGL(flat_obs_wgrad_kernel<64>, grid, dim3(kThreads), 0, st, src, F, rows, rpc, dy, ld_dy, partials, accumulate);
      break;
    case 128:
      hipLaunchKernelGGL(flat_obs_wgrad_kernel<128>, grid, dim3(kThreads), 0, st, src, F, rows, rpc, dy, ld_dy, partials, accumulate);
      break;
    default:
      hipLaunchKernelGGL(flat_obs_wgrad_kernel<256>, grid, dim3(kThreads), 0, st, src, F, rows, rpc, dy, ld_dy, partials, accumulate);
      break;
  }
  return launch_status();
}

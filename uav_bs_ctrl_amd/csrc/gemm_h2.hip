// Dense layers on the f16 matrix cores with exactly scaled two-term splits ("f16x2", see csrc/gru_h2.hip): Y[M, N] = X[M, K] B[N, K]^T
// (+ bias) (+ Y) (ReLU), fp32 in / out / accumulate, THREE f16 x f16 MFMA products per fp32 product instead of bf16x3's six.
// Replaces the same products as csrc/gemm_x3.hip - the input-gradient halves of the recurrent step under loss.backward()
// (/root/reference/algos/madrqn/learner.py:157 through gnn_agents.py:246, :99): d x = [d_gi || d_proj] [W_ih[:, :H]; Wp[:, :H]],
// d h += d_gh W_hh, and d(K1 output) = d y W_aggr of the time-batched encoder - wherever the kernel that PRODUCED the activation
// operand also hands over its row maxima (the power-of-two row scales; a maximum is order-independent: deterministic):
//   * uavgnn_gru_gates_bwd_fused_sums_rowmax   max over the rows of d_gi and d_gh (one wavefront owns a row of H = 256),
//   * uavgnn_relu_bwd_colsum_rowmax            max over the rows of the masked gradient (one wavefront owns a row of C = 256),
//   * uavgnn_row_absmax                        anything else, as a pass of its own (d_proj: 96 columns).
// Up to two bounds per row (two producers of a two-source operand); the row's scale comes from their maximum.
//
// Arithmetic, error and non-finite behaviour: csrc/gru_h2.hip's header (the shared device helpers: csrc/f16x2.h).  B (the weight,
// [N, K] or its transpose) is split per OUTPUT row by uavgnn_split_h2: f16 planes [2][N][K] + 2^-e per row.
//
// Kernel: gemm_x3.hip's eight-wave kernel (256 x 128 output tile, waves of 64 x 64 = 2 x 2 tiles of v_mfma_f32_32x32x16_f16, LDS
// double-buffered with ONE barrier per 32-wide K slice, two-source X loader) with two planes: 48 KB per LDS stage instead of 72, 24
// MFMAs per slice and wavefront instead of 48.
#include "common.h"
#include "f16x2.h"

namespace uavgnn {
namespace {

using namespace h2;

constexpr int BN = 128, BK = 32, BM8 = 256, NT = 512;
constexpr int PA = BM8 * 4, PB = BN * 4;               // 16-byte chunks per split plane of the X / B tile
constexpr int BUF = 2 * PA + 2 * PB;                   // chunks per buffer (48 KB)

// The epilogue's ReLU.  fmaxf(NaN, 0) is 0: the plain maximum turned every output of a row that holds Inf / NaN, or whose bound is too
// small, into 0 - a plausible number, against the contract of gru_h2.hip's header (tests/test_f16x2_nt_edges_gpu.py::test_contract_rows).
// A NaN passes; every number gets fmaxf's bits.
__device__ __forceinline__ float relu_keep_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

// W [R, C] (row stride ld) -> planes [2][R][C] (transpose: [2][C][R]) + winv[rows of the output] = 2^-e: one workgroup per output row
__global__ __launch_bounds__(256) void split_h2_kernel(const float* __restrict__ W, int ld, int R, int C, int transpose,
                                                       unsigned short* __restrict__ planes, float* __restrict__ winv) {
  __shared__ float red[4];
  const int orow = blockIdx.x, tid = threadIdx.x;
  const int ocol_n = transpose ? R : C;
  const size_t n = static_cast<size_t>(transpose ? C : R) * ocol_n;
  auto at = [&](int j) { return transpose ? W[static_cast<size_t>(j) * ld + orow] : W[static_cast<size_t>(orow) * ld + j]; };
  float m = 0.f;
  for (int j = tid; j < ocol_n; j += 256) m = fmaxf(m, fabsf(at(j)));
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const int se = scale_exp(m);
  const float s = pow2f(se);
  for (int j = 2 * tid; j < ocol_n; j += 512) {
    const Split2 sp = split_pair(at(j), at(j + 1), s);
    *reinterpret_cast<unsigned*>(planes + static_cast<size_t>(orow) * ocol_n + j) = sp.hi;
    *reinterpret_cast<unsigned*>(planes + n + static_cast<size_t>(orow) * ocol_n + j) = sp.lo;
  }
  if (tid == 0) winv[orow] = pow2f(-se);
}

template <bool ACC, bool RELU, bool IL>
__global__ __launch_bounds__(NT) void gemm_nt_h2w8_kernel(const float* __restrict__ X, int ldx, int M, int K,
                                                          const unsigned short* __restrict__ Bp, int N, const float* __restrict__ winv,
                                                          const float* __restrict__ bias, float* __restrict__ Y, int ldy,
                                                          int row_blocks, int col_blocks, const float* __restrict__ X2, int ldx2,
                                                          int ns1, const float* __restrict__ rm1, const float* __restrict__ rm2,
                                                          float* __restrict__ rm2_out) {
  // buffer b: X planes [2][256][4] then B planes [2][128][4]; the accumulating instantiations park the 256 x 128 output tile here (132 KB)
  constexpr int kTileChunks = BM8 * (BN + 4) / 4;
#ifndef UAVGNN_GEMM_H2_TILE_STORE
#define UAVGNN_GEMM_H2_TILE_STORE 1   /* 0: the non-accumulating instantiations store straight from the D layout (64 dword stores per lane) */
#endif
  constexpr bool kTileStore = ACC || UAVGNN_GEMM_H2_TILE_STORE;
  __shared__ u32x4 smem[(kTileStore && kTileChunks > 2 * BUF) ? kTileChunks : 2 * BUF];
  __shared__ float sInv[BM8];       // 2^-e of the block's rows
  __shared__ float sRow2[BM8];      // rm2_out: the row maxima of X2 this workgroup computed itself
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, lh = lane >> 5, sw = swz32(l32);
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int rb = (slot / col_blocks) * 8 + xcd, cb = slot - (slot / col_blocks) * col_blocks;
  if (rb >= row_blocks) return;
  const int m0 = rb * BM8, n0 = cb * BN;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  // X loader: float4 q = tid + 512 i (i < 4) -> row tid / 8 + 64 i, k = 4 (tid % 8)
  const int lr = tid >> 3, c4 = tid & 7;
  unsigned xo[4], xo2[4];
  float sca[4];
  auto bound = [&](int row) {   // the row's bound: the larger of the (up to two) producers'
    const float a = rm1[row];
    return rm2 != nullptr ? fmaxf(a, rm2[row]) : a;
  };
  const bool own2 = rm2_out != nullptr;   // the second source has no producer that bounds it: this launch takes its row maxima itself
  float m2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = min(m0 + lr + 64 * i, M - 1);
    xo[i] = static_cast<unsigned>(row) * ldx + 4 * c4;
    xo2[i] = static_cast<unsigned>(row) * ldx2 + 4 * c4;
  }
  if (own2) {
    // the eight threads of a row (consecutive lanes) read its K - K1 columns as float4 c4, c4 + 8, ...: 96 columns = three per thread and
    // row, requested with the first slices of X; Inf / NaN make the bound infinite (the contract of uavgnn_row_absmax).  Every column
    // block computes the same maxima (a maximum is order-independent: bit-identical); column block 0 writes them out.
    const int nq = (K - ns1 * BK) / 4;
    bool bad[4] = {false, false, false, false};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      for (int q = c4; q < nq; q += 8) {
        const float4 v = *reinterpret_cast<const float4*>(X2 + xo2[i] + 4 * (q - c4));
        const float a0 = fabsf(v.x), a1 = fabsf(v.y), a2 = fabsf(v.z), a3 = fabsf(v.w);
        bad[i] |= !(a0 <= 3.4028234663852886e38f) | !(a1 <= 3.4028234663852886e38f) | !(a2 <= 3.4028234663852886e38f) |
                  !(a3 <= 3.4028234663852886e38f);
        m2[i] = fmaxf(fmaxf(m2[i], fmaxf(a0, a1)), fmaxf(a2, a3));
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (bad[i]) m2[i] = INFINITY;
      m2[i] = fmaxf(m2[i], __shfl_xor(m2[i], 1));
      m2[i] = fmaxf(m2[i], __shfl_xor(m2[i], 2));
      m2[i] = fmaxf(m2[i], __shfl_xor(m2[i], 4));
      if (c4 == 0) {
        sRow2[lr + 64 * i] = m2[i];
        if (cb == 0 && m0 + lr + 64 * i < M) rm2_out[m0 + lr + 64 * i] = m2[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = min(m0 + lr + 64 * i, M - 1);
    sca[i] = pow2f(scale_exp(own2 ? fmaxf(rm1[row], m2[i]) : bound(row)));
  }
  if (!own2 && tid < BM8) sInv[tid] = pow2f(-scale_exp(bound(min(m0 + tid, M - 1))));
  const int sa_w = lr * 32 + (((c4 >> 1) ^ swz32(lr)) * 8) + (c4 & 1) * 4;   // f16 units inside an X plane
  // B loader: chunk q = tid + 512 i (i < 2): plane i, row tid / 4, chunk tid % 4
  unsigned bo[2];
  int sbw[2];
  const unsigned plane = static_cast<unsigned>(N) * K;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = tid >> 2, c = tid & 3;
    bo[i] = i * plane + static_cast<unsigned>(min(n0 + row, N - 1)) * K + 8 * c;
    sbw[i] = 2 * PA + i * PB + row * 4 + (c ^ swz32(row));
  }
  const int ns = K / BK;
  float4 ra[4];
  u32x4 rw[2];
  auto gload_a = [&](int t) {
    const bool second = t >= ns1;                                  // wave-uniform
    const float* __restrict__ src = second ? X2 : X;
    const unsigned k0 = static_cast<unsigned>(second ? t - ns1 : t) * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const float4*>(src + ((second ? xo2[i] : xo[i]) + k0));
  };
  auto gload_w = [&](int t) {
    const unsigned k0 = static_cast<unsigned>(t) * BK;
#pragma unroll
    for (int i = 0; i < 2; ++i) rw[i] = *reinterpret_cast<const u32x4*>(Bp + (bo[i] + k0));
  };
  auto gload = [&](int t) {
    gload_a(t);
    gload_w(t);
  };
  auto lstore_a = [&](int buf, int i) {
    unsigned short* sa = reinterpret_cast<unsigned short*>(smem + buf * BUF) + sa_w;
    stage4(sa + 64 * i * 32, PA * 8, ra[i], sca[i]);
  };
  auto lstore_a_planes = [&](int buf, int i, u32x2 hi, u32x2 lo) {   // stage4's two stores, for the loop that places the split's steps itself
    unsigned short* sa = reinterpret_cast<unsigned short*>(smem + buf * BUF) + sa_w + 64 * i * 32;
    *reinterpret_cast<u32x2*>(sa) = hi;
    *reinterpret_cast<u32x2*>(sa + PA * 8) = lo;
  };
  auto lstore_b = [&](int buf) {
    u32x4* sb = smem + buf * BUF;
#pragma unroll
    for (int i = 0; i < 2; ++i) sb[sbw[i]] = rw[i];
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) lstore_a(buf, i);
    lstore_b(buf);
  };
  struct Half {
    f16x8 a[2][2], b[2][2];   // [tile][plane]
  };
#define UAVGNN_H2_READ(F, buf, kh)                                                                                 \
  {                                                                                                                \
    const u32x4* sb = smem + (buf) * BUF;                                                                          \
    _Pragma("unroll") for (int a = 0; a < 2; ++a) _Pragma("unroll") for (int pl = 0; pl < 2; ++pl) {               \
      F.a[a][pl] = as_frag(sb[pl * PA + (wm + a * 32 + l32) * 4 + ((2 * (kh) + lh) ^ sw)]);                        \
      F.b[a][pl] = as_frag(sb[2 * PA + pl * PB + (wn + a * 32 + l32) * 4 + ((2 * (kh) + lh) ^ sw)]);               \
    }                                                                                                              \
  }
#define UAVGNN_H2_TERM(ia, ib)                                                                      \
  _Pragma("unroll") for (int a = 0; a < 2; ++a) _Pragma("unroll") for (int b = 0; b < 2; ++b)      \
      acc[a][b] = mfma32(F.a[a][ia], F.b[b][ib], acc[a][b]);
#define UAVGNN_H2_MFMA(F_)                                            \
  {                                                                   \
    const Half& F = F_;                                               \
    UAVGNN_H2_TERM(0, 1) UAVGNN_H2_TERM(1, 0) UAVGNN_H2_TERM(0, 0)    \
  }
  gload(0);
  lstore(0);
  gload(min(1, ns - 1));
  __syncthreads();
  if (own2 && tid < BM8) sInv[tid] = pow2f(-scale_exp(fmaxf(rm1[min(m0 + tid, M - 1)], sRow2[tid])));   // (read behind the loop's barriers)
  const bool early = wave < 4;
  Half f0, f1;
  UAVGNN_H2_READ(f0, 0, 0)
  if (IL) {
    for (int t = 0; t < ns; ++t) {
      UAVGNN_H2_READ(f1, t & 1, 1)
      __builtin_amdgcn_sched_barrier(0);
      const Half& F = f0;
      const int tn = min(t + 2, ns - 1);
      lstore_b((t + 1) & 1);
      gload_w(tn);
      UAVGNN_H2_TERM(0, 1)
#pragma unroll
      for (int sg = 0; sg < 4; ++sg) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      // The split steps are asm, which the scheduler's instruction groups do not see: the eight MFMAs of the two remaining terms take
      // one step each (four single-pass instructions in a 32-cycle gap), row i's stores ride with the next row's first step, and each
      // MFMA with its share is a region of its own.  The loads of slice t + 2 follow the last step, which frees their registers.
      u32x2 sh[4], sl[4];
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const int i = g >> 1;
        if (g < 4) acc[g >> 1][g & 1] = mfma32(F.a[g >> 1][1], F.b[g & 1][0], acc[g >> 1][g & 1]);
        else acc[(g - 4) >> 1][g & 1] = mfma32(F.a[(g - 4) >> 1][0], F.b[g & 1][0], acc[(g - 4) >> 1][g & 1]);
        if ((g & 1) == 0) {
          if (i > 0) lstore_a_planes((t + 1) & 1, i - 1, sh[i - 1], sl[i - 1]);
          sh[i] = split4_hi(ra[i], scale4(sca[i]));
        } else {
          sl[i] = split4_lo(ra[i], scale4(sca[i]), sh[i]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      lstore_a_planes((t + 1) & 1, 3, sh[3], sl[3]);
      gload_a(tn);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
      UAVGNN_H2_READ(f0, (t + 1) & 1, 0)
      __builtin_amdgcn_sched_barrier(0);
      UAVGNN_H2_MFMA(f1)
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    for (int t = 0; t < ns; ++t) {
      UAVGNN_H2_READ(f1, t & 1, 1)
      if (early) {
        lstore((t + 1) & 1);                 // slice t + 1 (the tail re-stages the last slice: unconditional, straight-line)
        gload(min(t + 2, ns - 1));
      }
      __builtin_amdgcn_sched_barrier(0);
      UAVGNN_H2_MFMA(f0)
      __builtin_amdgcn_sched_barrier(0);
      if (!early) {
        lstore((t + 1) & 1);
        gload(min(t + 2, ns - 1));
      }
      __syncthreads();
      UAVGNN_H2_READ(f0, (t + 1) & 1, 0)
      __builtin_amdgcn_sched_barrier(0);
      UAVGNN_H2_MFMA(f1)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef UAVGNN_H2_MFMA
#undef UAVGNN_H2_TERM
#undef UAVGNN_H2_READ
  // un-scaling: two exact power-of-two factors per element (2^-e_col first: weights are small, it cannot overflow; then 2^-e_row)
  if constexpr (kTileStore) {
  if ((ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0 && n0 + BN <= N) {
    // Y (+)= product through an LDS tile (see gemm_x3.hip: row-contiguous float4 accesses - 16 per lane instead of 64 dword stores
    // straight from the D layout; accumulating: a read-modify-write with one exposed round trip per tile)
    constexpr int LDT = BN + 4;
    float* sT = reinterpret_cast<float*>(smem);           // [256][LDT] fp32
    static_assert(BM8 * LDT * 4 <= static_cast<int>(sizeof(smem)), "the output tile fits the LDS array");
    __syncthreads();                                     // the last fragment reads of the stale buffer
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = n0 + wn + b * 32 + l32;
        const float bv = bias != nullptr ? bias[col] : 0.f, ci = winv[col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int lrow = wm + a * 32 + 8 * (i >> 2) + 4 * lh + (i & 3);
          sT[lrow * LDT + wn + b * 32 + l32] = acc[a][b][i] * ci * sInv[lrow] + bv;
        }
      }
    float4 yv[16];
    if constexpr (ACC) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int idx = tid + NT * q, row = idx >> 5, cc = idx & 31;
        yv[q] = *reinterpret_cast<const float4*>(Y + static_cast<size_t>(min(m0 + row, M - 1)) * ldy + n0 + 4 * cc);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int idx = tid + NT * q, row = idx >> 5, cc = idx & 31;
      const float4 t = *reinterpret_cast<const float4*>(sT + row * LDT + 4 * cc);
      float4 o = t;
      if constexpr (ACC) o = {yv[q].x + t.x, yv[q].y + t.y, yv[q].z + t.z, yv[q].w + t.w};
      if (RELU) o = {relu_keep_nan(o.x), relu_keep_nan(o.y), relu_keep_nan(o.z), relu_keep_nan(o.w)};
      if (m0 + row < M) *reinterpret_cast<float4*>(Y + static_cast<size_t>(m0 + row) * ldy + n0 + 4 * cc) = o;
    }
    return;
  }
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int col = n0 + wn + b * 32 + l32;
    if (col >= N) continue;
    const float bv = bias != nullptr ? bias[col] : 0.f, ci = winv[col];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int lrow = wm + a * 32 + 8 * (i >> 2) + 4 * lh + (i & 3);
        const int row = m0 + lrow;
        if (row < M) {
          float* p = Y + static_cast<size_t>(row) * ldy + col;
          float v = acc[a][b][i] * ci * sInv[lrow] + bv;
          if (ACC) v += *p;
          if (RELU) v = relu_keep_nan(v);
          *p = v;
        }
      }
  }
}

// ---- 128 x 64 output tiles: products with 64 output columns (d c = d_gi W_ih[:, H:] of the recurrent step, [N, 768] x [768, 64]) --------
// The 256 x 128-tile kernel above would run such a product on N / 256 workgroups with half of every tile empty.  Here eight wavefronts of
// 32 x 32 (ONE v_mfma_f32_32x32x16_f16 tile each: 4 x 2 over the 128 x 64 tile) share the same staging layout (swizzle, planes) and the
// same three-term arithmetic in the same order over K; N = 32 768 rows are 256 workgroups, one round of the CUs.  The kernel is bound by
// streaming X once (9.7 GFLOP against 100 MB at the step's shape) with ONE workgroup per CU, so what counts is the bytes a CU keeps in
// flight: a stage holds TWO 32-wide K slices (two sub-buffers in the layout above, one barrier per 64 columns of K) and the loads of
// the next stage - 4 float4 of X and 2 chunks of B per thread, 48 KB per CU - are in flight across a whole stage of MFMAs.  (A register
// ring that ran three 32-wide slices ahead was tried first: rolled, the compiler drains every outstanding load at the loop's back edge;
// unrolled, it re-schedules the loads next to their uses - either way one slice, 24 KB, in flight: 35.5 us against the vendor's 33.3.)
constexpr int BM6 = 128, BN6 = 64;
constexpr int PA6 = BM6 * 4, PB6 = BN6 * 4;            // 16-byte chunks per split plane of the X / B tile of ONE 32-wide slice
constexpr int SUB6 = 2 * PA6 + 2 * PB6;                // chunks per slice (24 KB)
constexpr int BUF6 = 2 * SUB6;                         // chunks per stage: two slices (48 KB)

__global__ __launch_bounds__(NT) void gemm_nt_h2n64_kernel(const float* __restrict__ X, int ldx, int M, int K,
                                                           const unsigned short* __restrict__ Bp, int N, const float* __restrict__ winv,
                                                           float* __restrict__ Y, int ldy, int col_blocks, const float* __restrict__ rm1) {
  constexpr int LDT = BN6 + 4;
  static_assert(BM6 * LDT * 4 <= 2 * BUF6 * 16, "the output tile fits the staging buffers");
  __shared__ u32x4 smem[2 * BUF6];
  __shared__ float sInv[BM6];       // 2^-e of the block's rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, lh = lane >> 5, sw = swz32(l32);
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int rb = blockIdx.x / col_blocks, cb = blockIdx.x - rb * col_blocks;
  const int m0 = rb * BM6, n0 = cb * BN6;

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  // X loader, per slice: float4 q = tid + 512 i (i < 2) -> row tid / 8 + 64 i, k = 4 (tid % 8); rows past M: clamped loads, masked stores
  const int lr = tid >> 3, c4 = tid & 7;
  unsigned xo[2];
  float sca[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = min(m0 + lr + 64 * i, M - 1);
    xo[i] = static_cast<unsigned>(row) * ldx + 4 * c4;
    sca[i] = pow2f(scale_exp(rm1[row]));
  }
  if (tid < BM6) sInv[tid] = pow2f(-scale_exp(rm1[min(m0 + tid, M - 1)]));
  const int sa_w = lr * 32 + (((c4 >> 1) ^ swz32(lr)) * 8) + (c4 & 1) * 4;   // f16 units inside an X plane
  // B loader, per slice: ONE chunk per thread: plane tid / 256, row (tid / 4) % 64, chunk tid % 4 (N % 64 == 0: every row exists)
  const int bpl = tid >> 8, brow = (tid >> 2) & 63, bc = tid & 3;
  const unsigned bo = bpl * (static_cast<unsigned>(N) * K) + static_cast<unsigned>(n0 + brow) * K + 8 * bc;
  const int sbw = 2 * PA6 + bpl * PB6 + brow * 4 + (bc ^ swz32(brow));
  const int ns = K / (2 * BK);      // stages (K % 64 == 0)
  float4 ra[2][2];                  // [slice of the stage][i]
  u32x4 rw[2];
  auto gload = [&](int t) {
    const unsigned k0 = static_cast<unsigned>(min(t, ns - 1)) * (2 * BK);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < 2; ++i) ra[s][i] = *reinterpret_cast<const float4*>(X + (xo[i] + k0 + s * BK));
      rw[s] = *reinterpret_cast<const u32x4*>(Bp + (bo + k0 + s * BK));
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4* sb = smem + buf * BUF6 + s * SUB6;
      unsigned short* sa = reinterpret_cast<unsigned short*>(sb) + sa_w;
#pragma unroll
      for (int i = 0; i < 2; ++i) stage4(sa + 64 * i * 32, PA6 * 8, ra[s][i], sca[i]);
      sb[sbw] = rw[s];
    }
  };
  struct Half {
    f16x8 a[2], b[2];   // [plane]
  };
#define UAVGNN_N64_READ(F, buf, s, kh)                                                                     \
  {                                                                                                        \
    const u32x4* sb = smem + (buf) * BUF6 + (s) * SUB6;                                                    \
    _Pragma("unroll") for (int pl = 0; pl < 2; ++pl) {                                                     \
      F.a[pl] = as_frag(sb[pl * PA6 + (wm + l32) * 4 + ((2 * (kh) + lh) ^ sw)]);                           \
      F.b[pl] = as_frag(sb[2 * PA6 + pl * PB6 + (wn + l32) * 4 + ((2 * (kh) + lh) ^ sw)]);                 \
    }                                                                                                      \
  }
#define UAVGNN_N64_MFMA(F)                 \
  {                                        \
    acc = mfma32(F.a[0], F.b[1], acc);     \
    acc = mfma32(F.a[1], F.b[0], acc);     \
    acc = mfma32(F.a[0], F.b[0], acc);     \
  }
  gload(0);
  lstore(0);
  gload(1);
  __syncthreads();
  Half f0, f1, f2, f3;
  UAVGNN_N64_READ(f0, 0, 0, 0)
  for (int t = 0; t < ns; ++t) {
    const int cur = t & 1;
    UAVGNN_N64_READ(f1, cur, 0, 1)
    lstore(cur ^ 1);                       // stage t + 1 (the tail re-stages the last stage: unconditional, straight-line)
    gload(t + 2);
    __builtin_amdgcn_sched_barrier(0);
    UAVGNN_N64_MFMA(f0)
    UAVGNN_N64_READ(f2, cur, 1, 0)
    UAVGNN_N64_MFMA(f1)
    UAVGNN_N64_READ(f3, cur, 1, 1)
    UAVGNN_N64_MFMA(f2)
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    UAVGNN_N64_READ(f0, cur ^ 1, 0, 0)
    __builtin_amdgcn_sched_barrier(0);
    UAVGNN_N64_MFMA(f3)
    __builtin_amdgcn_sched_barrier(0);
  }
#undef UAVGNN_N64_MFMA
#undef UAVGNN_N64_READ
  // un-scaling as above (2^-e_col, then 2^-e_row), then Y through an LDS tile: row-contiguous float4 stores
  float* sT = reinterpret_cast<float*>(smem);             // [128][LDT] fp32
  __syncthreads();                                       // the last fragment reads of the stale buffer
  {
    const float ci = winv[n0 + wn + l32];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int lrow = wm + 8 * (i >> 2) + 4 * lh + (i & 3);
      sT[lrow * LDT + wn + l32] = acc[i] * ci * sInv[lrow];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = tid + NT * q, row = idx >> 4, cc = idx & 15;
    if (m0 + row < M)
      *reinterpret_cast<float4*>(Y + static_cast<size_t>(m0 + row) * ldy + n0 + 4 * cc) =
          *reinterpret_cast<const float4*>(sT + row * LDT + 4 * cc);
  }
}

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_gemm_h2_supported(int M, int N, int K) {
  // 32-bit element offsets inside the kernel: every operand below 2^31 elements
  return (M > 0 && N > 0 && K >= BK && K % BK == 0 && static_cast<long long>(M) * K < (1LL << 31) &&
          2LL * N * K < (1LL << 31)) ? 1 : 0;
}

// bytes of the `planes` of a weight with `n_out` output rows and contraction length K: [2][n_out][K] f16 + n_out floats
extern "C" long long uavgnn_split_h2_bytes(int n_out, int K) {
  if (n_out <= 0 || K <= 0) return 0;
  return 4LL * n_out * K + 4LL * n_out;
}

// W [R, C] (row stride ld): transpose = 0 -> B = W (n_out = R, K = C: y = x W^T); transpose = 1 -> B = W^T (n_out = C, K = R: dx = dy W)
extern "C" int uavgnn_split_h2(const float* W, int ld, int R, int C, int transpose, void* planes, uavgnn_stream_t stream) {
  if (!W || !planes || R <= 0 || C <= 0 || ld < C) return UAVGNN_EINVAL;
  const int n_out = transpose ? C : R, K = transpose ? R : C;
  if ((K & 1) || (reinterpret_cast<uintptr_t>(planes) & 15)) return UAVGNN_EUNSUPPORTED;
  unsigned short* p = static_cast<unsigned short*>(planes);
  float* winv = reinterpret_cast<float*>(p + 2LL * n_out * K);
  hipLaunchKernelGGL(split_h2_kernel, dim3(n_out), dim3(256), 0, static_cast<hipStream_t>(stream), W, ld, R, C, transpose, p, winv);
  return launch_status();
}

// Y = [X (K1 columns) || X2 (K - K1 columns; NULL: one source, K1 = K)] B^T (+ bias) (+ Y) (ReLU) on the f16x2 arithmetic.
// rowmax / rowmax2 (the second may be NULL): per row of the activation operand an upper bound of max |.| over the row - the larger of
// the two is used - tight to within its power of two, from the kernels that produced the operand.  epilogue: UAVGNN_GEMM_ACCUMULATE,
// UAVGNN_GEMM_RELU, UAVGNN_GEMM_STAGING_INTERLEAVED of uavgnn_gemm_nt_x3.  The eight-wave kernel only (no tile variants).
static int gemm_nt_h2_launch(const float* X, int ldx, int K1, const float* X2, int ldx2, int M, int K, const float* rowmax,
                             const float* rowmax2, float* rowmax2_out, const void* planes, int N, const float* bias, float* Y, int ldy,
                             int epilogue, uavgnn_stream_t stream) {
  if (M < 0 || !X || !planes || !Y || !rowmax || ldx < K1 || ldy < N || K1 <= 0 || K1 > K || (X2 == nullptr) != (K1 == K) ||
      (X2 != nullptr && ldx2 < K - K1) || (rowmax2_out != nullptr && (X2 == nullptr || rowmax2 != nullptr)))
    return UAVGNN_EINVAL;
  if (M == 0) return 0;
  if (!uavgnn_gemm_h2_supported(M, N, K) || (ldx & 3) || static_cast<long long>(M) * ldx >= (1LL << 31) ||
      ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(planes)) & 15) ||
      (epilogue & (UAVGNN_GEMM_TILE_128 | UAVGNN_GEMM_TILE_64)))
    return UAVGNN_EUNSUPPORTED;
  if (X2 != nullptr && ((K1 % BK) || (ldx2 & 3) || static_cast<long long>(M) * ldx2 >= (1LL << 31) || (reinterpret_cast<uintptr_t>(X2) & 15)))
    return UAVGNN_EUNSUPPORTED;
  const int ns1 = K1 / BK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned short* bp = static_cast<const unsigned short*>(planes);
  const float* winv = reinterpret_cast<const float*>(bp + 2LL * N * K);
  const bool acc = (epilogue & UAVGNN_GEMM_ACCUMULATE) != 0, relu = (epilogue & UAVGNN_GEMM_RELU) != 0;
  const int col_blocks = (N + BN - 1) / BN, row_blocks = (M + BM8 - 1) / BM8;
  const dim3 grid(((row_blocks + 7) / 8) * 8 * col_blocks), block(NT);
#define UAVGNN_H2_GEMM(ACC, RELU, IL)                                                                                              \
  hipLaunchKernelGGL((gemm_nt_h2w8_kernel<ACC, RELU, IL>), grid, block, 0, st, X, ldx, M, K, bp, N, winv, bias, Y, ldy, row_blocks, \
                     col_blocks, X2, ldx2, ns1, rowmax, rowmax2, rowmax2_out)
#define UAVGNN_H2_GEMM_IL(IL)                         \
  if (acc && relu) UAVGNN_H2_GEMM(true, true, IL);    \
  else if (acc) UAVGNN_H2_GEMM(true, false, IL);      \
  else if (relu) UAVGNN_H2_GEMM(false, true, IL);     \
  else UAVGNN_H2_GEMM(false, false, IL);
  if (epilogue & UAVGNN_GEMM_STAGING_INTERLEAVED) { UAVGNN_H2_GEMM_IL(true) }
  else { UAVGNN_H2_GEMM_IL(false) }
#undef UAVGNN_H2_GEMM_IL
#undef UAVGNN_H2_GEMM
  return launch_status();
}

extern "C" int uavgnn_gemm_nt_h2(const float* X, int ldx, int K1, const float* X2, int ldx2, int M, int K, const float* rowmax,
                                 const float* rowmax2, const void* planes, int N, const float* bias, float* Y, int ldy, int epilogue,
                                 uavgnn_stream_t stream) {
  return gemm_nt_h2_launch(X, ldx, K1, X2, ldx2, M, K, rowmax, rowmax2, nullptr, planes, N, bias, Y, ldy, epilogue, stream);
}

// ... for a second source WITHOUT a producer that bounds its rows: the launch takes the row maxima of X2 [M, K - K1] itself (its workgroups
// read their 256 rows of X2 once more in front of the first slice - 96 columns at the recurrent step: a microsecond against the 8-us pass of
// uavgnn_row_absmax) and writes them to rowmax2_out [M] (Inf for a row that holds Inf / NaN; what uavgnn_row_absmax(X2) returns, bit for bit).
extern "C" int uavgnn_gemm_nt_h2_rm2(const float* X, int ldx, int K1, const float* X2, int ldx2, int M, int K, const float* rowmax,
                                     float* rowmax2_out, const void* planes, int N, const float* bias, float* Y, int ldy, int epilogue,
                                     uavgnn_stream_t stream) {
  if (!rowmax2_out) return UAVGNN_EINVAL;
  return gemm_nt_h2_launch(X, ldx, K1, X2, ldx2, M, K, rowmax, nullptr, rowmax2_out, planes, N, bias, Y, ldy, epilogue, stream);
}

// Y [M, N] = X [M, K] B^T on 128 x 64 output tiles (products with few output columns: d c of the recurrent step).  One source, no bias,
// no accumulation, no ReLU; N % 64 == 0, K % 64 == 0, ldy % 4 == 0, Y 16-byte aligned (rows leave through float4 stores); otherwise the operands and
// the arithmetic of uavgnn_gemm_nt_h2 - the accumulation order over K is the same, so a column computed here equals that kernel's.
extern "C" int uavgnn_gemm_nt_h2_n64(const float* X, int ldx, int M, int K, const float* rowmax, const void* planes, int N, float* Y,
                                     int ldy, uavgnn_stream_t stream) {
  if (M < 0 || !X || !planes || !Y || !rowmax || K <= 0 || N <= 0 || ldx < K || ldy < N) return UAVGNN_EINVAL;
  if (M == 0) return 0;
  if (!uavgnn_gemm_h2_supported(M, N, K) || (N % BN6) || (K % (2 * BK)) || (ldx & 3) || (ldy & 3) || static_cast<long long>(M) * ldx >= (1LL << 31) ||
      ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(Y)) & 15))
    return UAVGNN_EUNSUPPORTED;
  const unsigned short* bp = static_cast<const unsigned short*>(planes);
  const float* winv = reinterpret_cast<const float*>(bp + 2LL * N * K);
  const int col_blocks = N / BN6, row_blocks = (M + BM6 - 1) / BM6;
  hipLaunchKernelGGL(gemm_nt_h2n64_kernel, dim3(row_blocks * col_blocks), dim3(NT), 0, static_cast<hipStream_t>(stream), X, ldx, M, K, bp,
                     N, winv, Y, ldy, col_blocks, rowmax);
  return launch_status();
}

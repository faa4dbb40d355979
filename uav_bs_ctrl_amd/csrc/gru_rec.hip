// The recurrent half of the GRU cell for FEW rows (tens to hundreds: the reference's own operating point, 32 sequences x 1 or 8 agents,
// algos/drqn/config.py / algos/madrqn/config.py) - what is left of nn.GRUCell once the input projection gi = x W_ih^T + b_ih has been
// taken out of the time loop (it does not depend on h, so a no-communication agent computes it for all T + 1 steps in one GEMM):
//
//   forward   gh = h W_hh^T + b_hh, r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h
//   backward  the gate gradients from the saved [N, 4H] pre-activation set (the layout of uavgnn_gru_cell_fwd) and
//             dh_prev = dh z + d_gh W_hh                       - uavgnn_gru_gates_bwd_fused + a vendor GEMM in one launch
//
// Both kernels are parallel over (16-row tile) x (16 hidden columns): 32 rows x H = 256 are 32 workgroups with no communication
// between them.  A workgroup's four wavefronts split the contraction into 16-wide slices (wavefront w takes slices w, w + 4, ...),
// each accumulates exact fp32 products in fp32 on v_mfma_f32_16x16x4_f32 in a fixed order (the operand maps of csrc/head.hip: lane
// (i, g) feeds the four components of one float4 to four MFMAs as K slot g), and the four partial tiles are added through LDS in the
// order ((0 + 1) + (2 + 3)): bit-reproducible from launch to launch.  Row i of an output tile depends on row i of the A operand only,
// so a NaN row stays in its row.  The sigmoid / tanh are csrc/gru_fused.hip's (the accurate forms), so the backward kernel recomputes
// exactly the gate values the forward kernel applied.
//
// The backward kernel recomputes the gate gradients of its WHOLE row tile (16 x 3H values, 48 KB of LDS at H = 256) in every one of
// its H / 16 column-block workgroups - the contraction of dh_prev runs over all 3H columns of d_gh - and writes its own column block
// of d_gi / d_gh.  That is 16 x the pointwise work of the gate kernel on a few thousand elements, against one launch and one [N, 3H]
// round trip through HBM saved.
#include "common.h"

namespace uavgnn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRecMaxH = 256;
constexpr int kRecTile = 16;                       // rows per tile = hidden columns per block

__device__ __forceinline__ float rec_sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// NSW: 16-wide contraction slices per wavefront (H / 64 rounded up)
template <int NSW, bool SAVE>
__global__ __launch_bounds__(256) void gru_rec_fwd_kernel(const float* __restrict__ gi, int ld_gi, const float* __restrict__ h, int ld_h,
                                                          int N, int H, const float* __restrict__ W_hh, const float* __restrict__ b_hh,
                                                          float* __restrict__ h_out, int ld_ho, float* __restrict__ pre) {
  __shared__ float sP[4][3][kRecTile * kRecTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.x * kRecTile, c0 = blockIdx.y * kRecTile;
  const int ns = H / 16;
  const float* __restrict__ hr = h + static_cast<size_t>(min(row0 + j, N - 1)) * ld_h + 4 * g;
  const float* __restrict__ wr = W_hh + static_cast<size_t>(c0 + j) * H + 4 * g;
  const size_t gate_stride = static_cast<size_t>(H) * H;
  float4 a[NSW], w[NSW][3];
#pragma unroll
  for (int q = 0; q < NSW; ++q) {
    const int s = wave + 4 * q;
    if (s < ns) {
      a[q] = ld4(hr + 16 * s);
#pragma unroll
      for (int gate = 0; gate < 3; ++gate) w[q][gate] = ld4(wr + gate * gate_stride + 16 * s);
    }
  }
  f32x4 acc[3];
#pragma unroll
  for (int gate = 0; gate < 3; ++gate) acc[gate] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < NSW; ++q) {
    if (wave + 4 * q < ns) {
#pragma unroll
      for (int gate = 0; gate < 3; ++gate) acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].x, w[q][gate].x, acc[gate], 0, 0, 0);
#pragma unroll
      for (int gate = 0; gate < 3; ++gate) acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].y, w[q][gate].y, acc[gate], 0, 0, 0);
#pragma unroll
      for (int gate = 0; gate < 3; ++gate) acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].z, w[q][gate].z, acc[gate], 0, 0, 0);
#pragma unroll
      for (int gate = 0; gate < 3; ++gate) acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].w, w[q][gate].w, acc[gate], 0, 0, 0);
    }
  }
  // D layout: lane (j, g) holds column j of rows 4 g .. 4 g + 3
#pragma unroll
  for (int gate = 0; gate < 3; ++gate)
#pragma unroll
    for (int r = 0; r < 4; ++r) sP[wave][gate][(4 * g + r) * kRecTile + j] = acc[gate][r];
  __syncthreads();
  const int row = row0 + (tid >> 4), c = c0 + (tid & 15);
  if (row >= N) return;
  float gh[3];
#pragma unroll
  for (int gate = 0; gate < 3; ++gate)
    gh[gate] = ((sP[0][gate][tid] + sP[1][gate][tid]) + (sP[2][gate][tid] + sP[3][gate][tid])) + b_hh[gate * H + c];
  const float* __restrict__ gp = gi + static_cast<size_t>(row) * ld_gi + c;
  const float pr = gp[0] + gh[0], pz = gp[H] + gh[1], gin = gp[2 * H], ghn = gh[2];
  const float hv = h[static_cast<size_t>(row) * ld_h + c];
  const float rr = rec_sigmoidf(pr), zz = rec_sigmoidf(pz);
  const float nn = tanhf(fmaf(rr, ghn, gin));
  h_out[static_cast<size_t>(row) * ld_ho + c] = fmaf(zz, hv - nn, nn);
  if (SAVE) {
    float* p = pre + static_cast<size_t>(row) * 4 * H + c;
    p[0] = pr;
    p[H] = pz;
    p[2 * H] = gin;
    p[3 * H] = ghn;
  }
}

// NSW: 16-wide contraction slices per wavefront (3H / 64 rounded up)
template <int NSW>
__global__ __launch_bounds__(256) void gru_rec_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ h, int ld_h,
                                                          const float* __restrict__ d_hout, const float* __restrict__ d_carry, int N,
                                                          int H, const float* __restrict__ W_hh, float* __restrict__ d_gi,
                                                          float* __restrict__ d_gh, float* __restrict__ dh_prev) {
  // row stride 3H + 4 floats: the 16 rows of a ds_read_b128 lane group start 4 banks apart
  __shared__ __attribute__((aligned(16))) float sG[kRecTile * (3 * kRecMaxH + 4)];
  __shared__ float sP[4][kRecTile * kRecTile];
  __shared__ float sZ[kRecTile * kRecTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.x * kRecTile, c0 = blockIdx.y * kRecTile;
  const int LD = 3 * H + 4, HV = H / 4;
  const int ns = 3 * H / 16;
  const float* __restrict__ wp = W_hh + static_cast<size_t>(4 * g) * H + c0 + j;
  // every W_hh element of this wavefront is requested before the gate gradients are formed (NSW x 4 dwords per lane in flight)
  float b[NSW][4];
#pragma unroll
  for (int q = 0; q < NSW; ++q) {
    const int s = wave + 4 * q;
    if (s < ns) {
      const float* __restrict__ ws = wp + static_cast<size_t>(16 * s) * H;
#pragma unroll
      for (int c = 0; c < 4; ++c) b[q][c] = ws[static_cast<size_t>(c) * H];
    }
  }
  for (int idx = tid; idx < kRecTile * HV; idx += 256) {
    const int lrow = idx / HV, col = (idx - lrow * HV) * 4;
    const int row = row0 + lrow;
    float dr[4] = {0.f, 0.f, 0.f, 0.f}, dz[4] = {0.f, 0.f, 0.f, 0.f}, dnh[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < N) {
      const float* p = pre + static_cast<size_t>(row) * 4 * H + col;
      const float4 pr = ld4(p), pz = ld4(p + H), gin = ld4(p + 2 * H), ghn = ld4(p + 3 * H);
      const float4 hh = ld4(h + static_cast<size_t>(row) * ld_h + col);
      float4 dho = make_float4(0.f, 0.f, 0.f, 0.f);
      if (d_hout != nullptr) dho = ld4(d_hout + static_cast<size_t>(row) * H + col);
      if (d_carry != nullptr) {
        const float4 dc = ld4(d_carry + static_cast<size_t>(row) * H + col);
        dho.x += dc.x;
        dho.y += dc.y;
        dho.z += dc.z;
        dho.w += dc.w;
      }
      const float a_pr[4] = {pr.x, pr.y, pr.z, pr.w}, a_pz[4] = {pz.x, pz.y, pz.z, pz.w};
      const float a_gi[4] = {gin.x, gin.y, gin.z, gin.w}, a_gh[4] = {ghn.x, ghn.y, ghn.z, ghn.w};
      const float a_h[4] = {hh.x, hh.y, hh.z, hh.w}, a_d[4] = {dho.x, dho.y, dho.z, dho.w};
      float dni[4], dhz[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {                      // the arithmetic of gru_gates_bwd_fused_kernel
        const float r = rec_sigmoidf(a_pr[t]), z = rec_sigmoidf(a_pz[t]);
        const float n = tanhf(fmaf(r, a_gh[t], a_gi[t]));
        const float dn_pre = a_d[t] * (1.f - z) * (1.f - n * n);
        dni[t] = dn_pre;
        dnh[t] = dn_pre * r;
        dr[t] = dn_pre * a_gh[t] * r * (1.f - r);
        dz[t] = a_d[t] * (a_h[t] - n) * z * (1.f - z);
        dhz[t] = a_d[t] * z;
      }
      if (col >= c0 && col < c0 + kRecTile) {            // this workgroup's column block of the outputs
        float* gi_o = d_gi + static_cast<size_t>(row) * 3 * H + col;
        float* gh_o = d_gh + static_cast<size_t>(row) * 3 * H + col;
        *reinterpret_cast<float4*>(gi_o) = make_float4(dr[0], dr[1], dr[2], dr[3]);
        *reinterpret_cast<float4*>(gi_o + H) = make_float4(dz[0], dz[1], dz[2], dz[3]);
        *reinterpret_cast<float4*>(gi_o + 2 * H) = make_float4(dni[0], dni[1], dni[2], dni[3]);
        *reinterpret_cast<float4*>(gh_o) = make_float4(dr[0], dr[1], dr[2], dr[3]);
        *reinterpret_cast<float4*>(gh_o + H) = make_float4(dz[0], dz[1], dz[2], dz[3]);
        *reinterpret_cast<float4*>(gh_o + 2 * H) = make_float4(dnh[0], dnh[1], dnh[2], dnh[3]);
#pragma unroll
        for (int t = 0; t < 4; ++t) sZ[lrow * kRecTile + col - c0 + t] = dhz[t];
      }
    }
    float* sg = sG + lrow * LD + col;                    // rows >= N: zeros (their products are never written)
    *reinterpret_cast<float4*>(sg) = make_float4(dr[0], dr[1], dr[2], dr[3]);
    *reinterpret_cast<float4*>(sg + H) = make_float4(dz[0], dz[1], dz[2], dz[3]);
    *reinterpret_cast<float4*>(sg + 2 * H) = make_float4(dnh[0], dnh[1], dnh[2], dnh[3]);
  }
  __syncthreads();
  // dh_prev[:, c0 + j] += sum_k d_gh[:, k] W_hh[k, c0 + j]: A from LDS (lane (i, g): columns 16 s + 4 g .. + 3 of row i), B element of
  // MFMA (s, c), K slot g: W_hh[16 s + 4 g + c, c0 + j] - 64 contiguous bytes per K row and instruction
  const float* ap = sG + j * LD + 4 * g;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < NSW; ++q) {
    const int s = wave + 4 * q;
    if (s < ns) {
      const float4 a = ld4(ap + 16 * s);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[q][0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[q][1], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[q][2], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[q][3], acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) sP[wave][(4 * g + r) * kRecTile + j] = acc0[r] + acc1[r];
  __syncthreads();
  const int row = row0 + (tid >> 4), c = c0 + (tid & 15);
  if (row < N) dh_prev[static_cast<size_t>(row) * H + c] = sZ[tid] + ((sP[0][tid] + sP[1][tid]) + (sP[2][tid] + sP[3][tid]));
}

// [p, p + bytes) ranges of two row-major operands intersect
inline bool rec_overlap(const float* a, int ld_a, const float* b, int ld_b, int N, int H) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  const uintptr_t a1 = a0 + 4 * (static_cast<uintptr_t>(N - 1) * ld_a + H), b1 = b0 + 4 * (static_cast<uintptr_t>(N - 1) * ld_b + H);
  return a0 < b1 && b0 < a1;
}

inline bool rec_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace
}  // namespace uavgnn

using namespace uavgnn;

extern "C" int uavgnn_gru_rec_supported(int H) { return (H >= 16 && H <= kRecMaxH && H % 16 == 0) ? 1 : 0; }

extern "C" int uavgnn_gru_rec_fwd(const float* gi, int ld_gi, const float* h, int ld_h, int N, int H, const float* W_hh,
                                  const float* b_hh, float* h_out, int ld_ho, float* pre_save, uavgnn_stream_t stream) {
  if (N < 0 || H <= 0 || !gi || !h || !W_hh || !b_hh || !h_out || ld_gi < 3 * H || ld_h < H || ld_ho < H) return UAVGNN_EINVAL;
  if (!uavgnn_gru_rec_supported(H) || (ld_gi & 3) || (ld_h & 3) || (ld_ho & 3) || rec_misaligned(gi) || rec_misaligned(h) ||
      rec_misaligned(W_hh) || rec_misaligned(h_out) || rec_misaligned(pre_save))
    return UAVGNN_EUNSUPPORTED;
  if (N == 0) return 0;
  // every workgroup reads whole rows of h while others write column blocks of h_out
  if (rec_overlap(h, ld_h, h_out, ld_ho, N, H)) return UAVGNN_EINVAL;
  const dim3 grid((N + kRecTile - 1) / kRecTile, H / kRecTile), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define UAVGNN_REC(NSW_)                                                                                                          \
  do {                                                                                                                            \
    if (pre_save != nullptr)                                                                                                      \
      hipLaunchKernelGGL((gru_rec_fwd_kernel<NSW_, true>), grid, block, 0, st, gi, ld_gi, h, ld_h, N, H, W_hh, b_hh, h_out, ld_ho, \
                         pre_save);                                                                                               \
    else                                                                                                                          \
      hipLaunchKernelGGL((gru_rec_fwd_kernel<NSW_, false>), grid, block, 0, st, gi, ld_gi, h, ld_h, N, H, W_hh, b_hh, h_out, ld_ho, \
                         pre_save);                                                                                               \
  } while (0)
  if (H <= 64)
    UAVGNN_REC(1);
  else if (H <= 128)
    UAVGNN_REC(2);
  else
    UAVGNN_REC(4);
#undef UAVGNN_REC
  return launch_status();
}

extern "C" int uavgnn_gru_rec_bwd(const float* pre, const float* h, int ld_h, const float* d_hout, const float* d_carry, int N, int H,
                                  const float* W_hh, float* d_gi, float* d_gh, float* dh_prev, uavgnn_stream_t stream) {
  if (N < 0 || H <= 0 || !pre || !h || !W_hh || !d_gi || !d_gh || !dh_prev || ld_h < H) return UAVGNN_EINVAL;
  if (!uavgnn_gru_rec_supported(H) || (ld_h & 3) || rec_misaligned(pre) || rec_misaligned(h) || rec_misaligned(d_hout) ||
      rec_misaligned(d_carry) || rec_misaligned(W_hh) || rec_misaligned(d_gi) || rec_misaligned(d_gh) || rec_misaligned(dh_prev))
    return UAVGNN_EUNSUPPORTED;
  if (N == 0) return 0;
  // every workgroup reads whole rows of d_hout / d_carry while others write column blocks of dh_prev
  if ((d_hout && rec_overlap(d_hout, H, dh_prev, H, N, H)) || (d_carry && rec_overlap(d_carry, H, dh_prev, H, N, H))) return UAVGNN_EINVAL;
  const dim3 grid((N + kRecTile - 1) / kRecTile, H / kRecTile), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define UAVGNN_REC(NSW_) \
  hipLaunchKernelGGL((gru_rec_bwd_kernel<NSW_>), grid, block, 0, st, pre, h, ld_h, d_hout, d_carry, N, H, W_hh, d_gi, d_gh, dh_prev)
  if (H <= 64)
    UAVGNN_REC(3);
  else if (H <= 128)
    UAVGNN_REC(6);
  else
    UAVGNN_REC(12);
#undef UAVGNN_REC
  return launch_status();
}

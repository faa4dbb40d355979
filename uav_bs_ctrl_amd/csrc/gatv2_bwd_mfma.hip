// The matrix-core instantiation of the K1 backward (gatv2_bwd_kernel<4, 4, 64, true, true> of gatv2.hip), in a translation
// unit of its own because it must be compiled WITHOUT packed fp32 instructions (build.py: -target-feature -packed-fp32-ops).
//
// Measured on MI355X (tools/ubench/mfma_pk_hazard.hip, profiles/r04_mfma_pk_hazard.txt): a v_pk_fma_f32 / v_pk_mul_f32 whose
// op_sel takes the HIGH dword of src1 for the LOW result (op_sel:[0,1,0] - what the compiler emits for  lo = a.x * b.y + c.x)
// returns a wrong low result in lanes 48-63 when an MFMA with 128-bit operands (v_mfma_f32_16x16x32_bf16 / _f16,
// v_mfma_f32_32x32x16_bf16: all measured) is issued to the same SIMD in the very next issue slot - by the same wave (every time; ONE s_nop 0 between the two is enough) or by another wave of the SIMD (now and then,
// and nothing a wave can do about it).  Registers are independent: it is not a data hazard.  The fp32 MFMA 16x16x4 and the
// 64-bit-operand bf16 MFMA do not do it, other operand selects do not do it, plain v_fma_f32 does not do it.  ROCm 7.2's
// compiler knows no such hazard: the first build of this kernel staged the attention dots with exactly that instruction
// while other waves of the SIMD ran the matrix-core loop and lost the gk[1] * x[1] term of head 0 or 2 in sixteen edges of a
// destination now and then (bit-irreproducible gradients).  tools/isa_audit.py (tests/test_isa_audit.py) checks the shipped
// library for the pattern: no kernel with 16-bit-operand MFMAs may hold such an instruction.
#define UAVGNN_GATV2_BWD_MFMA_TU 1
#include <type_traits>

#include "gatv2.hip"

// ---------------------------------------------------------------------------------------------------------------------------------
// gatv2_bwd_resident_kernel: the same class (F_src 4, nh 4, D 64, 16 .. onepass_max_deg <= 128 in-edges; cls = 1 of the launcher)
// with the matrix-core accumulators RESIDENT over all destinations of a wavefront.
//
// Everything the old kernel folded after each destination is linear across destinations with per-channel coefficients, except
// the terms of S1 (they meet the destination's own x_v and c_v):
//   d W_s[n,:] += attn[n] (c_abs S2[n,:] + c_lin P[k,:]) + g[n] Sb[k,:]     -> sum_v S2, sum_v P, and g (x) Sb per destination
//   d attn[n]  += c_abs (c[n] S1[n] + W_s[n,:].S2[n,:]) + c_lin W_s[n,:].P  -> sum_v c S1, sum_v S2, sum_v P
//   der = attn c_abs S1 -> d b_s, d b_d, d W_d (x) x_v                       -> sum_v S1, sum_v x_v0 S1, sum_v x_v1 S1
// so the sign-weighted products of a destination are ADDED to the accumulators of the previous ones.  The rows of the V operand
// are ordered so that the three bf16 terms of S1 are rows 0..2 (lanes 0..15, registers 0..2 of every channel tile): after a
// destination those three registers are read (S1 is bit-identical to the old kernel's), moved to lane <-> channel by two
// permlane swaps per head and zeroed; the 12 rows of S2 (3 + 4 t + f) stay in the accumulators until the wavefront is done.
// The input-space sums come out of the staging registers (lane <-> edge): Sb and P by one 16-value wave reduction each
// (wave_totals16), G too; P is kept as a running sum.  The LDS conversion of the accumulators and the channel epilogue run
// once per wavefront instead of once per destination.
namespace uavgnn {
namespace {

__device__ __forceinline__ float readlane_f(float v, int l) {
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l));
}
// 16 per-lane values v[4 r + i] -> their totals over the 64 lanes: t[i] holds the total of v[4 r + i] in every lane of row r (16
// lanes).  Halves by permlane32_swap, rows by permlane16_swap, then four DPP adds inside each row: a fixed tree, deterministic.
__device__ __forceinline__ void wave_totals16(const float (&v)[16], float (&t)[4]) {
  float w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {   // w[i]: value i in lanes 0..31, value i + 8 in lanes 32..63
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 8]), false, false);
    w[i] = __uint_as_float(s[0]) + __uint_as_float(s[1]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {   // row r: value i + 4 r
    const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(w[i]), __float_as_uint(w[i + 4]), false, false);
    t[i] = row16_allsum(__uint_as_float(s[0]) + __uint_as_float(s[1]));
  }
}

// k1_split of two values at once, packed the way the V operand wants them: (a_t | b_t << 16) of the three terms.  One conversion
// instruction per term converts both values (k1_split converts each value into both halves and the caller merges two words);
// each half is the same round-to-nearest conversion, the same bits.
__device__ __forceinline__ K1Split k1_split_pair(float a, float b) {
  K1Split s;
  s.h1 = __builtin_bit_cast(unsigned, __builtin_convertvector(k1_f32x2{a, b}, k1_bf16x2));
  const float a1 = a - __uint_as_float(s.h1 << 16), b1 = b - __uint_as_float(s.h1 & 0xffff0000u);
  s.h2 = __builtin_bit_cast(unsigned, __builtin_convertvector(k1_f32x2{a1, b1}, k1_bf16x2));
  const float a2 = a1 - __uint_as_float(s.h2 << 16), b2 = b1 - __uint_as_float(s.h2 & 0xffff0000u);
  s.h3 = __builtin_bit_cast(unsigned, __builtin_convertvector(k1_f32x2{a2, b2}, k1_bf16x2));
  return s;
}

// LEAN: fewer instructions per destination (the kernel issues ~2 200 per 80-edge destination and its time is their issue time,
// DESIGN.md section 5): the V operands of two edges split by k1_split_pair; the W operand of a channel tile read as three words +
// the bias word instead of a 16-byte read whose last word is then overwritten; the S1 rows zeroed by DPP moves, their sign put
// on behind the swaps.
// HT: a last trip of at most 16 edges runs on its first score tile only.  false / false: the kernel as first shipped; same bits
// out of all four.
template <bool LEAN, bool HT>
__global__ __launch_bounds__(kThreads, UAVGNN_BWD_OCC) void gatv2_bwd_resident_kernel(
    const float* __restrict__ x_src, const float* __restrict__ x_dst, const int32_t* __restrict__ seg_off,
    const int32_t* __restrict__ dst_order, int N,
    const float* __restrict__ W_s, const float* __restrict__ b_s, const float* __restrict__ W_d,
    const float* __restrict__ b_d, const float* __restrict__ attn, float slope, const float* __restrict__ out,
    const float* __restrict__ d_out, int ld_out, const float* __restrict__ a_save, float* __restrict__ partial,
    int onepass_max_deg) {
  constexpr int FS = 4, NH = 4, D = 64, H = NH * D, J = H / kWave, CT = H / 16;
  constexpr int P = partial_len<FS>(H);
  constexpr int ES = FS + 2 * NH;   // staged floats per edge: x[FS], de[NH], (unused)[NH] - the stride of the old kernel
  // LDS: staged edges (two 64-edge chunks per wavefront) | V operands [head][lane] per wavefront | W operands of the score
  // products (the fold buffer of the end takes their place) | bias words -c per wavefront + one all-zero table
  constexpr int szE = kWavesPerBlock * 2 * kWave * ES * 4, szV = kWavesPerBlock * NH * kWave * 16, szWop = CT * kWave * 16;
  constexpr int szC = (kWavesPerBlock + 1) * CT * 32 * 4, szD = 3 * H * 4;
  constexpr int oE = 0, oV = oE + szE, oWop = oV + szV, oC = oWop + szWop, oD = oC + szC, kLdsBytes = oD + szD;
  static_assert(P * 4 <= szWop, "fold buffer aliases the score operands");
  static_assert(kLdsBytes <= 80 * 1024, "two workgroups per CU");
  static_assert(kWave * 20 * 4 <= 2 * kWave * ES * 4, "the final conversion of the accumulators fits the staging area");
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  k1_u32x4* const sWop = reinterpret_cast<k1_u32x4*>(lds + oWop);
  float* const sRed = reinterpret_cast<float*>(lds + oWop);
  float* const sD = reinterpret_cast<float*>(lds + oD);   // W_d[:, 0] | W_d[:, 1] | b_d + b_s: the destination term c = W_d x_v + b_d + b_s

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, g4 = lane >> 4;
  const float c_lin = 0.5f * (1.f + slope), c_abs = 0.5f * (1.f - slope);

  for (int i = tid; i < CT * kWave; i += kThreads) {   // lane (j = channel of the tile, kg = feature)
    const int ct = i >> 6, l = i & 63;
    sWop[i] = k1_a_operand(0.f - W_s[(16 * ct + (l & 15)) * FS + (l >> 4)], 0.f, 0);   // -W: the score MFMA yields -(z + c)
  }
  for (int i = tid; i < CT * 32; i += kThreads) reinterpret_cast<unsigned*>(lds + oC)[kWavesPerBlock * CT * 32 + i] = 0u;
  for (int n = tid; n < H; n += kThreads) {
    sD[n] = W_d[2 * n];
    sD[H + n] = W_d[2 * n + 1];
    sD[2 * H + n] = b_d[n] + b_s[n];
  }
  for (int i = lane; i < NH * kWave; i += kWave)   // the zero row of every operand is never written again
    (reinterpret_cast<k1_u32x4*>(lds + oV) + wave * NH * kWave)[i] = k1_u32x4{0u, 0u, 0u, 0u};

  // lane <-> channel n = lane + 64 j, head j
  float Ws[J][FS];
  float aWs[J][FS], aWr0[J], aWr1[J], abr[J], sS1[J], sX0[J], sX1[J];   // sum_v c_v S1_v = W_d[:, 0] sX0 + W_d[:, 1] sX1 + bc sS1
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int n = lane + kWave * j;
#pragma unroll
    for (int f = 0; f < FS; ++f) {
      Ws[j][f] = W_s[n * FS + f];
      aWs[j][f] = 0.f;
    }
    aWr0[j] = aWr1[j] = abr[j] = sS1[j] = sX0[j] = sX1[j] = 0.f;
  }
  float accP[FS];   // running sum of P: lanes of row k hold P[k][0..3]
#pragma unroll
  for (int f = 0; f < FS; ++f) accP[f] = 0.f;
  bwd_f32x4 acc[CT];   // resident: rows 0..2 (S1 terms) are drained per destination, rows 3..14 (S2) at the end
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = bwd_f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  float* __restrict__ ew = reinterpret_cast<float*>(lds + oE) + wave * 2 * kWave * ES;
  k1_u32x4* __restrict__ vw = reinterpret_cast<k1_u32x4*>(lds + oV) + wave * NH * kWave;
  unsigned* __restrict__ cwt = reinterpret_cast<unsigned*>(lds + oC) + wave * CT * 32;
  // lane (channel j16, K group g4) of the score operand: bias word from the wavefront's table (K groups 0, 1) or the zero table
  const unsigned* __restrict__ cwl = reinterpret_cast<const unsigned*>(lds + oC) +
      (g4 < 2 ? wave * CT * 32 + 16 * g4 + j16 : kWavesPerBlock * CT * 32 + (lane & 31));

  auto load_rows = [&](const int v, float (&o)[J], float (&gr)[J]) {
    const float* __restrict__ orow = out + static_cast<size_t>(v) * ld_out;
    const float* __restrict__ grow = d_out + static_cast<size_t>(v) * ld_out;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      o[j] = orow[lane + kWave * j];
      gr[j] = grow[lane + kWave * j];
    }
  };

  auto process = [&](const float (&o_)[J], const float (&gr_)[J], const int e0, const int deg, const float xv0, const float xv1) {
    float g[J], c[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      g[j] = o_[j] > 0.f ? gr_[j] : 0.f;  // ReLU mask
      aWr0[j] = fmaf(g[j], xv0, aWr0[j]);
      aWr1[j] = fmaf(g[j], xv1, aWr1[j]);
      abr[j] += g[j];
      const int n = lane + kWave * j;
      c[j] = fmaf(sD[H + n], xv1, fmaf(sD[n], xv0, sD[2 * H + n]));
    }
    // G[k][f] = sum_d g[k,d] W_s[k,d,f] (head k = register j), broadcast through SGPRs
    float G[NH][FS];
    {
      float gv[16], gt[4];
#pragma unroll
      for (int j = 0; j < J; ++j)
#pragma unroll
        for (int f = 0; f < FS; ++f) gv[4 * j + f] = g[j] * Ws[j][f];
      wave_totals16(gv, gt);
#pragma unroll
      for (int k = 0; k < NH; ++k)
#pragma unroll
        for (int f = 0; f < FS; ++f) G[k][f] = readlane_f(gt[f], 16 * k);
    }
    // stage the edges (lane <-> edge, slots lane and 64 + lane): x_u and de_uk = a_uk (G[k].x_u - T[k]) in LDS; Sb and P from the
    // same registers
    float x[2][FS], a[2][NH], dt[2][NH], t[NH], sb[16];
#pragma unroll
    for (int k = 0; k < NH; ++k) t[k] = 0.f;
#pragma unroll
    for (int m = 0; m < 16; ++m) sb[m] = 0.f;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int slot = ch * kWave + lane;
      if (slot < deg) {
        const int u = e0 + slot;
        load_row<FS>(x_src + static_cast<size_t>(u) * FS, x[ch]);
        load_row<NH>(a_save + static_cast<size_t>(u) * NH, a[ch]);
      } else {
#pragma unroll
        for (int f = 0; f < FS; ++f) x[ch][f] = 0.f;
#pragma unroll
        for (int k = 0; k < NH; ++k) a[ch][k] = 0.f;
      }
    }
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
#pragma unroll
      for (int k = 0; k < NH; ++k) {
        float d = 0.f;
#pragma unroll
        for (int f = 0; f < FS; ++f) d = fmaf(G[k][f], x[ch][f], d);
        dt[ch][k] = d;
        t[k] = fmaf(a[ch][k], d, t[k]);
#pragma unroll
        for (int f = 0; f < FS; ++f) sb[4 * k + f] = fmaf(a[ch][k], x[ch][f], sb[4 * k + f]);
      }
      if (ch * kWave < deg)
        *reinterpret_cast<bwd_f32x4*>(ew + (ch * kWave + lane) * ES) = bwd_f32x4{x[ch][0], x[ch][1], x[ch][2], x[ch][3]};
    }
    float T[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) T[k] = wave_total_dpp(t[k]);
    {
      float st[4];
      wave_totals16(sb, st);
#pragma unroll
      for (int j = 0; j < J; ++j)
#pragma unroll
        for (int f = 0; f < FS; ++f) aWs[j][f] = fmaf(g[j], readlane_f(st[f], 16 * j), aWs[j][f]);
    }
    {
      float pv[16], pt[4];
#pragma unroll
      for (int m = 0; m < 16; ++m) pv[m] = 0.f;
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) {
        float de[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) {
          de[k] = a[ch][k] * (dt[ch][k] - T[k]);
#pragma unroll
          for (int f = 0; f < FS; ++f) pv[4 * k + f] = fmaf(de[k], x[ch][f], pv[4 * k + f]);
        }
        if (ch * kWave < deg)
          *reinterpret_cast<bwd_f32x4*>(ew + (ch * kWave + lane) * ES + FS) = bwd_f32x4{de[0], de[1], de[2], de[3]};
      }
      wave_totals16(pv, pt);
#pragma unroll
      for (int f = 0; f < FS; ++f) accP[f] += pt[f];
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {   // channel lane + 64 j = tile (lane >> 4) + 4 j, column lane & 15
      const K1Split sc = k1_split(0.f - c[j]);
      unsigned* q = cwt + ((lane >> 4) + 4 * j) * 32 + (lane & 15);
      q[0] = (sc.h1 & 0xffffu) | (sc.h2 & 0xffff0000u);
      q[16] = sc.h3 & 0xffffu;
    }
    wave_sync();

    // ---- per-(edge, channel) sign-weighted sums on the matrix cores, added to the resident accumulators -------------------------
    const bwd_f32x4 czero = {0.f, 0.f, 0.f, 0.f};
    unsigned k_sign = 0x80008000u, k_one = 0x3F803F80u;
    asm volatile("" : "+v"(k_sign), "+v"(k_one));
    // one trip: 32 edges as two 16-edge score tiles and one K = 32 accumulation per channel tile.  HALF (the last trip when at most
    // 16 edges are left): the second tile's edges are padding - no score products, no sign words and no V operands for them;
    // their K positions of the accumulation take zeros on both sides (the V words of tile 1 in LDS are the previous trip's).
    auto trip = [&](const int tp, auto half_c) {
      constexpr bool HALF = decltype(half_c)::value;
      const float* const et = ew + 32 * tp * ES;   // slot 32 tp
      if constexpr (HALF) {   // lane (edge i16, head h): one edge's half-words
        int ln = lane;   // opaque: this trip's addresses are worked out here, not kept in registers over the whole kernel
        asm volatile("" : "+v"(ln));
        const int i16 = ln & 15, h = ln >> 4;
        const float* er = et + i16 * ES;
        const bwd_f32x4 xa = *reinterpret_cast<const bwd_f32x4*>(er);
        const float da = er[FS + h];
        const float va[5] = {da, da * xa[0], da * xa[1], da * xa[2], da * xa[3]};
        const int skew = (i16 >> 2) + 4 * h;
        unsigned short* dst = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned*>(vw) + (h * kWave + (i16 >> 2) * 16) * 4 +
                                                                ((i16 & 3) >> 1)) + (i16 & 1);
#pragma unroll
        for (int f = 0; f < 5; ++f) {
          const K1Split sa = k1_split(va[f]);
          const int r0 = f == 0 ? 0 : 2 + f, dr = f == 0 ? 1 : 4;
          dst[((r0 + 0 * dr + skew) & 15) * 8] = static_cast<unsigned short>(sa.h1);
          dst[((r0 + 1 * dr + skew) & 15) * 8] = static_cast<unsigned short>(sa.h2);
          dst[((r0 + 2 * dr + skew) & 15) * 8] = static_cast<unsigned short>(sa.h3);
        }
      } else {
        const int ep = lane & 15, h = lane >> 4;
        const int e_a = 2 * ep, i16 = e_a & 15;
        const float* er = et + e_a * ES;
        const bwd_f32x4 xa = *reinterpret_cast<const bwd_f32x4*>(er), xb = *reinterpret_cast<const bwd_f32x4*>(er + ES);
        const float da = er[FS + h], db = er[ES + FS + h];
        const float va[5] = {da, da * xa[0], da * xa[1], da * xa[2], da * xa[3]};
        const float vb[5] = {db, db * xb[0], db * xb[1], db * xb[2], db * xb[3]};
        const int skew = (i16 >> 2) + 4 * h;
        unsigned* dst = reinterpret_cast<unsigned*>(vw) + (h * kWave + (i16 >> 2) * 16) * 4 + (((i16 & 3) + 4 * (e_a >> 4)) >> 1);
#pragma unroll
        for (int f = 0; f < 5; ++f) {   // row of term tt of value f: tt (f = 0, the S1 rows) or 3 + 4 tt + f - 1 (S2)
          const int r0 = f == 0 ? 0 : 2 + f, dr = f == 0 ? 1 : 4;
          if constexpr (LEAN) {
            const K1Split sp = k1_split_pair(va[f], vb[f]);
            dst[((r0 + 0 * dr + skew) & 15) * 4] = sp.h1;
            dst[((r0 + 1 * dr + skew) & 15) * 4] = sp.h2;
            dst[((r0 + 2 * dr + skew) & 15) * 4] = sp.h3;
          } else {
            const K1Split sa = k1_split(va[f]), sb2 = k1_split(vb[f]);
            dst[((r0 + 0 * dr + skew) & 15) * 4] = (sa.h1 & 0xffffu) | (sb2.h1 & 0xffff0000u);
            dst[((r0 + 1 * dr + skew) & 15) * 4] = (sa.h2 & 0xffffu) | (sb2.h2 & 0xffff0000u);
            dst[((r0 + 2 * dr + skew) & 15) * 4] = (sa.h3 & 0xffffu) | (sb2.h3 & 0xffff0000u);
          }
        }
      }
      constexpr int NT = HALF ? 1 : 2;
      k1_bf16x8 xop[NT];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) xop[tt] = k1_b_operand(et[(16 * tt + j16) * ES + g4], 0x3F803F80u);
      wave_sync_lds();
      auto v_operand = [&](const int i) {
        k1_u32x4 v = vw[i];
        if constexpr (HALF) v[2] = v[3] = 0u;
        return v;
      };
      k1_u32x4 vop = v_operand(16 * g4 + ((j16 + g4) & 15)), vop_n = v_operand(kWave + 16 * g4 + ((j16 + g4 + 4) & 15));
      auto w_operand = [&](const int ct_) {
        if constexpr (LEAN) {   // three words + the bias word into four registers of their own: a 16-byte read whose last word
          // is then overwritten makes the second read wait for the first (a full LDS round trip per channel tile)
          const unsigned* wp = reinterpret_cast<const unsigned*>(sWop + ct_ * kWave + lane);
          const uint2 w01 = *reinterpret_cast<const uint2*>(wp);
          return __builtin_bit_cast(k1_bf16x8, k1_u32x4{w01.x, w01.y, wp[2], cwl[ct_ * 32]});
        }
        k1_u32x4 w = sWop[ct_ * kWave + lane];
        w[3] = cwl[ct_ * 32];
        return __builtin_bit_cast(k1_bf16x8, w);
      };
      k1_bf16x8 w_nn = w_operand(1);
      bwd_f32x4 d0, d1 = czero;
      {
        const k1_bf16x8 w0 = w_operand(0);
        d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xop[0], w0, czero, 0, 0, 0);
        if constexpr (!HALF) d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xop[NT - 1], w0, czero, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        bwd_f32x4 e0_ = d0, e1_ = d1;
        if (ct + 1 < CT) {
          e0_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xop[0], w_nn, czero, 0, 0, 0);
          if constexpr (!HALF) e1_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xop[NT - 1], w_nn, czero, 0, 0, 0);
          if (ct + 2 < CT) w_nn = w_operand(ct + 2);
          __builtin_amdgcn_sched_barrier(0);
        }
        k1_u32x4 sg = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 2; ++q) {   // d = -(z + c): the sign bits of two edges' values side by side over 1.0
          const unsigned p0 = __builtin_amdgcn_perm(__float_as_uint(d0[2 * q + 1]), __float_as_uint(d0[2 * q]), 0x07060302u);
          sg[q] = (p0 & k_sign) | (k_one & ~k_sign);
          if constexpr (!HALF) {
            const unsigned p1 = __builtin_amdgcn_perm(__float_as_uint(d1[2 * q + 1]), __float_as_uint(d1[2 * q]), 0x07060302u);
            sg[2 + q] = (p1 & k_sign) | (k_one & ~k_sign);
          }
        }
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(k1_bf16x8, vop), __builtin_bit_cast(k1_bf16x8, sg),
                                                          acc[ct], 0, 0, 0);
        if ((ct & 3) == 3 && ct + 1 < CT) {
          vop = vop_n;
          if (ct + 5 < CT) vop_n = v_operand(((ct + 5) >> 2) * kWave + 16 * g4 + ((j16 + g4 + 4 * ((ct + 5) >> 2)) & 15));
        }
        __builtin_amdgcn_sched_barrier(0);
        d0 = e0_;
        d1 = e1_;
      }
      wave_sync_lds();
    };
    {
      int tp = 0;
      for (; 32 * tp + (HT ? 16 : 0) < deg; ++tp) trip(tp, std::false_type{});
      if (HT && 32 * tp < deg) trip(tp, std::true_type{});
    }
    // ---- S1 of this destination: rows 0..2 of every tile (lanes 0..15), then zeroed; tile 4 k + r -> row r of head k ---------
    float s1[CT];
    const bool s1_lane = lane < 16;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const float sum = (acc[ct][0] + acc[ct][1]) + acc[ct][2];
      s1[ct] = LEAN ? sum : -sum;   // LEAN: the sign goes on behind the swaps (4 values, not 16)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        if constexpr (LEAN)   // a DPP move that writes row 0 (lanes 0..15) only, in place: the select drags ~40 register copies behind it
          acc[ct][i] = __uint_as_float(__builtin_amdgcn_update_dpp(__float_as_uint(acc[ct][i]), 0u, 0xE4, 0x1, 0xf, false));
        else
          acc[ct][i] = s1_lane ? 0.f : acc[ct][i];
      }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(s1[4 * j]), __float_as_uint(s1[4 * j + 1]), false, false);
      const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(s1[4 * j + 2]), __float_as_uint(s1[4 * j + 3]), false, false);
      const auto s = __builtin_amdgcn_permlane32_swap(r[0], q[0], false, false);
      const float S1 = LEAN ? -__uint_as_float(s[0]) : __uint_as_float(s[0]);   // channel lane + 64 j
      sS1[j] += S1;
      sX0[j] = fmaf(xv0, S1, sX0[j]);
      sX1[j] = fmaf(xv1, S1, sX1[j]);
    }
    wave_sync();
  };

  // destinations of the class in a fixed order: 64 destinations' meta data by vector loads + v_readlane (the old kernel's loop)
  const int stride = gridDim.x * kWavesPerBlock;
  const int it0 = blockIdx.x * kWavesPerBlock + wave;
  for (int kb = 0; it0 + kb * stride < N; kb += kWave) {
    const int my_it = it0 + (kb + lane) * stride;
    const bool mine = my_it < N;
    const int m_v = mine ? (dst_order ? dst_order[my_it] : my_it) : 0;
    const int m_e0 = mine ? seg_off[m_v] : 0;
    const int m_e1 = mine ? seg_off[m_v + 1] : 0;
    const float2 m_xv = mine ? *reinterpret_cast<const float2*>(x_dst + 2 * m_v) : make_float2(0.f, 0.f);
    const int cnt = min(kWave, (N - it0 - kb * stride + stride - 1) / stride);
    auto in_cls = [&](const int i) {
      const int dg = __builtin_amdgcn_readlane(m_e1, i) - __builtin_amdgcn_readlane(m_e0, i);
      return dg >= kMfMinDeg && dg <= onepass_max_deg;
    };
    float on[J], gn[J];                       // rows of the NEXT destination are in flight while this one computes
    int ii = 0;
    while (ii < cnt && !in_cls(ii)) ++ii;
    if (ii < cnt) load_rows(__builtin_amdgcn_readlane(m_v, ii), on, gn);
    while (ii < cnt) {
      float oc[J], gc[J];
#pragma unroll
      for (int j = 0; j < J; ++j) {
        oc[j] = on[j];
        gc[j] = gn[j];
      }
      int nx = ii + 1;
      while (nx < cnt && !in_cls(nx)) ++nx;
      if (nx < cnt) load_rows(__builtin_amdgcn_readlane(m_v, nx), on, gn);
      const int e0 = __builtin_amdgcn_readlane(m_e0, ii);
      process(oc, gc, e0, __builtin_amdgcn_readlane(m_e1, ii) - e0,
              __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(m_xv.x), ii)),
              __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(m_xv.y), ii)));
      ii = nx;
    }
  }

  // ---- once per wavefront: S2 out of the accumulators (through LDS, lane <-> channel), then the channel epilogue -----------------
  float abs_[J], aWd0[J], aWd1[J], abd[J], aatt[J];
  {
    constexpr int kCvLd = 20;
    int le = lane;   // the indices of this once-per-wavefront block are made here, not carried (spilled) through the loops above
    if constexpr (HT) asm volatile("" : "+v"(le));
    float* __restrict__ cv = ew;
#pragma unroll
    for (int k = 0; k < NH; ++k) {
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) *reinterpret_cast<bwd_f32x4*>(cv + (c4 * 16 + j16) * kCvLd + 4 * g4) = acc[4 * k + c4];
      wave_sync_lds();
      float r[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bwd_f32x4 t4 = *reinterpret_cast<const bwd_f32x4*>(cv + lane * kCvLd + 4 * q);
        r[4 * q] = t4[0]; r[4 * q + 1] = t4[1]; r[4 * q + 2] = t4[2]; r[4 * q + 3] = t4[3];
      }
      wave_sync_lds();
      const float att = attn[le + kWave * k];
      float wS2 = 0.f, wP = 0.f;
#pragma unroll
      for (int f = 0; f < FS; ++f) {
        const float S2 = -((r[3 + f] + r[7 + f]) + r[11 + f]);
        const float pkf = readlane_f(accP[f], 16 * k);
        wS2 = fmaf(Ws[k][f], S2, wS2);
        wP = fmaf(Ws[k][f], pkf, wP);
        aWs[k][f] = fmaf(att, fmaf(c_abs, S2, c_lin * pkf), aWs[k][f]);
      }
      const int n = lane + kWave * k;
      const float cS1 = fmaf(sD[H + n], sX1[k], fmaf(sD[n], sX0[k], sD[2 * H + n] * sS1[k]));
      aatt[k] = fmaf(c_abs, cS1 + wS2, c_lin * wP);
      const float der = att * c_abs;
      abd[k] = der * sS1[k];
      abs_[k] = abr[k] + abd[k];
      aWd0[k] = der * sX0[k];
      aWd1[k] = der * sX1[k];
    }
  }

  // fold the 4 waves in fixed order through LDS, then one partial row per workgroup (layout of the old kernel)
  __syncthreads();   // the fold buffer aliases the score operands
  for (int w = 0; w < kWavesPerBlock; ++w) {
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int n = lane + kWave * j;
        auto put = [&](int idx, float val) { sRed[idx] = (w == 0) ? val : sRed[idx] + val; };
#pragma unroll
        for (int f = 0; f < FS; ++f) put(n * FS + f, aWs[j][f]);
        int o = H * FS;
        put(o + n, abs_[j]);
        o += H;
        put(o + 2 * n, aWd0[j]);
        put(o + 2 * n + 1, aWd1[j]);
        o += 2 * H;
        put(o + n, abd[j]);
        o += H;
        put(o + n, aatt[j]);
        o += H;
        put(o + 2 * n, aWr0[j]);
        put(o + 2 * n + 1, aWr1[j]);
        o += 2 * H;
        put(o + n, abr[j]);
      }
    }
    __syncthreads();
  }
  float* __restrict__ prow = partial + static_cast<size_t>(blockIdx.x) * P;
  for (int i = tid; i < P; i += kThreads) prow[i] = sRed[i];
}

}  // namespace

int gatv2_bwd_resident_launch(const float* x_src, const float* x_dst, const int32_t* seg_off, const int32_t* dst_order, int N,
                              const float* W_s, const float* b_s, const float* W_d, const float* b_d, const float* attn, float slope,
                              const float* out, const float* d_out, int ld_out, const float* a_save, float* partial,
                              int onepass_max_deg, int grid, hipStream_t st) {
  if (onepass_max_deg > 2 * kWave) return UAVGNN_EINVAL;   // two staged 64-edge chunks per destination
  // A/B switches, read at every call like UAVGNN_K1_BWD_RESIDENT: UAVGNN_K1_BWD_LEAN=0 and UAVGNN_K1_BWD_HALFTRIP=0 (see the
  // kernel's template parameters; both 0: the kernel as first shipped; same bits out)
  auto off = [](const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0';
  };
  const bool lean = !off("UAVGNN_K1_BWD_LEAN"), ht = !off("UAVGNN_K1_BWD_HALFTRIP");
#define UAVGNN_RESIDENT_LAUNCH(LEANV, HTV)                                                                                          \
  hipLaunchKernelGGL((gatv2_bwd_resident_kernel<LEANV, HTV>), dim3(grid), dim3(kThreads), 0, st, x_src, x_dst, seg_off, dst_order, \
                     N, W_s, b_s, W_d, b_d, attn, slope, out, d_out, ld_out, a_save, partial, onepass_max_deg)
  if (lean && ht) UAVGNN_RESIDENT_LAUNCH(true, true);
  else if (lean) UAVGNN_RESIDENT_LAUNCH(true, false);
  else if (ht) UAVGNN_RESIDENT_LAUNCH(false, true);
  else UAVGNN_RESIDENT_LAUNCH(false, false);
#undef UAVGNN_RESIDENT_LAUNCH
  return launch_status();
}
}  // namespace uavgnn

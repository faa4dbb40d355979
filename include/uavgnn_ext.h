/*
 * uavgnn_ext.h - entry points of libuavgnn_ext.so: capabilities that replace no call site of the reference implementation.
 *
 * uavgnn.h stays the drop-in boundary (one entry per reference call site); what the device loop adds beyond the reference lives
 * here, in a shared object of its own, with the same conventions: every pointer is DEVICE memory unless said otherwise, every call
 * is asynchronous on `stream`, the result is 0, a negated hipError_t, or one of uavgnn.h's UAVGNN_E* codes (uavgnn_strerror of the
 * main library names them).
 *
 * ---- noisy-net Q head (csrc/ext/noisy_head.hip; Fortunato et al., "Noisy Networks for Exploration", ICLR 2018, factorised form) ----
 *
 *   W = W_mu + W_sigma (.) (f_out f_in^T),   b = b_mu + b_sigma (.) f_out,   q = h W^T + b,   f(z) = sign(z) sqrt|z|
 *
 * with standard normals xi_in [H], xi_out [A], f_in = f(xi_in), f_out = f(xi_out).
 *
 * THE NOISE STREAM.  One definition for every entry below, keyed by a DEVICE int64 pair rng = {seed, step}:
 *   block(row, b)  = the four output words w0..w3 of Philox4x32-10 (csrc/common.h) at the counter
 *                    (row, b, step low word, step high word) under the key (seed low word, seed high word);
 *   u_k            = ((w_k >> 9) + 0.5) * 2^-23       in (0, 1), exact in fp32 (the mapping of uavgnn_gumbel_noise);
 *   z0 = r cos(2 pi u1), z1 = r sin(2 pi u1), r = sqrt(-2 ln u0);   z2, z3 the same way from (u2, u3)
 *                    (logf, sqrtf and sincospif(2 u): the accurate routines, no fast intrinsics);
 *   xi_in [row, 4 b  + k] = z_k of block(row, b)             b  < ceil(H / 4)
 *   xi_out[row, 4 b' + k] = z_k of block(row, 0x10000 + b')  b' < ceil(A / 4)
 * Nothing else enters: a value depends on (seed, step, row, column) only, never on the launch geometry.  No entry point advances the
 * step; the caller does, in stream order (an in-place device add replays under hipGraph capture), once per consuming launch.
 */
#ifndef UAVGNN_EXT_H
#define UAVGNN_EXT_H

#include "uavgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* H in {64, 128, 256} and 1 <= A <= 16: the set of uavgnn_head_supported. */
int uavgnn_noisy_head_supported(int H, int A);

/* Mode "rows" in ONE launch: row r of the launch draws xi_in[r, :], xi_out[r, :] of the stream at the pair *rng and
 *   q[r, j] = (sum_k h[r, k] W_mu[j, k] + b_mu[j]) + f_out[r, j] * (sum_k (h[r, k] * f_in[r, k]) W_sigma[j, k] + b_sigma[j]).
 * The schedule of uavgnn_head_fwd - one wavefront per 16-row tile, v_mfma_f32_16x16x4_f32, both weights in registers - with a second
 * accumulator chain whose A operand is h[r, k] * f_in[r, k], rounded once in fp32.  The epilogue is evaluated in exactly the order
 * written above, each operation rounded once (no fused multiply-add).  No LDS, no atomics, plain vector stores: the same operands and
 * the same pair give the same bits.  The noise is never written to memory.
 * h [N, H] (row stride ld_h), W_mu / W_sigma [A, H] (row stride ld_w, shared), b_mu / b_sigma [A], q [N, A] (row stride ld_q).
 * A NULL operand, N < 0 or a stride below the row length: UAVGNN_EINVAL.  (H, A) outside uavgnn_noisy_head_supported, ld_h % 4 != 0,
 * ld_w % 4 != 0, or h / W_mu / W_sigma not 16-byte aligned: UAVGNN_EUNSUPPORTED.  N == 0: 0, nothing is launched.  Rows >= N and
 * columns >= A of q are never written. */
int uavgnn_noisy_head_fwd(const float* h, int ld_h, int N, int H, const float* W_mu, const float* W_sigma, int ld_w, const float* b_mu,
                          const float* b_sigma, int A, const long long* rng, float* q, int ld_q, uavgnn_stream_t stream);

/* The values f(xi) exactly as uavgnn_noisy_head_fwd uses them at the pair *rng (the same bits): f_in [N, H], f_out [N, A], both
 * contiguous; either may be NULL (not written).  Consumes nothing.  Any N >= 0, 1 <= H <= 262144, 1 <= A <= 262144 (the range of the
 * two block indices); UAVGNN_EINVAL otherwise or when rng is NULL.  N == 0: 0, nothing is launched. */
int uavgnn_noisy_noise(const long long* rng, int N, int H, int A, float* f_in, float* f_out, uavgnn_stream_t stream);

/* Mode "shared" in ONE launch: one draw (row 0 of the stream at the pair *rng) folded into effective parameters,
 *   W_eff[j, k] = W_mu[j, k] + W_sigma[j, k] * (f_out[j] * f_in[k]),   b_eff[j] = b_mu[j] + b_sigma[j] * f_out[j],
 * each operation rounded once in fp32 in the order written.  W_mu / W_sigma [A, H] (row stride ld_w >= H), W_eff [A, H] contiguous,
 * b_eff [A]; f_in [H] and f_out [A] receive the draw (what uavgnn_noisy_fold_bwd needs; the bits of uavgnn_noisy_noise's row 0).
 * Any A >= 1 and H >= 1 within the stream's range (above), no alignment requirement.  A NULL operand, A < 1, H < 1 or ld_w < H:
 * UAVGNN_EINVAL. */
int uavgnn_noisy_fold(const float* W_mu, const float* W_sigma, int ld_w, const float* b_mu, const float* b_sigma, int A, int H,
                      const long long* rng, float* W_eff, float* b_eff, float* f_in, float* f_out, uavgnn_stream_t stream);

/* The transpose of the fold with respect to the sigmas (the means' gradients are dW_eff and db_eff themselves):
 *   dW_sigma[j, k] = dW_eff[j, k] * (f_out[j] * f_in[k]),   db_sigma[j] = db_eff[j] * f_out[j],
 * each operation rounded once in fp32.  dW_eff [A, H] (row stride ld >= H), db_eff [A], dW_sigma [A, H] contiguous, db_sigma [A].
 * A NULL operand, A < 1, H < 1 or ld < H: UAVGNN_EINVAL. */
int uavgnn_noisy_fold_bwd(const float* dW_eff, int ld, const float* db_eff, const float* f_in, const float* f_out, int A, int H,
                          float* dW_sigma, float* db_sigma, uavgnn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* UAVGNN_EXT_H */

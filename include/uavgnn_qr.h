/*
 * uavgnn_qr.h - entry points of libuavgnn_qr.so: the distributional (quantile-regression) value head and its TD tail.
 *
 * QR-DQN (Dabney et al., "Distributional Reinforcement Learning with Quantile Regression", AAAI 2018): the head gives K quantile
 * values theta[a, 0..K) per action at the fixed fractions tau_i = (2 i + 1) / (2 K); Q(a) is their mean.  No value support
 * [v_min, v_max] exists anywhere.  The conventions are those of uavgnn_ext.h: every pointer is DEVICE memory, every call is
 * asynchronous on `stream`, the result is 0, a negated hipError_t, or one of uavgnn.h's UAVGNN_E* codes (uavgnn_strerror of the main
 * library names them; this header defines no code of its own).
 *
 * Operands are contiguous fp32 unless said otherwise.  No atomics, plain vector stores: the same operands give the same bits whatever
 * the launch geometry.  K in {8, 16, 32, 64} (powers of two: 1 / K and every tau_i are exact in fp32, a row of quantiles fits a
 * wavefront) and 1 <= A <= 64: the set of uavgnn_qr_supported.
 *
 * Argument errors: a size below 1, a NULL required operand, a wrong G, kappa <= 0 or n_step < 1 give UAVGNN_EINVAL and nothing is
 * launched; (A, K) outside uavgnn_qr_supported gives UAVGNN_EUNSUPPORTED (the entries without an A are asked with A = 1).
 *
 * Fixed orders of summation (csrc/qr/quantile.hip): every sum over k or j of a lane runs in ascending index, one rounding per
 * operation (no contraction into fused multiply-adds); a sum across the K lanes of a row is the butterfly at lane distances
 * K/2, K/4, ..., 1; the loss is the sum of per-workgroup partial sums (each: its rows in ascending order per lane group, the lane
 * groups by the 64-lane butterfly, the four wavefronts in ascending order), added in ascending workgroup order by one workgroup.
 */
#ifndef UAVGNN_QR_H
#define UAVGNN_QR_H

#include "uavgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when 1 <= A <= 64 and K in {8, 16, 32, 64}, else 0. */
int uavgnn_qr_supported(int A, int K);

/* W_bar[a, h] = (sum_k W[a*K + k, h], ascending k) * (1/K); b_bar[a] likewise from b [A*K].
 * W [A*K, H] with row stride ld_w >= H; W_bar [A, H] and b_bar [A] contiguous.  One launch. */
int uavgnn_qr_mean_fold(const float* W, int ld_w, const float* b, int A, int K, int H,
                        float* W_bar, float* b_bar, uavgnn_stream_t stream);

/* theta_pol [T+1, N, A, K], theta_tgt [T, N, A, K], acts [T, N] int64 ->
 *   theta_a   [T, N, K] = theta_pol[t, n, acts[t, n], :]   (NaN for an index outside [0, A); nothing is read there)
 *   next_acts [T, N] int32 (may be NULL) = argmax_a of the per-action quantile sum (ascending k) of theta_pol[t+1] if double_q,
 *                       else of theta_tgt[t]; the first maximum wins, a NaN counts as the maximum (the rule of uavgnn_td_select_fwd)
 *   theta_next[T, N, K] = theta_tgt[t, n, next_acts[t, n], :]
 *   q_pol     [T+1, N, A] (may be NULL) = the policy's per-action means, (sum_k, ascending k) * (1/K). */
int uavgnn_qr_select_fwd(const float* theta_pol, const float* theta_tgt, const long long* acts,
                         int T, long long N, int A, int K, int double_q,
                         float* theta_a, float* theta_next, int* next_acts, float* q_pol,
                         uavgnn_stream_t stream);

/* d_theta_pol [T+1, N, A, K]: EVERY element is written (d_theta_a [T, N, K] at the taken action, exact zeros elsewhere and in all of
 * row T; a row whose action is outside [0, A) is all zeros). */
int uavgnn_qr_select_bwd(const float* d_theta_a, const long long* acts,
                         int T, long long N, int A, int K,
                         float* d_theta_pol, uavgnn_stream_t stream);

/* theta_a, theta_next [T, B, C, K]; rews [T, B, Cr], Cr = 1 or C; dones [T, B, 1]; weights [B] or NULL (= 1);
 * c_t = gamma (1 - done_t); kappa > 0; tau_i = (2 i + 1) / (2 K).
 * n-step target per quantile j, m = min(n_step, T - t) (the definition of UAVGNN_TD_NSTEP), evaluated innermost first:
 *     y_j   = sum_{k<m} (prod_{l<k} c_{t+l}) r_{t+k} + (prod_{l<m} c_{t+l}) theta_next[t+m-1, j]
 *     u_ij  = y_j - theta_i
 *     L(u)  = u^2 / 2 if |u| <= kappa, else kappa (|u| - kappa / 2)
 *     row loss l = sum_i (1/K) sum_j |tau_i - [u_ij < 0]| L(u_ij) / kappa                          (QR-DQN eq. 10)
 *     loss [1]     = sum_rows w_b l / (T B C), two stages in a fixed order through workspace [G]
 *     g [T,B,C,K]  = d loss / d theta_i
 *                  = -(w_b / (T B C)) (1/K) sum_j |tau_i - [u_ij < 0]| clamp(u_ij, -kappa, kappa) / kappa
 *     td [T,B,C]   = mean_i theta_i - mean_j y_j      (the sign of uavgnn_td_return_fwd's q - y; what a priority update consumes)
 * The targets carry no gradient.  G = uavgnn_qr_loss_partials(T, B, C, K). */
int uavgnn_qr_loss_fwd(const float* theta_a, const float* theta_next, const float* rews, int Cr,
                       const float* dones, const float* weights,
                       int T, int B, int C, int K, float gamma, int n_step, float kappa,
                       float* td, float* g, float* loss, float* workspace, int G,
                       uavgnn_stream_t stream);

/* The number of fp32 partial sums uavgnn_qr_loss_fwd needs in `workspace` (>= 1), or an error code (< 0). */
int uavgnn_qr_loss_partials(int T, int B, int C, int K);

#ifdef __cplusplus
}
#endif

#endif /* UAVGNN_QR_H */

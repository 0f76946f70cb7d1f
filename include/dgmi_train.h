/*
 * dgmi_train.h — C ABI of libdgmi.so, part 9: the decoder MLP on a pair list in TRAINING: logits with dropout in one
 * kernel, every gradient from a recompute, nothing of size n_pairs x 128 kept between the two.
 *
 * Same conventions as dgmi.h / dgmi_given.h: device pointers, asynchronous on `stream`, never synchronises, allocates
 * nothing (capturable), returns DGMI_OK or a negative dgmi_status.
 */
#ifndef DGMI_TRAIN_H_
#define DGMI_TRAIN_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------------------------------------------------------------------------
 * Operands as in dgmi_given.h: X (n_query, 128) and C (n_cand, 128) fp32 with leading dimensions ldx / ldc, W2 (64, 128)
 * row-major, b2 and w3 64 floats, b3 ONE float, the list (pair_query[e], pair_cand[e]), e < n_pairs, int32 ids in any
 * order, duplicates allowed.  h1, h2 name the two widths; only 128 / 64 are taken.
 *
 *   h1[e, k] = m1[e, k] relu(X[q_e, k] + C[c_e, k])                          k < 128
 *   z2[e, h] = b2[h] + sum_k W2[h, k] h1[e, k],   h2[e, h] = m2[e, h] relu(z2[e, h])     h < 64
 *   logit[e] = b3 + sum_h w3[h] h2[e, h]
 * with the dropout factors m_l[e, j] = 1 / (1 - p) where keep(seed, l, e, j) and 0 elsewhere.  keep is a pure function
 * of the seed, the layer, the list POSITION e and the unit j (csrc/dgmi_pair_dropout.h: a 32-bit hash below
 * floor((1 - p) 2^32)); 1 / (1 - p) is rounded once to fp32.  The seed is ONE int64 read from device memory (seed_dev) by
 * the kernels, so a captured launch draws a new mask whenever the caller has written a new seed before a replay.  With
 * p = 0 every logit is bit-identical to dgmi_pair_mlp_score_list_f32's for the same operands.
 *
 * Non-finite operands.  A DROPPED unit is exactly 0, whatever value lies under it: the factor 0 is a select, not a
 * product, so a NaN or an Inf in X or C does not pass a dropped unit, forward or backward.  A KEPT unit follows IEEE:
 * relu keeps NaN (relu(NaN) = NaN, relu(+Inf) = +Inf, relu(-Inf) = 0), 0 * Inf and Inf - Inf are NaN, and the sums
 * carry them on.  The relu gate of the backward is [z > 0], which is false for NaN.  A pair whose every non-finite unit
 * is dropped therefore has a finite logit and finite dz1; one pair's values never reach another pair's logit or dz1
 * row.  out_dW2 and out_dw3 are sums over the pairs and follow IEEE too: a kept non-finite h1[e, k] (h2[e, h]) makes
 * column k of out_dW2 (entry h of out_dw3) NaN even where dlogit[e] = 0, because 0 * NaN is NaN.  This is NOT the torch
 * chain, whose dropout multiplies by a mask (NaN * 0 = NaN under a dropped unit as well).
 *
 * dgmi_pair_mlp_train_forward_f32: out_logit[e], e < n_pairs.  A listed pair with an id outside
 * [0, n_query) x [0, n_cand) reads nothing, sets out_info[0] = 1 and gets logit NaN; out_info is 2 int32, cleared first.
 *
 * dgmi_pair_mlp_train_backward_f32: given the forward's operands, p, the seed and dlogit[e] = dLoss / dlogit[e], with
 *   dz2[e, h] = dlogit[e] w3[h] m2[e, h] [z2[e, h] > 0],   dz1[e, k] = m1[e, k] [X + C > 0] sum_h W2[h, k] dz2[e, h]:
 *   out_dz1 (n_pairs, 128) fp32, leading dimension ld_dz1: dz1, the gradient of both X[q_e] and C[c_e] (the caller's
 *           segment sums over the list give dX and dC)
 *   out_dW2 (64, 128) = sum_e dz2[e] h1[e]^T,  out_db2 (64) = sum_e dz2[e],  out_dw3 (64) = sum_e dlogit[e] h2[e],
 *   out_db3 (1) = sum_e dlogit[e].
 * A pair out of range contributes nothing, gets a zero dz1 row and sets out_info[0] = 1.  Sums: every workgroup adds
 * the list blocks of a static assignment in a fixed order and writes its partial sums to the workspace, and one small
 * kernel adds the partials in a fixed order of workgroups.  No float atomics: the results are the same bits from run to run.
 * The workspace also holds dz2 (n_pairs x 64 fp32) between the two recompute kernels.
 *
 * Errors, returned before any launch: DGMI_ERR_INVALID_ARG for a null pointer, widths other than 128 / 64, ldx, ldc or
 * ld_dz1 < 128 or not a multiple of 4, X / C / W2 / out_dz1 not 16-byte aligned, p outside [0, 1) (NaN included),
 * n_query, n_cand or n_pairs negative or beyond int32; DGMI_ERR_WORKSPACE (backward only) for a workspace below
 * dgmi_pair_mlp_train_workspace_bytes(n_pairs).  n_pairs = 0 returns DGMI_OK: the forward writes nothing, the backward
 * writes zeros to out_dW2 / out_db2 / out_dw3 / out_db3 and needs no workspace.  The workspace size is monotone in
 * n_pairs, and 0 for n_pairs <= 0 or beyond int32.
 * ------------------------------------------------------------------------- */
DGMI_API size_t dgmi_pair_mlp_train_workspace_bytes(int64_t n_pairs);
DGMI_API int dgmi_pair_mlp_train_forward_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                             int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                             const float* w3, const float* b3, const int32_t* pair_query,
                                             const int32_t* pair_cand, int64_t n_pairs, float p, const int64_t* seed_dev,
                                             float* out_logit, int32_t* out_info, dgmi_stream_t stream);
DGMI_API int dgmi_pair_mlp_train_backward_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                              int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                              const float* w3, const float* b3, const int32_t* pair_query,
                                              const int32_t* pair_cand, int64_t n_pairs, float p, const int64_t* seed_dev,
                                              const float* dlogit, float* out_dz1, int64_t ld_dz1, float* out_dW2,
                                              float* out_db2, float* out_dw3, float* out_db3, int32_t* out_info,
                                              void* workspace, size_t workspace_bytes, dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_TRAIN_H_ */

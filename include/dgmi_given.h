/*
 * dgmi_given.h — C ABI of libdgmi.so, part 6: the trained decoder on GIVEN drug-disease pairs.
 *
 * The reverse of dgmi_pairs.h / dgmi_rank.h / dgmi_above.h, which answer "which pairs are best": here the caller names
 * the pairs and gets each pair's logit and its filtered position among all candidates of its query row, the quantity
 * behind hits@k and MRR.  Same conventions as dgmi.h: device pointers, asynchronous on `stream`, never synchronises,
 * allocates nothing (capturable), returns DGMI_OK or a negative dgmi_status.
 */
#ifndef DGMI_GIVEN_H_
#define DGMI_GIVEN_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------------------------------------------------------------------------
 * The decoder MLP on a list of (query, candidate) pairs.
 *
 *   X: (n_query, 128) fp32, leading dimension ldx: the query side (Q to rank a pair among all drugs of its disease, P
 *      to rank it among all diseases of its drug)
 *   C: (n_cand, 128)  fp32, leading dimension ldc: the candidate side (the other one)
 *   with P = hd W1[:, :F]^T + b1 and Q = hs W1[:, F:]^T (MLPDecoder.lin1 split), a pair (q, c) scores
 *   logit(q, c) = b3 + sum_{h<64} w3[h] relu(b2[h] + sum_{k<128} W2[h, k] relu(X[q, k] + C[c, k]))
 *   W2: (64, 128) row-major (lin2.weight); b2, w3: 64 floats; b3: ONE float (device pointer: no host read).
 * h1, h2 name the two widths; only 128 / 64 are taken.  Every logit is bit-identical to the one
 * dgmi_pair_mlp_topk_f32, dgmi_pair_mlp_row_topk_f32 and dgmi_pair_mlp_emit_f32 compute for the same pair.
 *
 * The list: (pair_query[e], pair_cand[e]), e < n_pairs, int32 ids in any order; duplicates are allowed and get equal
 * results.  A listed pair with an id outside [0, n_query) x [0, n_cand) reads nothing, sets out_info[0] = 1 and gets
 * logit NaN, above = total = -1; the other pairs of the list still get their results.
 *
 * dgmi_pair_mlp_score_list_f32: out_logit[e] = logit(pair e).  n_pairs scores.
 *
 * dgmi_pair_mlp_rank_list_f32: out_logit as above and, over the candidates c' != pair_cand[e] with
 * (pair_query[e], c') NOT in the known list (known_query[i], known_cand[i]), i < n_known (int32 COO ids in any order,
 * duplicates allowed; n_known = 0 takes every candidate):
 *   out_total[e] = how many such c' there are,
 *   out_above[e] = how many of them rank before the listed pair in the order of dgmi_rank.h: logit descending, ties
 *                  by candidate id ascending, NaN after every number, -0 equal to +0.
 * The listed pair never counts itself, and whether it is in the known list changes nothing (the filtered protocol: a
 * held-out positive is normally part of the association matrix).  So out_above[e] + 1 is the pair's filtered rank and
 * out_total[e] + 1 the length of the list it is ranked in.  A known id outside [0, n_query) x [0, n_cand) is skipped
 * and sets out_info[1] = 1; it never faults.  Cost: n_pairs x n_cand scores, every listed pair scans its whole row;
 * the counters are integers, so the results do not depend on scheduling.
 *
 * Errors, returned before any launch: DGMI_ERR_INVALID_ARG for a null pointer, ldx or ldc < 128 or not a multiple
 * of 4, X / C / W2 not 16-byte aligned, widths other than 128 / 64, n_query, n_cand or n_pairs beyond int32, a
 * negative count, n_known > 0 without ids; DGMI_ERR_WORKSPACE (rank_list only) for a workspace below
 * dgmi_pair_rank_workspace_bytes(n_query, n_cand, n_pairs): the known-pair bitmap, one bit per (candidate, query).
 * n_pairs = 0 returns DGMI_OK and writes nothing; with n_query = 0 or n_cand = 0 every listed pair is out of range
 * and no workspace is needed.  The workspace size is 0 for invalid or empty inputs.
 * ------------------------------------------------------------------------- */
DGMI_API size_t dgmi_pair_rank_workspace_bytes(int64_t n_query, int64_t n_cand, int64_t n_pairs);
DGMI_API int dgmi_pair_mlp_score_list_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                          int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                          const float* w3, const float* b3, const int32_t* pair_query,
                                          const int32_t* pair_cand, int64_t n_pairs, float* out_logit, int32_t* out_info,
                                          dgmi_stream_t stream);
DGMI_API int dgmi_pair_mlp_rank_list_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                         int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                         const float* w3, const float* b3, const int32_t* pair_query,
                                         const int32_t* pair_cand, int64_t n_pairs, const int32_t* known_query,
                                         const int32_t* known_cand, int64_t n_known, float* out_logit, int32_t* out_above,
                                         int32_t* out_total, int32_t* out_info, void* workspace, size_t workspace_bytes,
                                         dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_GIVEN_H_ */

/*
 * dgmi_rank.h — C ABI of libdgmi.so, part 3: per-row rankings of drug-disease pairs with the trained decoder.
 *
 * The per-entity counterpart of dgmi_pairs.h: for every disease, the drugs that fit it best (or for every drug, its
 * best new indications), instead of the k best pairs of the whole matrix.  Same conventions as dgmi.h: device
 * pointers, asynchronous on `stream`, never synchronises, allocates nothing, returns DGMI_OK or a negative
 * dgmi_status.
 */
#ifndef DGMI_RANK_H_
#define DGMI_RANK_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest k per row the on-chip top-k takes */
#define DGMI_ROW_TOPK_MAX_K 128

/* -------------------------------------------------------------------------
 * All-pairs decoder MLP with a fused top-k per query row.
 *
 *   X: (n_query, 128) fp32, leading dimension ldx: the query side (P for per-drug lists, Q for per-disease lists)
 *   C: (n_cand, 128)  fp32, leading dimension ldc: the candidate side (the other one)
 *   with P = hd W1[:, :F]^T + b1 and Q = hs W1[:, F:]^T (MLPDecoder.lin1 split), every pair (q, c) scores
 *   logit(q, c) = b3 + sum_{h<64} w3[h] relu(b2[h] + sum_{k<128} W2[h, k] relu(X[q, k] + C[c, k]))
 *   W2: (64, 128) row-major (lin2.weight); b2, w3: 64 floats; b3: ONE float (device pointer: no host read).
 * h1, h2 name the two widths; only 128 / 64 are taken.  Every logit is bit-identical to the one
 * dgmi_pair_mlp_topk_f32 computes for the same (drug, disease) pair.
 *
 * Candidates of row q are the c with (q, c) NOT in the known list (known_query[e], known_cand[e]), e < n_known:
 * int32 COO ids in any order, duplicates allowed; n_known = 0 takes every pair.  A known id outside
 * [0, n_query) x [0, n_cand) is skipped and sets out_info[1] = 1; it never faults.
 *
 * Result, per query row q: the min(k, #candidates of q) candidates with the largest logit, ordered by logit
 * descending, ties by candidate id ascending; NaN logits rank after every number.  out_cand[q k + r] and
 * out_logit[q k + r] for r < out_count[q]; the slots past the count hold id -1 and logit NaN.
 * out_info[0] = the sum of the counts, out_info[1] = the out-of-range flag.
 *
 * Errors, returned before any launch: DGMI_ERR_INVALID_ARG for a null pointer, ldx or ldc < 128 or not a multiple
 * of 4, X / C / W2 not 16-byte aligned, widths other than 128 / 64, k outside 1..DGMI_ROW_TOPK_MAX_K, n_query or
 * n_cand beyond int32, a negative count, n_known > 0 without ids; DGMI_ERR_WORKSPACE for a workspace below
 * dgmi_row_topk_workspace_bytes(n_query, n_cand, k).  n_query = 0 returns DGMI_OK and writes nothing; n_cand = 0
 * writes counts of 0 (and the padding) and needs no workspace.  The workspace size is 0 for invalid or empty inputs.
 * ------------------------------------------------------------------------- */
DGMI_API size_t dgmi_row_topk_workspace_bytes(int64_t n_query, int64_t n_cand, int32_t k);
DGMI_API int dgmi_pair_mlp_row_topk_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                        int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                        const float* w3, const float* b3, const int32_t* known_query,
                                        const int32_t* known_cand, int64_t n_known, int32_t k, int32_t* out_cand,
                                        float* out_logit, int32_t* out_count, int32_t* out_info, void* workspace,
                                        size_t workspace_bytes, dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_RANK_H_ */

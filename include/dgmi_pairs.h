/*
 * dgmi_pairs.h — C ABI of libdgmi.so, part 2: ranking drug-disease pairs with the trained decoder.
 *
 * Replaces the scoring loop of the reference's get_top_novel_predictions (train.py:26-151): every pair
 * that is not a known association is scored by the decoder MLP (layers.py:341-375, eval mode) and the
 * k best are returned.  Same conventions as dgmi.h: device pointers, asynchronous on `stream`, never
 * synchronises, allocates nothing, returns DGMI_OK or a negative dgmi_status.
 */
#ifndef DGMI_PAIRS_H_
#define DGMI_PAIRS_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest k the on-chip top-k takes */
#define DGMI_PAIR_TOPK_MAX_K 1024

/* -------------------------------------------------------------------------
 * All-pairs decoder MLP with a fused top-k.
 *
 *   P: (n_drug, 128) fp32, leading dimension ldp = hd W1[:, :F]^T + b1   (MLPDecoder.lin1 split)
 *   Q: (n_dis, 128)  fp32, leading dimension ldq = hs W1[:, F:]^T
 *   logit(i, j) = b3 + sum_{h<64} w3[h] relu(b2[h] + sum_{k<128} W2[h, k] relu(P[i, k] + Q[j, k]))
 *   W2: (64, 128) row-major (lin2.weight); b2, w3: 64 floats; b3: ONE float (device pointer: no host read).
 * h1, h2 name the two widths; only 128 / 64 are taken (the widths of the reference decoder).
 * Every logit is exact fp32 arithmetic (f32 MFMA, f32 FMA): the same bits run to run.
 *
 * Candidates are the pairs (i, j) NOT in the known list (known_drug[e], known_dis[e]), e < n_known: int32
 * COO ids in any order, duplicates allowed; n_known = 0 takes every pair.  A known id outside
 * [0, n_drug) x [0, n_dis) is skipped and sets out_info[1] = 1; it never faults.
 *
 * Result: the min(k, #candidates) candidates with the largest logit, ordered by logit descending, ties by
 * (drug, disease) ascending; NaN logits rank after every number.  out_drug / out_dis / out_logit hold k
 * entries each; out_info[0] = the number returned, out_info[1] = the out-of-range flag.
 *
 * Errors, returned before any launch: DGMI_ERR_INVALID_ARG for a null pointer, ldp or ldq < 128 or not a
 * multiple of 4, P / Q / W2 not 16-byte aligned, widths other than 128 / 64, k outside
 * 1..DGMI_PAIR_TOPK_MAX_K, n_drug or n_dis beyond int32, a negative count; DGMI_ERR_WORKSPACE for a
 * workspace below dgmi_pair_topk_workspace_bytes(n_drug, n_dis, k).  An empty problem (n_drug or n_dis 0)
 * returns DGMI_OK and writes nothing.
 * ------------------------------------------------------------------------- */
DGMI_API size_t dgmi_pair_topk_workspace_bytes(int64_t n_drug, int64_t n_dis, int32_t k);
DGMI_API int dgmi_pair_mlp_topk_f32(const float* P, int64_t ldp, int64_t n_drug, const float* Q, int64_t ldq,
                                    int64_t n_dis, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                    const float* w3, const float* b3, const int32_t* known_drug,
                                    const int32_t* known_dis, int64_t n_known, int32_t k, int32_t* out_drug,
                                    int32_t* out_dis, float* out_logit, int32_t* out_info, void* workspace,
                                    size_t workspace_bytes, dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_PAIRS_H_ */

/*
 * dgmi_above.h — C ABI of libdgmi.so, part 4: listing every novel drug-disease pair at or above a score cut.
 *
 * The threshold counterpart of dgmi_pairs.h: instead of the k <= 1024 best pairs kept on chip, every pair that is not
 * a known association and whose decoder logit reaches a cut is appended to a device buffer, and an exact 64-bit count
 * is kept.  A record sort puts the buffer into the documented order; together they also carry a top-k beyond 1024
 * (MLPDecoder.top_pairs_deep).  Same conventions as dgmi.h: device pointers, asynchronous on `stream`, never
 * synchronises, allocates nothing, returns DGMI_OK or a negative dgmi_status.
 */
#ifndef DGMI_ABOVE_H_
#define DGMI_ABOVE_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest record buffer an emit pass fills, and the largest n the record sort takes */
#define DGMI_PAIR_EMIT_MAX_RECORDS (1 << 24)

/* -------------------------------------------------------------------------
 * All-pairs decoder MLP with a streaming emit of the pairs at or above a cut.
 *
 * P, Q, W2, b2, w3, b3, h1, h2, the known list and out_info[1] are those of dgmi_pair_mlp_topk_f32 (dgmi_pairs.h),
 * and every logit is bit-identical to the one that function and dgmi_pair_mlp_row_topk_f32 return for the pair.
 *
 * A pair (i, j) qualifies iff it is not known and key(logit) >= key(min_logit), key being the ranking key of the
 * top-k functions.  For a numeric cut this is logit >= min_logit in fp32: inclusive, -0 and +0 one value, and a NaN
 * logit never qualifies (min_logit = -inf included).  A NaN min_logit has the lowest key and selects EVERY novel
 * pair, NaN logits included: the way to say "everything".
 *
 * out_count[0] (int64) = the number of qualifying pairs, exact whatever the capacity.  The first
 * min(out_count[0], capacity) slots of out_drug / out_dis / out_logit receive records, in an order that depends on
 * scheduling (sort them with dgmi_pair_records_sort_f32); nothing is written at or past `capacity`.  When the count
 * exceeds the capacity, the stored records are an unspecified subset of the qualifying pairs.  capacity = 0 is the
 * count-only query; the three record pointers may then be null.  A returned logit is the canonical value of its key,
 * as in the top-k functions: -0 comes back as +0, a NaN as the default quiet NaN.
 * out_info: two int32; out_info[0] = 0, out_info[1] = the out-of-range flag of the known list.
 *
 * Errors, returned before any launch: DGMI_ERR_INVALID_ARG for a null pointer (the record pointers only when
 * capacity > 0), ldp or ldq < 128 or not a multiple of 4, P / Q / W2 not 16-byte aligned, widths other than 128 / 64,
 * capacity outside 0..DGMI_PAIR_EMIT_MAX_RECORDS, n_drug or n_dis beyond int32, a negative count, n_known > 0 without
 * ids; DGMI_ERR_WORKSPACE for a workspace below dgmi_pair_emit_workspace_bytes(n_drug, n_dis).  An empty problem
 * (n_drug or n_dis 0) needs no P, Q or workspace and stores a count of 0.  The workspace size is 0 for invalid or
 * empty inputs.
 * ------------------------------------------------------------------------- */
DGMI_API size_t dgmi_pair_emit_workspace_bytes(int64_t n_drug, int64_t n_dis);
DGMI_API int dgmi_pair_mlp_emit_f32(const float* P, int64_t ldp, int64_t n_drug, const float* Q, int64_t ldq,
                                    int64_t n_dis, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                    const float* w3, const float* b3, const int32_t* known_drug,
                                    const int32_t* known_dis, int64_t n_known, float min_logit, int64_t capacity,
                                    int32_t* out_drug, int32_t* out_dis, float* out_logit, int64_t* out_count,
                                    int32_t* out_info, void* workspace, size_t workspace_bytes, dgmi_stream_t stream);

/* -------------------------------------------------------------------------
 * Sort n (drug, dis, logit) records in place into the ranking order: logit descending, ties by (drug, dis) ascending,
 * NaN logits after every number (among themselves by id); -0 and +0 tie.  A stable LSD radix sort on the device; the
 * result is a function of the multiset of records alone.  Ids must be non-negative.  Logits come back canonical (see
 * above).  n is a host value, 0..DGMI_PAIR_EMIT_MAX_RECORDS; n = 0 returns DGMI_OK and touches nothing.
 * DGMI_ERR_INVALID_ARG for a null pointer or n out of range, DGMI_ERR_WORKSPACE for a workspace below
 * dgmi_pair_records_sort_workspace_bytes(n) (0 for n out of range or 0).
 * ------------------------------------------------------------------------- */
DGMI_API size_t dgmi_pair_records_sort_workspace_bytes(int64_t n);
DGMI_API int dgmi_pair_records_sort_f32(int32_t* drug, int32_t* dis, float* logit, int64_t n, void* workspace,
                                        size_t workspace_bytes, dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_ABOVE_H_ */

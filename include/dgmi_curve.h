/*
 * dgmi_curve.h — C ABI of libdgmi.so, part 7: exact ROC / precision-recall areas of scored samples on the device.
 *
 * The metric lines of the reference's evaluation (evaluation.py:55-65: `auc(*roc_curve)`, `auc(recall, precision)`, the
 * 0.5 cut behind accuracy and F1) without the device-to-host copy and the host sort, overall or per segment (per
 * disease, per drug).  Same conventions as dgmi.h: device pointers, asynchronous on `stream`, never synchronises,
 * allocates nothing (capturable), inputs are not modified, returns DGMI_OK or a negative dgmi_status.
 */
#ifndef DGMI_CURVE_H_
#define DGMI_CURVE_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------------------------------------------------------------------------
 * n samples: score[i] fp32, label[i] fp32, and with n_segments > 0 an int32 segment[i] in [0, n_segments).
 * n_segments = 0: no segments (`segment` is not read and may be NULL), everything is segment 0 and S = 1; otherwise
 * S = n_segments.
 *
 * Inside a segment the samples are grouped by the ranking key of their score (the order of dgmi_rank.h): -0 and +0
 * are one value, every NaN is one group below all numbers.  Groups in descending key order, g = 1..G, hold p_g
 * positives and n_g negatives; TP_g, FP_g are the running sums (TP_0 = FP_0 = 0), P = TP_G, N = FP_G.
 *   U2    = sum_g n_g (2 TP_{g-1} + p_g)                                   int64, exact
 *   auroc = (double)U2 / (double)(2 P N)                                   NaN iff P N = 0
 *   aupr  = (1 / (2 P)) sum_g p_g (pi_g + pi_{g-1}),  pi_g = TP_g / (TP_g + FP_g) in float64, pi_0 = 1
 *                                                                          NaN iff P = 0
 *   TPt, FPt = the positives / negatives with score >= threshold, compared in fp32; a NaN score never qualifies and a
 *   NaN threshold admits nothing.
 * auroc is the trapezoid area of the ROC curve over the distinct thresholds with its (0, 0) start point; aupr is the
 * trapezoid area of precision over recall with the (recall 0, precision 1) end point.
 *
 * out_count: S x 6 int64, row s = (P, N, TPt, FPt, G, U2) of segment s.   out_area: S x 2 float64, (auroc, aupr).
 * out_info[0], flags that are never an error code and never cause a fault:
 *   bit 0  some score is NaN
 *   bit 1  some label is neither 0.0 nor 1.0; such a label counts as positive iff it is != 0
 *   bit 2  some segment id is outside [0, n_segments); that sample is left out of every segment
 *
 * The integer outputs are functions of the input multiset.  The float64 sum behind aupr is evaluated in an order fixed
 * by the sorted sequence and the kernels' fixed tiling, without floating-point atomics: two runs, and any permutation
 * of the samples, give the same bits.
 *
 * Errors, returned before any launch: DGMI_ERR_INVALID_ARG for a null score / label / out_count / out_area / out_info,
 * n < 0 or n >= 2^31, n_segments < 0 or > 2^24, segment == NULL with n_segments > 0; DGMI_ERR_WORKSPACE for a
 * workspace below dgmi_curve_areas_workspace_bytes(n, n_segments).  score and label may be NULL when n = 0.
 * n = 0 writes zeros and NaN areas for every segment and returns DGMI_OK.  The workspace size is 0 for invalid input.
 * ------------------------------------------------------------------------- */
#define DGMI_CURVE_MAX_SEGMENTS (1 << 24)

DGMI_API size_t dgmi_curve_areas_workspace_bytes(int64_t n, int64_t n_segments);
DGMI_API int dgmi_curve_areas_f32(const float* score, const float* label, const int32_t* segment, int64_t n,
                                  int64_t n_segments, float threshold, int64_t* out_count, double* out_area,
                                  int32_t* out_info, void* workspace, size_t workspace_bytes, dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_CURVE_H_ */

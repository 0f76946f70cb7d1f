/*
 * dgmi_bf16.h — C ABI of libdgmi.so, part 5: the XCD-local SpMM gathering from a bf16 copy of the feature table.
 *
 * Mixed-precision message passing: only the gathered operand is bf16 — rounded once, round-to-nearest-even, after the
 * source scale has been multiplied in fp32 —; products, sums, partial planes and the output stay fp32:
 *
 *   xb[j] = bf16_rne(src_scale[j] * X[j])                                   dgmi_rows_to_bf16
 *   Y[i]  = dst_scale[i] * sum_{e: dst(e) = i} w_e * float(xb[src(e)])      dgmi_spmm_sliced_bf16
 *
 * w_e is 1, vals[e], or the multiplicity carried in the id word (dgmi.h, dgmi_spmm_sliced_f32).  The sum of a row is
 * taken in exactly the order dgmi_spmm_sliced_f32 takes it, so the result is reproducible bit for bit and equals that
 * function's result on the upcast table whenever both run with the same rows per lane group and row chunks.
 * A gathered row is 2F bytes instead of 4F.
 *
 * Same conventions as dgmi.h: device pointers, asynchronous on `stream`, never synchronises, allocates nothing, returns
 * DGMI_OK or a negative dgmi_status.  bf16 values travel as their 16-bit patterns (uint16_t).
 */
#ifndef DGMI_BF16_H_
#define DGMI_BF16_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------------------------------------------------------------------------
 * out[r, c] = bf16_rne(scale[r] * X[r, c]) for r < n, c < F; scale may be null (no scaling).  One streaming pass: the
 * table is read once and half of it written.  The product is taken in fp32 and rounded once; the result is, bit for
 * bit, what an IEEE fp32 -> bf16 round-to-nearest-even conversion gives for every finite value, the infinities and
 * denormals (values beyond the largest bf16 round to infinity); a NaN stays a NaN with an unspecified payload.
 * ldx / ldo: leading dimensions of X / out in elements.
 *
 * DGMI_ERR_INVALID_ARG: negative size, null X / out on a non-empty problem, F % 8 != 0, ldx < F or ldx % 4 != 0,
 * ldo < F or ldo % 8 != 0, X or out not 16-byte aligned.  DGMI_ERR_TOO_LARGE: F beyond int32.  n == 0 or F == 0
 * returns DGMI_OK and touches nothing.
 * ------------------------------------------------------------------------- */
DGMI_API int dgmi_rows_to_bf16(const float* X, int64_t ldx, const float* scale, int64_t n, int64_t F, uint16_t* out,
                               int64_t ldo, dgmi_stream_t stream);

/* -------------------------------------------------------------------------
 * The XCD-local product over a source-sliced layout (dgmi_csr_sliced_from_coo_i32 / _from_csr_i32) with a bf16 table.
 * The argument list is that of dgmi_spmm_sliced_f32 without src_scale (it belongs to dgmi_rows_to_bf16): X holds
 * n_src rows of F bf16 values with leading dimension ldx (elements); every other argument — vals, eid / keep / n_keep
 * (edge dropout on the fly), dst_scale, column_passes, id_multiplicity, the epilogue — means what it means there.
 * `planes` is fp32 scratch of dgmi_spmm_sliced_planes_bytes(n_dst, n_slices, F) bytes, as for the fp32 product.  It is
 * always required, but may go unused: a product the library runs in its workgroup-owned form (rows summed in LDS, one
 * launch; the same bits) writes no planes.
 *
 * DGMI_ERR_INVALID_ARG (never a fault) unless F % 8 == 0, ldx >= F, ldx % 8 == 0, ldy >= F, ldy % 4 == 0 and X, Y and
 * planes are 16-byte aligned; and for everything dgmi_spmm_sliced_f32 refuses.  DGMI_ERR_WORKSPACE for short planes.
 * ------------------------------------------------------------------------- */
DGMI_API int dgmi_spmm_sliced_bf16(const int32_t* segptr, const int32_t* indices, const float* vals, const int32_t* eid,
                                   const uint32_t* keep, int32_t n_keep, const uint16_t* X, int64_t ldx,
                                   const float* dst_scale, float* Y, int64_t ldy, int64_t n_dst, int64_t n_src, int64_t F,
                                   int32_t n_slices, int32_t column_passes, int32_t id_multiplicity, void* planes,
                                   size_t planes_bytes, int32_t act, float act_slope, const float* out_mask,
                                   int64_t ld_mask, float out_mask_scale, dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_BF16_H_ */

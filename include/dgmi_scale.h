/*
 * dgmi_scale.h — C ABI of libdgmi.so: the workgroup-owned XCD-local product with the scale of the gathered rows as a
 * CODE in the id words, Y = diag(dst_scale) A diag(src_scale) X without the pass that scales X beforehand.
 *
 * Where src_scale is a node constant (a degree normalisation fixed with the graph) the caller binds it to the id words
 * once: src_scale takes at most 2^DGMI_SCALE_CODE_BITS distinct bit patterns, table[code] lists them, and the id word
 * of an edge is  src | code(src) << DGMI_SCALE_CODE_SHIFT  (| (m - 1) << 28 with multiplicities, as
 * dgmi_spmm_sliced_f32's id_multiplicity).  The kernel keeps the table in LDS and multiplies each gathered row by its
 * entry, rounded once, before the row joins the sum: bit for bit the product dgmi_scale_rows_f32 followed by
 * dgmi_spmm_sliced_f32 gives on the same layout.
 *
 * Only the owned form's scaled kernel masks such id words.  It is built for an fp32 table in the form of one 16-wave
 * workgroup per CU, for the lane-group widths its measured product classes run at; every other product is declined,
 * and coded id words must never be handed to another entry point.
 *
 * Same conventions as dgmi.h.
 */
#ifndef DGMI_SCALE_H_
#define DGMI_SCALE_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DGMI_SCALE_CODE_SHIFT 17 /* ids are < 2^17 */
#define DGMI_SCALE_CODE_BITS 11  /* at most 2048 table entries */

/* -------------------------------------------------------------------------
 * 1 when dgmi_spmm_owned_scaled_f32 would run the product of these arguments, 0 when it would decline it.  Host
 * arithmetic only: no launch, no stream, no allocation.  It declines: n_src > 2^17, n_codes outside 1 .. 2048, a
 * product the owned form does not take under the current launch parameters (`sliced_owned`, dgmi_set_tuning) or whose
 * class keeps the pre-scale pass (`sliced_owned_scaled`: 0 = decline everything, 1 = every product the kernel is built
 * for, -1 = the measured classes — and, while `sliced_owned` = 1 forces the form, all it is built for), a lane-group width the kernel is not built at, a table of 4 GiB or more, a forced
 * phase gate or two-workgroup form, and an LDS plan without room for the 8 KiB table.
 * ------------------------------------------------------------------------- */
DGMI_API int32_t dgmi_spmm_owned_scaled_takes(int64_t n_dst, int64_t n_src, int64_t F, int64_t ldx, int32_t n_slices,
                                              int32_t id_multiplicity, int32_t n_codes);

/* -------------------------------------------------------------------------
 * Y[n_dst, F] = diag(dst_scale) A diag(table[code]) X over a layout of dgmi_csr_sliced_from_coo_i32 / _from_csr_i32
 * whose id words `coded_indices` carry the codes (above).  X, Y, F, ldx, ldy, dst_scale (nullable), n_slices,
 * id_multiplicity and the epilogue as dgmi_spmm_sliced_f32; no value stream, no edge dropout, no workspace.
 * `table`: n_codes floats on the device.
 *
 * *taken = 1: the product was launched.  *taken = 0 with DGMI_OK: declined (dgmi_spmm_owned_scaled_takes), nothing was
 * launched and Y is untouched — the caller runs dgmi_scale_rows_f32 + dgmi_spmm_sliced_f32 on the PLAIN id words.
 * ------------------------------------------------------------------------- */
DGMI_API int dgmi_spmm_owned_scaled_f32(const int32_t* segptr, const int32_t* coded_indices, const float* X, int64_t ldx,
                                        const float* table, int32_t n_codes, const float* dst_scale, float* Y, int64_t ldy,
                                        int64_t n_dst, int64_t n_src, int64_t F, int32_t n_slices, int32_t id_multiplicity,
                                        int32_t act, float act_slope, const float* out_mask, int64_t ld_mask,
                                        float out_mask_scale, int32_t* taken, dgmi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_SCALE_H_ */

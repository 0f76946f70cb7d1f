/*
 * dgmi_layout.h — C ABI of libdgmi.so, part 7: how many source slices the layout of an XCD-local product should have.
 *
 * dgmi_csr_sliced_from_coo_i32 / _from_csr_i32 build a layout of any slice count up to 64, and dgmi_spmm_sliced_f32 runs
 * on any of them.  The pair of launches (gather into planes, plane reduce) pins one slice to each of the 8 XCDs, so its
 * layouts have 8.  The workgroup-owned form (rows summed in LDS, no planes) walks the slices one after the other and
 * takes any count; for one measured class of products a layout of 16 slices, each small enough for an L2 at full width,
 * is faster.  A caller that owns the layouts asks this function before it builds one.
 *
 * Same conventions as dgmi.h.  Host arithmetic only: no launch, no stream, no allocation.
 */
#ifndef DGMI_LAYOUT_H_
#define DGMI_LAYOUT_H_

#include "dgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -------------------------------------------------------------------------
 * The slice count of the layout for the plain fp32 product Y[n_dst, F] = A X[n_src, F] — unit edge values, or
 * (id_multiplicity = 1) integer multiplicities in the id words; no value stream, no in-kernel src_scale, no edge
 * dropout on the fly: products with one of those run the pair, on a layout of 8 slices.
 *
 * Returns 8 for every shape but the measured class (unit values, a table of 48-64 MiB whose 16 slices give the owned
 * form one column round and one row round with one workgroup per CU: 100 000 sources -> 50 000 rows at F = 128), for
 * which it returns 16.  The launch-parameter override `sliced_owned_slices` (dgmi_set_tuning; 0 = this rule) forces a
 * count for every shape the owned form can plan at that count.  Always 8 when the owned form is switched off
 * (`sliced_owned` = 0), when row chunking is forced, and for arguments the product would refuse.
 * The answer is a speed matter only: the product of a layout is correct at any slice count.
 * ------------------------------------------------------------------------- */
DGMI_API int32_t dgmi_sliced_layout_slices(int64_t n_dst, int64_t n_src, int64_t F, int32_t id_multiplicity);

#ifdef __cplusplus
}
#endif

#endif /* DGMI_LAYOUT_H_ */

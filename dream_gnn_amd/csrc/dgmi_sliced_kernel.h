// dgmi_sliced_kernel.h — the one gather body of the XCD-local SpMM (dgmi_sliced.hip), whatever the element type of the
// gathered table: the run lookup, the row boundaries, the id prefetch, KEEP, the multiplicities, the fast path and the
// boundary path.  What differs between an fp32 and a bf16 table — the columns a lane owns, the registers of a gathered
// row, the sums and how a batch joins them, the stores of a plane row — is a ROW POLICY (SlicedRowF32, SlicedRowBf16)
// over the members the workgroup-owned form's policies use too (RowF32, RowBf16: dgmi_sliced_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgmi_sliced_common.h"

namespace dgmi {
namespace {

// An fp32 table: a lane owns 4 columns, a lane group up to 256.
struct SlicedRowF32 : RowF32 {
  static constexpr bool kSrcScale = true;  // the forms with a per-source scale are built

  static __device__ __forceinline__ Reg none() { return make_float4(0.f, 0.f, 0.f, 0.f); }

  // the canonical step, edge by edge (the four columns are the ILP)
  template <bool WEIGHTED>
  static __device__ __forceinline__ void batch(Acc& acc, const Reg (&v)[kUnroll], const float (&w)[kUnroll]) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) add<WEIGHTED>(acc, WEIGHTED ? w[u] : 1.f, v[u]);
  }

  static __device__ __forceinline__ void store(float* p, const Acc& acc) { store_plane_row(p, acc); }
};

// A bf16 table: a lane owns 8 columns (one 16-B load per gathered row), so a lane group is half as wide as the fp32
// kernel's for the same F.  No source-scale form: the scale belongs to the conversion pass (rows_to_bf16).
struct SlicedRowBf16 : RowBf16 {
  static constexpr bool kSrcScale = false;

  static __device__ __forceinline__ Reg none() { return Reg{0u, 0u, 0u, 0u}; }

  // dword by dword: the same edge-by-edge step on each column pair, one dword's 16 widened values at a time
  template <bool WEIGHTED>
  static __device__ __forceinline__ void batch(Acc& acc, const Reg (&v)[kUnroll], const float (&w)[kUnroll]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k > 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) add_pair<WEIGHTED>(acc.p[k], WEIGHTED ? w[u] : 1.f, v[u][k]);
    }
  }

  static __device__ __forceinline__ void store(float* p, const Acc& acc) {
    store_plane_row(p, half(acc, 0));
    store_plane_row(p + 4, half(acc, 1));
  }
};

// A (row, slice) segment is short (deg / n_slices: 12-25 edges at config 4).  In the slice-major layout the segments of
// consecutive rows of one slice are contiguous, so each LPR-lane *group* of the wave (F=128, fp32: a half-wave) streams
// the edges of kRowsPerGroup consecutive rows as ONE run — ids read LPR at a time by the group's own lanes, one gathered
// source row per group per wave-instruction, 8 gathers in flight per group — and cuts the running sum at the row
// boundaries (held one per lane, fetched with ds_bpermute when crossed).  No bubble between rows, no cross-group
// reduction.
//
// The sum of a (row, slice) segment is CANONICAL: acc starts at +0 and takes the segment's edges in layout order,
// acc = acc + x_p (unit values) or acc = fmaf(w_p, x_p, acc) (w_p: the edge's factors multiplied in the order below; x_p
// of a bf16 table after the exact widening), whether a batch of 8 lies inside one row (no boundary tests) or crosses a
// boundary (per-edge tests).  With the planes added in slice order, a product is a function of the layout and the
// operands alone: not of the rows per lane group, the lane-group width, the row chunks, the column passes, the tapered
// tail, the touchers or — for a table of bf16 values — of the table's element width: both kernels are this body.
//
// grid.x = n_slices * (worker blocks + toucher blocks); the rows of a worker block's lane groups: sliced_run
// (dgmi_sliced_common.h).  block b: slice = b % n_slices.
// Rows [row_begin, row_end) of every slice; plane row index is relative to row_begin.
// KEEP: edge dropout on the fly — an edge whose keep(eid[p]) fails (dgmi_keep.h) is flagged in the sign
// bit of its source id; its gather repeats the group's previous row (an L1 hit — never one fixed row,
// which would turn 10 % of all gathers into traffic on a single L2 channel) and its contribution is
// replaced by zeros: a select, not 0 * x — Inf / NaN behind a dropped edge must not leak.
// VALS: 0 = unit edge values; 1 = vals[p]; 2 = small integer multiplicities carried in the id words themselves (bits
// kMultShift..30 hold m - 1): the reference's adjacencies are D^-1 (A + A^T + I) (data_loader.py:297-308, utils.py:11-17),
// i.e. value = row scale x multiplicity — the scale goes where dst_scale / src_scale go, the multiplicity rides with the
// id: no value stream (4 B / edge), no second cross-lane hand-off per edge.
template <typename Row, int LPR, int VALS, bool HAS_SS, bool KEEP, bool OFF32>
__device__ __forceinline__ void sliced_body(const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices,
                                            const float* __restrict__ vals, const typename Row::Elem* __restrict__ X,
                                            int64_t ldx, const float* __restrict__ src_scale, float* __restrict__ planes,
                                            int64_t ldp, int64_t n_dst, int64_t row_begin, int64_t row_end, int F,
                                            int n_slices, const int32_t* __restrict__ eid, const KeepSeg* __restrict__ keep,
                                            int n_keep, int touch_lead, const SlicedRuns& runs, int touch_group) {
  typedef typename Row::Elem Elem;
  static_assert(Row::kSrcScale || !HAS_SS, "no source-scale form for this table");
  constexpr int G = kWave / LPR;
  constexpr bool HAS_VALS = VALS == 1;
  constexpr bool MULT = VALS == 2;
  constexpr bool WEIGHTED = HAS_VALS || HAS_SS || MULT;  // a per-edge factor exists
  constexpr bool W_LANE = HAS_VALS || HAS_SS;            // ... and travels in a register of its own
  constexpr int kIdMask = MULT ? (int)kMultIdMask : 0x7fffffff;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int grp = lane / LPR, glane = lane % LPR, gbase = grp * LPR;
  const int slice = (int)(blockIdx.x % (unsigned)n_slices);
  int64_t block = blockIdx.x / (unsigned)n_slices;
  if (touch_group > 0 &&
      touch_ahead<HAS_VALS, KEEP>(segptr, indices, vals, eid, n_dst, row_begin, row_end, slice, runs, touch_lead, touch_group,
                                  lane, wave, block))
    return;
  const SlicedRun run = sliced_run(runs, block, wave * G + grp);
  const int nr = run.rows;  // < LPR: a group's row boundaries live one per lane
  if (nr == 0) return;  // whole group idle (lanes of other groups carry on)
  const int64_t row0 = row_begin + run.first;
  int col = ((int)blockIdx.y * LPR + glane) * Row::kCols;
  const bool col_ok = col < F;  // F is a multiple of the columns a lane owns: all of them or none
  if (!col_ok) col = 0;
  const Elem* Xc = X + col;
  const uint32_t row_bytes = (uint32_t)ldx * (uint32_t)sizeof(Elem), col_bytes = (uint32_t)col * (uint32_t)sizeof(Elem);
  const int32_t* sp = segptr + (int64_t)slice * n_dst + row0;
  float* prow = planes + ((int64_t)slice * (row_end - row_begin) + (row0 - row_begin)) * ldp + col;

  const KeepPre first = first_seg<KEEP>(keep, n_keep);
  const int my_b = sp[glane < nr ? glane : nr];  // lane k holds boundary k (k <= nr)
  // v of lane k of this lane's group (k < LPR): ds_bpermute by the lane's byte address
  const int gaddr = gbase * 4;
  auto from = [&](int v, int k) { return __builtin_amdgcn_ds_bpermute(gaddr + 4 * k, v); };
  const int e_begin = from(my_b, 0);
  const int e_end = from(my_b, nr);
  int r = 0;
  int next_b = from(my_b, 1);
  typename Row::Acc acc = Row::zero();
  // ids (and weights) one batch ahead of the gathers that use them: lane k of a group fetches edge k of the batch at q
  int nxt_idx = 0;
  float nxt_w = 0.f;
  auto prefetch = [&](int b) {
    const int q = b + glane < e_end ? b + glane : b;
    nxt_idx = fetch_id<KEEP>(indices, eid, first, keep, n_keep, q);
    if (W_LANE) {
      nxt_w = HAS_VALS ? vals[q] : 1.f;
      if (HAS_SS) nxt_w *= src_scale[(KEEP || MULT) ? nxt_idx & kIdMask : nxt_idx];
    }
  };
  int last_row = -1;  // KEEP: the row this group gathered last (where a dropped edge's load is parked)
  if (e_begin < e_end) prefetch(e_begin);
  for (int base = e_begin; base < e_end; base += LPR) {
    const int n = min(LPR, e_end - base);
    const int my_idx = nxt_idx;
    const float my_w = nxt_w;
    if (base + LPR < e_end) prefetch(base + LPR);
    for (int j = 0; j < n; j += kUnroll) {
      typename Row::Reg v[kUnroll];
      float w[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int e = j + u;  // < LPR
        int idx = from(my_idx, e);
        if (W_LANE) w[u] = __int_as_float(from(__float_as_int(my_w), e));
        if (MULT) {  // the multiplicity arrived with the id
          const float m = (float)(((idx >> kMultShift) & kMultMax) + 1);
          w[u] = W_LANE ? w[u] * m : m;
        }
        const bool dropped = KEEP && idx < 0;
        if (KEEP) {
          idx = dropped && last_row >= 0 ? last_row : idx & kIdMask;
          last_row = idx;
        } else if (MULT) {
          idx &= kIdMask;
        }
        v[u] = Row::template load<OFF32>(X, Xc, idx, ldx, row_bytes, col_bytes);
        if (dropped) v[u] = Row::none();
      }
      // fast path (group-uniform): all 8 edges belong to the current row -> no per-edge boundary tests; the same
      // in-order sum as below (a timing-only build that took it for EVERY batch gained 2-7 %: the slow path is not what
      // holds the kernel at 0.81 of the gather probe — profiles/r03_swept_experiment/README.md)
      if (base + j + kUnroll <= next_b) {
        Row::template batch<WEIGHTED>(acc, v, w);
        continue;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int p = base + j + u;
        if (p < e_end) {  // group-uniform
          while (p >= next_b) {  // row(s) ended before this edge: emit them (empty rows emit zeros)
            if (col_ok) Row::store(prow + (int64_t)r * ldp, acc);
            acc = Row::zero();
            ++r;
            next_b = from(my_b, r + 1);
          }
          Row::template add<WEIGHTED>(acc, WEIGHTED ? w[u] : 1.f, v[u]);
        }
      }
    }
  }
  for (; r < nr; ++r) {  // the last non-empty row, then any trailing empty rows
    if (col_ok) Row::store(prow + (int64_t)r * ldp, acc);
    acc = Row::zero();
  }
}

}  // namespace
}  // namespace dgmi

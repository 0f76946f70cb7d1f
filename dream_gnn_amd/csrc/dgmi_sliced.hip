// dgmi_sliced.hip — XCD-local CSR SpMM for gfx950 (MI355X).
//
// MI355X has 8 XCDs, each with a private 4 MiB L2; workgroups are dealt round-robin over the
// XCDs (block b runs on XCD b % 8 — a speed observation, never relied on for correctness).
// A uniformly random gather over a 25-50 MB feature table hits L2 only ~27 % of the time and
// runs at the Infinity-Cache rate (~8 TB/s).  If every workgroup on XCD s only ever gathers
// source rows from slice s of the table (1/8 of it: 3-6 MB, i.e. L2-sized), the same gather
// runs 2.4-3x faster (measured: 19-26 TB/s algorithmic).
//
// So the graph is stored as 8 column-blocked CSRs (dgmi_csr.hip, key = slice * n_rows + row)
// and block b processes rows of slice b % 8 only, writing a partial row into plane b % 8;
// a second, streaming kernel adds the 8 planes in slice order (deterministic) and applies
// dst_scale.  Extra traffic: 2 * 8 * N_dst * 4F bytes of plane write + read, against
// nnz * 4F bytes of gather that now come out of L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgmi_sliced_common.h"

namespace dgmi {
namespace {

// A (row, slice) segment is short (deg / n_slices: 12-25 edges at config 4).  In the slice-major
// layout the segments of consecutive rows of one slice are contiguous, so each LPR-lane *group*
// of the wave (F=128: a half-wave) streams the edges of kRowsPerGroup consecutive rows as ONE
// run — ids read LPR at a time by the group's own lanes, one gathered source row per group per
// wave-instruction, 8 gathers in flight per group — and cuts the running sum at the row
// boundaries (held one per lane, fetched with ds_bpermute when crossed).  No bubble between
// rows, no cross-group reduction.
//
// The sum of a (row, slice) segment is CANONICAL: acc starts at +0 and takes the segment's edges in layout order,
// acc = acc + x_p (unit values) or acc = fmaf(w_p, x_p, acc) (w_p: the edge's factors multiplied in the order below),
// whether a batch of 8 lies inside one row (no boundary tests) or crosses a boundary (per-edge tests).  With the planes
// added in slice order, a product is a function of the layout and the operands alone: not of the rows per lane group,
// the lane-group width, the row chunks, the column passes, the tapered tail, the touchers or — for a table of bf16 values
// — of the table's element width (dgmi_sliced_bf16.hip computes the same).
//
// grid.x = n_slices * (worker blocks + toucher blocks); the rows of a worker block's lane groups: sliced_run
// (dgmi_sliced_common.h).  block b: slice = b % n_slices.
// Rows [row_begin, row_end) of every slice; plane row index is relative to row_begin.
// KEEP: edge dropout on the fly — an edge whose keep(eid[p]) fails (dgmi_keep.h) is flagged in the sign
// bit of its source id; its gather repeats the group's previous row (an L1 hit — never one fixed row,
// which would turn 10 % of all gathers into traffic on a single L2 channel) and its contribution is
// replaced by zeros.
// VALS: 0 = unit edge values; 1 = vals[p]; 2 = small integer multiplicities carried in the id words themselves (bits
// kMultShift..30 hold m - 1): the reference's adjacencies are D^-1 (A + A^T + I) (data_loader.py:297-308, utils.py:11-17),
// i.e. value = row scale x multiplicity — the scale goes where dst_scale / src_scale go, the multiplicity rides with the
// id: no value stream (4 B / edge), no second cross-lane hand-off per edge.
template <int LPR, int VALS, bool HAS_SS, bool KEEP, bool OFF32>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void spmm_sliced_vec4_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices,
    const float* __restrict__ vals, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ src_scale, float* __restrict__ planes, int64_t ldp, int64_t n_dst,
    int64_t row_begin, int64_t row_end, int F, int n_slices, const int32_t* __restrict__ eid,
    const KeepSeg* __restrict__ keep, int n_keep, int touch_lead, SlicedRuns runs, int touch_group) {
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
  int col = ((int)blockIdx.y * LPR + glane) * 4;
  const bool col_ok = col < F;
  if (!col_ok) col = 0;
  const float* Xc = X + col;
  const uint32_t row_bytes = (uint32_t)ldx * 4u, col_bytes = (uint32_t)col * 4u;
  const int32_t* sp = segptr + (int64_t)slice * n_dst + row0;
  float* prow = planes + ((int64_t)slice * (row_end - row_begin) + (row0 - row_begin)) * ldp + col;

  const KeepPre first = first_seg<KEEP>(keep, n_keep);
  const int my_b = sp[glane < nr ? glane : nr];  // lane k holds boundary k (k <= nr)
  const int e_begin = __shfl(my_b, gbase, kWave);
  const int e_end = __shfl(my_b, gbase + nr, kWave);
  int r = 0;
  int next_b = __shfl(my_b, gbase + 1, kWave);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // ids (and weights) one batch ahead of the gathers that use them
  int nxt_idx = 0;
  float nxt_w = 0.f;
  int last_row = -1;  // KEEP: the row this group gathered last (where a dropped edge's load is parked)
  if (e_begin < e_end) {
    const int q = e_begin + glane < e_end ? e_begin + glane : e_begin;
    nxt_idx = fetch_id<KEEP>(indices, eid, first, keep, n_keep, q);
    if (W_LANE) {
      nxt_w = HAS_VALS ? vals[q] : 1.f;
      if (HAS_SS) nxt_w *= src_scale[(KEEP || MULT) ? nxt_idx & kIdMask : nxt_idx];
    }
  }
  for (int base = e_begin; base < e_end; base += LPR) {
    const int n = min(LPR, e_end - base);
    const int my_idx = nxt_idx;
    const float my_w = nxt_w;
    if (base + LPR < e_end) {
      const int nb = base + LPR;
      const int q = nb + glane < e_end ? nb + glane : nb;
      nxt_idx = fetch_id<KEEP>(indices, eid, first, keep, n_keep, q);
      if (W_LANE) {
        nxt_w = HAS_VALS ? vals[q] : 1.f;
        if (HAS_SS) nxt_w *= src_scale[(KEEP || MULT) ? nxt_idx & kIdMask : nxt_idx];
      }
    }
    for (int j = 0; j < n; j += kUnroll) {
      float4 v[kUnroll];
      float w[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int e = j + u;  // < LPR
        int idx = __shfl(my_idx, gbase + e, kWave);
        if (W_LANE) w[u] = __shfl(my_w, gbase + e, kWave);
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
        v[u] = ld_row<OFF32>(X, Xc, idx, ldx, row_bytes, col_bytes);
        if (dropped) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      // fast path (group-uniform): all 8 edges belong to the current row -> no per-edge boundary tests; the same
      // in-order sum as below (the four columns are the ILP) (a timing-only build that took it for EVERY batch gained
      // 2-7 %: the slow path is not what holds the kernel at 0.81 of the gather probe —
      // profiles/r03_swept_experiment/README.md)
      if (base + j + kUnroll <= next_b) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (WEIGHTED) {
            acc.x = fmaf(w[u], v[u].x, acc.x);
            acc.y = fmaf(w[u], v[u].y, acc.y);
            acc.z = fmaf(w[u], v[u].z, acc.z);
            acc.w = fmaf(w[u], v[u].w, acc.w);
          } else {
            acc.x += v[u].x;
            acc.y += v[u].y;
            acc.z += v[u].z;
            acc.w += v[u].w;
          }
        }
        continue;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int p = base + j + u;
        if (p < e_end) {  // group-uniform
          while (p >= next_b) {  // row(s) ended before this edge: emit them (empty rows emit zeros)
            if (col_ok) store_plane_row(prow + (int64_t)r * ldp, acc);
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            ++r;
            next_b = __shfl(my_b, gbase + r + 1, kWave);
          }
          if (WEIGHTED) {
            acc.x = fmaf(w[u], v[u].x, acc.x);
            acc.y = fmaf(w[u], v[u].y, acc.y);
            acc.z = fmaf(w[u], v[u].z, acc.z);
            acc.w = fmaf(w[u], v[u].w, acc.w);
          } else {
            acc.x += v[u].x;
            acc.y += v[u].y;
            acc.z += v[u].z;
            acc.w += v[u].w;
          }
        }
      }
    }
  }
  for (; r < nr; ++r) {  // the last non-empty row, then any trailing empty rows
    if (col_ok) store_plane_row(prow + (int64_t)r * ldp, acc);
    acc = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// Y[row] = dst_scale[row] * (plane_0[row] + plane_1[row] + ...) in slice order; one float4 per
// thread, all S plane loads of an element in flight together (S known at compile time for the
// usual 8 slices).  dst_scale and Y already point at the chunk's first row.
template <bool HAS_DS, int S>
__global__ __launch_bounds__(256) void reduce_planes_kernel(const float* __restrict__ planes, int64_t ldp,
                                                            int64_t rows, int F4, int n_slices,
                                                            const float* __restrict__ dst_scale,
                                                            float* __restrict__ Y, int64_t ldy, Epilogue ep) {
  const int64_t total = rows * F4;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t plane_stride = rows * ldp;
  const bool dense = (ldp == 4 * (int64_t)F4) && (ldy == ldp);  // element t of a plane is at offset 4t
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    int64_t row, poff, yoff;
    if (dense) {
      row = t / F4;
      poff = yoff = 4 * t;
    } else {
      row = t / F4;
      const int c = (int)(t - row * F4) * 4;
      poff = row * ldp + c;
      yoff = row * ldy + c;
    }
    const float* p = planes + poff;
    float4 acc;
    if (S > 0) {
      float4 v[S > 0 ? S : 1];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p + s * plane_stride));
        v[s] = make_float4(t.x, t.y, t.z, t.w);
      }
      acc = v[0];
#pragma unroll
      for (int s = 1; s < S; ++s) {
        acc.x += v[s].x;
        acc.y += v[s].y;
        acc.z += v[s].z;
        acc.w += v[s].w;
      }
    } else {
      acc = *reinterpret_cast<const float4*>(p);
      for (int s = 1; s < n_slices; ++s) {
        const float4 v = *reinterpret_cast<const float4*>(p + s * plane_stride);
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
    }
    if (HAS_DS) {
      const float d = dst_scale[row];
      acc.x *= d;
      acc.y *= d;
      acc.z *= d;
      acc.w *= d;
    }
    *reinterpret_cast<float4*>(Y + yoff) = epilogue4(ep, acc, row, (int)(yoff - row * ldy));
  }
}

// The reduce of one row chunk: planes, dst_scale, Y and ep.mask all start at the chunk's first row.
hipError_t reduce_planes(const float* planes, int64_t ldp, int64_t rows, int64_t F, int64_t n_slices, const float* ds, float* y,
                         int64_t ldy, const Epilogue& ep, hipStream_t s) {
  const int F4 = (int)(F / 4);
  int64_t blocks = (rows * F4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
#define DGMI_REDUCE(D, S)                                                                                        \
  hipLaunchKernelGGL((reduce_planes_kernel<D, S>), dim3((unsigned)blocks), dim3(256), 0, s, planes, ldp, rows, F4, \
                     (int)n_slices, ds, y, ldy, ep)
  if (n_slices == 8) {
    if (ds) DGMI_REDUCE(true, 8); else DGMI_REDUCE(false, 8);
  } else {
    if (ds) DGMI_REDUCE(true, 0); else DGMI_REDUCE(false, 0);
  }
#undef DGMI_REDUCE
  return hipGetLastError();
}

template <int LPR>
hipError_t launch_sliced(const SlicedArgs& a, int64_t row_begin, int64_t row_end, hipStream_t s) {
  const SlicedGeometry g = sliced_geometry(row_begin, row_end, a.F, a.n_src, a.ldx, a.n_slices, LPR, a.x_bytes);
  dim3 block(kWave * kWavesPerBlock);
  const int key = (a.vals ? 4 : (a.id_mult ? 8 : 0)) | (a.src_scale ? 2 : 0) | (a.n_keep > 0 ? 1 : 0);
#define DGMI_LAUNCH_O(V, S, K, O)                                                                                      \
  hipLaunchKernelGGL((spmm_sliced_vec4_kernel<LPR, V, S, K, O>), g.grid, block, 0, s, a.segptr, a.indices, a.vals,      \
                     static_cast<const float*>(a.X), a.ldx, a.src_scale, a.planes, a.ldp, a.n_dst, row_begin, row_end, \
                     (int)a.F, (int)a.n_slices, a.eid, static_cast<const KeepSeg*>(a.keep), a.n_keep, g.touch_lead, g.runs, \
                     g.touch_group)
#define DGMI_LAUNCH(V, S, K)                                              \
  do {                                                                    \
    if (g.off32) DGMI_LAUNCH_O(V, S, K, true); else DGMI_LAUNCH_O(V, S, K, false); \
  } while (0)
  switch (key) {
    case 0: DGMI_LAUNCH(0, false, false); break;
    case 1: DGMI_LAUNCH(0, false, true); break;
    case 2: DGMI_LAUNCH(0, true, false); break;
    case 3: DGMI_LAUNCH(0, true, true); break;
    case 4: DGMI_LAUNCH(1, false, false); break;
    case 5: DGMI_LAUNCH(1, false, true); break;
    case 6: DGMI_LAUNCH(1, true, false); break;
    case 7: DGMI_LAUNCH(1, true, true); break;
    case 8: DGMI_LAUNCH(2, false, false); break;
    case 9: DGMI_LAUNCH(2, false, true); break;
    case 10: DGMI_LAUNCH(2, true, false); break;
    default: DGMI_LAUNCH(2, true, true); break;
  }
#undef DGMI_LAUNCH
#undef DGMI_LAUNCH_O
  return hipGetLastError();
}

hipError_t launch_gather_f32(const SlicedArgs& a, int lpr, int64_t r0, int64_t r1, hipStream_t s) {
  switch (lpr) {
    case 8: return launch_sliced<8>(a, r0, r1, s);
    case 16: return launch_sliced<16>(a, r0, r1, s);
    case 32: return launch_sliced<32>(a, r0, r1, s);
    default: return launch_sliced<64>(a, r0, r1, s);
  }
}

}  // namespace

hipError_t spmm_sliced_chunks(const SlicedArgs& a, SlicedGather gather, hipStream_t s) {
  if (a.n_dst == 0 || a.F == 0) return hipSuccess;
  // Row chunks: the 8 partial planes of a chunk (chunk_rows * n_slices * 4F bytes, <= ~32 MB) are
  // written and read back while still resident in the 256 MiB Infinity Cache, and the same
  // plane buffer is reused by every chunk.
  const int64_t chunk = a.chunk_rows > 0 ? a.chunk_rows : a.n_dst;
  for (int64_t r0 = 0; r0 < a.n_dst; r0 += chunk) {
    const int64_t r1 = r0 + chunk < a.n_dst ? r0 + chunk : a.n_dst;
    const int lpr = sliced_lpr(a.F, a.n_src, a.n_slices, a.n_dst, a.full_width, a.n_keep, a.x_bytes, tuning().sliced_lpr);
    hipError_t err = gather(a, lpr, r0, r1, s);
    if (err != hipSuccess) return err;
    Epilogue ep = a.ep;  // rows of this chunk start at r0
    if (ep.mask != nullptr) ep.mask += r0 * ep.ldm;
    err = reduce_planes(a.planes, a.ldp, r1 - r0, a.F, a.n_slices, a.dst_scale ? a.dst_scale + r0 : nullptr, a.Y + r0 * a.ldy,
                        a.ldy, ep, s);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

hipError_t spmm_sliced_f32(const SlicedArgs& a, hipStream_t s) {
  if (a.x_bytes != 4) return hipErrorInvalidValue;
  bool owned = false;  // the plane-free form, where it applies and is selected (dgmi_owned.hip)
  const hipError_t err = spmm_owned_try(a, s, &owned);
  if (err != hipSuccess || owned) return err;
  return spmm_sliced_chunks(a, launch_gather_f32, s);
}

}  // namespace dgmi

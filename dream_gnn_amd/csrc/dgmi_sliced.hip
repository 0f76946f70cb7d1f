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
//
// The gathered table is fp32 or a bf16 copy of it (rows_to_bf16, dgmi_sliced_bf16.hip): a row of 2F bytes, the slice of
// a 100 000-source table at F = 128 3.2 MB — it fits an XCD's 4 MiB L2 at full width.  Products, sums, planes and Y are
// fp32 either way.  Both gather kernels are ONE body (sliced_body, dgmi_sliced_kernel.h: the canonical sum, the grid,
// KEEP and VALS are described there) under a row policy each, launched through one table of instantiations; the result
// from a bf16 table is bit-identical to the fp32 product of the upcast table, whatever the launch geometry of either.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgmi_sliced_kernel.h"

namespace dgmi {
namespace {

// An fp32 table: a lane owns 4 columns.
template <int LPR, int VALS, bool HAS_SS, bool KEEP, bool OFF32>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void spmm_sliced_vec4_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices,
    const float* __restrict__ vals, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ src_scale, float* __restrict__ planes, int64_t ldp, int64_t n_dst,
    int64_t row_begin, int64_t row_end, int F, int n_slices, const int32_t* __restrict__ eid,
    const KeepSeg* __restrict__ keep, int n_keep, int touch_lead, SlicedRuns runs, int touch_group) {
  sliced_body<SlicedRowF32, LPR, VALS, HAS_SS, KEEP, OFF32>(segptr, indices, vals, X, ldx, src_scale, planes, ldp, n_dst, row_begin,
                                                            row_end, F, n_slices, eid, keep, n_keep, touch_lead, runs, touch_group);
}

// A bf16 table: a lane owns 8 columns.  Built for five waves per SIMD (96 VGPRs) like the fp32 kernel's forms without a
// source scale; a per-edge weight together with dropout on the fly or with 8-lane groups needs more: four waves, no scratch.
template <int LPR, int VALS, bool KEEP, bool OFF32>
__global__ __launch_bounds__(kWave* kWavesPerBlock, (VALS != 0 && (KEEP || LPR == 8)) ? 4 : 5) void spmm_sliced_bf16_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const uint16_t* __restrict__ X, int64_t ldx, float* __restrict__ planes, int64_t ldp, int64_t n_dst, int64_t row_begin,
    int64_t row_end, int F, int n_slices, const int32_t* __restrict__ eid, const KeepSeg* __restrict__ keep, int n_keep,
    int touch_lead, SlicedRuns runs, int touch_group) {
  sliced_body<SlicedRowBf16, LPR, VALS, false, KEEP, OFF32>(segptr, indices, vals, X, ldx, nullptr, planes, ldp, n_dst, row_begin,
                                                            row_end, F, n_slices, eid, keep, n_keep, touch_lead, runs, touch_group);
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

// One instantiation: the kernel of the table's element type in this form.  A bf16 table has no source-scale form
// (spmm_sliced refuses the request).
template <typename Row, int LPR, int VALS, bool HAS_SS, bool KEEP, bool OFF32>
void launch_form(const SlicedArgs& a, const SlicedGeometry& g, int64_t row_begin, int64_t row_end, hipStream_t s) {
  const dim3 block(kWave * kWavesPerBlock);
  const auto* X = static_cast<const typename Row::Elem*>(a.X);
  const auto* keep = static_cast<const KeepSeg*>(a.keep);
  if constexpr (!Row::kSrcScale) {
    if constexpr (!HAS_SS)
      hipLaunchKernelGGL((spmm_sliced_bf16_kernel<LPR, VALS, KEEP, OFF32>), g.grid, block, 0, s, a.segptr, a.indices, a.vals, X,
                         a.ldx, a.planes, a.ldp, a.n_dst, row_begin, row_end, (int)a.F, (int)a.n_slices, a.eid, keep, a.n_keep,
                         g.touch_lead, g.runs, g.touch_group);
  } else {
    hipLaunchKernelGGL((spmm_sliced_vec4_kernel<LPR, VALS, HAS_SS, KEEP, OFF32>), g.grid, block, 0, s, a.segptr, a.indices,
                       a.vals, X, a.ldx, a.src_scale, a.planes, a.ldp, a.n_dst, row_begin, row_end, (int)a.F, (int)a.n_slices,
                       a.eid, keep, a.n_keep, g.touch_lead, g.runs, g.touch_group);
  }
}

// The gather launch of one row chunk [row_begin, row_end) at lane-group width LPR: the table of instantiations, VALS
// (0 unit values, 1 a.vals, 2 a.id_mult) x source scale x dropout on the fly x 32-bit offsets.
template <typename Row, int LPR>
hipError_t launch_sliced(const SlicedArgs& a, int64_t row_begin, int64_t row_end, hipStream_t s) {
  typedef void (*Form)(const SlicedArgs&, const SlicedGeometry&, int64_t, int64_t, hipStream_t);
#define DGMI_FORMS(V, S) \
  {{launch_form<Row, LPR, V, S, false, false>, launch_form<Row, LPR, V, S, false, true>}, \
   {launch_form<Row, LPR, V, S, true, false>, launch_form<Row, LPR, V, S, true, true>}}
  static constexpr Form table[3][2][2][2] = {{DGMI_FORMS(0, false), DGMI_FORMS(0, true)},
                                             {DGMI_FORMS(1, false), DGMI_FORMS(1, true)},
                                             {DGMI_FORMS(2, false), DGMI_FORMS(2, true)}};
#undef DGMI_FORMS
  const SlicedGeometry g = sliced_geometry(row_begin, row_end, a.F, a.n_src, a.ldx, a.n_slices, LPR, a.x_bytes);
  table[a.vals ? 1 : (a.id_mult ? 2 : 0)][a.src_scale != nullptr][a.n_keep > 0][g.off32](a, g, row_begin, row_end, s);
  return hipGetLastError();
}

// The lane-group widths a table's element type has: 8 .. 64 of an fp32 table, 8 .. 32 of a bf16 one (sliced_lpr).
template <typename Row>
hipError_t launch_gather(const SlicedArgs& a, int lpr, int64_t r0, int64_t r1, hipStream_t s) {
  switch (lpr) {
    case 8: return launch_sliced<Row, 8>(a, r0, r1, s);
    case 16: return launch_sliced<Row, 16>(a, r0, r1, s);
    case 32: return launch_sliced<Row, 32>(a, r0, r1, s);
    default:
      if constexpr (Row::kMaxLpr >= 64)
        return launch_sliced<Row, 64>(a, r0, r1, s);
      else
        return launch_sliced<Row, 32>(a, r0, r1, s);
  }
}

// The chunk driver: cuts [0, n_dst) into row chunks; per chunk picks the lane-group width (sliced_lpr), runs the gather
// and then the plane reduce with the chunk's dst_scale / Y / mask offsets.
template <typename Row>
hipError_t spmm_sliced_chunks(const SlicedArgs& a, hipStream_t s) {
  if (a.n_dst == 0 || a.F == 0) return hipSuccess;
  // Row chunks: the 8 partial planes of a chunk (chunk_rows * n_slices * 4F bytes, <= ~32 MB) are
  // written and read back while still resident in the 256 MiB Infinity Cache, and the same
  // plane buffer is reused by every chunk.
  const int64_t chunk = a.chunk_rows > 0 ? a.chunk_rows : a.n_dst;
  for (int64_t r0 = 0; r0 < a.n_dst; r0 += chunk) {
    const int64_t r1 = r0 + chunk < a.n_dst ? r0 + chunk : a.n_dst;
    const int lpr = sliced_lpr(a.F, a.n_src, a.n_slices, a.n_dst, a.full_width, a.n_keep, a.x_bytes, tuning().sliced_lpr);
    hipError_t err = launch_gather<Row>(a, lpr, r0, r1, s);
    if (err != hipSuccess) return err;
    Epilogue ep = a.ep;  // rows of this chunk start at r0
    if (ep.mask != nullptr) ep.mask += r0 * ep.ldm;
    err = reduce_planes(a.planes, a.ldp, r1 - r0, a.F, a.n_slices, a.dst_scale ? a.dst_scale + r0 : nullptr, a.Y + r0 * a.ldy,
                        a.ldy, ep, s);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace

hipError_t spmm_sliced(const SlicedArgs& a, hipStream_t s) {
  if (a.x_bytes != 4 && a.x_bytes != 2) return hipErrorInvalidValue;
  if (a.x_bytes == 2 && a.src_scale != nullptr) return hipErrorInvalidValue;  // the source scale belongs to rows_to_bf16
  if (a.scale_table != nullptr) return hipErrorInvalidValue;  // coded id words: the pair's kernels do not mask them (dgmi_scale.h)
  bool owned = false;  // the plane-free form, where it applies and is selected (dgmi_owned.hip)
  const hipError_t err = spmm_owned_try(a, s, &owned);
  if (err != hipSuccess || owned) return err;
  return a.x_bytes == 4 ? spmm_sliced_chunks<SlicedRowF32>(a, s) : spmm_sliced_chunks<SlicedRowBf16>(a, s);
}

}  // namespace dgmi

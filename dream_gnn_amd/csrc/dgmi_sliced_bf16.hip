// dgmi_sliced_bf16.hip — the XCD-local CSR SpMM of dgmi_sliced.hip gathering from a bf16 copy of the feature table.
//
// What the gather kernel of dgmi_sliced.hip moves is nnz * 4F bytes of fp32 source rows; its rate (the L2 -> CU row-gather
// rate) is spent.  Here the gathered operand — and only it — is bf16: a row is 2F bytes, the slice of a 100 000-source
// table at F = 128 is 3.2 MB and fits an XCD's 4 MiB L2 at full width.  The table is made by ONE streaming pass
// (rows_to_bf16_kernel) that also applies the source scale, in fp32, before the single round-to-nearest-even:
//
//   xb[j]  = bf16_rne(src_scale[j] * X[j])
//   Y[i]   = dst_scale[i] * sum_{e: dst(e) = i} w_e * float(xb[src(e)])          (products, sums, planes, Y: fp32)
//
// Layout (segptr, id words, multiplicity bits 28..30, dropped flag in bit 31), row-boundary logic, touch-ahead blocks,
// batches of 8 gathers, the canonical in-order row sum and the plane order are those of spmm_sliced_vec4_kernel, so the
// result is bit-identical to the fp32 product of the upcast table, whatever the launch geometry of either.  A lane owns 8 columns (one 16-B load per gathered row), so a lane group is half as
// wide as the fp32 kernel's for the same F.  No source-scale variant: the scale belongs to the conversion pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgmi_sliced_common.h"

namespace dgmi {
namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));

// two fp32 -> one dword of two bf16, round-to-nearest-even (v_cvt_pk_bf16_f32); element 0 in the low half
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
  const v2f f = {lo, hi};
  const v2bf b = __builtin_convertvector(f, v2bf);
  return __builtin_bit_cast(uint32_t, b);
}

// out[r, :] = bf16_rne(scale[r] * X[r, :]); one thread per 8 columns: two 16-B loads, one 16-B store
template <bool HAS_SCALE>
__global__ __launch_bounds__(256) void rows_to_bf16_kernel(const float* __restrict__ X, int64_t ldx,
                                                           const float* __restrict__ scale, int64_t n, int F8,
                                                           uint16_t* __restrict__ out, int64_t ldo) {
  const int64_t total = n * F8;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const int64_t row = t / F8;
    const int c = (int)(t - row * F8) * 8;
    const float* src = X + row * ldx + c;
    float4 a = ld4(src), b = ld4(src + 4);
    if (HAS_SCALE) {
      const float s = scale[row];
      a.x *= s, a.y *= s, a.z *= s, a.w *= s;
      b.x *= s, b.y *= s, b.z *= s, b.w *= s;
    }
    const v4u o = {pack_bf16(a.x, a.y), pack_bf16(a.z, a.w), pack_bf16(b.x, b.y), pack_bf16(b.z, b.w)};
    *reinterpret_cast<v4u*>(out + row * ldo + c) = o;
  }
}

// The 16-B load of a lane's 8 columns and the exact widening (ld_row8, widen): dgmi_sliced_common.h — the workgroup-owned
// form (OwnedRowBf16, dgmi_owned_kernel.h) gathers with them too.

// One dword (2 columns) of a fast-path batch: widen, and the canonical in-order sum of spmm_sliced_vec4_kernel
// (acc = fmaf(w, x, acc) or acc + x, edge by edge) on each of the two columns.
template <bool WEIGHTED, int K>
__device__ __forceinline__ void batch_pair(const v4u (&raw)[kUnroll], const float (&w)[kUnroll], float& acc0, float& acc1) {
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const uint32_t d = raw[u][K];
    const float lo = __uint_as_float(d << 16), hi = __uint_as_float(d & 0xffff0000u);
    if (WEIGHTED) {
      acc0 = fmaf(w[u], lo, acc0);
      acc1 = fmaf(w[u], hi, acc1);
    } else {
      acc0 += lo;
      acc1 += hi;
    }
  }
}

// The gather of spmm_sliced_vec4_kernel (dgmi_sliced.hip) with 8 columns per lane: see there for the grid, KEEP and
// VALS, and touch_ahead (dgmi_sliced_common.h) for the toucher blocks.  Every float4 operation of that kernel is done twice here (columns 0..3 in `a`,
// 4..7 in `b`), in the same order.  Built for five waves per SIMD (96 VGPRs) like that kernel's forms without a source scale;
// a per-edge weight together with dropout on the fly or with 8-lane groups needs 100-109 VGPRs: four waves, no scratch.
template <int LPR, int VALS, bool KEEP, bool OFF32>
__global__ __launch_bounds__(kWave* kWavesPerBlock, (VALS != 0 && (KEEP || LPR == 8)) ? 4 : 5) void spmm_sliced_bf16_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const float* __restrict__ vals,
    const uint16_t* __restrict__ X, int64_t ldx, float* __restrict__ planes, int64_t ldp, int64_t n_dst, int64_t row_begin,
    int64_t row_end, int F, int n_slices, const int32_t* __restrict__ eid, const KeepSeg* __restrict__ keep, int n_keep,
    int touch_lead, SlicedRuns runs, int touch_group) {
  constexpr int G = kWave / LPR;
  constexpr bool HAS_VALS = VALS == 1;
  constexpr bool MULT = VALS == 2;
  constexpr bool WEIGHTED = HAS_VALS || MULT;
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
  if (nr == 0) return;  // whole group idle
  const int64_t row0 = row_begin + run.first;
  int col = ((int)blockIdx.y * LPR + glane) * 8;
  const bool col_ok = col < F;  // F % 8 == 0: all 8 columns or none
  if (!col_ok) col = 0;
  const uint16_t* Xc = X + col;
  const uint32_t row_bytes = (uint32_t)ldx * 2u, col_bytes = (uint32_t)col * 2u;
  const int32_t* sp = segptr + (int64_t)slice * n_dst + row0;
  float* prow = planes + ((int64_t)slice * (row_end - row_begin) + (row0 - row_begin)) * ldp + col;

  const KeepPre first = first_seg<KEEP>(keep, n_keep);
  const int my_b = sp[glane < nr ? glane : nr];  // lane k holds boundary k (k <= nr)
  const int e_begin = __shfl(my_b, gbase, kWave);
  const int e_end = __shfl(my_b, gbase + nr, kWave);
  int r = 0;
  int next_b = __shfl(my_b, gbase + 1, kWave);
  float4 acc_a = make_float4(0.f, 0.f, 0.f, 0.f), acc_b = make_float4(0.f, 0.f, 0.f, 0.f);
  int nxt_idx = 0;
  float nxt_w = 0.f;
  int last_row = -1;  // KEEP: the row this group gathered last (where a dropped edge's load is parked)
  if (e_begin < e_end) {
    const int q = e_begin + glane < e_end ? e_begin + glane : e_begin;
    nxt_idx = fetch_id<KEEP>(indices, eid, first, keep, n_keep, q);
    if (HAS_VALS) nxt_w = vals[q];
  }
  for (int base = e_begin; base < e_end; base += LPR) {
    const int n = min(LPR, e_end - base);
    const int my_idx = nxt_idx;
    const float my_w = nxt_w;
    if (base + LPR < e_end) {
      const int nb = base + LPR;
      const int q = nb + glane < e_end ? nb + glane : nb;
      nxt_idx = fetch_id<KEEP>(indices, eid, first, keep, n_keep, q);
      if (HAS_VALS) nxt_w = vals[q];
    }
    for (int j = 0; j < n; j += kUnroll) {
      v4u raw[kUnroll];
      float w[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int e = j + u;  // < LPR
        int idx = __shfl(my_idx, gbase + e, kWave);
        if (HAS_VALS) w[u] = __shfl(my_w, gbase + e, kWave);
        if (MULT) w[u] = (float)(((idx >> kMultShift) & kMultMax) + 1);  // the multiplicity arrived with the id
        const bool dropped = KEEP && idx < 0;
        if (KEEP) {
          idx = dropped && last_row >= 0 ? last_row : idx & kIdMask;
          last_row = idx;
        } else if (MULT) {
          idx &= kIdMask;
        }
        raw[u] = ld_row8<OFF32>(X, Xc, idx, ldx, row_bytes, col_bytes);
        if (dropped) raw[u] = v4u{0u, 0u, 0u, 0u};  // a select, not 0 * x: Inf / NaN behind a dropped edge must not leak
      }
      // fast path (group-uniform): all 8 edges belong to the current row -> no per-edge boundary tests; dword by dword
      if (base + j + kUnroll <= next_b) {
        batch_pair<WEIGHTED, 0>(raw, w, acc_a.x, acc_a.y);
        __builtin_amdgcn_sched_barrier(0);  // one dword's 16 widened values at a time
        batch_pair<WEIGHTED, 1>(raw, w, acc_a.z, acc_a.w);
        __builtin_amdgcn_sched_barrier(0);
        batch_pair<WEIGHTED, 2>(raw, w, acc_b.x, acc_b.y);
        __builtin_amdgcn_sched_barrier(0);
        batch_pair<WEIGHTED, 3>(raw, w, acc_b.z, acc_b.w);
        continue;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int p = base + j + u;
        if (p < e_end) {  // group-uniform
          while (p >= next_b) {  // row(s) ended before this edge: emit them (empty rows emit zeros)
            if (col_ok) {
              store_plane_row(prow + (int64_t)r * ldp, acc_a);
              store_plane_row(prow + (int64_t)r * ldp + 4, acc_b);
            }
            acc_a = acc_b = make_float4(0.f, 0.f, 0.f, 0.f);
            ++r;
            next_b = __shfl(my_b, gbase + r + 1, kWave);
          }
          const float4 va = widen(raw[u].x, raw[u].y), vb = widen(raw[u].z, raw[u].w);
          if (WEIGHTED) {
            acc_a.x = fmaf(w[u], va.x, acc_a.x);
            acc_a.y = fmaf(w[u], va.y, acc_a.y);
            acc_a.z = fmaf(w[u], va.z, acc_a.z);
            acc_a.w = fmaf(w[u], va.w, acc_a.w);
            acc_b.x = fmaf(w[u], vb.x, acc_b.x);
            acc_b.y = fmaf(w[u], vb.y, acc_b.y);
            acc_b.z = fmaf(w[u], vb.z, acc_b.z);
            acc_b.w = fmaf(w[u], vb.w, acc_b.w);
          } else {
            acc_a.x += va.x;
            acc_a.y += va.y;
            acc_a.z += va.z;
            acc_a.w += va.w;
            acc_b.x += vb.x;
            acc_b.y += vb.y;
            acc_b.z += vb.z;
            acc_b.w += vb.w;
          }
        }
      }
    }
  }
  for (; r < nr; ++r) {  // the last non-empty row, then any trailing empty rows
    if (col_ok) {
      store_plane_row(prow + (int64_t)r * ldp, acc_a);
      store_plane_row(prow + (int64_t)r * ldp + 4, acc_b);
    }
    acc_a = acc_b = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

template <int LPR>
hipError_t launch_sliced_bf16(const SlicedArgs& a, int64_t row_begin, int64_t row_end, hipStream_t s) {
  const SlicedGeometry g = sliced_geometry(row_begin, row_end, a.F, a.n_src, a.ldx, a.n_slices, LPR, a.x_bytes);
  dim3 block(kWave * kWavesPerBlock);
  const int key = (a.vals ? 2 : (a.id_mult ? 4 : 0)) | (a.n_keep > 0 ? 1 : 0);
#define DGMI_LAUNCH_O(V, K, O)                                                                                         \
  hipLaunchKernelGGL((spmm_sliced_bf16_kernel<LPR, V, K, O>), g.grid, block, 0, s, a.segptr, a.indices, a.vals,        \
                     static_cast<const uint16_t*>(a.X), a.ldx, a.planes, a.ldp, a.n_dst, row_begin, row_end, (int)a.F, \
                     (int)a.n_slices, a.eid, static_cast<const KeepSeg*>(a.keep), a.n_keep, g.touch_lead, g.runs,      \
                     g.touch_group)
#define DGMI_LAUNCH(V, K)                                                    \
  do {                                                                       \
    if (g.off32) DGMI_LAUNCH_O(V, K, true); else DGMI_LAUNCH_O(V, K, false); \
  } while (0)
  switch (key) {
    case 0: DGMI_LAUNCH(0, false); break;
    case 1: DGMI_LAUNCH(0, true); break;
    case 2: DGMI_LAUNCH(1, false); break;
    case 3: DGMI_LAUNCH(1, true); break;
    case 4: DGMI_LAUNCH(2, false); break;
    default: DGMI_LAUNCH(2, true); break;
  }
#undef DGMI_LAUNCH
#undef DGMI_LAUNCH_O
  return hipGetLastError();
}

hipError_t launch_gather_bf16(const SlicedArgs& a, int lpr, int64_t r0, int64_t r1, hipStream_t s) {
  switch (lpr) {
    case 8: return launch_sliced_bf16<8>(a, r0, r1, s);
    case 16: return launch_sliced_bf16<16>(a, r0, r1, s);
    default: return launch_sliced_bf16<32>(a, r0, r1, s);
  }
}

}  // namespace

hipError_t rows_to_bf16(const float* X, int64_t ldx, const float* scale, int64_t n, int64_t F, uint16_t* out, int64_t ldo,
                        hipStream_t s) {
  if (n == 0 || F == 0) return hipSuccess;
  const int F8 = (int)(F / 8);
  int64_t blocks = (n * F8 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (scale != nullptr)
    hipLaunchKernelGGL(rows_to_bf16_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, X, ldx, scale, n, F8, out, ldo);
  else
    hipLaunchKernelGGL(rows_to_bf16_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, X, ldx, scale, n, F8, out, ldo);
  return hipGetLastError();
}

// Row chunks and the plane reduce: spmm_sliced_chunks (dgmi_sliced.hip); the column-pass rule, here on the bytes of a
// bf16 slice: sliced_lpr (dgmi_sliced_common.h).
hipError_t spmm_sliced_bf16(const SlicedArgs& a, hipStream_t s) {
  if (a.x_bytes != 2 || a.src_scale != nullptr) return hipErrorInvalidValue;  // the source scale belongs to rows_to_bf16
  bool owned = false;  // the plane-free form, where it applies and is selected (dgmi_owned.hip)
  const hipError_t err = spmm_owned_try(a, s, &owned);
  if (err != hipSuccess || owned) return err;
  return spmm_sliced_chunks(a, launch_gather_bf16, s);
}

}  // namespace dgmi

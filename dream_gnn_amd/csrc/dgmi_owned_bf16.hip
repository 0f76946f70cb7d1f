// dgmi_owned_bf16.hip — the workgroup-owned form of the XCD-local SpMM (dgmi_owned.hip) gathering from a bf16 table.
//
// The worker / toucher structure of spmm_owned_kernel with the per-row arithmetic of spmm_sliced_bf16_kernel
// (dgmi_sliced_bf16.hip): a lane owns 8 columns, a gathered row is one 16-byte load (ld_row8) widened by a shift and a
// mask (widen) into two float4 accumulators, columns 0..3 and 4..7.  The sum of a (row, slice) segment starts at +0 and
// takes the edges one at a time in layout order, acc + x or fmaf(m, x, acc); the segment sums of a row join in slice
// order in the row's LDS slot, dst_scale and the epilogue once, by the last slice's phase: bit-identical to the bf16 pair
// on the same layout, and to spmm_owned_kernel on the upcast table.  No atomics: only one lane group ever touches a
// given (row, phase).
//
// LDS.  A row of one column round is 32 LPR bytes, planar: the float4 of columns 0..3 of all LPR lanes first, then the
// float4 of columns 4..7 of all lanes — each of a lane's two 16-byte accesses is contiguous across its lane group (a
// 32-byte lane stride would make every access a two-way bank conflict).  The plan: owned_plan with cols_per_lane = 8
// (dgmi_owned_common.h).
//
// The task protocol is that of dgmi_owned.hip, word for word — one LDS counter, phase-major task order, the next task
// reserved (and its boundaries requested) before the current one runs, done[task] release-stored after a task's LDS
// writes and acquire-polled before the next one's first LDS access, the 16th wave as toucher — and so is its argument
// why this cannot deadlock: the lowest unfinished task never waits.  The rolling window of kOwnedWindow gathers
// (owned_window_*) is kept; every run starts cold and drains (the hand-over of dgmi_owned.hip is not built here: the
// bits are the same either way).
//
// Left out on purpose: the two-workgroup form (it lost on every class in fp32: profiles/owned_wgs/README.md) and the
// phase gate (measured as a loss in fp32: profiles/owned_rows/README.md) — so there are no arrive counters, no spin on
// another workgroup and no memset: nothing in this kernel waits for anything outside its own workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgmi_owned_common.h"
#include "dgmi_sliced_common.h"

namespace dgmi {
namespace {

constexpr int kOwnedTouchChunk = 4;  // tasks the toucher touches for at a time (as dgmi_owned.hip)
constexpr int kOwnedTouchLead = 8;   // tasks between the counter and the first task of the chunk it touches for

// VALS: 0 = unit edge values, 2 = multiplicities in the id words (dgmi_sliced.hip).  One workgroup of kOwnedWaves waves
// per CU, the last wave the toucher: 4 waves per SIMD, 128 VGPRs per lane.
template <int LPR, int VALS, bool OFF32>
__global__ __launch_bounds__(kWave* kOwnedWaves, 4) void spmm_owned_bf16_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const uint16_t* __restrict__ X, int64_t ldx,
    const float* __restrict__ dst_scale, float* __restrict__ Y, int64_t ldy, int64_t n_dst, int F, OwnedPlan pl, int workers,
    Epilogue ep) {
  constexpr bool MULT = VALS == 2;
  constexpr int kIdMask = MULT ? (int)kMultIdMask : 0x7fffffff;
  constexpr int kRowSlots = 2 * LPR;  // float4 slots of an LDS row: columns 0..3 of every lane, then columns 4..7
  extern __shared__ float4 lds_rows[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int grp = lane / LPR, glane = lane % LPR, gbase = grp * LPR;
  const int64_t wg = blockIdx.x;
  const int T = owned_wg_tasks(pl, wg);
  if (T == 0) return;  // block-uniform: a workgroup without rows
  int* done = reinterpret_cast<int*>(lds_rows + (size_t)pl.round_rows * kRowSlots);  // [tasks] phases finished on a task slot
  int* counter = done + pl.tasks;                                                   // next task
  for (int i = threadIdx.x; i < pl.tasks + 1; i += blockDim.x) done[i] = 0;
  __syncthreads();
  const int total = pl.phases * T;

  if (wave == kOwnedWaves - 1) {  // ---- the toucher ----
    // touches the next chunk of tasks once the counter is within the lead of it (also across a phase boundary)
    const int chunks_per_phase = (T + kOwnedTouchChunk - 1) / kOwnedTouchChunk, chunks = pl.phases * chunks_per_phase;
    int keepalive = 0, touched = 0;
    while (touched < chunks) {
      const int next = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const int P = touched / chunks_per_phase, t0 = (touched - P * chunks_per_phase) * kOwnedTouchChunk;
      if (P * T + t0 > next + kOwnedTouchLead) {
        __builtin_amdgcn_s_sleep(2);
        continue;
      }
      ++touched;
      // the rows of tasks [t0, t0 + chunk): consecutive rows of one slice, hence one run of boundaries and of ids
      const OwnedPhase ph = owned_phase(pl, P);
      const int64_t in_round = owned_round_rows(pl, wg, ph.row_round);
      const int64_t lds_first = (int64_t)t0 * pl.G * pl.R;
      int64_t lds_last = lds_first + (int64_t)kOwnedTouchChunk * pl.G * pl.R;
      if (lds_last > in_round) lds_last = in_round;
      if (lds_first < lds_last) {  // (not: a short last round)
        const int32_t* sp_s = segptr + (int64_t)ph.slice * n_dst;
        const int64_t r_first = owned_task(pl, wg, ph.row_round, t0, 0).row0, r_last = r_first + (lds_last - lds_first);
        const int64_t rp = lane == 0 ? r_first : (lane == 1 ? r_last : r_first + (int64_t)(lane - 1) * 32);
        int v = 0;
        if (rp <= r_last) v = sp_s[rp];
        keepalive ^= v;
        const int e0 = __builtin_amdgcn_readlane(v, 0), e1 = __builtin_amdgcn_readlane(v, 1);
        for (int64_t p = (int64_t)e0 + (int64_t)lane * 32; p < e1; p += (int64_t)kWave * 32) keepalive ^= indices[p];
        asm volatile("" ::"v"(keepalive));  // the loads exist, and are waited for, without an instruction
      }
    }
    return;
  }

  // ---- the workers ----
  if (workers > 0 && wave >= workers) return;  // (sliced_owned_workers: the first `workers` of them run every task)
  auto grab = [&]() {
    int k = 0;
    if (lane == 0) k = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(k);
  };
  // lane j of a group holds boundary j of the group's rows (j <= rows); a task without rows reads segptr[0] into every
  // lane: an empty run as well
  auto boundaries = [&](const OwnedWork& t) {
    return segptr[t.rows == 0 ? 0 : (int64_t)t.slice * n_dst + t.row_base + (t.lds_row + (glane < t.rows ? glane : t.rows))];
  };
  // From the boundaries `b` of a task: the group's run [beg, end), its boundaries relative to beg, and the request of
  // the two id batches a run starts with (owned_window; nothing is read for a run without edges).
  int nxt_idx = 0, nxt_idx1 = 0, rel_b = 0;
  static_assert(kOwnedWindowFirstBatches == 2, "nxt_idx and nxt_idx1");
  auto first_ids_of = [&](int b, const OwnedWork& t, int& beg, int& end) {
    beg = __shfl(b, gbase, kWave);
    rel_b = b - beg;
    end = beg + __shfl(rel_b, gbase + t.rows, kWave);
    if (beg < end) {
      nxt_idx = indices[beg + owned_window_id_edge(0, glane, end - beg)];
      nxt_idx1 = indices[beg + owned_window_id_edge(1, glane, end - beg)];
    }
  };

  constexpr int W = kOwnedWindow;
  static_assert(W <= 8 && kMultShift == 28 && LPR % W == 0, "at most eight 4-bit multiplicity fields, shifted down from bit 28");
  v4u v[W];
  int idx[W];  // the ids of a group's W issues, read at its top: an issue is a multiply and a load
  // The multiplicity fields of the W rows in flight wait in one register, the next edge's in bits 32 - 4 W ..: a
  // consumed field is shifted out, a new one comes in at bit 28 (as dgmi_owned.hip).
  uint32_t mults = 0, mults_in = 0;
  auto read_ids = [&](int batch_idx) {  // lanes 0 .. W - 1 of the group's id batch
#pragma unroll
    for (int u = 0; u < W; ++u) {
      int id = __shfl(batch_idx, gbase + u, kWave);
      if (MULT) {
        mults_in = (mults_in >> 4) | ((uint32_t)id & ((uint32_t)kMultMax << kMultShift));
        id &= kIdMask;
      }
      idx[u] = id;
    }
    if (MULT) asm volatile("" : "+v"(mults_in));  // really one register: not the W id words kept for their fields
  };

  const uint32_t row_bytes = (uint32_t)ldx * 2u;
  int k = grab();
  OwnedWork w = owned_decode(pl, wg, T, k, grp);
  int e_begin = 0, e_end = 0;
  first_ids_of(boundaries(w), w, e_begin, e_end);
  int my_rel = rel_b;  // lane j of a group: boundary j of the group's rows (j <= rows), relative to e_begin
  while (k < total) {
    const int L = e_end - e_begin;  // the group's run: 0 without rows, or with rows that have no edge in this slice
    int col = (w.col_round * LPR + glane) * 8;
    const bool col_ok = col < F;  // F % 8 == 0: all 8 columns or none
    if (!col_ok) col = 0;         // such a lane gathers column 0 and keeps its sums to itself
    const uint16_t* Xc = X + col;
    const uint32_t col_bytes = (uint32_t)col * 2u;
    if (L > 0) {  // the prologue of the window: these gathers touch neither LDS nor Y and wait for nothing
      read_ids(nxt_idx);
#pragma unroll
      for (int u = 0; u < W; ++u) v[u] = ld_row8<OFF32>(X, Xc, idx[u], ldx, row_bytes, col_bytes);
      mults = mults_in;
    }
    const int k_next = grab();
    const int next_b = boundaries(owned_decode(pl, wg, T, k_next, grp));
    // the task that used these LDS rows in the phase before (this round's, or the last one of the round before)
    while (__hip_atomic_load(&done[w.task], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < w.phase) __builtin_amdgcn_s_sleep(1);

    const int nr = w.rows;
    float4* slot_a = lds_rows + (size_t)w.lds_row * kRowSlots + glane;  // columns 0..3; columns 4..7: LPR slots further
    // the segment sum of row r of the group joins the row's running sum
    auto commit = [&](int r, const float4& a, const float4& b) {
      float4* sa = slot_a + r * kRowSlots;
      if (w.slice == 0) {
        sa[0] = a;
        sa[LPR] = b;
        return;
      }
      float4 ta = sa[0], tb = sa[LPR];
      ta.x += a.x;
      ta.y += a.y;
      ta.z += a.z;
      ta.w += a.w;
      tb.x += b.x;
      tb.y += b.y;
      tb.z += b.z;
      tb.w += b.w;
      sa[0] = ta;
      sa[LPR] = tb;
    };
    // The last slice's phase writes Y: dst_scale and the epilogue once per row, after the task's gathers, from the sums
    // this lane has just left in LDS.
    auto write_rows = [&]() {
      if (w.slice != pl.slices - 1 || !col_ok) return;
      for (int r = 0; r < nr; ++r) {
        float4 ta = slot_a[r * kRowSlots], tb = slot_a[r * kRowSlots + LPR];
        const int64_t row = w.row_base + (w.lds_row + r);
        if (dst_scale != nullptr) {
          const float d = dst_scale[row];
          ta.x *= d;
          ta.y *= d;
          ta.z *= d;
          ta.w *= d;
          tb.x *= d;
          tb.y *= d;
          tb.z *= d;
          tb.w *= d;
        }
        float* y = Y + row * ldy + col;
        *reinterpret_cast<float4*>(y) = epilogue4(ep, ta, row, col);
        *reinterpret_cast<float4*>(y + 4) = epilogue4(ep, tb, row, col + 4);
      }
    };

    int r = 0;
    float4 acc_a = make_float4(0.f, 0.f, 0.f, 0.f), acc_b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (L > 0) {
      // The rolling window (owned_window, dgmi_owned_common.h): W rows in flight from the first group of a run to its
      // last; the sum takes the edges in order, one at a time, exactly as the pair's gather does.
      int row_end = e_begin + __shfl(my_rel, gbase + 1, kWave);
      auto add = [&](int u) {  // acc + x / fmaf(m, x, acc): the canonical step, on each of the 8 columns
        const float4 va = widen(v[u].x, v[u].y), vb = widen(v[u].z, v[u].w);
        if (MULT) {
          const float m = (float)(((mults >> (32 - 4 * W)) & (uint32_t)kMultMax) + 1u);
          mults >>= 4;
          acc_a.x = fmaf(m, va.x, acc_a.x);
          acc_a.y = fmaf(m, va.y, acc_a.y);
          acc_a.z = fmaf(m, va.z, acc_a.z);
          acc_a.w = fmaf(m, va.w, acc_a.w);
          acc_b.x = fmaf(m, vb.x, acc_b.x);
          acc_b.y = fmaf(m, vb.y, acc_b.y);
          acc_b.z = fmaf(m, vb.z, acc_b.z);
          acc_b.w = fmaf(m, vb.w, acc_b.w);
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
      };
      auto rows_before = [&](int p) {  // row(s) ended before edge p (empty rows commit zeros)
        while (p >= row_end) {
          commit(r, acc_a, acc_b);
          acc_a = acc_b = make_float4(0.f, 0.f, 0.f, 0.f);
          ++r;
          row_end = e_begin + __shfl(my_rel, gbase + r + 1, kWave);
        }
      };
      int ids = nxt_idx1;  // batch 1: the ids of group 0's issues
      // The scheduling barriers pin every gather right behind the consumption of the row it replaces: left alone, the
      // scheduler sinks each load down to its use and two are in flight instead of W.
      __builtin_amdgcn_sched_barrier(0);
      int p0 = e_begin;
      // group g (not the last of its run): W edges of the run, and something to issue
      for (int g = 0; p0 + W < e_end; ++g, p0 += W) {
        read_ids(ids);  // batch g + 1, requested W gathers ago or more
        ids = indices[e_begin + owned_window_id_edge(owned_window_request_batch(g), glane, L)];  // unconditional: clamped
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < W; ++u) {
          rows_before(p0 + u);
          add(u);
          v[u] = ld_row8<OFF32>(X, Xc, idx[u], ldx, row_bytes, col_bytes);
          __builtin_amdgcn_sched_barrier(0);
        }
        mults = mults_in;
      }
      // The last group: 1 .. W edges and nothing left to issue: the window drains.
#pragma unroll
      for (int u = 0; u < W; ++u) {
        if (p0 + u < e_end) {  // group-uniform
          rows_before(p0 + u);
          add(u);
        }
      }
    }
    if (nr > 0) {
      for (; r < nr; ++r) {  // the last non-empty row, then any trailing empty rows
        commit(r, acc_a, acc_b);
        acc_a = acc_b = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      write_rows();
    }
    // nothing of the next task but its number and its boundaries is kept across this one: decoded again, and its first
    // ids requested, after the task's last row
    const OwnedWork w_then = owned_decode(pl, wg, T, k_next, grp);
    int n_begin = 0, n_end = 0;
    first_ids_of(next_b, w_then, n_begin, n_end);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) __hip_atomic_store(&done[w.task], w.phase + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    k = k_next;
    w = w_then;
    my_rel = rel_b;
    e_begin = n_begin;
    e_end = n_end;
  }
}

template <int LPR>
hipError_t launch_owned_bf16_lpr(const SlicedArgs& a, const OwnedPlan& pl, int64_t grid, bool off32, hipStream_t s) {
  const int workers = tuning().sliced_owned_workers > 0 && tuning().sliced_owned_workers < kOwnedWorkers ? tuning().sliced_owned_workers : 0;
#define DGMI_OWNED_BF16(V, O)                                                                                            \
  do {                                                                                                                   \
    auto kern = spmm_owned_bf16_kernel<LPR, V, O>;                                                                       \
    static const hipError_t attr =                                                                                       \
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10); \
    if (attr != hipSuccess) return attr;                                                                                 \
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kWave* kOwnedWaves), pl.lds_bytes, s, a.segptr, a.indices,       \
                       static_cast<const uint16_t*>(a.X), a.ldx, a.dst_scale, a.Y, a.ldy, a.n_dst, (int)a.F, pl, workers, \
                       a.ep);                                                                                            \
  } while (0)
  if (a.id_mult) {
    if (off32) DGMI_OWNED_BF16(2, true); else DGMI_OWNED_BF16(2, false);
  } else {
    if (off32) DGMI_OWNED_BF16(0, true); else DGMI_OWNED_BF16(0, false);
  }
#undef DGMI_OWNED_BF16
  return hipGetLastError();
}

}  // namespace

// No gate and one workgroup per CU: sliced_owned_lag, sliced_owned_spin_ticks and sliced_owned_wgs are ignored for a
// bf16 table, and the plane workspace goes unused (there are no arrive counters).  `pl`: owned_plan(..., cols_per_lane = 8).
hipError_t launch_owned_bf16(const SlicedArgs& a, const OwnedPlan& pl, int lpr, int64_t grid, bool off32, hipStream_t s) {
  switch (lpr) {
    case 8: return launch_owned_bf16_lpr<8>(a, pl, grid, off32, s);
    case 16: return launch_owned_bf16_lpr<16>(a, pl, grid, off32, s);
    case 32: return launch_owned_bf16_lpr<32>(a, pl, grid, off32, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dgmi

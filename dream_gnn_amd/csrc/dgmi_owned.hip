// dgmi_owned.hip — the XCD-local SpMM without partial planes: destination rows owned by a WORKGROUP, summed in its LDS.
//
// The pair (dgmi_sliced.hip) pins each XCD to one slice of the feature table, so every destination row comes out in 8
// pieces that go through 8 planes of scratch and a second launch.  Here one persistent workgroup per CU owns a
// contiguous block of destination rows and walks the 8 slices one after the other, in order, over the SAME slice-major
// layout; the running row sums stay in its LDS and Y is written once, by the last slice's phase.  No atomics: the unit
// of work is a whole (row, slice) segment — one lane group sums it in registers exactly as the pair's gather does
// (canonical in-order sum from +0) and commits it to the row's LDS slot with one plain 16-byte read-modify-write per
// lane; only one lane group ever touches a given (row, phase).  The row sum takes its 8 segment sums in slice order,
// ((s0 + s1) + s2) + ..., dst_scale and the epilogue once: bit-identical to the pair on the same layout.
//
// The plan (rows per workgroup, rounds, phases, tasks): dgmi_owned_common.h.  Inside a workgroup the 15 worker waves
// take tasks from one LDS counter, phase-major then row-major; a wave reserves its next task (and requests that task's
// row boundaries) before it runs the current one.  Task t of phase P touches the LDS rows task t of phase P - 1
// touched: done[t] counts the phases finished on slot t, release-stored after a task's LDS writes and acquire-polled
// before the next one's first LDS access.  The lowest unfinished task never waits (everything before it is finished and
// a reserved task is only ever held by a wave that runs an earlier one), so this cannot deadlock; it also orders the
// reuse of the LDS rows by the next round.
//
// A worker keeps a ROLLING WINDOW of gathers in flight across its lane groups' whole runs (all R rows of the task):
// right after it has added edge e's row to the sum it issues edge e + W into the registers that row has left, so the
// gathers in flight stay at W from the first group of a run to its last instead of swinging between W and 0 once per
// batch — at 4 waves per SIMD nobody else fills that hole.  The sum still takes the edges one at a time, in order.  The
// window's index arithmetic (id batches of W, the clamp past the end of a run): owned_window, dgmi_owned_common.h.  It
// drains at the end of a task.  Measured (profiles/owned_window/README.md): W = 4 — no more rows in flight than the
// batches of 8 averaged, but never none; at W = 8 the unit-value products lose 4-8 points of L2 hits — runs the kNN-64
// classes 20 % and 9 % and the unit-value classes 6 % faster in loops of their own, the step of bench.py 5 %.
//
// The 16th wave is the toucher: it walks the same task order a few tasks ahead of the counter and touches one word per
// 128-B line of the boundaries and ids the workers are about to read (they issue no cold loads), and it keeps the
// ADVISORY phase gate: the workgroups of an XCD (label blockIdx % 8 — a speed assumption, as is their co-residency)
// should gather from the same slice at the same time, so a workgroup opens phase P for its workers once every workgroup
// of its label has finished phase P - 1 - lag, or a time bound has passed.  Leaders wait, the slowest never does, every
// spin is bounded and results never depend on it.  It is off unless asked for (kOwnedLag): measured, it costs more than it buys.
// A launch without a gate carries no gate work: no memset of the arrive counters, no counting of a phase's tasks.
//
// Two forms of the one kernel (WAVES): a 16-wave workgroup per CU, or — the cap of 1024 threads per workgroup lifted —
// two co-resident 12-wave workgroups per CU, each with half the LDS rows (owned_plan's wgs_per_cu): 22 workers instead
// of 15, 6 waves per SIMD.  Their co-residency is asked of the runtime once per kernel and LDS size; where it says no,
// the 16-wave form runs.  Nothing waits for the other workgroup of a CU.  Measured (profiles/owned_wgs/README.md): the
// kernel is short of waves (12 instead of 16 per CU: +17-23 %), yet 512 free-running workgroups drift over more slices
// than 256 and lose in L2 misses more than the waves return, so the built-in rule selects the second form for no class.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>

#include "dgmi_owned_common.h"
#include "dgmi_sliced_common.h"

namespace dgmi {
namespace {

constexpr int kOwnedTouchChunk = 4;      // tasks the toucher touches for at a time
constexpr int kOwnedTouchLead = 8;       // tasks between the counter and the first task of the chunk it touches for
constexpr int64_t kOwnedSpinTicks = 3000;  // 30 us of the 100 MHz real-time counter: a stuck gate falls through
constexpr int64_t kOwnedMinRows = 32768;   // built-in rule: below, a workgroup has too few tasks per phase
// Built-in gate: none.  A closed gate drains the workgroup — a task lives ~5 us of a ~15 us phase — so lag 0 costs
// 35-45 % and lag 1 25-30 % of a product, far more than the L2 hits it buys (profiles/owned_rows/README.md).
constexpr int kOwnedLag = -1;

struct OwnedWork {  // task k of a workgroup, decoded (wave-uniform except row0 / lds_row / rows: per lane group)
  int phase, task, slice, col_round;
  int64_t row0;
  int lds_row, rows;
};

__device__ __forceinline__ OwnedWork owned_decode(const OwnedPlan& pl, int64_t wg, int T, int k, int grp) {
  OwnedWork w;
  w.phase = k / T;
  w.task = k - w.phase * T;
  const OwnedPhase ph = owned_phase(pl, w.phase);
  w.slice = ph.slice;
  w.col_round = ph.col_round;
  const OwnedTask t = owned_task(pl, wg, ph.row_round, w.task, grp);
  w.row0 = t.row0;
  w.lds_row = t.lds_row;
  w.rows = t.rows;
  return w;
}

// VALS: 0 = unit edge values, 2 = multiplicities in the id words (dgmi_sliced.hip).  WAVES: waves of the workgroup, the
// last one the toucher: kOwnedWaves (one workgroup per CU, 4 waves per SIMD) or kOwnedPairWaves (two co-resident
// workgroups per CU, 6 waves per SIMD: the register budget the second launch bound asks the compiler for).
template <int LPR, int VALS, bool OFF32, int WAVES>
__global__ __launch_bounds__(kWave* WAVES, WAVES == kOwnedWaves ? 4 : 6) void spmm_owned_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ dst_scale, float* __restrict__ Y, int64_t ldy, int64_t n_dst, int F, OwnedPlan pl,
    unsigned* __restrict__ arrive, int lag, int64_t spin_ticks, Epilogue ep) {
  constexpr bool MULT = VALS == 2;
  constexpr int kIdMask = MULT ? (int)kMultIdMask : 0x7fffffff;
  extern __shared__ float4 lds_rows[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int grp = lane / LPR, glane = lane % LPR, gbase = grp * LPR;
  const int64_t wg = blockIdx.x;
  const int T = owned_wg_tasks(pl, wg);
  if (T == 0) return;  // block-uniform: a workgroup without rows
  int* done = reinterpret_cast<int*>(lds_rows + (size_t)pl.round_rows * LPR);  // [tasks] phases finished on a task slot
  int* phase_cnt = done + pl.tasks;                                           // [phases] tasks finished of a phase (gate only)
  int* counter = phase_cnt + pl.phases;                                       // next task
  int* open = counter + 1;                                                    // highest phase the gate has opened
  for (int i = threadIdx.x; i < pl.tasks + pl.phases + 2; i += blockDim.x) done[i] = 0;
  __syncthreads();
  const int total = pl.phases * T;
  const int label = (int)(blockIdx.x & 7u);

  if (wave == WAVES - 1) {  // ---- the toucher ----
    const unsigned n_label = (unsigned)((pl.active - label + 7) >> 3);  // active workgroups with this label (>= 1: this one)
    const unsigned* my_arrive = arrive + (size_t)label * pl.phases;
    // One loop does both jobs and blocks in neither: touch the next chunk of tasks once the counter is within the lead
    // of it (also across a phase boundary: while the workers stand at a closed gate the first tasks behind it get
    // touched), and open the next phase once its condition holds.
    const int chunks_per_phase = (T + kOwnedTouchChunk - 1) / kOwnedTouchChunk, chunks = pl.phases * chunks_per_phase;
    const int last_gate = lag >= 0 ? pl.phases - 1 : 0;
    int keepalive = 0, touched = 0, opened = 0;
    bool waiting = false;
    uint64_t wait_start = 0;
    while (touched < chunks || opened < last_gate) {
      bool idle = true;
      const int next = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (touched < chunks) {
        const int P = touched / chunks_per_phase, t0 = (touched - P * chunks_per_phase) * kOwnedTouchChunk;
        if (P * T + t0 <= next + kOwnedTouchLead) {
          ++touched;
          idle = false;
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
      }
      if (opened < last_gate) {
        const int P = opened + 1, need = P - 1 - lag;
        bool ok = need < 0 || __hip_atomic_load(&my_arrive[need], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_label;
        if (!ok && next >= P * T) {  // this workgroup's workers stand at the gate: the bound runs from here
          const uint64_t now = __builtin_amdgcn_s_memrealtime();
          if (!waiting) {
            waiting = true;
            wait_start = now;
          } else if (now - wait_start >= (uint64_t)spin_ticks) {
            ok = true;
          }
        }
        if (ok) {
          opened = P;
          waiting = false;
          idle = false;
          __hip_atomic_store(open, P, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      if (idle) __builtin_amdgcn_s_sleep(2);
    }
    return;
  }

  // ---- the workers ----
  auto grab = [&]() {
    int k = 0;
    if (lane == 0) k = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(k);
  };
  // lane j of a group holds boundary j of the group's rows (j <= rows)
  auto boundaries = [&](int k) {
    if (k >= total) return 0;
    const OwnedWork w = owned_decode(pl, wg, T, k, grp);
    if (w.rows == 0) return 0;
    return segptr[(int64_t)w.slice * n_dst + w.row0 + (glane < w.rows ? glane : w.rows)];
  };
  // id batch `batch` (0 / 1: the two a run starts with, owned_window) of a group whose boundaries have arrived
  auto first_ids = [&](int my_b, int rows, int batch) {
    const int e_begin = __shfl(my_b, gbase, kWave), e_end = __shfl(my_b, gbase + rows, kWave);
    if (rows == 0 || e_begin >= e_end) return 0;
    return indices[e_begin + owned_window_id_edge(batch, glane, e_end - e_begin)];
  };
  static_assert(kOwnedWindowFirstBatches == 2, "nxt_idx and nxt_idx1");

  const uint32_t row_bytes = (uint32_t)ldx * 4u;
  int k = grab();
  int my_b = boundaries(k);
  int nxt_idx = k < total ? first_ids(my_b, owned_decode(pl, wg, T, k, grp).rows, 0) : 0;
  int nxt_idx1 = k < total ? first_ids(my_b, owned_decode(pl, wg, T, k, grp).rows, 1) : 0;
  while (k < total) {
    const OwnedWork w = owned_decode(pl, wg, T, k, grp);
    const int k_next = grab();
    const int next_b = boundaries(k_next);  // in flight during this task's gathers
    if (lag >= 0)
      while (__hip_atomic_load(open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < w.phase) __builtin_amdgcn_s_sleep(1);
    // the task that used these LDS rows in the phase before (this round's, or the last one of the round before)
    while (__hip_atomic_load(&done[w.task], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < w.phase) __builtin_amdgcn_s_sleep(1);

    const int nr = w.rows;
    int col = (w.col_round * LPR + glane) * 4;
    const bool col_ok = col < F;
    if (!col_ok) col = 0;  // such a lane gathers column 0 and keeps its sums to itself
    const float* Xc = X + col;
    const uint32_t col_bytes = (uint32_t)col * 4u;
    float4* slot = lds_rows + (size_t)w.lds_row * LPR + glane;
    // the segment sum of row r of the group joins the row's running sum
    auto commit = [&](int r, const float4& acc) {
      if (w.slice == 0) {
        slot[r * LPR] = acc;
        return;
      }
      float4 t = slot[r * LPR];
      t.x += acc.x;
      t.y += acc.y;
      t.z += acc.z;
      t.w += acc.w;
      slot[r * LPR] = t;
    };
    // The last slice's phase writes Y: dst_scale and the epilogue once per row, after the task's gathers — not inside
    // commit, where the scale, the mask and the addresses of Y would be live next to 8 gathered rows — from the sums
    // this lane has just left in LDS.
    auto write_rows = [&]() {
      if (w.slice != kOwnedSlices - 1 || !col_ok) return;
      for (int r = 0; r < nr; ++r) {
        float4 t = slot[r * LPR];
        const int64_t row = w.row0 + r;
        if (dst_scale != nullptr) {
          const float d = dst_scale[row];
          t.x *= d;
          t.y *= d;
          t.z *= d;
          t.w *= d;
        }
        *reinterpret_cast<float4*>(Y + row * ldy + col) = epilogue4(ep, t, row, col);
      }
    };

    if (nr > 0) {
      const int e_begin = __shfl(my_b, gbase, kWave);
      const int e_end = __shfl(my_b, gbase + nr, kWave);
      int r = 0;
      int row_end = __shfl(my_b, gbase + 1, kWave);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e_begin < e_end) {
        // The rolling window (owned_window, dgmi_owned_common.h): W rows in flight from the prologue to the last group;
        // the sum takes the edges in order, one at a time, exactly as the pair's gather does.
        constexpr int W = kOwnedWindow;
        static_assert(W <= 8 && kMultShift == 28 && LPR % W == 0, "at most eight 4-bit multiplicity fields, shifted down from bit 28");
        const int L = e_end - e_begin;
        float4 v[W];
        int idx[W];  // the ids of a group's W issues, read at its top: an issue is a multiply and a load
        // The multiplicity fields of the W rows in flight wait in one register, the next edge's in bits 32 - 4 W ..: a
        // consumed field is shifted out, a new one comes in at bit 28.  Those of the W ids read at a group's top collect
        // in a second register and replace the first after the group.
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
        auto add = [&](int u) {  // acc + x / fmaf(m, x, acc): the canonical step
          if (MULT) {
            const float m = (float)(((mults >> (32 - 4 * W)) & (uint32_t)kMultMax) + 1u);
            mults >>= 4;
            acc.x = fmaf(m, v[u].x, acc.x);
            acc.y = fmaf(m, v[u].y, acc.y);
            acc.z = fmaf(m, v[u].z, acc.z);
            acc.w = fmaf(m, v[u].w, acc.w);
          } else {
            acc.x += v[u].x;
            acc.y += v[u].y;
            acc.z += v[u].z;
            acc.w += v[u].w;
          }
        };
        auto rows_before = [&](int p) {  // row(s) ended before edge p (empty rows commit zeros)
          while (p >= row_end) {
            commit(r, acc);
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            ++r;
            row_end = __shfl(my_b, gbase + r + 1, kWave);
          }
        };
        read_ids(nxt_idx);
        int ids = nxt_idx1;  // the id batch of the next issues
#pragma unroll
        for (int u = 0; u < W; ++u) v[u] = ld_row<OFF32>(X, Xc, idx[u], ldx, row_bytes, col_bytes);
        mults = mults_in;
        // The scheduling barriers pin every gather right behind the consumption of the row it replaces: left alone, the
        // scheduler sinks each load down to its use and two are in flight instead of W.
        __builtin_amdgcn_sched_barrier(0);
        int p0 = e_begin;
        for (int g = 0; p0 + W < e_end; ++g, p0 += W) {  // group g: W edges of the run, and something to issue
          read_ids(ids);  // batch g + 1, requested W gathers ago or more
          ids = indices[e_begin + owned_window_id_edge(owned_window_request_batch(g), glane, L)];  // unconditional: clamped
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < W; ++u) {
            rows_before(p0 + u);
            add(u);
            v[u] = ld_row<OFF32>(X, Xc, idx[u], ldx, row_bytes, col_bytes);
            __builtin_amdgcn_sched_barrier(0);
          }
          mults = mults_in;
        }
#pragma unroll
        for (int u = 0; u < W; ++u) {  // the last group: 1 .. W edges, nothing left to issue — the window drains
          if (p0 + u < e_end) {        // group-uniform
            rows_before(p0 + u);
            add(u);
          }
        }
      }
      for (; r < nr; ++r) {  // the last non-empty row, then any trailing empty rows
        commit(r, acc);
        acc = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      write_rows();
    }
    // the next task's first ids, requested before this one is reported (its boundaries arrived long ago)
    nxt_idx = k_next < total ? first_ids(next_b, owned_decode(pl, wg, T, k_next, grp).rows, 0) : 0;
    nxt_idx1 = k_next < total ? first_ids(next_b, owned_decode(pl, wg, T, k_next, grp).rows, 1) : 0;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      __hip_atomic_store(&done[w.task], w.phase + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (lag >= 0) {  // only a gate reads the arrive counters: without one nobody counts a phase's tasks either
        const int finished = __hip_atomic_fetch_add(&phase_cnt[w.phase], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (finished == T - 1)
          __hip_atomic_fetch_add(&arrive[(size_t)label * pl.phases + w.phase], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    k = k_next;
    my_b = next_b;
  }
}

int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 0;
    return n;
  }();
  return cus;
}

// The built-in rule: the classes (column rounds, row rounds, multiplicities in the ids, bytes of the source table) whose
// product, inside the step of bench.py, was faster with this form than with the pair by more than the pair's own
// run-to-run spread.  Three classes cleared that:
//  - a full-width table of 8 L2-sized slices gathered into twice a workgroup's LDS rows (config 4's 50 000 sources ->
//    100 000 rows, unit values): profiles/owned_rows/README.md;
//  - with the rolling gather window (profiles/owned_window/README.md) both kNN-64 classes: the half-width 100 000-node
//    one (two column rounds, one row round, 51 MB table: -10 %) and the full-width 50 000-node one (one column round, one
//    row round: -7 %).
// The two-pass unit-value products (100 000 sources -> 50 000 rows) are within a spread of the pair: they stay on it.
// `pl`: the plan of one workgroup per CU, which names the class.  0 = the pair, 1 = one 16-wave workgroup per CU,
// 2 = two 12-wave workgroups per CU.  No class takes 2: forced for all 8 products of the step it ran every one of them
// 30-35 % slower than the pair (profiles/owned_wgs/README.md); it stays behind sliced_owned_wgs = 2.
int owned_class_form(const OwnedPlan& pl, bool id_mult, int64_t table_bytes) {
  const auto mib = [&](int64_t lo, int64_t hi) { return table_bytes >= (lo << 20) && table_bytes <= (hi << 20); };
  if (pl.col_rounds == 1 && pl.row_rounds == 2 && !id_mult && mib(16, 32)) return 1;
  if (pl.col_rounds == 2 && pl.row_rounds == 1 && id_mult && mib(48, 64)) return 1;
  if (pl.col_rounds == 1 && pl.row_rounds == 1 && id_mult && mib(16, 32)) return 1;
  return 0;
}

// Whether `wgs` workgroups of `threads` threads and `lds` bytes of dynamic LDS of this kernel are resident on one CU
// together, by the runtime's occupancy query; asked once per kernel and LDS size.  A speed question only: a grid that
// does not co-reside runs in two rounds and is still correct, so the caller then takes the one-workgroup form.
bool owned_coresident(const void* kern, int threads, size_t lds, int wgs) {
  static std::mutex mu;
  static std::map<std::pair<const void*, size_t>, int> known;
  std::lock_guard<std::mutex> lock(mu);
  auto it = known.find({kern, lds});
  if (it == known.end()) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, threads, lds) != hipSuccess) {
      (void)hipGetLastError();
      n = 0;
    }
    it = known.emplace(std::make_pair(kern, lds), n).first;
  }
  return it->second >= wgs;
}

// `resident` (the two-workgroup form only): false = its workgroups would not share a CU, nothing was launched.  The
// 8-lane groups with multiplicities are not built in that form: they do not fit its 80 VGPRs without scratch.
template <int LPR, int WAVES>
hipError_t launch_owned(const SlicedArgs& a, const OwnedPlan& pl, int64_t grid, bool off32, int lag, int64_t spin_ticks,
                        hipStream_t s, bool* resident) {
  constexpr int kWgsPerCu = WAVES == kOwnedWaves ? 1 : 2;
  unsigned* arrive = reinterpret_cast<unsigned*>(a.planes);
  *resident = true;
#define DGMI_OWNED(V, O)                                                                                                  \
  do {                                                                                                                    \
    if constexpr (kWgsPerCu > 1 && LPR == 8 && V == 2) {                                                                  \
      *resident = false;                                                                                                  \
      return hipSuccess;                                                                                                  \
    } else {                                                                                                              \
    auto kern = spmm_owned_kernel<LPR, V, O, WAVES>;                                                                      \
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                               \
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (160 << 10) / kWgsPerCu); \
    if (attr != hipSuccess) return attr;                                                                                  \
    if (kWgsPerCu > 1 && !owned_coresident(reinterpret_cast<const void*>(kern), kWave * WAVES, pl.lds_bytes, kWgsPerCu)) { \
      *resident = false;                                                                                                  \
      return hipSuccess;                                                                                                  \
    }                                                                                                                     \
    if (lag >= 0) { /* only a gate reads the arrive counters */                                                           \
      const hipError_t err = hipMemsetAsync(arrive, 0, sizeof(unsigned) * 8 * (size_t)pl.phases, s);                      \
      if (err != hipSuccess) return err;                                                                                  \
    }                                                                                                                     \
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kWave* WAVES), pl.lds_bytes, s, a.segptr, a.indices,              \
                       static_cast<const float*>(a.X), a.ldx, a.dst_scale, a.Y, a.ldy, a.n_dst, (int)a.F, pl, arrive, lag, \
                       spin_ticks, a.ep);                                                                                 \
    }                                                                                                                     \
  } while (0)
  if (a.id_mult) {
    if (off32) DGMI_OWNED(2, true); else DGMI_OWNED(2, false);
  } else {
    if (off32) DGMI_OWNED(0, true); else DGMI_OWNED(0, false);
  }
#undef DGMI_OWNED
  return hipGetLastError();
}

}  // namespace

hipError_t spmm_owned_try(const SlicedArgs& a, hipStream_t s, bool* taken) {
  *taken = false;
  const Tuning& tune = tuning();
  if (tune.sliced_owned == 0) return hipSuccess;
  if (a.x_bytes != 4 || a.vals != nullptr || a.src_scale != nullptr || a.n_keep != 0 || a.n_slices != kOwnedSlices ||
      tune.sliced_chunk_rows > 0 || a.chunk_rows < a.n_dst || a.n_dst == 0 || a.F == 0)
    return hipSuccess;
  // a forced grid counts workgroups, whichever form runs them
  const int64_t grid = tune.sliced_owned_grid > 0 ? tune.sliced_owned_grid : device_cus();
  if (grid < 1) return hipSuccess;
  const int lpr = sliced_lpr(a.F, a.n_src, a.n_slices, a.n_dst, a.full_width, a.n_keep, a.x_bytes, tune.sliced_lpr);
  // the one-workgroup plan names the class and is what a two-workgroup launch that cannot co-reside falls back to
  const OwnedPlan pl = owned_plan(a.n_dst, a.F, lpr, grid, tune.sliced_owned_rows, tune.sliced_owned_lds_rows);
  if (!pl.ok || pl.lds_bytes > (size_t)(160 << 10)) return hipSuccess;
  // the arrive counters live in the first bytes of the caller's plane workspace (n_slices * n_dst * ldp floats)
  const auto arrive_fits = [&](const OwnedPlan& p) {
    return sizeof(unsigned) * 8 * (size_t)p.phases <= sizeof(float) * (size_t)a.n_slices * (size_t)a.n_dst * (size_t)a.ldp;
  };
  if (!arrive_fits(pl)) return hipSuccess;
  const int rule = a.n_dst < kOwnedMinRows ? 0 : owned_class_form(pl, a.id_mult, a.n_src * a.ldx * (int64_t)sizeof(float));
  if (tune.sliced_owned != 1 && rule == 0) return hipSuccess;
  const int form = tune.sliced_owned_wgs == 1 || tune.sliced_owned_wgs == 2 ? tune.sliced_owned_wgs : (rule == 2 ? 2 : 1);
  const bool off32 = !tune.sliced_no_off32 && (a.n_src * a.ldx + a.F) * 4 < ((int64_t)1 << 32);
  const int64_t spin = tune.sliced_owned_spin_ticks > 0 ? tune.sliced_owned_spin_ticks : kOwnedSpinTicks;
  const int lag = tune.sliced_owned_lag >= -1 ? tune.sliced_owned_lag : kOwnedLag;
  *taken = true;
  bool resident = true;
  if (form == 2) {
    const int64_t grid2 = tune.sliced_owned_grid > 0 ? grid : 2 * grid;
    const OwnedPlan pl2 = owned_plan(a.n_dst, a.F, lpr, grid2, tune.sliced_owned_rows, tune.sliced_owned_lds_rows, 2);
    if (pl2.ok && pl2.lds_bytes <= (size_t)(80 << 10) && arrive_fits(pl2)) {
      hipError_t err;
      switch (lpr) {
        case 8: err = launch_owned<8, kOwnedPairWaves>(a, pl2, grid2, off32, lag, spin, s, &resident); break;
        case 16: err = launch_owned<16, kOwnedPairWaves>(a, pl2, grid2, off32, lag, spin, s, &resident); break;
        case 32: err = launch_owned<32, kOwnedPairWaves>(a, pl2, grid2, off32, lag, spin, s, &resident); break;
        default: err = launch_owned<64, kOwnedPairWaves>(a, pl2, grid2, off32, lag, spin, s, &resident); break;
      }
      if (err != hipSuccess || resident) return err;
    }
  }
  switch (lpr) {
    case 8: return launch_owned<8, kOwnedWaves>(a, pl, grid, off32, lag, spin, s, &resident);
    case 16: return launch_owned<16, kOwnedWaves>(a, pl, grid, off32, lag, spin, s, &resident);
    case 32: return launch_owned<32, kOwnedWaves>(a, pl, grid, off32, lag, spin, s, &resident);
    default: return launch_owned<64, kOwnedWaves>(a, pl, grid, off32, lag, spin, s, &resident);
  }
}

}  // namespace dgmi

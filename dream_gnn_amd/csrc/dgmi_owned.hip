// dgmi_owned.hip — the XCD-local SpMM without partial planes: destination rows owned by a WORKGROUP, summed in its LDS.
//
// The pair (dgmi_sliced.hip) pins each XCD to one slice of the feature table, so every destination row comes out in 8
// pieces that go through 8 planes of scratch and a second launch.  Here one persistent workgroup per CU owns a
// contiguous block of destination rows and walks the slices one after the other, in order, over the SAME slice-major
// layout; the running row sums stay in its LDS and Y is written once, by the last slice's phase.  Nothing binds a
// workgroup to an XCD, so the layout may have any number S of slices the builders make (OwnedPlan::slices; 8 in the
// text below): where 8 slices of a table do not fit an L2 at full width, 16 do (dgmi_sliced_layout_slices, at the end).
// No atomics: the unit of work is a whole (row, slice) segment — one lane group sums it in registers exactly as the
// pair's gather does (canonical in-order sum from +0) and commits it to the row's LDS slot with one plain 16-byte
// read-modify-write per lane; only one lane group ever touches a given (row, phase).  The row sum takes its S segment
// sums in slice order, ((s0 + s1) + s2) + ..., dst_scale and the epilogue once: bit-identical to the pair on the same
// layout.
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
// window's index arithmetic (id batches of W, the clamp past the end of a run): owned_window, dgmi_owned_common.h.
// Measured (profiles/owned_window/README.md): W = 4 — no more rows in flight than the batches of 8 averaged, but never
// none; at W = 8 the unit-value products lose 4-8 points of L2 hits — runs the kNN-64 classes 20 % and 9 % and the
// unit-value classes 6 % faster in loops of their own, the step of bench.py 5 %.
//
// The window is HANDED OVER from task to task (owned_carry, dgmi_owned_common.h; the 16-wave form with multiplicities
// in the ids — the other instantiations keep the draining loop, see CARRY): in the last group of
// its run a lane group refills every slot, right behind its consumption, with the first W edges of its run in the
// wave's next task — that task's ids, its column offset — so the next task starts with its window full: no prologue,
// no wait for ids.  The next task's boundaries are requested when it is reserved and taken over at ONE wave-uniform
// point per task, behind the wait for done[]: there its run is found, its first two id batches and its scales are
// requested, and the wait for the boundaries is the wait for the carried gathers the first group needs at once.  A run
// behind a run without edges starts cold, as does a wave's first; a run in front of one without edges hands nothing over,
// and past the last task nothing is issued.  A task is decoded once, when it is reserved.  The sums, their order and every bit stay what they were.  Measured:
// profiles/owned_carry/README.md.
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
//
// A bf16 table (x_bytes == 2) takes the same form through the same launcher (spmm_owned_try) and the same plan with 8
// columns per lane; its kernel — the 16-wave form without a gate — is dgmi_owned_bf16.hip, its classes are
// owned_class_form's for x_bytes == 2.
#include <hip/hip_runtime.h>
#include <limits.h>
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
constexpr int kOwnedWideSlices = 16;       // the slice count of the one class whose layout is not the pair's (dgmi_sliced_layout_slices)
constexpr int kOwnedAssumedCus = 256;      // workgroups the layout rule plans for where no device can be asked (MI355X)

// VALS: 0 = unit edge values, 2 = multiplicities in the id words (dgmi_sliced.hip).  WAVES: waves of the workgroup, the
// last one the toucher: kOwnedWaves (one workgroup per CU, 4 waves per SIMD) or kOwnedPairWaves (two co-resident
// workgroups per CU, 6 waves per SIMD: the register budget the second launch bound asks the compiler for).
template <int LPR, int VALS, bool OFF32, int WAVES>
__global__ __launch_bounds__(kWave* WAVES, WAVES == kOwnedWaves ? 4 : 6) void spmm_owned_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ dst_scale, float* __restrict__ Y, int64_t ldy, int64_t n_dst, int F, OwnedPlan pl,
    unsigned* __restrict__ arrive, int lag, int64_t spin_ticks, int workers, Epilogue ep) {
  constexpr bool MULT = VALS == 2;
  constexpr int kIdMask = MULT ? (int)kMultIdMask : 0x7fffffff;
  // The window is handed from task to task (false: every run starts cold — the same bits).  Not in the two-workgroup
  // form: next to its 80 VGPRs the window and the next task's run do not stay in registers across the boundary.  Not
  // for unit values either: measured (profiles/owned_carry/README.md), their products lose 2 points of L2 hits and
  // 0.3-0.6 % of their time to it, while the products with multiplicities gain.
  constexpr bool CARRY = WAVES == kOwnedWaves && MULT;
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
  // lane j of a group holds dst_scale of the group's row j: only the last slice's phase, which writes Y, asks for it
  auto scales = [&](const OwnedWork& t) {
    if (!CARRY || dst_scale == nullptr || t.slice != pl.slices - 1 || t.rows == 0) return 0.f;
    return dst_scale[t.row_base + (t.lds_row + (glane < t.rows ? glane : t.rows - 1))];
  };
  // The hand-over point of a task, WAVE-UNIFORM and right behind the wait for done[]: the boundaries `b` of the NEXT
  // task, requested when it was reserved, are waited for — with them (vmcnt is in order) the gathers the task before
  // has carried into this one, which this task's first group consumes at once; nothing else is in flight.  It finds
  // the group's run [beg, end) in the next task, keeps its boundaries relative to beg, requests the two id batches a
  // run starts with (owned_window; nothing is read for a run without edges) and the scales of the next task's rows;
  // those requested at the task before are this task's (my_ds): write_rows waits for no load.  Why here and not a
  // group later, without any wait: the lane groups of a wave diverge, and the compiler counts the loads in flight
  // along every path through the linearised branches — also those on which a group has issued nothing; a load
  // consumed inside a branch is, for it, still pending after the branch, and the next wait for it (or for the
  // registers it has left) empties the window.  At a uniform point every count is exact
  // (profiles/owned_carry/README.md).
  int nxt_idx = 0, nxt_idx1 = 0, rel_b = 0;
  float my_ds = 0.f, nxt_ds = 0.f;
  static_assert(kOwnedWindowFirstBatches == 2, "nxt_idx and nxt_idx1");
  auto hand_over = [&](int b, const OwnedWork& nxt, int& beg, int& end) {
    beg = __shfl(b, gbase, kWave);
    rel_b = b - beg;
    end = beg + __shfl(rel_b, gbase + nxt.rows, kWave);
    if (beg < end) {  // lane l of batch 0 holds the id slot l % W is refilled with, or the prologue issues
      nxt_idx = indices[beg + owned_carry_slot_edge(glane % kOwnedWindow, end - beg)];
      nxt_idx1 = indices[beg + owned_window_id_edge(owned_carry_start_batch(), glane, end - beg)];
    }
    my_ds = nxt_ds;
    nxt_ds = scales(nxt);
  };

  // The window (owned_window, owned_carry: dgmi_owned_common.h) lives across the tasks of a wave.
  constexpr int W = kOwnedWindow;
  static_assert(W <= 8 && kMultShift == 28 && LPR % W == 0, "at most eight 4-bit multiplicity fields, shifted down from bit 28");
  float4 v[W];
  int idx[W];   // the ids of a group's W issues, read at its top: an issue is a multiply and a load
  int nidx[W];  // the ids of the W edges the last group of a run carries into the next task
  // The multiplicity fields of the W rows in flight wait in one register, the next edge's in bits 32 - 4 W ..: a
  // consumed field is shifted out, a new one comes in at bit 28.  Those of the W ids read at a group's top collect
  // in a second register and replace the first after the group.
  uint32_t mults = 0, mults_in = 0, nmults = 0;
  bool carried = false;  // per lane group: its window is full of the first W edges of the run it is about to sum
  auto read_batch = [&](int batch_idx, int (&out)[W], uint32_t& fields) {  // lanes 0 .. W - 1 of the group's id batch
#pragma unroll
    for (int u = 0; u < W; ++u) {
      int id = __shfl(batch_idx, gbase + u, kWave);
      if (MULT) {
        fields = (fields >> 4) | ((uint32_t)id & ((uint32_t)kMultMax << kMultShift));
        id &= kIdMask;
      }
      out[u] = id;
    }
    if (MULT) asm volatile("" : "+v"(fields));  // really one register: not the W id words kept for their fields
  };
  auto read_ids = [&](int batch_idx) { read_batch(batch_idx, idx, mults_in); };

  const uint32_t row_bytes = (uint32_t)ldx * 4u;
  int k = grab();
  OwnedWork w = owned_decode(pl, wg, T, k, grp);
  int e_begin = 0, e_end = 0;
  hand_over(boundaries(w), w, e_begin, e_end);
  int my_rel = rel_b;  // lane j of a group: boundary j of the group's rows (j <= rows), relative to e_begin
  while (k < total) {
    const int L = e_end - e_begin;  // the group's run: 0 without rows, or with rows that have no edge in this slice
    int col = (w.col_round * LPR + glane) * 4;
    const bool col_ok = col < F;
    if (!col_ok) col = 0;  // such a lane gathers column 0 and keeps its sums to itself
    const float* Xc = X + col;
    const uint32_t col_bytes = (uint32_t)col * 4u;
    // A cold start (the first task of a wave, or a run before this one without edges): the prologue of the window.
    if (L > 0 && !carried) {
      read_ids(nxt_idx);
#pragma unroll
      for (int u = 0; u < W; ++u) v[u] = ld_row<OFF32>(X, Xc, idx[u], ldx, row_bytes, col_bytes);
      mults = mults_in;
    }
    const int k_next = grab();
    const OwnedWork w_next = owned_decode(pl, wg, T, k_next, grp);
    const int next_b = boundaries(w_next);
    int n_begin = 0, n_end = 0;  // the group's run in the next task
    if (lag >= 0)
      while (__hip_atomic_load(open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < w.phase) __builtin_amdgcn_s_sleep(1);
    // the task that used these LDS rows in the phase before (this round's, or the last one of the round before)
    while (__hip_atomic_load(&done[w.task], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < w.phase) __builtin_amdgcn_s_sleep(1);
    const int first_ids = nxt_idx1;  // this run's batch 1 (owned_carry_start_batch), before the next run's replaces it
    static_assert(owned_carry_start_batch() == 1, "nxt_idx1");
    if (CARRY) hand_over(next_b, w_next, n_begin, n_end);

    const int nr = w.rows;
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
    // this lane has just left in LDS.  The scales were requested when the task was reserved and have arrived (my_ds): no load
    // stands between the task's sums and the release of done[].
    auto write_rows = [&]() {
      if (w.slice != pl.slices - 1) return;
      for (int r = 0; r < nr; ++r) {
        float d = 0.f;
        if (CARRY) d = __shfl(my_ds, gbase + r, kWave);  // (by every lane of the group)
        if (!col_ok) continue;
        float4 t = slot[r * LPR];
        const int64_t row = w.row_base + (w.lds_row + r);
        if (dst_scale != nullptr) {
          if (!CARRY) d = dst_scale[row];
          t.x *= d;
          t.y *= d;
          t.z *= d;
          t.w *= d;
        }
        *reinterpret_cast<float4*>(Y + row * ldy + col) = epilogue4(ep, t, row, col);
      }
    };

    bool carry = false;             // whether the group hands its window over to its run in the next task
    int r = 0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (L > 0) {
      // The rolling window (owned_window, dgmi_owned_common.h): W rows in flight from the first group of a run to its
      // last; the sum takes the edges in order, one at a time, exactly as the pair's gather does.
      int row_end = e_begin + __shfl(my_rel, gbase + 1, kWave);
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
          row_end = e_begin + __shfl(my_rel, gbase + r + 1, kWave);
        }
      };
      int ids = first_ids;  // the id batch of the next issues, whether the run starts warm or cold
      // The scheduling barriers pin every gather right behind the consumption of the row it replaces: left alone, the
      // scheduler sinks each load down to its use and two are in flight instead of W.
      __builtin_amdgcn_sched_barrier(0);
      int p0 = e_begin;
      carry = CARRY && owned_carry(L, n_end - n_begin);
      auto group = [&](int g) {  // group g (not the last of its run): W edges of the run, and something to issue
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
      };
      // Where this run and the group's run in the next task both have edges (owned_carry) the last group refills slot u,
      // right behind its consumption, with edge u of that run — lane u of its batch 0 (owned_carry_slot_edge), the next
      // task's column offset — and the next task starts with its window full.  These gathers touch neither LDS nor Y
      // and wait for neither done[] nor the gate.  The batch is read behind group 0 (owned_carry_read_group), W gathers
      // after its request; a run of one or two groups reads it before its last group, and waits.
      // Groups 0 and 1 of a run of three groups or more stand in one straight line in front of the loop, the read between
      // them: the form in which the compiler keeps the ring v[] in place (a single group in front of its rotated loop
      // makes it copy a slot behind a vmcnt(0), and so does a read under a condition inside the loop).
      static_assert(owned_carry_read_group(2 * W + 1) == 0 && owned_carry_read_group(2 * W) == -1, "behind group 0 of three or more");
      int g = 0;
      if (owned_carry_read_group(L) == 0) {
        group(0);
        p0 += W;
        if (carry) read_batch(nxt_idx, nidx, nmults);
        group(1);
        p0 += W;
        g = 2;
      } else {
        if (p0 + W < e_end) {
          group(0);
          p0 += W;
          g = 1;
        }
        if (carry) read_batch(nxt_idx, nidx, nmults);  // a run of one or two groups: waits for the batch
      }
      for (; p0 + W < e_end; ++g, p0 += W) group(g);
      // The last group: 1 .. W edges and nothing left to issue of this run.
      const float* Xn = X;
      uint32_t ncol_bytes = 0;
      if (carry) {
        int ncol = (w_next.col_round * LPR + glane) * 4;
        if (ncol >= F) ncol = 0;
        Xn = X + ncol;
        ncol_bytes = (uint32_t)ncol * 4u;
      }
      __builtin_amdgcn_sched_barrier(0);
      if (carry) {  // (a path of its own: one that issues under a condition would be waited for as if it had not)
#pragma unroll
        for (int u = 0; u < W; ++u) {
          if (p0 + u < e_end) {  // group-uniform
            rows_before(p0 + u);
            add(u);
          }
          v[u] = ld_row<OFF32>(X, Xn, nidx[u], ldx, row_bytes, ncol_bytes);
          __builtin_amdgcn_sched_barrier(0);
        }
        mults = nmults;
      } else {  // the window drains
#pragma unroll
        for (int u = 0; u < W; ++u) {
          if (p0 + u < e_end) {
            rows_before(p0 + u);
            add(u);
          }
        }
      }
    }
    if (nr > 0) {
      for (; r < nr; ++r) {  // the last non-empty row, then any trailing empty rows
        commit(r, acc);
        acc = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      write_rows();
    }
    // the draining form keeps nothing of the next task but its number across this one: decoded again, and its first
    // ids requested, after the task's last row
    const OwnedWork w_then = CARRY ? w_next : owned_decode(pl, wg, T, k_next, grp);
    if (!CARRY) hand_over(next_b, w_then, n_begin, n_end);
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
    w = w_then;
    my_rel = rel_b;
    e_begin = n_begin;
    e_end = n_end;
    carried = carry;
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
// The two-pass unit-value products (100 000 sources -> 50 000 rows) are within a spread of the pair on the 8-slice layout
// and stay on it there.  On a layout of 16 slices (dgmi_sliced_layout_slices below; profiles/owned_slices/README.md) a
// slice of their table fits an L2 at full width, and their plan is the first class's: one column round, one row round,
// 16 phases.
// The measured classes are classes of a slice count: the first three of 8 slices, the last of 16.
// `pl`: the plan of one workgroup per CU, which names the class.  0 = the pair, 1 = one 16-wave workgroup per CU,
// 2 = two 12-wave workgroups per CU.  No class takes 2: forced for all 8 products of the step it ran every one of them
// 30-35 % slower than the pair (profiles/owned_wgs/README.md); it stays behind sliced_owned_wgs = 2.
// `x_bytes`: bytes per element of the gathered table.  The classes of a bf16 table (x_bytes == 2: dgmi_owned_bf16.hip;
// column rounds of 8 lpr columns, table bytes in bf16) are classes of their own, measured on their own against the bf16
// pair on the 8-slice layout (tools/bf16_owned_ab.py, profiles/owned_bf16/README.md).  All four classes of the eight
// config-4 products cleared the bar — the owned median below the pair's by more than the pair's min .. max spread — with
// -20 % to -30 % of the product, conversion pass included: every one is a single column round of 16-lane groups over
// slices that fit an L2 at full width.
int owned_class_form(const OwnedPlan& pl, bool id_mult, int64_t table_bytes, int x_bytes) {
  const auto mib = [&](int64_t lo, int64_t hi) { return table_bytes >= (lo << 20) && table_bytes <= (hi << 20); };
  if (x_bytes == 2) {
    if (pl.slices != kOwnedSlices || pl.col_rounds != 1) return 0;
    if (pl.row_rounds == 1 && !id_mult && mib(16, 32)) return 1;  // 100 000 sources -> 50 000 rows, unit values
    if (pl.row_rounds == 2 && !id_mult && mib(8, 16)) return 1;   // 50 000 sources -> 100 000 rows, unit values
    if (pl.row_rounds == 2 && id_mult && mib(16, 32)) return 1;   // kNN-64 at 100 000 nodes
    if (pl.row_rounds == 1 && id_mult && mib(8, 16)) return 1;    // kNN-64 at 50 000 nodes
    return 0;
  }
  if (x_bytes != 4) return 0;
  if (pl.slices == kOwnedSlices) {
    if (pl.col_rounds == 1 && pl.row_rounds == 2 && !id_mult && mib(16, 32)) return 1;
    if (pl.col_rounds == 2 && pl.row_rounds == 1 && id_mult && mib(48, 64)) return 1;
    if (pl.col_rounds == 1 && pl.row_rounds == 1 && id_mult && mib(16, 32)) return 1;
  }
  if (pl.slices == kOwnedWideSlices && pl.col_rounds == 1 && pl.row_rounds == 1 && !id_mult && mib(48, 64)) return 1;
  return 0;
}

// The built-in R's tasks-per-phase target of a class: kOwnedPhaseTasksMult for the two kNN-64 classes of the rule above,
// which were measured with the hand-over (profiles/owned_carry/README.md: R = 3 instead of 4), kOwnedPhaseTasks for
// every other product — also for ids with multiplicities of shapes nobody has measured.  (R does not enter the class.)
int owned_class_phase_tasks(const OwnedPlan& pl, bool id_mult, int64_t table_bytes, int x_bytes) {
  if (x_bytes != 4) return kOwnedPhaseTasks;  // no bf16 class has been measured with another target
  const auto mib = [&](int64_t lo, int64_t hi) { return table_bytes >= (lo << 20) && table_bytes <= (hi << 20); };
  if (pl.slices != kOwnedSlices) return kOwnedPhaseTasks;
  if (pl.col_rounds == 2 && pl.row_rounds == 1 && id_mult && mib(48, 64)) return kOwnedPhaseTasksMult;
  if (pl.col_rounds == 1 && pl.row_rounds == 1 && id_mult && mib(16, 32)) return kOwnedPhaseTasksMult;
  return kOwnedPhaseTasks;
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
  const int workers = tuning().sliced_owned_workers > 0 && tuning().sliced_owned_workers < WAVES - 1 ? tuning().sliced_owned_workers : 0;
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
                       spin_ticks, workers, a.ep);                                                                               \
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
  if ((a.x_bytes != 4 && a.x_bytes != 2) || a.vals != nullptr || a.src_scale != nullptr || a.n_keep != 0 || a.n_slices < 1 || a.n_slices > kOwnedMaxSlices ||
      tune.sliced_chunk_rows > 0 || a.chunk_rows < a.n_dst || a.n_dst == 0 || a.F == 0)
    return hipSuccess;
  // Tuning::sliced_owned_slices is the knob of the fp32 layout experiment (dgmi_sliced_layout_slices, at the end): it
  // names the slice count of the layouts made FOR the owned form.  No layout is ever made for it on behalf of a bf16
  // product — the layout rule is fp32's, a bf16 product stays on the pair's 8-slice layout whatever the knob says — so a
  // process that runs that experiment keeps what it ran for a bf16 table before this form took one: the pair.
  if (a.x_bytes == 2 && tune.sliced_owned_slices > 0) return hipSuccess;
  // a forced grid counts workgroups, whichever form runs them
  const int64_t grid = tune.sliced_owned_grid > 0 ? tune.sliced_owned_grid : device_cus();
  if (grid < 1) return hipSuccess;
  const int lpr = sliced_lpr(a.F, a.n_src, a.n_slices, a.n_dst, a.full_width, a.n_keep, a.x_bytes, tune.sliced_lpr);
  // the one-workgroup plan names the class and is what a two-workgroup launch that cannot co-reside falls back to
  // the plan with the general tasks-per-phase target names the class; the two measured kNN-64 classes then take theirs
  const int slices = (int)a.n_slices;
  const int cols = 16 / a.x_bytes;  // the columns of a lane's one 16-B load: 4 of an fp32 table, 8 of a bf16 one
  const int64_t table_bytes = a.n_src * a.ldx * (int64_t)a.x_bytes;
  OwnedPlan pl = owned_plan(a.n_dst, a.F, lpr, grid, tune.sliced_owned_rows, tune.sliced_owned_lds_rows, 1, kOwnedPhaseTasks, slices, cols);
  const int phase_tasks = a.n_dst < kOwnedMinRows ? kOwnedPhaseTasks : owned_class_phase_tasks(pl, a.id_mult, table_bytes, a.x_bytes);
  if (pl.ok && phase_tasks != kOwnedPhaseTasks)
    pl = owned_plan(a.n_dst, a.F, lpr, grid, tune.sliced_owned_rows, tune.sliced_owned_lds_rows, 1, phase_tasks, slices, cols);
  if (!pl.ok || pl.lds_bytes > (size_t)(160 << 10)) return hipSuccess;
  const int rule = a.n_dst < kOwnedMinRows ? 0 : owned_class_form(pl, a.id_mult, table_bytes, a.x_bytes);
  if (tune.sliced_owned != 1 && rule == 0) return hipSuccess;
  const bool off32 = !tune.sliced_no_off32 && (a.n_src * a.ldx + a.F) * a.x_bytes < ((int64_t)1 << 32);
  if (a.x_bytes == 2) {
    // The bf16 kernel (dgmi_owned_bf16.hip) is built in one form only — one 16-wave workgroup per CU, no phase gate —
    // so sliced_owned_lag, sliced_owned_spin_ticks and sliced_owned_wgs are ignored for a bf16 table, and without
    // arrive counters nothing is asked of the plane workspace.
    *taken = true;
    return launch_owned_bf16(a, pl, lpr, grid, off32, s);
  }
  // the arrive counters live in the first bytes of the caller's plane workspace (n_slices * n_dst * ldp floats)
  const auto arrive_fits = [&](const OwnedPlan& p) {
    return sizeof(unsigned) * 8 * (size_t)p.phases <= sizeof(float) * (size_t)a.n_slices * (size_t)a.n_dst * (size_t)a.ldp;
  };
  if (!arrive_fits(pl)) return hipSuccess;
  const int form = tune.sliced_owned_wgs == 1 || tune.sliced_owned_wgs == 2 ? tune.sliced_owned_wgs : (rule == 2 ? 2 : 1);
  const int64_t spin = tune.sliced_owned_spin_ticks > 0 ? tune.sliced_owned_spin_ticks : kOwnedSpinTicks;
  const int lag = tune.sliced_owned_lag >= -1 ? tune.sliced_owned_lag : kOwnedLag;
  *taken = true;
  bool resident = true;
  if (form == 2) {
    const int64_t grid2 = tune.sliced_owned_grid > 0 ? grid : 2 * grid;
    const OwnedPlan pl2 = owned_plan(a.n_dst, a.F, lpr, grid2, tune.sliced_owned_rows, tune.sliced_owned_lds_rows, 2, kOwnedPhaseTasks, slices);
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

// The slice count of the layout a plain fp32 product of this shape should be given (include/dgmi_layout.h).  8 — the
// pair's binding of a slice to an XCD — for everything but the class of owned_class_form that was measured on 16
// slices; Tuning::sliced_owned_slices forces a count for every product the form can plan.  It asks the launcher's own
// sliced_lpr / owned_plan / owned_class_form with the slice count in question, so a layout is only ever made wide for
// a product spmm_owned_try then takes.
int sliced_layout_slices(int64_t n_dst, int64_t n_src, int64_t F, bool id_mult) {
  const Tuning& tune = tuning();
  if (n_dst < 1 || n_src < 1 || F < 1 || F % 4 != 0 || tune.sliced_owned == 0 || tune.sliced_chunk_rows > 0) return kOwnedSlices;
  const int forced = tune.sliced_owned_slices;
  const int slices = forced > 0 ? (forced < kOwnedMaxSlices ? forced : kOwnedMaxSlices) : kOwnedWideSlices;
  if (slices == kOwnedSlices) return kOwnedSlices;
  // the layout's row boundaries are int32 words, and the launcher chunks planes beyond 4 GiB (dgmi_api.hip): the pair's then
  if (n_dst * slices >= INT32_MAX || n_dst * slices * F * (int64_t)sizeof(float) > ((int64_t)4096 << 20)) return kOwnedSlices;
  const int64_t grid = tune.sliced_owned_grid > 0 ? tune.sliced_owned_grid : (device_cus() > 0 ? device_cus() : kOwnedAssumedCus);
  const int lpr = sliced_lpr(F, n_src, slices, n_dst, false, 0, 4, tune.sliced_lpr);
  const OwnedPlan pl = owned_plan(n_dst, F, lpr, grid, tune.sliced_owned_rows, tune.sliced_owned_lds_rows, 1, kOwnedPhaseTasks, slices);
  if (!pl.ok || pl.lds_bytes > (size_t)(160 << 10)) return kOwnedSlices;
  if (forced > 0) return slices;
  if (n_dst < kOwnedMinRows) return kOwnedSlices;
  return owned_class_form(pl, id_mult, n_src * F * (int64_t)sizeof(float), 4) == 1 ? slices : kOwnedSlices;
}

}  // namespace dgmi

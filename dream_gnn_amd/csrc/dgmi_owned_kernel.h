// dgmi_owned_kernel.h — the one kernel body of the workgroup-owned form of the XCD-local SpMM (dgmi_owned.hip): the task
// protocol, the toucher and the rolling gather window, whatever the element type of the gathered table.  What differs
// between an fp32 and a bf16 table — the columns a lane owns, the registers of a gathered row, the accumulators, the
// LDS slots of a row and the stores of Y — is a ROW POLICY (OwnedRowF32, OwnedRowBf16): a template argument whose
// members are all force-inlined.
//
// The plan (rows per workgroup, rounds, phases, tasks): dgmi_owned_common.h.  Inside a workgroup the 15 worker waves
// take tasks from one LDS counter, phase-major then row-major; a wave reserves its next task (and requests that task's
// row boundaries) before it runs the current one.  Task t of phase P touches the LDS rows task t of phase P - 1
// touched: done[t] counts the phases finished on slot t, release-stored after a task's LDS writes and acquire-polled
// before the next one's first LDS access.  The lowest unfinished task never waits (everything before it is finished and
// a reserved task is only ever held by a wave that runs an earlier one), so this cannot deadlock; it also orders the
// reuse of the LDS rows by the next round.  The order inside a task is part of that argument: reserve the next task,
// request its boundaries, wait for done[], touch LDS, wave barrier, release.
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
// The window is HANDED OVER from task to task (owned_carry, dgmi_owned_common.h; the 16-wave form of an fp32 table with
// multiplicities in the ids — the other instantiations keep the draining loop, see CARRY): in the last group of
// its run a lane group refills every slot, right behind its consumption, with the first W edges of its run in the
// wave's next task — that task's ids, its column offset — so the next task starts with its window full: no prologue,
// no wait for ids.  The next task's boundaries are requested when it is reserved and taken over at ONE wave-uniform
// point per task, behind the wait for done[]: there its run is found, its first two id batches and its scales are
// requested, and the wait for the boundaries is the wait for the carried gathers the first group needs at once.  A run
// behind a run without edges starts cold, as does a wave's first; a run in front of one without edges hands nothing over,
// and past the last task nothing is issued.  A task is decoded once, when it is reserved.  The sums, their order and
// every bit are those of the draining loop.  Measured: profiles/owned_carry/README.md.
//
// The last wave is the toucher: it walks the same task order a few tasks ahead of the counter and touches one word per
// 128-B line of the boundaries and ids the workers are about to read (they issue no cold loads), and — under GATE — it
// keeps the ADVISORY phase gate: the workgroups of an XCD (label blockIdx % 8 — a speed assumption, as is their
// co-residency) should gather from the same slice at the same time, so a workgroup opens phase P for its workers once
// every workgroup of its label has finished phase P - 1 - lag, or a time bound has passed.  Leaders wait, the slowest
// never does, every spin is bounded and results never depend on it.  It is off unless asked for (lag < 0): measured, it
// costs more than it buys.  A launch without a gate carries no gate work: no memset of the arrive counters, no counting
// of a phase's tasks; a kernel built without GATE has no gate code, and nothing in it waits for anything outside its
// own workgroup.
//
// The DUTY form has no toucher: all 16 waves are workers and the touching is a DUTY of task slots (owned_duty_*,
// dgmi_owned_common.h).  The wave that reserves the first slot of a chunk of `duty_chunk` slots touches, right after the
// reservation and before anything else — before it requests that task's boundaries, before it runs the task it holds —
// the same words the toucher touches for the chunk that lies `duty_lead` slots ahead (the first duty also for the
// chunks in front of that), as many lines per wave-instruction as there are lanes, and then goes on as any worker.  It
// pays one exposed cold latency per level (the ends of the boundaries, which name the ids, then the ids' lines, which
// are waited for with whatever the wave waits for next); no other wave pays anything.  A duty waits for NOTHING but its
// own loads: it polls nothing, reads neither done[] nor the counter nor anything another workgroup writes, and what it
// loads is read-only for the launch.  So the argument above holds word for word: inside a workgroup the 16 worker
// waves take tasks from one LDS counter, phase-major then row-major; a wave reserves its next task (does that slot's
// duty, if it has one, which ends after two load latencies, and requests that task's row boundaries) before it runs the
// current one.  done[t] is release-stored after a task's LDS writes and acquire-polled before the next one's first LDS
// access.  The lowest unfinished task never waits (everything before it is finished and a reserved task is only ever
// held by a wave that runs an earlier one — a wave in a duty holds one reserved task and runs an earlier one, or none:
// its duty returns and it runs it), so this cannot deadlock.  The order inside a task: reserve the next task, its duty,
// request its boundaries, wait for done[], touch LDS, wave barrier, release.  The form is built without GATE (the
// advisory gate lives in the toucher): a launch that asks for a gate takes the form with a toucher.  Nothing of a sum
// differs: every product is bit for bit the toucher form's.  Measured: profiles/owned_duty/README.md.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dgmi_owned_common.h"
#include "dgmi_sliced_common.h"

namespace dgmi {
namespace {

// An fp32 table (columns, load, sums and the canonical step: RowF32, dgmi_sliced_common.h): one float4 of the LPR
// slots of an LDS row.
struct OwnedRowF32 : RowF32 {
  static constexpr int kLaneSlots = 1;  // float4 LDS slots per lane and row
  static constexpr bool kCarry = true;  // the hand-over may be built (measured: profiles/owned_carry/README.md)
  static constexpr bool kPeel = true;   // groups 0 and 1 of a run stand in front of the group loop (owned_body)

  // the segment sum joins the running sum in this lane's slot of the row (`first`: slice 0 starts it).  (LPR goes
  // unused here and in sum: the body calls both policies alike, and the bf16 one's second half lies LPR slots further.)
  template <int LPR>
  static __device__ __forceinline__ void commit(float4* slot, bool first, const Acc& acc) {
    if (first) {
      *slot = acc;
      return;
    }
    float4 t = *slot;
    t.x += acc.x;
    t.y += acc.y;
    t.z += acc.z;
    t.w += acc.w;
    *slot = t;
  }

  // the row's finished sum of this lane's columns, out of LDS; dst_scale; the epilogue and Y
  template <int LPR>
  static __device__ __forceinline__ Acc sum(const float4* slot) {
    return *slot;
  }

  static __device__ __forceinline__ void scale(Acc& t, float d) {
    t.x *= d;
    t.y *= d;
    t.z *= d;
    t.w *= d;
  }

  static __device__ __forceinline__ void write(const Acc& t, float* y, const Epilogue& ep, int64_t row, int col) {
    *reinterpret_cast<float4*>(y) = epilogue4(ep, t, row, col);
  }
};

// A bf16 table (columns, load, the sums as four column pairs and the canonical step: RowBf16, dgmi_sliced_common.h —
// the pair's gather, spmm_sliced_bf16_kernel, sums with the same members).  An LDS row of one column round is 2 LPR
// slots, planar: the float4 of columns 0..3 of all LPR lanes first, then the float4 of columns 4..7 of all lanes — each
// of a lane's two 16-byte accesses is contiguous across its lane group (a 32-byte lane stride would make every access a
// two-way bank conflict).  The plan: owned_plan with cols_per_lane = 8.
struct OwnedRowBf16 : RowBf16 {
  static constexpr int kLaneSlots = 2;
  static constexpr bool kCarry = false;  // the hand-over has not been measured on a bf16 table
  // One plain group loop.  With groups 0 and 1 in front of it, as the fp32 kernels have them, the products take the
  // same time, but all twelve kernels need 82-84 VGPRs instead of 72-80 and the compiler states 5 waves per SIMD where
  // the separate bf16 kernel stated 6 (profiles/owned_one_body/README.md).
  static constexpr bool kPeel = false;

  template <int LPR>
  static __device__ __forceinline__ Acc sum(const float4* slot) {
    return pairs(slot[0], slot[LPR]);
  }

  // both reads stand in front of both writes: committed half by half, the second read would wait behind the first write
  template <int LPR>
  static __device__ __forceinline__ void commit(float4* slot, bool first, const Acc& acc) {
    Acc t = acc;
    if (!first) {
      const Acc s = sum<LPR>(slot);
#pragma unroll
      for (int k = 0; k < 4; ++k) t.p[k] = s.p[k] + acc.p[k];
    }
    slot[0] = half(t, 0);
    slot[LPR] = half(t, 1);
  }

  static __device__ __forceinline__ void scale(Acc& t, float d) {
#pragma unroll
    for (int k = 0; k < 4; ++k) t.p[k] *= d;
  }

  static __device__ __forceinline__ void write(const Acc& t, float* y, const Epilogue& ep, int64_t row, int col) {
    OwnedRowF32::write(half(t, 0), y, ep, row, col);
    OwnedRowF32::write(half(t, 1), y + 4, ep, row, col + 4);
  }
};

// a * b rounded to fp32 on its own.  The multiply instruction itself: written as a * b — also as __fmul_rn(a, b), also
// under `#pragma clang fp contract(off)` — the backend forms one v_pk_fma_f32 of it and the add that takes the product
// (seen in the assembly), which rounds once where the pre-scaled table has rounded twice.  Not tried: building the
// unit with -ffp-contract=off (it would reach every kernel of the unit, whose bits are pinned), and
// __builtin_amdgcn_fmul_legacy (0 x inf is 0 there, not NaN).  The price: four v_mul_f32 where v_pk_mul_f32 would be two.
__device__ __forceinline__ float owned_mul_rn(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// VALS: 0 = unit edge values, 2 = multiplicities in the id words (dgmi_sliced.hip).  WAVES: waves of the workgroup, the
// last one the toucher (not under DUTY).  GATE: the phase gate is built (`arrive`, `lag` and `spin_ticks` are read under it only).
//
// SCALED: the id words carry, in bits kScaleShift .. kScaleShift + kScaleBits - 1, the CODE of the gathered row's scale
// (dgmi_kernels.h; ids are < 2^kScaleShift): `table[code]` is diag(src_scale)'s entry of that row, so the product is
// that of the table scaled row by row beforehand (scale_rows_f32) without the pass over it.  The workgroup copies the
// table (at most 2^kScaleBits floats) into LDS behind its control words, in front of the barrier that follows their
// zeroing.  An edge's scale is read from there when its gather is issued — one address per lane group: a broadcast —
// and waits beside the row in a ring of W registers, which the hand-over carries like the row.  The row joins the sum
// as s * x, rounded once (no contraction with the add or the multiplicity): bit for bit what the pre-scaled table
// gives.  Nothing else differs: the task protocol, the toucher and write_rows read no id word.
//
// DUTY: the form without a toucher (at the top of this file): all WAVES waves are workers; `duty_chunk` task slots per
// duty, which touches `duty_lead` slots ahead.  Built without GATE.
template <typename Row, int LPR, int VALS, bool OFF32, int WAVES, bool GATE, bool SCALED = false, bool DUTY = false>
__device__ __forceinline__ void owned_body(const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices,
                                           const typename Row::Elem* __restrict__ X, int64_t ldx,
                                           const float* __restrict__ dst_scale, float* __restrict__ Y, int64_t ldy,
                                           int64_t n_dst, int F, OwnedPlan pl, unsigned* __restrict__ arrive, int lag,
                                           int64_t spin_ticks, int workers, Epilogue ep,
                                           const float* __restrict__ table = nullptr, int n_codes = 0, int duty_chunk = 0,
                                           int duty_lead = 0) {
  static_assert(!DUTY || !GATE, "the phase gate lives in the toucher");
  typedef typename Row::Elem Elem;
  typedef typename Row::Acc Acc;
  constexpr bool MULT = VALS == 2;
  constexpr int kIdMask = SCALED ? (int)kScaleIdMask : (MULT ? (int)kMultIdMask : 0x7fffffff);
  static_assert(!SCALED || (std::is_same<Elem, float>::value && kScaleShift + kScaleBits <= kMultShift), "an fp32 table; the code lies below the multiplicity");
  constexpr int kRowSlots = Row::kLaneSlots * LPR;  // float4 slots of an LDS row
  // The window is handed from task to task (false: every run starts cold — the same bits).  Not in the two-workgroup
  // form: next to its 80 VGPRs the window and the next task's run do not stay in registers across the boundary.  Not
  // for unit values either: measured (profiles/owned_carry/README.md), their products lose 2 points of L2 hits and
  // 0.3-0.6 % of their time to it, while the products with multiplicities gain.
  constexpr bool CARRY = WAVES == kOwnedWaves && MULT && Row::kCarry;
  extern __shared__ float4 lds_rows[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int grp = lane / LPR, glane = lane % LPR, gbase = grp * LPR;
  const int64_t wg = blockIdx.x;
  const int T = owned_wg_tasks(pl, wg);
  if (T == 0) return;  // block-uniform: a workgroup without rows
  int* done = reinterpret_cast<int*>(lds_rows + (size_t)pl.round_rows * kRowSlots);  // [tasks] phases finished on a task slot
  int* phase_cnt = done + pl.tasks;                                                 // [phases] tasks finished of a phase (gate only)
  int* counter = phase_cnt + pl.phases;                                             // next task
  int* open = counter + 1;                                                          // highest phase the gate has opened
  for (int i = threadIdx.x; i < pl.tasks + pl.phases + 2; i += blockDim.x) done[i] = 0;
  // every code has a word, whatever the table's length: a code is an LDS address inside the launch's allocation
  float* lds_scale = reinterpret_cast<float*>(open + 1);  // [2^kScaleBits] (SCALED only: the launcher adds its bytes)
  if (SCALED)
    for (int i = threadIdx.x; i < (1 << kScaleBits); i += blockDim.x) lds_scale[i] = i < n_codes ? table[i] : 0.f;
  __syncthreads();
  const int total = pl.phases * T;
  const int label = (int)(blockIdx.x & 7u);

  if (!DUTY && wave == WAVES - 1) {  // ---- the toucher ----
    const unsigned n_label = (unsigned)((pl.active - label + 7) >> 3);  // active workgroups with this label (>= 1: this one)
    const unsigned* my_arrive = GATE ? arrive + (size_t)label * pl.phases : nullptr;
    // One loop does both jobs and blocks in neither: touch the next chunk of tasks once the counter is within the lead
    // of it (also across a phase boundary: while the workers stand at a closed gate the first tasks behind it get
    // touched), and open the next phase once its condition holds.
    const int chunks_per_phase = (T + kOwnedTouchChunk - 1) / kOwnedTouchChunk, chunks = pl.phases * chunks_per_phase;
    const int last_gate = GATE && lag >= 0 ? pl.phases - 1 : 0;
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
      if (GATE && opened < last_gate) {
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
  // (profiles/owned_carry/README.md).  The draining form calls it for the same requests after the task's last row.
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
  typename Row::Reg v[W];
  float sc[SCALED ? W : 1];  // SCALED: the scales of the W rows in flight
  int idx[W];   // the ids of a group's W issues, read at its top: an issue is a multiply and a load (SCALED: id and code)
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
        if (!SCALED) id &= kIdMask;
      }
      out[u] = id;  // SCALED: with its code, which issue() takes apart
    }
    if (MULT) asm volatile("" : "+v"(fields));  // really one register: not the W id words kept for their fields
  };
  auto read_ids = [&](int batch_idx) { read_batch(batch_idx, idx, mults_in); };

  const uint32_t row_bytes = (uint32_t)ldx * (uint32_t)sizeof(Elem);
  // the gather of slot u — and, SCALED, the read of its scale — of the row id word `word` names
  auto issue = [&](int u, const Elem* Xcol, int word, uint32_t cbytes) {
    if (SCALED) {
      sc[u] = lds_scale[((uint32_t)word >> kScaleShift) & ((1u << kScaleBits) - 1u)];
      word &= kIdMask;
    }
    v[u] = Row::template load<OFF32>(X, Xcol, word, ldx, row_bytes, cbytes);
  };
  // The duty of the task slot a wave has just reserved (DUTY; owned_duty_*, dgmi_owned_common.h): wave-uniform, and it
  // waits for its own loads only — first the two ends of a chunk's boundaries, which name its ids, then nothing: the ids'
  // lines are waited for with whatever the wave waits for next.  What it reads is read-only for the whole launch.
  const int duty_chunks = DUTY ? pl.phases * owned_touch_chunks(T, duty_chunk) : 0;
  const int duty_lead_chunks = DUTY ? owned_duty_lead_chunks(duty_lead, duty_chunk) : 0;
  auto duty = [&](int slot) {
    const int c = owned_duty_chunk(slot, T, duty_chunk, pl.phases);
    if (c < 0) return;
    const OwnedDutySpan span = owned_duty_span(c, duty_chunks, duty_lead_chunks);
    int keepalive = 0;
    for (int cc = span.first; cc < span.end; ++cc) {
      const OwnedTouchRows tr = owned_touch_rows(pl, wg, T, duty_chunk, cc);
      if (!tr.any) continue;  // (a short last round)
      const int32_t* sp_s = segptr + (int64_t)tr.slice * n_dst;
      int v = 0;  // lane 0: the first boundary, lane 1: the last
      for (int64_t j = lane;; j += kWave) {
        const int64_t rp = owned_touch_boundary(tr.r_first, tr.r_last, j);
        if (rp < 0) break;
        const int b = sp_s[rp];
        if (j < 2) v = b;
        keepalive ^= b;
      }
      const int e0 = __builtin_amdgcn_readlane(v, 0), e1 = __builtin_amdgcn_readlane(v, 1);
      for (int64_t j = lane;; j += kWave) {
        const int64_t p = owned_touch_id(e0, e1, j);
        if (p < 0) break;
        keepalive ^= indices[p];
      }
    }
    asm volatile("" ::"v"(keepalive));  // the loads exist without an instruction of their own
  };
  int k = grab();
  if (DUTY) duty(k);
  OwnedWork w = owned_decode(pl, wg, T, k, grp);
  int e_begin = 0, e_end = 0;
  hand_over(boundaries(w), w, e_begin, e_end);
  int my_rel = rel_b;  // lane j of a group: boundary j of the group's rows (j <= rows), relative to e_begin
  while (k < total) {
    const int L = e_end - e_begin;  // the group's run: 0 without rows, or with rows that have no edge in this slice
    int col = (w.col_round * LPR + glane) * Row::kCols;
    const bool col_ok = col < F;  // F is a multiple of the columns a lane owns: all of them or none
    if (!col_ok) col = 0;         // such a lane gathers column 0 and keeps its sums to itself
    const Elem* Xc = X + col;
    const uint32_t col_bytes = (uint32_t)col * (uint32_t)sizeof(Elem);
    // A cold start (the first task of a wave, or a run before this one without edges): the prologue of the window.
    if (L > 0 && !carried) {
      read_ids(nxt_idx);
#pragma unroll
      for (int u = 0; u < W; ++u) issue(u, Xc, idx[u], col_bytes);
      mults = mults_in;
    }
    const int k_next = grab();
    if (DUTY) duty(k_next);
    const OwnedWork w_next = owned_decode(pl, wg, T, k_next, grp);
    const int next_b = boundaries(w_next);
    int n_begin = 0, n_end = 0;  // the group's run in the next task
    if (GATE && lag >= 0)
      while (__hip_atomic_load(open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < w.phase) __builtin_amdgcn_s_sleep(1);
    // the task that used these LDS rows in the phase before (this round's, or the last one of the round before)
    while (__hip_atomic_load(&done[w.task], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < w.phase) __builtin_amdgcn_s_sleep(1);
    const int first_ids = nxt_idx1;  // this run's batch 1 (owned_carry_start_batch), before the next run's replaces it
    static_assert(owned_carry_start_batch() == 1, "nxt_idx1");
    if (CARRY) hand_over(next_b, w_next, n_begin, n_end);

    const int nr = w.rows;
    float4* slot = lds_rows + (size_t)w.lds_row * kRowSlots + glane;
    // the segment sum of row r of the group joins the row's running sum
    auto commit = [&](int r, const Acc& acc) { Row::template commit<LPR>(slot + r * kRowSlots, w.slice == 0, acc); };
    // The last slice's phase writes Y: dst_scale and the epilogue once per row, after the task's gathers — not inside
    // commit, where the scale, the mask and the addresses of Y would be live next to 8 gathered rows — from the sums
    // this lane has just left in LDS.  Under CARRY the scales were requested when the task was reserved and have
    // arrived (my_ds): no load stands between the task's sums and the release of done[].
    auto write_rows = [&]() {
      if (w.slice != pl.slices - 1) return;
      for (int r = 0; r < nr; ++r) {
        float d = 0.f;
        if (CARRY) d = __shfl(my_ds, gbase + r, kWave);  // (by every lane of the group)
        if (!col_ok) continue;
        Acc t = Row::template sum<LPR>(slot + r * kRowSlots);
        const int64_t row = w.row_base + (w.lds_row + r);
        if (dst_scale != nullptr) {
          if (!CARRY) d = dst_scale[row];
          Row::scale(t, d);
        }
        Row::write(t, Y + row * ldy + col, ep, row, col);
      }
    };

    bool carry = false;  // whether the group hands its window over to its run in the next task
    int r = 0;
    Acc acc = Row::zero();
    if (L > 0) {
      // The rolling window (owned_window, dgmi_owned_common.h): W rows in flight from the first group of a run to its
      // last; the sum takes the edges in order, one at a time, exactly as the pair's gather does.
      int row_end = e_begin + __shfl(my_rel, gbase + 1, kWave);
      auto add = [&](int u) {
        float m = 1.f;
        if (MULT) {
          m = (float)(((mults >> (32 - 4 * W)) & (uint32_t)kMultMax) + 1u);
          mults >>= 4;
        }
        if constexpr (SCALED) {  // s * x rounded on its own, as the pre-scale pass stores it
          const float s = sc[u];
          const float4 t = make_float4(owned_mul_rn(s, v[u].x), owned_mul_rn(s, v[u].y), owned_mul_rn(s, v[u].z), owned_mul_rn(s, v[u].w));
          Row::template add<MULT>(acc, m, t);
        } else {
          Row::template add<MULT>(acc, m, v[u]);
        }
      };
      auto rows_before = [&](int p) {  // row(s) ended before edge p (empty rows commit zeros)
        while (p >= row_end) {
          commit(r, acc);
          acc = Row::zero();
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
          issue(u, Xc, idx[u], col_bytes);
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
      // makes it copy a slot behind a vmcnt(0), and so does a read under a condition inside the loop).  A policy
      // without kPeel takes every group in the one loop.
      static_assert(Row::kPeel || !CARRY, "the hand-over reads the next task's batch between the peeled groups");
      static_assert(owned_carry_read_group(2 * W + 1) == 0 && owned_carry_read_group(2 * W) == -1, "behind group 0 of three or more");
      int g = 0;
      if (!Row::kPeel) {
      } else if (owned_carry_read_group(L) == 0) {
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
      const Elem* Xn = X;
      uint32_t ncol_bytes = 0;
      if (carry) {
        int ncol = (w_next.col_round * LPR + glane) * Row::kCols;
        if (ncol >= F) ncol = 0;
        Xn = X + ncol;
        ncol_bytes = (uint32_t)ncol * (uint32_t)sizeof(Elem);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (carry) {  // (a path of its own: one that issues under a condition would be waited for as if it had not)
#pragma unroll
        for (int u = 0; u < W; ++u) {
          if (p0 + u < e_end) {  // group-uniform
            rows_before(p0 + u);
            add(u);
          }
          issue(u, Xn, nidx[u], ncol_bytes);
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
        acc = Row::zero();
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
      if (GATE && lag >= 0) {  // only a gate reads the arrive counters: without one nobody counts a phase's tasks either
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

}  // namespace
}  // namespace dgmi

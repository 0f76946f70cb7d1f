// dgmi_owned_common.h — the plan of the workgroup-owned form of the XCD-local SpMM (dgmi_owned.hip): which destination
// rows a workgroup owns, how they are cut into rounds that fit its LDS, and which rows a task of a phase sums.  The
// kernel body (dgmi_owned_kernel.h), its launcher and the host tests (tests/test_owned_*_host.py) take the plan from
// owned_plan, a task from owned_decode (owned_phase / owned_task) and a workgroup's extents from owned_wg_tasks /
// owned_round_rows.  At the end: the index arithmetic of the kernel's rolling gather window (owned_window_*) and of its
// hand-over from task to task (owned_carry_*).
//
// Workgroup w owns the contiguous rows [w B, (w + 1) B), B = ceil(n_dst / grid).  LDS holds one fp32 partial row of one
// column tile (16 LPR bytes; 32 LPR where a lane owns 8 columns: a bf16 table) per owned row of the current ROW ROUND;
// the column tiles are the COLUMN ROUNDS.  A PHASE is (column round, row round, slice), slices 0 .. S - 1 innermost and
// in order: the row sums take their S segment sums in the order the plane reduce adds the planes.  S is the layout's
// slice count, a field of the plan (8 unless the caller says otherwise): nothing binds a workgroup to an XCD, so the
// form walks as many slices as the layout has.  A phase is cut into TASKS of G R consecutive rows of the round — one
// wave, R rows for each of its G = 64 / LPR lane groups; task t of every phase of a round covers the same LDS rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dgmi {

constexpr int kOwnedSlices = 8;                     // the slice count of a plan made without one (one slice per XCD, as the pair's layouts)
constexpr int kOwnedMaxSlices = 64;                 // what the layout builders take
constexpr int kOwnedWaves = 16;                     // waves per workgroup: 15 workers and the toucher, or (the duty form) 16 workers
constexpr int kOwnedWorkers = kOwnedWaves - 1;      // ... of the form with a toucher: the worker count the tasks-per-phase targets are stated for
constexpr int kOwnedDutyWorkers = kOwnedWaves;      // ... of the duty form (owned_duty_*, at the end)
constexpr int kOwnedPairWaves = 12;                 // the two-workgroups-per-CU form: 2 x (11 workers and a toucher)
constexpr int64_t kOwnedLdsRowBytes = 144 << 10;    // LDS budget of the partial rows (the CU has 160 KiB)
constexpr int kOwnedMaxPhases = 128;                // per-phase words live in LDS and in the arrive counters
constexpr int kOwnedPhaseTasks = 24;                // built-in R aims at this many tasks per phase
constexpr int kOwnedPhaseTasksMult = 32;            // ... of the two kNN-64 classes (measured with the hand-over: profiles/owned_carry; owned_class_phase_tasks)
constexpr int kOwnedMaxRows = 8;                    // built-in upper bound of R

struct OwnedPlan {
  bool ok;             // false: the form does not take this product (too many phases, nothing to do)
  int lpr, G, R;       // lane-group width, lane groups per wave, rows per lane group and task
  int col_rounds, row_rounds, phases;
  int slices;          // source slices of the layout: the innermost index of a phase
  int64_t wg_rows;     // B
  int64_t active;      // workgroups that own at least one row: 0 .. active - 1
  int round_rows;      // rows of a workgroup in one row round = LDS rows
  int tasks;           // task slots per phase of a workgroup that owns B rows
  int64_t n_dst;
  size_t lds_bytes;    // partial rows, then tasks + phases + 2 control words
};

struct OwnedPhase {
  int col_round, row_round, slice;
};

struct OwnedTask {
  int64_t row0;  // first destination row of the lane group
  int lds_row;   // its LDS row
  int rows;      // 0: nothing to do
};

// `lpr`: lane-group width (sliced_lpr); `R_req` <= 0: built-in — about kOwnedPhaseTasks tasks per phase, 1.6 per worker
// wave (measured, profiles/owned_rows/README.md: fewer, longer tasks leave waves idle at the end of a phase, more and
// shorter ones pay the start of a task — boundaries, then ids, then the first gathers — too often; a task still
// practically never waits for its predecessor of the phase before); `lds_rows_cap` > 0: at most that many LDS rows
// (forces row rounds); `wgs_per_cu`: 1 = one 16-wave workgroup per CU, 2 = two co-resident 12-wave workgroups, each with
// half the LDS rows and a tasks-per-phase target scaled to its 11 workers (`grid` counts workgroups either way);
// `phase_tasks_target`: the built-in R's aim for 15 workers (the launcher passes kOwnedPhaseTasksMult for the kNN-64 classes);
// `slices`: the slice count of the layout, 1 .. kOwnedMaxSlices; `cols_per_lane`: the columns a lane owns — 4 of an fp32
// table, 8 of a bf16 one (OwnedRowBf16, dgmi_owned_kernel.h): a column round is cols_per_lane lpr columns wide, and a row of it costs
// 4 cols_per_lane lpr bytes of LDS (the sums are fp32 either way); `workers`: the waves of a workgroup that take tasks
// — 0: all but a toucher (15, or 11 of the two-workgroup form), kOwnedDutyWorkers: the duty form's 16 — to which the
// tasks-per-phase target is scaled.
__host__ __device__ constexpr int owned_form_waves(int wgs_per_cu) { return wgs_per_cu == 2 ? kOwnedPairWaves : kOwnedWaves; }

__host__ __device__ inline OwnedPlan owned_plan(int64_t n_dst, int64_t F, int lpr, int64_t grid, int R_req, int64_t lds_rows_cap,
                                                int wgs_per_cu = 1, int phase_tasks_target = kOwnedPhaseTasks,
                                                int slices = kOwnedSlices, int cols_per_lane = 4, int workers = 0) {
  OwnedPlan p{};
  p.ok = false;
  p.n_dst = n_dst;
  if (workers == 0) workers = owned_form_waves(wgs_per_cu) - 1;  // a form with a toucher
  if (n_dst < 1 || F < 1 || grid < 1 || (wgs_per_cu != 1 && wgs_per_cu != 2) || (lpr != 8 && lpr != 16 && lpr != 32 && lpr != 64) ||
      slices < 1 || slices > kOwnedMaxSlices || (cols_per_lane != 4 && cols_per_lane != 8) || workers < 1 ||
      workers > owned_form_waves(wgs_per_cu))
    return p;
  p.lpr = lpr;
  p.slices = slices;
  p.G = 64 / lpr;
  p.col_rounds = (int)((F + cols_per_lane * lpr - 1) / (cols_per_lane * lpr));
  p.wg_rows = (n_dst + grid - 1) / grid;
  p.active = (n_dst + p.wg_rows - 1) / p.wg_rows;
  int64_t fit = kOwnedLdsRowBytes / wgs_per_cu / (4 * cols_per_lane * lpr);
  if (lds_rows_cap > 0 && lds_rows_cap < fit) fit = lds_rows_cap;
  const int64_t rounds = (p.wg_rows + fit - 1) / fit;
  if (rounds * p.col_rounds * slices > kOwnedMaxPhases) return p;
  p.row_rounds = (int)rounds;
  p.round_rows = (int)((p.wg_rows + rounds - 1) / rounds);  // <= fit
  p.phases = p.col_rounds * p.row_rounds * slices;
  int R = R_req;
  if (R <= 0) {
    // 1.6 tasks per worker wave: 24 for 15 workers, 18 for 11, 26 for the duty form's 16
    const int phase_tasks = (phase_tasks_target * workers + kOwnedWorkers / 2) / kOwnedWorkers;
    R = (p.round_rows + phase_tasks * p.G / 2) / (phase_tasks * p.G);  // rounded to nearest
    if (R > kOwnedMaxRows) R = kOwnedMaxRows;
  }
  if (R > lpr - 1) R = lpr - 1;  // a group's row boundaries live one per lane
  if (R < 1) R = 1;
  p.R = R;
  p.tasks = (p.round_rows + p.G * R - 1) / (p.G * R);
  p.lds_bytes = (size_t)p.round_rows * 4 * cols_per_lane * lpr + sizeof(int) * ((size_t)p.tasks + p.phases + 2);
  p.ok = true;
  return p;
}

// Rows workgroup `wg` owns (the last active one may own fewer; the ones after it none).
__host__ __device__ inline int64_t owned_wg_rows(const OwnedPlan& p, int64_t wg) {
  const int64_t left = p.n_dst - wg * p.wg_rows;
  return left < 0 ? 0 : (left < p.wg_rows ? left : p.wg_rows);
}

// Rows of workgroup `wg` in row round `row_round` (0 for a round a short workgroup does not reach).
__host__ __device__ inline int64_t owned_round_rows(const OwnedPlan& p, int64_t wg, int row_round) {
  const int64_t left = owned_wg_rows(p, wg) - (int64_t)row_round * p.round_rows;
  return left < 0 ? 0 : (left < p.round_rows ? left : p.round_rows);
}

// Task slots per phase of workgroup `wg`: the same in every phase (a slot whose rows a short last round does not have
// is an empty task), 0 for a workgroup without rows.
__host__ __device__ inline int owned_wg_tasks(const OwnedPlan& p, int64_t wg) {
  int64_t rows = owned_wg_rows(p, wg);
  if (rows > p.round_rows) rows = p.round_rows;
  return (int)((rows + p.G * p.R - 1) / (p.G * p.R));
}

__host__ __device__ inline OwnedPhase owned_phase(const OwnedPlan& p, int phase) {
  const int cq = phase / p.slices;
  return OwnedPhase{cq / p.row_rounds, cq % p.row_rounds, phase - cq * p.slices};
}

// Lane group `group` (0 .. G - 1) of task slot `task` in row round `row_round` of workgroup `wg`.
__host__ __device__ inline OwnedTask owned_task(const OwnedPlan& p, int64_t wg, int row_round, int task, int group) {
  const int64_t lds_row = ((int64_t)task * p.G + group) * p.R;
  int64_t rows = owned_round_rows(p, wg, row_round) - lds_row;
  rows = rows < 0 ? 0 : (rows < p.R ? rows : p.R);
  return OwnedTask{wg * p.wg_rows + (int64_t)row_round * p.round_rows + lds_row, (int)lds_row, (int)rows};
}

// Task k of a workgroup (T task slots per phase, phase-major), decoded for lane group `grp`: wave-uniform except
// lds_row / rows, which are the lane group's.  `k` past the last task: a task without rows.  A kernel decodes a task
// once, when a wave reserves it, and carries it.
struct OwnedWork {
  int phase, task, slice, col_round;
  int64_t row_base;  // the lane group's first destination row is row_base + lds_row
  int lds_row, rows;
};

__host__ __device__ __forceinline__ OwnedWork owned_decode(const OwnedPlan& pl, int64_t wg, int T, int k, int grp) {
  OwnedWork w;
  if (k >= pl.phases * T) {  // wave-uniform
    w.phase = pl.phases;
    w.task = w.slice = w.col_round = w.lds_row = w.rows = 0;
    w.row_base = 0;
    return w;
  }
  w.phase = k / T;
  w.task = k - w.phase * T;
  const OwnedPhase ph = owned_phase(pl, w.phase);
  w.slice = ph.slice;
  w.col_round = ph.col_round;
  const OwnedTask t = owned_task(pl, wg, ph.row_round, w.task, grp);
  w.row_base = t.row0 - t.lds_row;
  w.lds_row = t.lds_row;
  w.rows = t.rows;
  return w;
}

// The rolling gather window.  A lane group sums the L edges of its run (all the rows of its task, in order) with
// W = kOwnedWindow gathers in flight: a prologue issues edges 0 .. W - 1; GROUP g then consumes edges g W .. g W + W - 1
// in order and, right after consuming edge e, issues edge e + W into the registers e's row has just left — except in the
// last group (owned_window_groups(L) - 1), which issues nothing of its own run (it refills for the next task's: the
// hand-over below).  The ids arrive in BATCHES of W, whatever the lane-group
// width: one register, in which lane l of the group holds the id of edge b W + l % W of batch b, clamped to the run's
// last edge — so an edge issued past the end of the run gathers the run's last row again (an L1 hit, never one fixed
// row) and is never consumed.  Batches 0 and 1 are requested before the run starts (during the task before).  At its
// top group g reads the W ids of its issues (batch g + 1) out of the register and then requests batch g + 2 into it:
// a batch is read W gathers after it was requested, so, vmcnt being in order, waiting for it waits for nothing but
// gathers already consumed, and the request itself never waits.
// The kernel and the host test (tests/test_owned_window_host.py) take all of this from the functions below.
// The depth is measured (profiles/owned_window/README.md): inside the step of bench.py a window of 4 beats one of 8 on
// every class (8 in flight per lane group cost the unit-value products 4-8 points of L2 hits) and one of 2 loses 15 %.
constexpr int kOwnedWindow = 4;              // gathers in flight per lane group; divides every lane-group width
constexpr int kOwnedWindowFirstBatches = 2;  // id batches requested before a run starts

__host__ __device__ constexpr int owned_window_groups(int L) { return (L + kOwnedWindow - 1) / kOwnedWindow; }

// Group `g` (not the last one of its run) issues edges (g + 1) W + u, u = 0 .. W - 1, from lanes u of this id batch ...
__host__ __device__ constexpr int owned_window_issue_batch(int g) { return g + 1; }
// ... and requests this one at its top.
__host__ __device__ constexpr int owned_window_request_batch(int g) { return g + kOwnedWindowFirstBatches; }

// The edge (0-based in its run of L > 0 edges) whose id lane `lane` of a lane group loads for id batch `batch`: the clamp.
__host__ __device__ constexpr int owned_window_id_edge(int batch, int lane, int L) {
  return batch * kOwnedWindow + lane % kOwnedWindow < L ? batch * kOwnedWindow + lane % kOwnedWindow : L - 1;
}

// The hand-over.  A wave runs its tasks back to back, and a lane group's window survives the boundary between two of
// them: in the last group of its run in task A (L_a edges) the group refills slot u, right after consuming it (or at
// once, where the last group has no edge u), with edge u of its run in the wave's next task B (L_b edges) — B's id
// batch 0, B's column offset, the same clamp.  B then starts with its window full and aligned at slot 0: no prologue,
// its first group consumes at once, reads batch 1 out of the id register and requests batch 2 as any group does.  A
// window is carried only between two runs that both have edges; every other run starts cold (the prologue), and
// nothing is issued, and no id read, for a run without edges or past the last task.
// B's batches 0 and 1 are requested at the top of A — B's boundaries, requested when B was reserved, are waited for
// there, at a wave-uniform point, together with the gathers carried into A — and batch 0 is read behind A's group
// owned_carry_read_group(L_a), W gathers after its request.  A run of one or two groups (-1) reads it right before its
// last group, and waits.
// The kernel and the host test (tests/test_owned_carry_host.py) take all of this from the functions below.
__host__ __device__ constexpr bool owned_carry(int L_a, int L_b) { return L_a > 0 && L_b > 0; }

// The edge of B (0-based in its run of L_b > 0 edges) that slot `u` of A's last group is refilled with; its id is lane
// `u` of B's batch 0.
__host__ __device__ constexpr int owned_carry_slot_edge(int u, int L_b) { return owned_window_id_edge(0, u, L_b); }

// The group of A (not its last one) behind which B's batch 0 is read; -1: before the last group, with a wait.
__host__ __device__ constexpr int owned_carry_read_group(int L_a) { return owned_window_groups(L_a) >= 3 ? 0 : -1; }

// The id batch of B that its id register holds when a run starts (carried or cold): the one its group 0 reads.
__host__ __device__ constexpr int owned_carry_start_batch() { return owned_window_issue_batch(0); }

// The touching.  The workers issue no cold load of boundaries or ids: somebody reads one word per 128-B line of both a
// few task slots ahead of the task counter, CHUNK by chunk.  Chunk c of a workgroup with T task slots per phase is the
// task slots [t0, t0 + chunk) of phase P, c = P owned_touch_chunks(T, chunk) + t0 / chunk: consecutive rows
// [r_first, r_last) of one slice (owned_touch_rows), hence one run of boundaries — the words r_first .. r_last of the
// slice's segptr, touched at r_first, at r_last and every 32 words from r_first (owned_touch_boundary) — and one run of
// ids, [segptr[r_first], segptr[r_last]), touched every 32 words from its start (owned_touch_id).
// In the form with a toucher the last wave does that for chunk after chunk, as soon as the task counter is within
// kOwnedTouchLead slots of the chunk's first (dgmi_owned_kernel.h).  In the DUTY form every wave is a worker and the
// touching is a duty of task slots: the wave that reserves the first slot of chunk c (owned_duty_chunk) touches, before
// anything else, the chunks of owned_duty_span — chunk c + lead_chunks, the first duty also the chunks 0 .. lead_chunks
// in front of it — and then goes on as any worker.  Every chunk of the launch is touched by exactly one duty, a chunk
// past the last one by none, and a slot past the last task carries none.
// The kernel and the host test (tests/test_owned_duty_host.py) take all of this from the functions below.
constexpr int kOwnedTouchChunk = 4;      // task slots the toucher touches for at a time
constexpr int kOwnedTouchLead = 8;       // task slots between the counter and the first slot of the chunk it touches for
constexpr int kOwnedTouchLineWords = 32;  // 128 B of int32 words
// The duty form's built-in chunk is a WHOLE PHASE — the plan's task slots, OwnedPlan::tasks: one duty per phase, by the
// wave that reserves the phase's first task — and its lead one phase (measured: profiles/owned_duty/README.md — the
// fewer duties the better, from 4 slots per duty, which gains nothing over the toucher, to a phase per duty).

__host__ __device__ constexpr int owned_touch_chunks(int T, int chunk) { return (T + chunk - 1) / chunk; }  // per phase

struct OwnedTouchRows {
  bool any;                  // false: a short last round has none of the chunk's rows
  int slice;
  int64_t r_first, r_last;   // destination rows [r_first, r_last): boundary words r_first .. r_last of the slice
};

__host__ __device__ inline OwnedTouchRows owned_touch_rows(const OwnedPlan& pl, int64_t wg, int T, int chunk, int c) {
  const int per_phase = owned_touch_chunks(T, chunk);
  const int P = c / per_phase, t0 = (c - P * per_phase) * chunk;
  const OwnedPhase ph = owned_phase(pl, P);
  const int64_t in_round = owned_round_rows(pl, wg, ph.row_round);
  const int64_t lds_first = (int64_t)t0 * pl.G * pl.R;
  int64_t lds_last = lds_first + (int64_t)chunk * pl.G * pl.R;
  if (lds_last > in_round) lds_last = in_round;
  OwnedTouchRows r{lds_first < lds_last, ph.slice, 0, 0};
  if (r.any) {
    r.r_first = owned_task(pl, wg, ph.row_round, t0, 0).row0;
    r.r_last = r.r_first + (lds_last - lds_first);
  }
  return r;
}

// The j-th boundary word (a row number of the slice) touched for the rows [r_first, r_last); -1: none, and none after it.
__host__ __device__ constexpr int64_t owned_touch_boundary(int64_t r_first, int64_t r_last, int64_t j) {
  return j == 0 ? r_first : (j == 1 ? r_last : (r_first + (j - 1) * kOwnedTouchLineWords <= r_last ? r_first + (j - 1) * kOwnedTouchLineWords : -1));
}

// The j-th id word touched for the edges [e0, e1); -1: none, and none after it.
__host__ __device__ constexpr int64_t owned_touch_id(int64_t e0, int64_t e1, int64_t j) {
  return e0 + j * kOwnedTouchLineWords < e1 ? e0 + j * kOwnedTouchLineWords : -1;
}

// The chunk whose duty the wave that reserves task k takes (k counts the slots phase-major, as the task counter does);
// -1: none — a slot that is not the first of a chunk, or one past the last task.
__host__ __device__ inline int owned_duty_chunk(int k, int T, int chunk, int phases) {
  if (k < 0 || T < 1 || k >= phases * T) return -1;
  const int P = k / T, t = k - P * T;
  return t % chunk == 0 ? P * owned_touch_chunks(T, chunk) + t / chunk : -1;
}

__host__ __device__ constexpr int owned_duty_lead_chunks(int lead, int chunk) { return (lead + chunk - 1) / chunk; }

// The chunks [first, end) the duty of chunk c touches, of `chunks` = phases x owned_touch_chunks in all.
struct OwnedDutySpan {
  int first, end;
};

__host__ __device__ inline OwnedDutySpan owned_duty_span(int c, int chunks, int lead_chunks) {
  OwnedDutySpan s{c == 0 ? 0 : c + lead_chunks, c + lead_chunks + 1};
  if (s.end > chunks) s.end = chunks;
  if (s.first > s.end) s.first = s.end;
  return s;
}

}  // namespace dgmi

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
// The plan (rows per workgroup, rounds, phases, tasks): dgmi_owned_common.h.  The kernel body — the task protocol of the
// 15 worker waves and why it cannot deadlock, their rolling window of gathers and its hand-over from task to task, the
// toucher wave and its advisory phase gate (off unless asked for: kOwnedLag) — is owned_body, dgmi_owned_kernel.h, and is
// described there.  Here: the two kernels made of it, their launcher, and the rules that choose the form and the layout.
//
// Two forms of the one kernel (WAVES): a 16-wave workgroup per CU, or — the cap of 1024 threads per workgroup lifted —
// two co-resident 12-wave workgroups per CU, each with half the LDS rows (owned_plan's wgs_per_cu): 22 workers instead
// of 15, 6 waves per SIMD.  Their co-residency is asked of the runtime once per kernel and LDS size; where it says no,
// the 16-wave form runs.  Nothing waits for the other workgroup of a CU.  Measured (profiles/owned_wgs/README.md): the
// kernel is short of waves (12 instead of 16 per CU: +17-23 %), yet 512 free-running workgroups drift over more slices
// than 256 and lose in L2 misses more than the waves return, so the built-in rule selects the second form for no class.
//
// The DUTY form (spmm_owned_duty_kernel below; owned_body<..., DUTY>, dgmi_owned_kernel.h) has no toucher: all 16 waves
// take tasks, and once per phase the wave that reserves the phase's first task touches the boundaries and ids of the
// next phase.  It is what the four fp32 classes of the step run (owned_class_duty; profiles/owned_duty/README.md);
// everything it is not built for — other widths, 64-bit offsets, a gate, the two-workgroup form, a bf16 table — keeps
// the toucher.
//
// A bf16 table (x_bytes == 2) takes the same form through the same launcher (spmm_owned_try) and the same plan with 8
// columns per lane; its kernel — the 16-wave form without a gate — is spmm_owned_bf16_kernel below, its classes are
// owned_class_form's for x_bytes == 2.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "dgmi_owned_common.h"
#include "dgmi_owned_kernel.h"
#include "dgmi_sliced_common.h"

namespace dgmi {
namespace {

constexpr int64_t kOwnedSpinTicks = 3000;  // 30 us of the 100 MHz real-time counter: a stuck gate falls through
constexpr int64_t kOwnedMinRows = 32768;   // built-in rule: below, a workgroup has too few tasks per phase
// Built-in gate: none.  A closed gate drains the workgroup — a task lives ~5 us of a ~15 us phase — so lag 0 costs
// 35-45 % and lag 1 25-30 % of a product, far more than the L2 hits it buys (profiles/owned_rows/README.md).
constexpr int kOwnedLag = -1;
constexpr int kOwnedWideSlices = 16;       // the slice count of the one class whose layout is not the pair's (dgmi_sliced_layout_slices)
constexpr int kOwnedAssumedCus = 256;      // workgroups the layout rule plans for where no device can be asked (MI355X)

// The two kernels of the one body (owned_body, dgmi_owned_kernel.h), with one parameter list but for the table's
// element type.  VALS: 0 = unit edge values, 2 = multiplicities in the id words (dgmi_sliced.hip).
// An fp32 table.  WAVES: waves of the workgroup, the last one the toucher: kOwnedWaves (one workgroup per CU, 4 waves
// per SIMD) or kOwnedPairWaves (two co-resident workgroups per CU, 6 waves per SIMD: the register budget the second
// launch bound asks the compiler for).
template <int LPR, int VALS, bool OFF32, int WAVES>
__global__ __launch_bounds__(kWave* WAVES, WAVES == kOwnedWaves ? 4 : 6) void spmm_owned_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ dst_scale, float* __restrict__ Y, int64_t ldy, int64_t n_dst, int F, OwnedPlan pl,
    unsigned* __restrict__ arrive, int lag, int64_t spin_ticks, int workers, Epilogue ep) {
  owned_body<OwnedRowF32, LPR, VALS, OFF32, WAVES, true>(segptr, indices, X, ldx, dst_scale, Y, ldy, n_dst, F, pl, arrive, lag,
                                                         spin_ticks, workers, ep);
}

// A bf16 table: the 16-wave form without a gate — `arrive`, `lag` and `spin_ticks` go unread.  Left out on purpose: the
// two-workgroup form (it lost on every class in fp32: profiles/owned_wgs/README.md) and the phase gate (measured as a
// loss in fp32: profiles/owned_rows/README.md).
template <int LPR, int VALS, bool OFF32>
__global__ __launch_bounds__(kWave* kOwnedWaves, 4) void spmm_owned_bf16_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const uint16_t* __restrict__ X, int64_t ldx,
    const float* __restrict__ dst_scale, float* __restrict__ Y, int64_t ldy, int64_t n_dst, int F, OwnedPlan pl,
    unsigned* __restrict__ arrive, int lag, int64_t spin_ticks, int workers, Epilogue ep) {
  owned_body<OwnedRowBf16, LPR, VALS, OFF32, kOwnedWaves, false>(segptr, indices, X, ldx, dst_scale, Y, ldy, n_dst, F, pl, arrive,
                                                                 lag, spin_ticks, workers, ep);
}

// An fp32 table whose id words carry the code of the gathered row's scale (SCALED, dgmi_owned_kernel.h;
// include/dgmi_scale.h): the 16-wave form without a gate, 32-bit row offsets.  `table`: n_codes scales, copied into the
// 2^kScaleBits floats of LDS the launch adds behind the plan's.
constexpr size_t kOwnedScaleLdsBytes = sizeof(float) << kScaleBits;
template <int LPR, int VALS>
__global__ __launch_bounds__(kWave* kOwnedWaves, 4) void spmm_owned_scaled_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ dst_scale, float* __restrict__ Y, int64_t ldy, int64_t n_dst, int F, OwnedPlan pl, int workers,
    Epilogue ep, const float* __restrict__ table, int n_codes) {
  owned_body<OwnedRowF32, LPR, VALS, true, kOwnedWaves, false, true>(segptr, indices, X, ldx, dst_scale, Y, ldy, n_dst, F, pl, nullptr,
                                                                     -1, 0, workers, ep, table, n_codes);
}

// The DUTY form (dgmi_owned_kernel.h): sixteen workers, no toucher — the touching is a duty of every `duty_chunk`-th
// task slot, `duty_lead` slots ahead.  Built where the step of bench.py runs the form: an fp32 table, 32-bit offsets,
// 16 waves, no gate, the widths of the measured classes; plain (`table` == nullptr) and SCALED.  A bf16 table keeps its
// toucher: its kernels have not been measured in this form.
template <int LPR, int VALS, bool SCALED>
__global__ __launch_bounds__(kWave* kOwnedWaves, 4) void spmm_owned_duty_kernel(
    const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ dst_scale, float* __restrict__ Y, int64_t ldy, int64_t n_dst, int F, OwnedPlan pl, int workers,
    Epilogue ep, const float* __restrict__ table, int n_codes, int duty_chunk, int duty_lead) {
  owned_body<OwnedRowF32, LPR, VALS, true, kOwnedWaves, false, SCALED, true>(segptr, indices, X, ldx, dst_scale, Y, ldy, n_dst, F, pl,
                                                                             nullptr, -1, 0, workers, ep, table, n_codes, duty_chunk,
                                                                             duty_lead);
}

// The lane-group widths the scaled kernel — and the duty form, scaled or not — is built at: those of the product
// classes it was measured on (F = 128 at full and at half width).  Every other width is declined (the duty form: runs
// with a toucher).
constexpr bool owned_scaled_built(int lpr) { return lpr == 16 || lpr == 32; }
constexpr bool owned_duty_built(int lpr) { return owned_scaled_built(lpr); }

// The worker waves of a workgroup that take tasks (Tuning::sliced_owned_workers; 0: all `all` of them).
int owned_tuned_workers(int all) {
  const int w = tuning().sliced_owned_workers;
  return w > 0 && w < all ? w : 0;
}

// One launch of a kernel with the scaled kernel's parameter list (and `extra` behind it), `lds` bytes of dynamic LDS.
template <auto KERN, typename... Extra>
hipError_t launch_owned_tabled(const SlicedArgs& a, const OwnedPlan& pl, int64_t grid, size_t lds, int workers, hipStream_t s,
                               Extra... extra) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(KERN, dim3((unsigned)grid), dim3(kWave* kOwnedWaves), lds, s, a.segptr, a.indices,
                     static_cast<const float*>(a.X), a.ldx, a.dst_scale, a.Y, a.ldy, a.n_dst, (int)a.F, pl, workers, a.ep,
                     a.scale_table, a.n_codes, extra...);
  return hipGetLastError();
}

template <int LPR>
hipError_t launch_owned_scaled(const SlicedArgs& a, const OwnedPlan& pl, int64_t grid, hipStream_t s) {
  const size_t lds = pl.lds_bytes + kOwnedScaleLdsBytes;
  const int workers = owned_tuned_workers(kOwnedWorkers);
  if (a.id_mult) return launch_owned_tabled<&spmm_owned_scaled_kernel<LPR, 2>>(a, pl, grid, lds, workers, s);
  return launch_owned_tabled<&spmm_owned_scaled_kernel<LPR, 0>>(a, pl, grid, lds, workers, s);
}

// The duty form, plain (a.scale_table == nullptr: no table in LDS) or scaled; `pl`: the plan of kOwnedDutyWorkers workers.
template <int LPR>
hipError_t launch_owned_duty(const SlicedArgs& a, const OwnedPlan& pl, int64_t grid, hipStream_t s) {
  // built-in: a duty per phase, one phase ahead (dgmi_owned_common.h)
  const int chunk = tuning().sliced_owned_duty_chunk > 0 ? tuning().sliced_owned_duty_chunk : pl.tasks;
  const int lead = tuning().sliced_owned_duty_lead > 0 ? tuning().sliced_owned_duty_lead : chunk;
  const int workers = owned_tuned_workers(kOwnedDutyWorkers);
  if (a.scale_table != nullptr) {
    const size_t lds = pl.lds_bytes + kOwnedScaleLdsBytes;
    if (a.id_mult) return launch_owned_tabled<&spmm_owned_duty_kernel<LPR, 2, true>>(a, pl, grid, lds, workers, s, chunk, lead);
    return launch_owned_tabled<&spmm_owned_duty_kernel<LPR, 0, true>>(a, pl, grid, lds, workers, s, chunk, lead);
  }
  if (a.id_mult) return launch_owned_tabled<&spmm_owned_duty_kernel<LPR, 2, false>>(a, pl, grid, pl.lds_bytes, workers, s, chunk, lead);
  return launch_owned_tabled<&spmm_owned_duty_kernel<LPR, 0, false>>(a, pl, grid, pl.lds_bytes, workers, s, chunk, lead);
}

template <typename Row, int LPR, int VALS, bool OFF32, int WAVES>
constexpr auto owned_kernel() {
  if constexpr (std::is_same<Row, OwnedRowBf16>::value)
    return &spmm_owned_bf16_kernel<LPR, VALS, OFF32>;
  else
    return &spmm_owned_kernel<LPR, VALS, OFF32, WAVES>;
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
// `x_bytes`: bytes per element of the gathered table.  The classes of a bf16 table (x_bytes == 2: spmm_owned_bf16_kernel;
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

// `Row`: the row policy of the table's element type.  `resident` (the two-workgroup form only): false = its workgroups
// would not share a CU, nothing was launched.  The 8-lane groups with multiplicities are not built in that form: they
// do not fit its 80 VGPRs without scratch.
template <typename Row, int LPR, int WAVES>
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
    auto kern = owned_kernel<Row, LPR, V, O, WAVES>();                                                                    \
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
                       static_cast<const typename Row::Elem*>(a.X), a.ldx, a.dst_scale, a.Y, a.ldy, a.n_dst, (int)a.F, pl, \
                       arrive, lag, spin_ticks, workers, a.ep);                                                           \
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

// The lane-group widths a table's element type has: 8 .. 64 of an fp32 table, 8 .. 32 of a bf16 one (sliced_lpr).
template <typename Row, int WAVES>
hipError_t launch_owned_width(const SlicedArgs& a, const OwnedPlan& pl, int lpr, int64_t grid, bool off32, int lag,
                              int64_t spin_ticks, hipStream_t s, bool* resident) {
  switch (lpr) {
    case 8: return launch_owned<Row, 8, WAVES>(a, pl, grid, off32, lag, spin_ticks, s, resident);
    case 16: return launch_owned<Row, 16, WAVES>(a, pl, grid, off32, lag, spin_ticks, s, resident);
    case 32: return launch_owned<Row, 32, WAVES>(a, pl, grid, off32, lag, spin_ticks, s, resident);
    case 64:
      if constexpr (Row::kMaxLpr >= 64)
        return launch_owned<Row, 64, WAVES>(a, pl, grid, off32, lag, spin_ticks, s, resident);
      else
        return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}

// The classes of owned_class_form whose SCALED product (scale codes in the id words: no pre-scale pass, the scale out of
// LDS) beat pre-scale pass + plain kernel inside the step of bench.py by more than the latter's min .. max spread
// (profiles/owned_scale/README.md).  A class not named here keeps the pre-scale pass.
bool owned_class_scaled(const OwnedPlan& pl, bool id_mult, int64_t table_bytes) {
  const auto mib = [&](int64_t lo, int64_t hi) { return table_bytes >= (lo << 20) && table_bytes <= (hi << 20); };
  if (pl.slices == kOwnedSlices) {
    if (pl.col_rounds == 1 && pl.row_rounds == 2 && !id_mult && mib(16, 32)) return true;  // 50 000 sources -> 100 000 rows, unit values
    if (pl.col_rounds == 2 && pl.row_rounds == 1 && id_mult && mib(48, 64)) return true;   // kNN-64 at 100 000 nodes
    if (pl.col_rounds == 1 && pl.row_rounds == 1 && id_mult && mib(16, 32)) return true;   // kNN-64 at 50 000 nodes
  }
  if (pl.slices == kOwnedWideSlices && pl.col_rounds == 1 && pl.row_rounds == 1 && !id_mult && mib(48, 64)) return true;
  return false;
}

// The classes of owned_class_form whose product, inside the step of bench.py, is faster in the duty form than with a
// toucher by more than the toucher form's min .. max spread (profiles/owned_duty/README.md).
// All four fp32 classes of owned_class_form cleared that, plain and scaled.
bool owned_class_duty(const OwnedPlan& pl, bool id_mult, int64_t table_bytes) {
  const auto mib = [&](int64_t lo, int64_t hi) { return table_bytes >= (lo << 20) && table_bytes <= (hi << 20); };
  if (pl.slices == kOwnedSlices) {
    if (pl.col_rounds == 1 && pl.row_rounds == 2 && !id_mult && mib(16, 32)) return true;  // 50 000 sources -> 100 000 rows, unit values
    if (pl.col_rounds == 2 && pl.row_rounds == 1 && id_mult && mib(48, 64)) return true;   // kNN-64 at 100 000 nodes
    if (pl.col_rounds == 1 && pl.row_rounds == 1 && id_mult && mib(16, 32)) return true;   // kNN-64 at 50 000 nodes
  }
  if (pl.slices == kOwnedWideSlices && pl.col_rounds == 1 && pl.row_rounds == 1 && !id_mult && mib(48, 64)) return true;  // 100 000 sources -> 50 000 rows
  return false;
}

// `launch` = false: the decision alone (*taken as a launch would leave it), nothing is launched.
hipError_t owned_try(const SlicedArgs& a, hipStream_t s, bool* taken, bool launch);

}  // namespace

hipError_t spmm_owned_try(const SlicedArgs& a, hipStream_t s, bool* taken) {
  *taken = false;
  if (a.scale_table != nullptr) return hipErrorInvalidValue;  // coded id words come in through spmm_owned_scaled only
  return owned_try(a, s, taken, true);
}

bool spmm_owned_scaled_takes(const SlicedArgs& a) {
  bool taken = false;
  return a.scale_table != nullptr && owned_try(a, nullptr, &taken, false) == hipSuccess && taken;
}

hipError_t spmm_owned_scaled(const SlicedArgs& a, hipStream_t s, bool* taken) {
  *taken = false;
  if (a.scale_table == nullptr) return hipErrorInvalidValue;
  return owned_try(a, s, taken, true);
}

namespace {

hipError_t owned_try(const SlicedArgs& a, hipStream_t s, bool* taken, bool launch) {
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
  // the one-workgroup plan with the general tasks-per-phase target names the class — the two measured kNN-64 classes
  // then take theirs — and is what a two-workgroup launch that cannot co-reside falls back to
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
  bool resident = true;
  // The duty form (sixteen workers, no toucher): where it is built — an fp32 table, 32-bit offsets, the widths of the
  // measured classes — and nothing asks for what only the toucher form has (a gate, the two-workgroup form), for
  // sliced_owned_duty = 1 or a class of owned_class_duty.  Its plan is the same plan with the tasks-per-phase target of
  // 16 workers; should that one not fit, the toucher form runs.
  const int lag = tune.sliced_owned_lag >= -1 ? tune.sliced_owned_lag : kOwnedLag;
  OwnedPlan pl_duty{};
  if (a.x_bytes == 4 && off32 && owned_duty_built(lpr) && lag < 0 && tune.sliced_owned_wgs != 2 && rule != 2 &&
      (tune.sliced_owned_duty == 1 || (tune.sliced_owned_duty < 0 && rule == 1 && owned_class_duty(pl, a.id_mult, table_bytes)))) {
    pl_duty = owned_plan(a.n_dst, a.F, lpr, grid, tune.sliced_owned_rows, tune.sliced_owned_lds_rows, 1, phase_tasks, slices, cols, kOwnedDutyWorkers);
    if (pl_duty.lds_bytes + (a.scale_table != nullptr ? kOwnedScaleLdsBytes : 0) > (size_t)(160 << 10)) pl_duty.ok = false;
  }
  if (a.scale_table != nullptr) {
    // The scaled kernel: one form (16 waves, no gate, 32-bit offsets, an fp32 table) at the widths of its classes.  A
    // product outside it — or of a class that keeps the pre-scale pass — is declined: nothing else masks a coded id word.
    // (a forced owned form — sliced_owned = 1 — runs every product it can in that form, this one included)
    const bool wanted = tune.sliced_owned_scaled == 1 ||
                        (tune.sliced_owned_scaled < 0 && (tune.sliced_owned == 1 || (rule == 1 && owned_class_scaled(pl, a.id_mult, table_bytes))));
    if (!wanted || a.x_bytes != 4 || a.n_src > ((int64_t)1 << kScaleShift) || a.n_codes < 1 || a.n_codes > (1 << kScaleBits) ||
        !off32 || !owned_scaled_built(lpr) || pl.lds_bytes + kOwnedScaleLdsBytes > (size_t)(160 << 10) || tune.sliced_owned_lag >= 0 ||
        tune.sliced_owned_wgs == 2)
      return hipSuccess;
    *taken = true;
    if (!launch) return hipSuccess;
    if (pl_duty.ok) return lpr == 16 ? launch_owned_duty<16>(a, pl_duty, grid, s) : launch_owned_duty<32>(a, pl_duty, grid, s);
    return lpr == 16 ? launch_owned_scaled<16>(a, pl, grid, s) : launch_owned_scaled<32>(a, pl, grid, s);
  }
  if (!launch) return hipSuccess;
  if (a.x_bytes == 2) {
    // The bf16 kernel is built in one form only — one 16-wave workgroup per CU, no phase gate — so sliced_owned_lag,
    // sliced_owned_spin_ticks and sliced_owned_wgs are ignored for a bf16 table, and without arrive counters nothing
    // is asked of the plane workspace.
    *taken = true;
    return launch_owned_width<OwnedRowBf16, kOwnedWaves>(a, pl, lpr, grid, off32, -1, 0, s, &resident);
  }
  if (pl_duty.ok) {  // no gate, hence no arrive counters: nothing is asked of the plane workspace
    *taken = true;
    return lpr == 16 ? launch_owned_duty<16>(a, pl_duty, grid, s) : launch_owned_duty<32>(a, pl_duty, grid, s);
  }
  // the arrive counters live in the first bytes of the caller's plane workspace (n_slices * n_dst * ldp floats)
  const auto arrive_fits = [&](const OwnedPlan& p) {
    return sizeof(unsigned) * 8 * (size_t)p.phases <= sizeof(float) * (size_t)a.n_slices * (size_t)a.n_dst * (size_t)a.ldp;
  };
  if (!arrive_fits(pl)) return hipSuccess;
  const int form = tune.sliced_owned_wgs == 1 || tune.sliced_owned_wgs == 2 ? tune.sliced_owned_wgs : (rule == 2 ? 2 : 1);
  const int64_t spin = tune.sliced_owned_spin_ticks > 0 ? tune.sliced_owned_spin_ticks : kOwnedSpinTicks;
  *taken = true;
  if (form == 2) {
    const int64_t grid2 = tune.sliced_owned_grid > 0 ? grid : 2 * grid;
    const OwnedPlan pl2 = owned_plan(a.n_dst, a.F, lpr, grid2, tune.sliced_owned_rows, tune.sliced_owned_lds_rows, 2, kOwnedPhaseTasks, slices);
    if (pl2.ok && pl2.lds_bytes <= (size_t)(80 << 10) && arrive_fits(pl2)) {
      const hipError_t err = launch_owned_width<OwnedRowF32, kOwnedPairWaves>(a, pl2, lpr, grid2, off32, lag, spin, s, &resident);
      if (err != hipSuccess || resident) return err;
    }
  }
  return launch_owned_width<OwnedRowF32, kOwnedWaves>(a, pl, lpr, grid, off32, lag, spin, s, &resident);
}

}  // namespace

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

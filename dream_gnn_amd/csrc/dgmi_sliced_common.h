// dgmi_sliced_common.h — what the forms of the XCD-local SpMM share (the pair: dgmi_sliced.hip with the one gather body
// of dgmi_sliced_kernel.h; the workgroup-owned form: dgmi_owned.hip), for an fp32 and for a bf16 table: constants, the
// plane-row store, what the row policies of an element type have in common, the touch-ahead blocks, the launch geometry
// and the column-pass rule.  The two tables differ by the bytes of a gathered element (4 / 2), hence the columns a lane
// owns (one 16-B load: 4 / 8) and the widest lane group (64 / 32: 256 columns either way).  The host side (sliced_runs,
// sliced_run, sliced_geometry, sliced_lpr) is also what a stand-alone host program includes
// (tests/test_sliced_taper_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgmi_kernels.h"
#include "dgmi_segment.h"
#include "dgmi_tuning.h"

namespace dgmi {

// The workgroup-owned form (dgmi_owned.hip): rows summed in LDS, no planes, bit-identical to the pair, from an fp32 or
// a bf16 table.  *taken: the product was launched; false (and hipSuccess): the form does not take it and the caller
// runs the pair.
hipError_t spmm_owned_try(const SlicedArgs& a, hipStream_t s, bool* taken);

namespace {

constexpr int64_t kColumnPassMinRows = 32768;  // column passes only when a pass still has >= ~8k waves
constexpr int64_t kTaperRows = 8192;  // rows at the end of a chunk that take shorter runs (sliced_runs, sliced_geometry)
constexpr int kTouchLead = 24;   // worker blocks of a slice between a toucher and the blocks it touches for
constexpr int kTouchGroup = 8;   // worker blocks per toucher block
// Rows per lane group (< LPR: row boundaries live one per lane of the group): a speed knob only (the sums do not depend
// on it).  The step of bench.py on the canonical-order kernels, ms of the four half-width (16-lane, two-pass) products /
// of the four full-width (32-lane) ones at 2 / 3 / 4 / 6 / 8 / 12 / 15 rows (profiles/sliced_tail/README.md):
//   no taper      1.344 / 1.345 / 1.359 / 1.385 / 1.407 / 1.460 / 1.484     1.058 / 1.014 / 0.989 / 0.970 / 0.971 / 0.982 / 0.991
//   taper 8192    1.351 / 1.330 / 1.333 / 1.338 / 1.338                     1.072 / 1.020 / 0.997 / 0.969 / 0.961
// Without the taper the half-width products want 2-3 rows and the full-width ones 6-8 (what the short runs gave the
// half-width products was mostly a shorter drain); with it 8 rows are within 0.01 ms — half a run-to-run spread of the
// step — of the best value of either width at any taper, so one value serves every width.
constexpr int kRowsPerGroup = 8;

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store_plane_row(float* p, const float4& v) {
  // one streaming 16-B store: the planes are write-once / read-once; keep them from evicting
  // the XCD's slice of X out of L2
  // (ordinary stores instead: the step of bench.py 3.03 ms against 2.85 ms, profiles/r03_swept_experiment/)
  v4f t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(p));
}

// What the row policies of the two forms of the XCD-local SpMM share, per element type of the gathered table (the pair:
// SlicedRowF32 / SlicedRowBf16, dgmi_sliced_kernel.h; the workgroup-owned form: OwnedRowF32 / OwnedRowBf16,
// dgmi_owned_kernel.h): the columns a lane owns, the registers of a gathered row, its load, the sums and the canonical
// step acc + x / fmaf(w, x, acc).
// An fp32 table: a lane owns 4 columns — one 16-B load, one float4 sum.
struct RowF32 {
  typedef float Elem;
  typedef float4 Reg;  // a gathered row: this lane's columns
  typedef float4 Acc;
  static constexpr int kCols = 4;
  static constexpr int kMaxLpr = 64;  // the widest lane group: 256 columns either way

  static __device__ __forceinline__ Acc zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

  // Source row `idx` of the feature table.  OFF32: the table is < 4 GiB, so the byte offset fits 32 bits — one
  // v_mul_lo_u32 and a global_load with a scalar base and a 32-bit vector offset, instead of the six-instruction 64-bit
  // multiply-add chain a (int64 ldx) product costs per gathered row.  X is the (wave-uniform) table base, Xc = X + this
  // lane's column.
  template <bool OFF32>
  static __device__ __forceinline__ Reg load(const Elem* __restrict__ X, const Elem* __restrict__ Xc, int idx, int64_t ldx,
                                             uint32_t row_bytes, uint32_t col_bytes) {
    if (OFF32) return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(X) + ((uint32_t)idx * row_bytes + col_bytes));
    return ld4(Xc + (int64_t)idx * ldx);
  }

  template <bool WEIGHTED>
  static __device__ __forceinline__ void add(Acc& acc, float w, const Reg& x) {
    if (WEIGHTED) {
      acc.x = fmaf(w, x.x, acc.x);
      acc.y = fmaf(w, x.y, acc.y);
      acc.z = fmaf(w, x.z, acc.z);
      acc.w = fmaf(w, x.w, acc.w);
    } else {
      acc.x += x.x;
      acc.y += x.y;
      acc.z += x.z;
      acc.w += x.w;
    }
  }
};

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// A bf16 table: a lane owns 8 columns — one 16-B load, each of its four dwords widened by a shift and a mask into the
// two floats of one column PAIR.  The eight sums are kept as those four pairs, in two-element vectors: the adds are
// packed adds (or packed fmas) of a widened dword onto its pair, element for element what acc + x / fmaf(w, x, acc)
// give.  Left as eight scalars the compiler chooses the pairs of its packed adds itself, not always these, and moves
// the sums between them (profiles/owned_one_body/README.md).
struct RowBf16 {
  typedef uint16_t Elem;
  typedef v4u Reg;
  typedef float v2f __attribute__((ext_vector_type(2)));
  struct Acc {
    v2f p[4];  // columns (0, 1), (2, 3), (4, 5), (6, 7)
  };
  static constexpr int kCols = 8;
  static constexpr int kMaxLpr = 32;

  static __device__ __forceinline__ Acc zero() { return Acc{{v2f(0.f), v2f(0.f), v2f(0.f), v2f(0.f)}}; }
  static __device__ __forceinline__ Acc pairs(const float4& a, const float4& b) {
    return Acc{{v2f{a.x, a.y}, v2f{a.z, a.w}, v2f{b.x, b.y}, v2f{b.z, b.w}}};
  }
  static __device__ __forceinline__ float4 half(const Acc& t, int h) {  // columns 4 h .. 4 h + 3
    return make_float4(t.p[2 * h].x, t.p[2 * h].y, t.p[2 * h + 1].x, t.p[2 * h + 1].y);
  }

  // this lane's 8 columns of source row `idx`.  OFF32: see RowF32::load
  template <bool OFF32>
  static __device__ __forceinline__ Reg load(const Elem* __restrict__ X, const Elem* __restrict__ Xc, int idx, int64_t ldx,
                                             uint32_t row_bytes, uint32_t col_bytes) {
    if (OFF32) return *reinterpret_cast<const v4u*>(reinterpret_cast<const char*>(X) + ((uint32_t)idx * row_bytes + col_bytes));
    return *reinterpret_cast<const v4u*>(Xc + (int64_t)idx * ldx);
  }

  // one dword onto its pair.  bf16 -> fp32 is a shift (element 2k: the low half of dword k) or a mask (element 2k + 1): exact
  template <bool WEIGHTED>
  static __device__ __forceinline__ void add_pair(v2f& acc, float w, uint32_t d) {
    const v2f x = {__uint_as_float(d << 16), __uint_as_float(d & 0xffff0000u)};
    if (WEIGHTED)
      acc = __builtin_elementwise_fma(v2f(w), x, acc);
    else
      acc += x;
  }

  template <bool WEIGHTED>
  static __device__ __forceinline__ void add(Acc& acc, float w, const Reg& x) {
#pragma unroll
    for (int k = 0; k < 4; ++k) add_pair<WEIGHTED>(acc.p[k], w, x[k]);
  }
};

// Which destination rows a lane group sums.  A chunk's rows [0, n_rows) (relative to row_begin) are cut, in order, into
// three sections of runs: the body in runs of `run[0]` = R rows, then — the tapered tail — the first half of the last
// `taper` rows in runs of ceil(R / 2) and the second half in runs of ceil(R / 4), so that the blocks that start last are
// the shortest-lived ones and the launch drains quickly.  A worker block takes `groups` (4 waves x G lane groups)
// consecutive runs of ONE section; the last block of a section may be ragged.  The row sums do not depend on any of
// this (canonical order, dgmi_sliced.hip), and the taper is a function of the row count alone: not of the width, the
// slice or where the chunk lies.  sliced_runs is the host side (it also counts the blocks), sliced_run the mapping both
// gather kernels, the touchers and the host test use; nothing else computes it.
struct SlicedRuns {
  int64_t end[3];     // chunk-relative row at which each section ends (end[2] = n_rows)
  int64_t blocks[3];  // worker blocks up to the end of each section (blocks[2] = all worker blocks of a slice)
  int run[3];         // rows per lane group in each section
  int groups;         // lane groups per worker block
};

struct SlicedRun {
  int64_t first;  // chunk-relative first row; n_rows when the group has nothing to do
  int rows;
};

// `taper`: rows at the end of the chunk that take the shorter runs (clamped to [0, n_rows]).
__host__ __device__ inline SlicedRuns sliced_runs(int64_t n_rows, int R, int G, int64_t taper) {
  SlicedRuns t;
  taper = taper < 0 ? 0 : (taper < n_rows ? taper : n_rows);
  t.groups = kWavesPerBlock * G;
  t.run[0] = R;
  t.run[1] = (R + 1) / 2;
  t.run[2] = (R + 3) / 4;
  t.end[0] = n_rows - taper;
  t.end[1] = n_rows - taper / 2;
  t.end[2] = n_rows;
  int64_t blocks = 0, begin = 0;
  for (int s = 0; s < 3; ++s) {
    const int64_t per_block = (int64_t)t.groups * t.run[s];
    blocks += (t.end[s] - begin + per_block - 1) / per_block;
    t.blocks[s] = blocks;
    begin = t.end[s];
  }
  return t;
}

// The run of lane group `slot` (wave * G + group) of worker block `block` (numbered per slice, without the touchers).
// Slot 0 of a block is never idle, so sliced_run(t, block, 0).first is the block's first row (n_rows past the last block).
__host__ __device__ inline SlicedRun sliced_run(const SlicedRuns& t, int64_t block, int slot) {
  const int s = block < t.blocks[0] ? 0 : (block < t.blocks[1] ? 1 : 2);
  const int64_t begin = s > 0 ? t.end[s - 1] : 0, block0 = s > 0 ? t.blocks[s - 1] : 0;
  const int64_t first = begin + ((block - block0) * t.groups + slot) * t.run[s];
  if (block >= t.blocks[2] || first >= t.end[s]) return SlicedRun{t.end[2], 0};
  const int64_t left = t.end[s] - first;
  return SlicedRun{first, (int)(left < t.run[s] ? left : t.run[s])};
}

// Touch-ahead.  The id stream and the row boundaries are read once, so a wave's first two loads (boundaries, then
// ids — dependent) miss every cache, and it gathers nothing for two memory latencies of its ~20 us life: inside a
// training step, where the other products have pushed this one's ids out of the Infinity Cache, that is 10-25 % of the
// product.  Every (touch_group + 1)-th block of a slice therefore gathers nothing: it touches the boundaries and the id
// lines (one word per 128-B line) of the touch_group worker blocks that start touch_lead worker blocks further on IN THE
// SAME SLICE — same XCD, same L2, a few microseconds later — and leaves.  Nobody waits for these loads but the toucher
// (vmcnt is in order: a worker that issued them would hold its own first gathers back).  A hint: results never depend on it.
// The blocks it touches for are the worker blocks that really start there: their rows come from sliced_run.
// `block`: this block's number within its slice, touchers included.  True: the block was a toucher and is done
// (block-uniform); false: a worker, `block` renumbered without the touchers.
template <bool HAS_VALS, bool KEEP>
__device__ __forceinline__ bool touch_ahead(const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices,
                                            const float* __restrict__ vals, const int32_t* __restrict__ eid, int64_t n_dst,
                                            int64_t row_begin, int64_t row_end, int slice, const SlicedRuns& runs,
                                            int touch_lead, int touch_group, int lane, int wave, int64_t& block) {
  const int64_t t = block / (touch_group + 1);
  if (block % (touch_group + 1) == 0) {
    __shared__ int range[2];
    const int32_t* sp_s = segptr + (int64_t)slice * n_dst;
    const int64_t ahead = t * touch_group + touch_lead;
    const int64_t r_first = row_begin + sliced_run(runs, ahead, 0).first;
    if (r_first >= row_end) return true;  // block-uniform
    const int64_t r_last = row_begin + sliced_run(runs, ahead + touch_group, 0).first;  // row_end past the last block
    int keepalive = 0;
    if (wave == 0) {  // lanes 0 / 1: the id range of those blocks; the others: one word per line of their boundaries
      const int64_t rp = lane == 0 ? r_first : (lane == 1 ? r_last : r_first + (int64_t)(lane - 1) * 32);
      if (rp <= r_last) {
        const int v = sp_s[rp];
        if (lane < 2) range[lane] = v;
        keepalive = v;
      }
    }
    __syncthreads();
    const int e0 = range[0], e1 = range[1];
    for (int64_t p = (int64_t)e0 + (int64_t)threadIdx.x * 32; p < e1; p += (int64_t)blockDim.x * 32) {
      keepalive ^= indices[p];
      if (HAS_VALS) keepalive ^= __float_as_int(vals[p]);
      if (KEEP) keepalive ^= eid[p];
    }
    asm volatile("" ::"v"(keepalive));  // the loads exist, and are waited for, without an instruction
    return true;
  }
  block -= t + 1;  // worker blocks are numbered without the touchers
  return false;
}

// What one gather launch looks like on the host.
struct SlicedGeometry {
  int R;                // rows per lane group (the body's; the tapered tail's are shorter)
  SlicedRuns runs;      // rows -> worker blocks and lane groups
  int64_t workers;      // worker blocks per slice
  int64_t touchers;     // toucher blocks per slice
  dim3 grid;            // x: n_slices * (workers + touchers); y: column tiles of lpr lanes
  int touch_lead, touch_group;
  bool off32;           // the table is < 4 GiB: 32-bit byte offsets
};

// `elem_bytes`: bytes per element of the gathered table (ldx in elements); a lane owns the 16 / elem_bytes columns of
// one 16-B load.
inline SlicedGeometry sliced_geometry(int64_t row_begin, int64_t row_end, int64_t F, int64_t n_src, int64_t ldx,
                                      int64_t n_slices, int lpr, int elem_bytes) {
  SlicedGeometry g;
  const int G = kWave / lpr, cols = 16 / elem_bytes;
  // Rows per lane group and the tapered tail.  Both are speed knobs only: a row's sum does not depend on where its run
  // starts (dgmi_sliced.hip).  Tuning::sliced_rows forces one value for every width, Tuning::sliced_taper_rows the
  // taper's extent (-1: off) (tools, tests).
  // The taper: a worker block lives ~55 us and a launch is only 2-4 rounds of blocks, so at the end of the grid every CU
  // drains for most of a block life; with the last rows in runs of R / 2 and R / 4 the last blocks are short ones.  Step
  // of bench.py at 8 rows, taper off / 2048 / 4096 / 8192 / 16384 / 32768 rows: 2.423 / 2.388 / 2.362 / 2.343 / 2.347 /
  // 2.366 ms (profiles/sliced_tail/README.md).  Never more than a quarter of the chunk (not measured: short runs cost the
  // full-width products up to 9 % when they cover all rows, the 2-row column above).
  const Tuning& tune = tuning();
  const int rows_req = tune.sliced_rows > 0 ? tune.sliced_rows : kRowsPerGroup;
  g.R = rows_req < 1 ? 1 : (rows_req < lpr ? rows_req : lpr - 1);
  const int64_t quarter = (row_end - row_begin) / 4;
  const int64_t taper = tune.sliced_taper_rows < 0 ? 0
                        : (tune.sliced_taper_rows > 0 ? tune.sliced_taper_rows : (kTaperRows < quarter ? kTaperRows : quarter));
  g.runs = sliced_runs(row_end - row_begin, g.R, G, taper);
  g.workers = g.runs.blocks[2];
  g.off32 = !tune.sliced_no_off32 && (n_src * ldx + F) * elem_bytes < ((int64_t)1 << 32);
  // Touch-ahead (see touch_ahead): one toucher per kTouchGroup worker blocks, kTouchLead worker blocks ahead.  An XCD starts
  // ~7 blocks of its slice per us, so 24 blocks are ~3.5 us of lead — a memory latency, and short enough for the touched
  // lines to still be in its L2.  Step of bench.py: no touching 2.724 ms; wave 0 of every block touching for the block 16 /
  // 24 / 32 further on 2.553 / 2.548 / 2.548; toucher blocks, one per 4 / 8 / 16 workers 2.526 / 2.528 / 2.530
  // (profiles/r03_touch_ahead/).  Tuning::sliced_touch_lead overrides the lead (tools/cold_ids_probe.py; 0 = no touchers).
  g.touch_lead = tune.sliced_touch_lead >= 0 ? tune.sliced_touch_lead : kTouchLead;
  g.touch_group = g.touch_lead > 0 ? kTouchGroup : 0;
  g.touchers = g.touch_group > 0 ? (g.workers + g.touch_group - 1) / g.touch_group : 0;
  g.grid = dim3((unsigned)((g.workers + g.touchers) * n_slices), (unsigned)((F + cols * lpr - 1) / (cols * lpr)));
  return g;
}

// Lane-group width = column tile of (16 / elem_bytes) * lpr columns.  Widest group whose last column tile is still
// >= 85 % used (pick_lpr, dgmi_kernels.h) — unless
// the slice of X one XCD gathers from (n_src / n_slices rows x 16 LPR bytes) is larger than its 4 MiB
// L2: then half the width.  The column tiles are grid.y, dispatched one after the other, so the XCD
// sweeps its slice twice at half the footprint.  Measured at F = 128, fp32: 100k-source table (6.4 -> 3.2 MB
// per pass, bench.py) 0.379 -> 0.365 ms unweighted, 0.512 -> 0.464 ms kNN-64 weighted; config-5 shards
// (tools/cfg5_forms_probe.py) 204 MB table 0.740 -> 0.663 ms, 409 MB table 0.741 -> 0.712 ms (the halves
// of all 8 slices together fit the 256 MiB Infinity Cache; a quarter width gains nothing more).  A
// 50k-source table (already 3.2 MB per slice) loses 10-18 % when halved, so the rule is tied to the
// footprint; and a graph whose time is set by a few very long (virtual) rows pays their dependent gather
// chain once per pass (Zipf(1.2) cut into 2048-edge virtual rows: 0.47 -> 0.62 ms; at the 512 edges
// ops._SplitSliced uses the passes win again, 0.435 -> 0.418 ms): such a caller can ask for full width.
// With edge dropout on the fly every pass re-evaluates keep(eid[p]) per edge (0.386 -> 0.408 ms): full width.
// Half-width groups also mean half as many waves per pass (n_dst / 4 at F = 128): with few, long rows the
// launch no longer fills the chip (config-5 edge-scaled shard, 6250 rows of 1600 edges: 0.382 -> 0.440 ms),
// so the rule needs kColumnPassMinRows destination rows.
// The rule counts the bytes of the table as gathered: at 2 bytes per column a 100 000-source table at F = 128
// (3.2 MB per slice) stays at full width.
// `forced` (Tuning::sliced_lpr, tools) forces a width the element type has: 8 .. 64 (fp32), 8 .. 32 (bf16).
inline int sliced_lpr(int64_t F, int64_t n_src, int64_t n_slices, int64_t n_dst, bool full_width, int n_keep, int elem_bytes,
                      int forced) {
  const int cols = 16 / elem_bytes, widest = 256 / cols;
  int lpr = pick_lpr(F, cols, widest);
  if (lpr >= 32 && !full_width && n_keep == 0 && n_dst >= kColumnPassMinRows) {
    const int64_t width = 16 * (int64_t)lpr < elem_bytes * F ? 16 * (int64_t)lpr : elem_bytes * F;
    const int64_t slice_bytes = (n_src + n_slices - 1) / n_slices * width;
    if (slice_bytes > (4 << 20)) lpr /= 2;
  }
  if (forced == 8 || forced == 16 || forced == 32 || (forced == 64 && widest == 64)) lpr = forced;
  return lpr;
}

}  // namespace
}  // namespace dgmi

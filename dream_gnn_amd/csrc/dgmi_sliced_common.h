// dgmi_sliced_common.h — what the two XCD-local SpMM translation units share (dgmi_sliced.hip: fp32 table;
// dgmi_sliced_bf16.hip: bf16 table): constants, the plane-row store, the touch-ahead blocks, the launch geometry, the
// column-pass rule and the chunk driver.  The two differ by the bytes of a gathered element (4 / 2), hence the columns a
// lane owns (one 16-B load: 4 / 8) and the widest lane group (64 / 32: 256 columns either way).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgmi_kernels.h"
#include "dgmi_segment.h"
#include "dgmi_tuning.h"

namespace dgmi {

// The gather launch of one row chunk [row_begin, row_end) at lane-group width `lpr`, for the element type of a.X.
typedef hipError_t (*SlicedGather)(const SlicedArgs& a, int lpr, int64_t row_begin, int64_t row_end, hipStream_t s);

// The chunk driver (dgmi_sliced.hip): cuts [0, n_dst) into row chunks; per chunk picks the lane-group width
// (sliced_lpr below), runs `gather` and then the plane reduce with the chunk's dst_scale / Y / mask offsets.
hipError_t spmm_sliced_chunks(const SlicedArgs& a, SlicedGather gather, hipStream_t s);

namespace {

constexpr int64_t kColumnPassMinRows = 32768;  // column passes only when a pass still has >= ~8k waves
constexpr int kRowsPerGroup = 8;  // < LPR (row boundaries live one per lane of the group)
constexpr int kTouchLead = 24;   // worker blocks of a slice between a toucher and the blocks it touches for
constexpr int kTouchGroup = 8;   // worker blocks per toucher block

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store_plane_row(float* p, const float4& v) {
  // one streaming 16-B store: the planes are write-once / read-once; keep them from evicting
  // the XCD's slice of X out of L2
  // (ordinary stores instead: the step of bench.py 3.03 ms against 2.85 ms, profiles/r03_swept_experiment/)
  v4f t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(p));
}

// Touch-ahead.  The id stream and the row boundaries are read once, so a wave's first two loads (boundaries, then
// ids — dependent) miss every cache, and it gathers nothing for two memory latencies of its ~20 us life: inside a
// training step, where the other products have pushed this one's ids out of the Infinity Cache, that is 10-25 % of the
// product.  Every (touch_group + 1)-th block of a slice therefore gathers nothing: it touches the boundaries and the id
// lines (one word per 128-B line) of the touch_group worker blocks that start touch_lead worker blocks further on IN THE
// SAME SLICE — same XCD, same L2, a few microseconds later — and leaves.  Nobody waits for these loads but the toucher
// (vmcnt is in order: a worker that issued them would hold its own first gathers back).  A hint: results never depend on it.
// `block`: this block's number within its slice, touchers included.  True: the block was a toucher and is done
// (block-uniform); false: a worker, `block` renumbered without the touchers.
template <int LPR, bool HAS_VALS, bool KEEP>
__device__ __forceinline__ bool touch_ahead(const int32_t* __restrict__ segptr, const int32_t* __restrict__ indices,
                                            const float* __restrict__ vals, const int32_t* __restrict__ eid, int64_t n_dst,
                                            int64_t row_begin, int64_t row_end, int slice, int R, int touch_lead,
                                            int touch_group, int lane, int wave, int64_t& block) {
  constexpr int G = kWave / LPR;
  const int64_t t = block / (touch_group + 1);
  if (block % (touch_group + 1) == 0) {
    __shared__ int range[2];
    const int32_t* sp_s = segptr + (int64_t)slice * n_dst;
    const int64_t rows_blk = (int64_t)kWavesPerBlock * G * R;
    const int64_t r_first = row_begin + (t * touch_group + touch_lead) * rows_blk;
    if (r_first >= row_end) return true;  // block-uniform
    const int64_t r_last = min(r_first + touch_group * rows_blk, row_end);
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
  int R;                // rows per lane group
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
  // Rows per lane group.  In the step (cold id stream, touch-ahead on), G edges/s at 4 / 6 / 8 / 12 / 15 rows: half-width
  // products 31.8 / 31.2 / 30.8 / 28.2 / 27.9, full-width ones 28.4 / 29.5 / 30.1 / 30.2 / 30.3, the step 30.8 / 31.0 / 31.0 /
  // 30.1 / 29.7.  One value for every width: where a group's run starts decides how its batches of 8 are cut, so a
  // width-dependent value would make the column passes round differently from the full-width pass (they are bit-identical,
  // test_xcd_sliced_column_passes).  Tuning::sliced_rows forces a value (tools).
  const Tuning& tune = tuning();
  const int rows_req = tune.sliced_rows > 0 ? tune.sliced_rows : kRowsPerGroup;
  g.R = rows_req < 1 ? 1 : (rows_req < lpr ? rows_req : lpr - 1);
  const int64_t per_block = (int64_t)kWavesPerBlock * G * g.R;
  g.workers = (row_end - row_begin + per_block - 1) / per_block;
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

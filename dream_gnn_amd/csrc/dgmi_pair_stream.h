// dgmi_pair_stream.h — what the pair decoder kernels share around the scorer of dgmi_pair_score.h (gfx950).  Device
// side: the constants of the two task mappings, the two ranking keys with their pad entry, and the ballot append of the
// two "lane column" kernels.  Host side: the two task planners, the operand checks and the known-pair bitmap setup.
// Included by dgmi_pairs.hip (global top-k), dgmi_pairs_above.hip (every pair above a cut), dgmi_pairs_rows.hip (per-row
// top-k) and dgmi_pairs_given.hip (list scorer, count scan).
//
// Every kernel keeps 32 "lane" rows per wave in VGPRs (one per lane column) and reads "stream" rows from LDS two at a
// time.  In the lane-column mapping (global top-k, emit) a task is (a chunk of stream rows, 128 lane rows): the four
// waves hold four different sets of 32 lane rows and all walk the whole chunk.  In the shared-row mapping (per-row
// top-k, count scan) a task is (32 lane items, a segment of the stream axis): the four waves hold the SAME 32 lane rows
// and split each staged chunk.
//
// What is NOT here, on purpose: the staging loop, the task loops and the bitonic sorts stay in each kernel.  One
// staging helper taking a callable for the source row, one loop per mapping with the consumer as a sink, and one sort on
// a key policy were written, and each changes the code the compiler emits for the scoring loop around it: the staging
// helper alone takes the count scan from 289 to 319 wait states between its MFMAs and splits three of its packed adds;
// the shared sort changes all four kernels that sort.  What is here leaves every kernel's instructions exactly what
// they were (profiles/pairs_one_stream/kernel_isa_identity.txt); sharing more needs timing on the device first.
#ifndef DGMI_PAIR_STREAM_H_
#define DGMI_PAIR_STREAM_H_

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dgmi_pair_score.h"

namespace {

constexpr int kThreads = 256;            // 4 waves
constexpr int kGrid = 256;               // persistent workgroups (one per CU)
constexpr int kLaneRows = 32;            // lane rows per wave (one per lane column)
constexpr int kRowStride = 2 * 68;       // a row in LDS: two 64-float halves, 4 floats apart (conflict-free broadcast)
constexpr int kSub = 4;                  // stream rows a wave scores between two fill checks
// lane columns
constexpr int kGroupCols = 4 * kLaneRows;  // lane rows per task
constexpr int kMaxChunk = 64;              // stream rows per task (at most)
// shared rows
constexpr int kChunk = 128;              // stream rows staged in LDS at a time
constexpr int kTaskTarget = 16 * kGrid;  // tasks wanted: >= 16 rounds keeps the last one short
constexpr int kMaxSeg = 256;             // segments of the stream axis, at most
constexpr int kMinSeg = 32;              // stream rows per segment, at least
// merges
constexpr int kMaxFan = 64;              // sorted lists one merge workgroup takes, at most
constexpr size_t kAlign = 256;           // workspace sections

struct LaneColumnPlan {
  int chunk, n_groups, grid;  // stream rows per task, groups of kGroupCols lane rows, workgroups
  int64_t n_tasks, nwords;    // (chunk, group) tasks, stream-major; bitmap words per stream row
};

struct SegmentPlan {
  int n_groups, seg, n_seg, grid;  // groups of kLaneRows lane items, stream rows per segment, segments, workgroups
  int64_t n_tasks, nwords;         // (group, segment) tasks, segment-major; bitmap words per stream row
};

// ---------------------------------------------------------------------------------------------------------------------
// ranking keys

// A key is a view of SoA lists in LDS with `better` (the total order) and `pad`, which writes an entry below every
// candidate: a real NaN pair has the same logit key but smaller ids.

// the full ranking key: logit descending, then drug ascending, then disease ascending
struct PairKey {
  uint32_t *f, *i, *j;
  static __device__ __forceinline__ bool better(uint32_t fa, uint32_t ia, uint32_t ja, uint32_t fb, uint32_t ib, uint32_t jb) {
    return fa > fb || (fa == fb && (ia < ib || (ia == ib && ja < jb)));
  }
  __device__ __forceinline__ void pad(int e) const { f[e] = 0u, i[e] = 0xffffffffu, j[e] = 0xffffffffu; }
};

// the per-row ranking key: logit descending, then candidate ascending
struct RowKey {
  uint32_t *f, *c;
  static __device__ __forceinline__ bool better(uint32_t fa, uint32_t ca, uint32_t fb, uint32_t cb) {
    return fa > fb || (fa == fb && ca < cb);
  }
  __device__ __forceinline__ void pad(int e) const { f[e] = 0u, c[e] = 0xffffffffu; }
};

// ---------------------------------------------------------------------------------------------------------------------
// lane columns: the append of the global top-k and of the emit kernel

// The lanes with q set append (f, i, j) to the SoA buffer (ef, ei, ej) of `cap` entries at their ballot rank: one LDS
// atomic on the fill *used per wave.
__device__ __forceinline__ void ballot_append(bool q, uint32_t f, uint32_t i, uint32_t j, int lane, int* used, uint32_t* ef,
                                              uint32_t* ei, uint32_t* ej, int cap) {
  const uint64_t m = __ballot(q);
  if (m != 0) {
    const int leader = __ffsll((unsigned long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(used, __popcll(m));
    base = __shfl(base, leader);
    if (q) {
      const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (pos < cap) {  // always: at most kSub * kGroupCols appends between two checks
        ef[pos] = f;
        ei[pos] = i;
        ej[pos] = j;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

inline size_t bitmap_bytes(int64_t n_stream, int64_t nwords) { return align_up((size_t)n_stream * (size_t)nwords * 4); }

inline LaneColumnPlan lane_column_plan(int64_t n_stream, int64_t n_lane) {
  LaneColumnPlan p;
  p.n_groups = (int)((n_lane + kGroupCols - 1) / kGroupCols);
  // enough tasks for ~4 per workgroup on small problems; 64-row chunks otherwise
  p.chunk = kMaxChunk;
  while (p.chunk > 2 && ((n_stream + p.chunk - 1) / p.chunk) * p.n_groups < 4 * kGrid) p.chunk >>= 1;
  p.n_tasks = ((n_stream + p.chunk - 1) / p.chunk) * p.n_groups;
  p.grid = (int)(p.n_tasks < kGrid ? p.n_tasks : kGrid);
  p.nwords = (n_lane + 31) / 32;
  return p;
}

// n_lane_items items on the lane columns (query rows, or listed pairs), each against all n_cand stream rows; the bitmap
// has a bit per (stream row, query row)
inline SegmentPlan segment_plan(int64_t n_lane_items, int64_t n_cand, int64_t n_query) {
  SegmentPlan p;
  p.n_groups = (int)((n_lane_items + kLaneRows - 1) / kLaneRows);
  // split the stream axis until there are ~16 tasks per workgroup: 50 000 query rows take 3 segments, 10 000 listed pairs
  // 14, a single lane item 256
  int64_t s = (kTaskTarget + p.n_groups - 1) / p.n_groups;
  if (s > kMaxSeg) s = kMaxSeg;
  if (s > (n_cand + kMinSeg - 1) / kMinSeg) s = (n_cand + kMinSeg - 1) / kMinSeg;
  if (s < 1) s = 1;
  p.seg = (int)((n_cand + s - 1) / s);
  p.n_seg = (int)((n_cand + p.seg - 1) / p.seg);
  p.n_tasks = (int64_t)p.n_groups * p.n_seg;
  p.grid = (int)(p.n_tasks < kGrid ? p.n_tasks : kGrid);
  p.nwords = (n_query + 31) / 32;
  return p;
}

// the largest fan-in whose lists of k entries one merge workgroup of merge_cap entries sorts
inline int merge_fan(int merge_cap, int k) {
  int kp = 1;
  while (kp < k) kp <<= 1;
  const int fan = merge_cap / kp;
  return fan > kMaxFan ? kMaxFan : fan;
}

// The checks every entry point makes of its extents ...
inline bool check_pair_extents(int32_t h1, int32_t h2, int64_t n_a, int64_t n_b, int64_t n_known) {
  return h1 == kH1 && h2 == kH2 && n_a >= 0 && n_b >= 0 && n_known >= 0 && n_a <= INT32_MAX && n_b <= INT32_MAX;
}

// ... of its known list ...
inline bool check_known(const int32_t* known_a, const int32_t* known_b, int64_t n_known) {
  return n_known == 0 || (known_a != nullptr && known_b != nullptr);
}

// ... and, for a problem that is not empty, of the two tables and the decoder.
inline bool check_pair_operands(const float* A, int64_t lda, const float* B, int64_t ldb, const float* W2, const float* b2,
                                const float* w3, const float* b3) {
  if (A == nullptr || B == nullptr || W2 == nullptr || b2 == nullptr || w3 == nullptr || b3 == nullptr) return false;
  return lda >= kH1 && ldb >= kH1 && lda % 4 == 0 && ldb % 4 == 0 && !misaligned(A) && !misaligned(B) && !misaligned(W2);
}

// Clear the n_stream x nwords bitmap and set the bit of every known pair (stream ks[e], lane kl[e]); an id out of
// range sets info[1].  bitmap == nullptr with n_stream = 0 only flags: every id is out of range, nothing is written.
inline hipError_t build_known_bitmap(const int32_t* ks, const int32_t* kl, int64_t n_known, int64_t n_stream, int64_t n_lane,
                                     int64_t nwords, uint32_t* bitmap, int32_t* info, hipStream_t s) {
  if (bitmap != nullptr) {
    const hipError_t err = hipMemsetAsync(bitmap, 0, (size_t)n_stream * (size_t)nwords * 4, s);
    if (err != hipSuccess) return err;
  }
  int64_t blocks = (n_known + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(known_bitmap_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ks, kl, n_known, (int)n_stream, (int)n_lane,
                     nwords, bitmap, info);
  return hipSuccess;
}

}  // namespace

#endif  // DGMI_PAIR_STREAM_H_

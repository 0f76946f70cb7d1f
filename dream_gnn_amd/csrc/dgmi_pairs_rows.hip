// dgmi_pairs_rows.hip — all-pairs MLP decoder with an on-chip top-k per query row (gfx950): novel candidates per
// disease (queries = diseases, candidates = drugs) or per drug (queries = drugs, candidates = diseases).
//
// Same scorer as dgmi_pairs.hip (dgmi_pair_score.h): the queries sit on the lane columns (X in VGPRs, 32 rows per
// wave), the candidates stream through LDS two at a time.  For per-disease lists that is the global kernel's own
// mapping; for per-drug lists Q rows stream where P rows do there.  relu(X + C) = relu(P + Q) bit for bit, and the MFMA
// operand layout, step order and epilogue order are the shared ones, so every logit equals the global kernel's.
//
// The ranking key, the task geometry (segment_plan, shared with the count scan of dgmi_pairs_given.hip) and the host
// prologue are those of dgmi_pair_stream.h; the candidate loop and the sort stay here (that header says why).
//
// Top-k.  A task is (32 query rows, a segment of the candidate axis); a persistent grid of one workgroup per CU takes
// them segment-major, so concurrent workgroups read the same candidate rows.  The four waves of a workgroup share the
// task's 32 rows and split each 128-candidate chunk (32 candidates each).  Every row owns a 256-entry LDS region: its
// best-k list, followed by an append buffer.  A lane appends its row's pair (LDS atomic on the row's fill) when it
// beats the row's threshold, the k-th key of the row's list, kept in the lane's registers.  Every 4 candidates per wave
// (at most 16 appends per row) the workgroup checks a flag; once a row is past 240 entries every row's region is
// bitonic-sorted on the full key, cut to k, and the thresholds are reloaded.  At the end of the task each row's sorted
// list goes to the workspace; a merge kernel reduces a row's segment lists, in rounds of up to 64 lists, to its result.
// Every comparison is on the full key (logit, candidate id), so the result does not depend on scheduling.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dgmi.h"
#include "dgmi_pair_stream.h"
#include "dgmi_rank.h"

namespace {

constexpr int kRows = kLaneRows;          // query rows per task (one per lane column)
constexpr int kPerWave = kChunk / 4;      // candidates of a chunk per wave
constexpr int kRowCap = 256;              // LDS list + append buffer per row, entries
constexpr int kTrigger = kRowCap - 4 * kSub;  // sort when a row holds more: at most 4 kSub appends per row per period
constexpr int kMergeThreads = 256;        // this file's own: a grid-stride over (row, output list), static LDS
constexpr int kMergeCap = 4096;           // entries one merge workgroup sorts (the global merge sorts 8192 in dynamic LDS)
constexpr int kMergeGrid = 8192;

static_assert(DGMI_ROW_TOPK_MAX_K <= kTrigger, "a row's list must fit below the sort trigger");

// Bitonic sort, descending, of `rows` lists of n (a power of two) entries each, list r at r * stride_r of the SoA
// arrays (f, c).  All threads of the block; ends with a barrier.
__device__ void rows_sort_desc(uint32_t* f, uint32_t* c, int rows, int stride_r, int n, int tid, int nthr) {
  const int half_n = n >> 1;
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < rows * half_n; t += nthr) {
        const int r = t / half_n, u = t - r * half_n;
        const int lo = 2 * u - (u & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const int a = r * stride_r + lo, b = r * stride_r + hi;
        const uint32_t fl = f[a], fh = f[b], cl = c[a], ch = c[b];
        if (RowKey::better(fh, ch, fl, cl) == desc) {
          f[a] = fh;
          f[b] = fl;
          c[a] = ch;
          c[b] = cl;
        }
      }
      __syncthreads();
    }
  }
}

struct RowArgs {
  const float* X;  // query side, on the lane columns
  int64_t ldx;
  const float* C;  // candidate side, streamed
  int64_t ldc;
  int n_query, n_cand;
  const float* W2;
  const float* b2;
  const float* w3;
  const float* b3;
  const uint32_t* bitmap;  // nullptr: nothing known; else word (c, q / 32) at c * nwords + q / 32
  int64_t nwords;
  int k, n_groups, n_seg, seg;
  int64_t n_tasks;
  uint32_t* part_f;  // [n_query][n_seg][k]
  uint32_t* part_c;
  int32_t* part_n;   // [n_query][n_seg]
};

__global__ __launch_bounds__(kThreads) void pair_mlp_row_topk_kernel(RowArgs a) {
  __shared__ __attribute__((aligned(16))) float c_lds[kChunk * kRowStride];
  __shared__ uint32_t ef[kRows * kRowCap], ec[kRows * kRowCap];
  __shared__ int s_used[kRows];
  __shared__ int s_need, s_max;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int k = a.k;
  uint32_t* const rf = ef + col * kRowCap;  // this lane's row region
  uint32_t* const rc = ec + col * kRowCap;

  PairDecoder dec;  // this lane's W2 operands and epilogue constants
  load_decoder(dec, a.W2, a.b2, a.w3, a.b3, half, col);

  bool full = false;  // the lane's row holds k entries: (tf, tc) is its k-th key
  uint32_t tf = 0u, tc = 0xffffffffu;

  // sort every row's list + buffer, keep the best k, reload the thresholds.  Called by the whole block after a barrier.
  auto select = [&]() {
    if (tid == 0) s_max = 0;
    __syncthreads();
    if (tid < kRows) atomicMax(&s_max, s_used[tid]);
    __syncthreads();
    const int m = s_max < kRowCap ? s_max : kRowCap;
    int np = 1;
    while (np < m) np <<= 1;
    for (int e = tid; e < kRows * np; e += kThreads) {
      const int r = e / np, p = e - r * np;
      if (p >= s_used[r]) RowKey{ef, ec}.pad(r * kRowCap + p);
    }
    __syncthreads();
    rows_sort_desc(ef, ec, kRows, kRowCap, np, tid, kThreads);
    const int n = s_used[col];
    full = n >= k;
    if (full) {
      tf = rf[k - 1];
      tc = rc[k - 1];
    }
    __syncthreads();  // everyone has read the fills and thresholds
    if (tid < kRows && s_used[tid] > k) s_used[tid] = k;
    if (tid == 0) s_need = 0;
    __syncthreads();
  };

  // offer the lane row's pair with candidate c; lanes 32..63 hold the same pairs and never append
  auto offer = [&](bool valid, float logit, uint32_t c) {
    const uint32_t f = order_key(logit);
    if (half == 0 && valid && (!full || RowKey::better(f, c, tf, tc))) {
      const int pos = atomicAdd(&s_used[col], 1);
      if (pos < kRowCap) {  // always: at most 4 kSub appends per row between two checks
        rf[pos] = f;
        rc[pos] = c;
      }
      if (pos >= kTrigger) s_need = 1;
    }
  };

  for (int64_t task = blockIdx.x; task < a.n_tasks; task += gridDim.x) {
    const int g = (int)(task % a.n_groups), sidx = (int)(task / a.n_groups);
    const int q0 = g * kRows;
    const int c_begin = sidx * a.seg;
    const int c_end = a.n_cand - c_begin < a.seg ? a.n_cand : c_begin + a.seg;
    const int qrow = q0 + col;
    const bool row_ok = qrow < a.n_query;
    float x[kH1 / 2];
    load_lane_row(x, a.X + (int64_t)(row_ok ? qrow : a.n_query - 1) * a.ldx, half);
    const bool words = a.bitmap != nullptr;
    const uint32_t* bm = a.bitmap + (words ? g : 0);
    full = false;
    tf = 0u;
    tc = 0xffffffffu;
    __syncthreads();  // the previous task's write-out has read the lists
    if (tid < kRows) s_used[tid] = 0;
    if (tid == 0) s_need = 0;

    for (int cc = c_begin; cc < c_end; cc += kChunk) {
      const int nc = c_end - cc < kChunk ? c_end - cc : kChunk;
      __syncthreads();  // the previous chunk's readers of c_lds are done
      for (int e = tid; e < nc * 32; e += kThreads) {
        const int r = e >> 5, c4 = e & 31;
        const float4 v = *reinterpret_cast<const float4*>(a.C + (int64_t)(cc + r) * a.ldc + 4 * c4);
        *reinterpret_cast<float4*>(c_lds + r * kRowStride + 68 * (c4 >> 4) + 4 * (c4 & 15)) = v;
      }
      __syncthreads();
      const int lo = wave * kPerWave;
      const int hi = nc < lo + kPerWave ? nc : lo + kPerWave;  // this wave's candidates [lo, hi) of the chunk
      const int per = nc < kPerWave ? nc : kPerWave;           // the busiest wave's: the same periods for all
      for (int p0 = 0; p0 < per; p0 += kSub) {
        const int d_end = lo + p0 + kSub < hi ? lo + p0 + kSub : hi;
        for (int da = lo + p0; da < d_end; da += 2) {
          const bool has_b = da + 1 < d_end;
          const int db = has_b ? da + 1 : da;
          const uint32_t kwa = words ? bm[(int64_t)(cc + da) * a.nwords] : 0u;
          const uint32_t kwb = words ? bm[(int64_t)(cc + db) * a.nwords] : 0u;
          float la, lb;
          score_two(c_lds + da * kRowStride + 68 * half, c_lds + db * kRowStride + 68 * half, x, dec, la, lb);
          offer(row_ok && !((kwa >> col) & 1u), la, (uint32_t)(cc + da));
          offer(has_b && row_ok && !((kwb >> col) & 1u), lb, (uint32_t)(cc + db));
        }
        __syncthreads();  // this period's appends are in
        const int need = s_need;
        __syncthreads();  // everyone has read the flag before anyone appends again
        if (need) select();
      }
    }

    __syncthreads();
    select();
    for (int e = tid; e < kRows * k; e += kThreads) {
      const int r = e / k, p = e - r * k;
      if (q0 + r < a.n_query && p < s_used[r]) {
        const int64_t o = ((int64_t)(q0 + r) * a.n_seg + sidx) * k + p;
        a.part_f[o] = ef[r * kRowCap + p];
        a.part_c[o] = ec[r * kRowCap + p];
      }
    }
    if (tid < kRows && q0 + tid < a.n_query) a.part_n[(int64_t)(q0 + tid) * a.n_seg + sidx] = s_used[tid];
  }
}

// One round of the reduction: work item w = (row q, output list b) merges the row's lists [b fan, (b + 1) fan) of
// `n_in` sorted lists into its best k.  The last round (n_out = 1) writes the row's result, its padding and its count.
__global__ __launch_bounds__(kMergeThreads) void row_merge_kernel(const uint32_t* __restrict__ in_f, const uint32_t* __restrict__ in_c,
                                                                 const int32_t* __restrict__ in_n, int64_t n_query, int n_in, int k,
                                                                 int fan, int n_out, uint32_t* __restrict__ out_f,
                                                                 uint32_t* __restrict__ out_c, int32_t* __restrict__ out_n,
                                                                 int32_t* __restrict__ res_cand, float* __restrict__ res_logit,
                                                                 int32_t* __restrict__ res_count, int32_t* __restrict__ info) {
  __shared__ uint32_t f[kMergeCap], c[kMergeCap];
  __shared__ int s_total;
  const int tid = threadIdx.x;
  const int64_t n_work = n_query * n_out;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t q = w / n_out;
    const int b = (int)(w - q * n_out);
    const int first = b * fan;
    const int nl = n_in - first < fan ? n_in - first : fan;
    const int64_t lists = q * n_in + first;
    int np = 1;
    while (np < nl * k) np <<= 1;
    __syncthreads();  // the previous item is written out
    if (tid == 0) {
      int t = 0;
      for (int l = 0; l < nl; ++l) t += in_n[lists + l];
      s_total = t;
    }
    for (int e = tid; e < np; e += kMergeThreads) {
      const int l = e / k, p = e - l * k;
      if (l < nl && p < in_n[lists + l]) {
        const int64_t src = (lists + l) * k + p;
        f[e] = in_f[src];
        c[e] = in_c[src];
      } else {
        RowKey{f, c}.pad(e);
      }
    }
    __syncthreads();
    rows_sort_desc(f, c, 1, 0, np, tid, kMergeThreads);
    const int keep = s_total < k ? s_total : k;
    if (res_cand != nullptr) {
      for (int e = tid; e < k; e += kMergeThreads) {
        res_cand[q * k + e] = e < keep ? (int32_t)c[e] : -1;
        res_logit[q * k + e] = e < keep ? key_logit(f[e]) : __uint_as_float(0x7fc00000u);
      }
      if (tid == 0) {
        res_count[q] = keep;
        atomicAdd(&info[0], keep);
      }
    } else {
      const int64_t o = (q * n_out + b) * k;
      for (int e = tid; e < keep; e += kMergeThreads) {
        out_f[o + e] = f[e];
        out_c[o + e] = c[e];
      }
      if (tid == 0) out_n[q * n_out + b] = keep;
    }
  }
}

// n_cand = 0: every row is empty
__global__ __launch_bounds__(256) void row_empty_kernel(int64_t n_query, int k, int32_t* __restrict__ res_cand,
                                                        float* __restrict__ res_logit, int32_t* __restrict__ res_count) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_query * k; e += (int64_t)gridDim.x * 256) {
    res_cand[e] = -1;
    res_logit[e] = __uint_as_float(0x7fc00000u);
    if (e % k == 0) res_count[e / k] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct RowPlan {
  SegmentPlan tasks;
  int fan;
  size_t bitmap, parts_a, parts_b, total;  // byte offsets / size
};

size_t parts_bytes(int64_t n_lists, int k) { return align_up((size_t)n_lists * (size_t)k * 8) + align_up((size_t)n_lists * 4); }

RowPlan make_row_plan(int64_t n_query, int64_t n_cand, int k) {
  RowPlan p;
  p.tasks = segment_plan(n_query, n_cand, n_query);
  p.fan = merge_fan(kMergeCap, k);
  p.bitmap = 0;
  p.parts_a = bitmap_bytes(n_cand, p.tasks.nwords);
  p.parts_b = p.parts_a + parts_bytes(n_query * p.tasks.n_seg, k);
  // a second list buffer only when a row's segment lists take more than one merge round
  p.total = p.parts_b + (p.tasks.n_seg > p.fan ? parts_bytes(n_query * ((p.tasks.n_seg + p.fan - 1) / p.fan), k) : 0);
  return p;
}

struct Parts {
  uint32_t *f, *c;
  int32_t* n;
};

Parts parts_at(void* ws, size_t off, int64_t n_lists, int k) {
  char* b = static_cast<char*>(ws) + off;
  const size_t m = (size_t)n_lists * (size_t)k;
  Parts l;
  l.f = reinterpret_cast<uint32_t*>(b);
  l.c = l.f + m;
  l.n = reinterpret_cast<int32_t*>(b + align_up(m * 8));
  return l;
}

}  // namespace

extern "C" {

DGMI_API size_t dgmi_row_topk_workspace_bytes(int64_t n_query, int64_t n_cand, int32_t k) {
  if (n_query <= 0 || n_cand <= 0 || n_query > INT32_MAX || n_cand > INT32_MAX || k < 1 || k > DGMI_ROW_TOPK_MAX_K) return 0;
  return make_row_plan(n_query, n_cand, k).total;
}

DGMI_API int dgmi_pair_mlp_row_topk_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                        int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                        const float* w3, const float* b3, const int32_t* known_query,
                                        const int32_t* known_cand, int64_t n_known, int32_t k, int32_t* out_cand,
                                        float* out_logit, int32_t* out_count, int32_t* out_info, void* workspace,
                                        size_t workspace_bytes, dgmi_stream_t stream) {
  if (!check_pair_extents(h1, h2, n_query, n_cand, n_known) || k < 1 || k > DGMI_ROW_TOPK_MAX_K) return DGMI_ERR_INVALID_ARG;
  if (n_query == 0) return DGMI_OK;
  if (out_cand == nullptr || out_logit == nullptr || out_count == nullptr || out_info == nullptr) return DGMI_ERR_INVALID_ARG;
  if (!check_known(known_query, known_cand, n_known)) return DGMI_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_cand == 0) {  // every row is empty, whatever the operands
    if (hipMemsetAsync(out_info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
    int64_t blocks = (n_query * k + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(row_empty_kernel, dim3((unsigned)blocks), dim3(256), 0, s, n_query, (int)k, out_cand, out_logit,
                       out_count);
    // every known id is out of range: flag it
    if (n_known > 0 && build_known_bitmap(known_cand, known_query, n_known, 0, n_query, 0, nullptr, out_info, s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
    return hipGetLastError() == hipSuccess ? DGMI_OK : DGMI_ERR_LAUNCH;
  }
  if (!check_pair_operands(X, ldx, C, ldc, W2, b2, w3, b3)) return DGMI_ERR_INVALID_ARG;
  const RowPlan plan = make_row_plan(n_query, n_cand, k);
  const SegmentPlan& tasks = plan.tasks;
  if (workspace == nullptr || workspace_bytes < plan.total) return DGMI_ERR_WORKSPACE;

  if (hipMemsetAsync(out_info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  uint32_t* bitmap = nullptr;
  if (n_known > 0) {
    bitmap = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + plan.bitmap);
    if (build_known_bitmap(known_cand, known_query, n_known, n_cand, n_query, tasks.nwords, bitmap, out_info, s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
  }

  const Parts pa = parts_at(workspace, plan.parts_a, n_query * tasks.n_seg, k);
  RowArgs args{X, ldx, C, ldc, (int)n_query, (int)n_cand, W2, b2, w3, b3, bitmap, tasks.nwords, k, tasks.n_groups,
               tasks.n_seg, tasks.seg, tasks.n_tasks, pa.f, pa.c, pa.n};
  hipLaunchKernelGGL(pair_mlp_row_topk_kernel, dim3((unsigned)tasks.grid), dim3(kThreads), 0, s, args);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;

  // rounds: lists A -> B -> A ... until each row's lists are one, written as the result
  const int64_t n_b = (tasks.n_seg + plan.fan - 1) / plan.fan;
  const Parts pb = plan.tasks.n_seg > plan.fan ? parts_at(workspace, plan.parts_b, n_query * n_b, k)
                                          : Parts{nullptr, nullptr, nullptr};
  int n_in = tasks.n_seg;
  bool in_a = true;
  for (;;) {
    const int n_out = (n_in + plan.fan - 1) / plan.fan;
    const bool last = n_out == 1;
    const Parts src = in_a ? pa : pb, dst = in_a ? pb : pa;
    int64_t grid = n_query * n_out;
    if (grid > kMergeGrid) grid = kMergeGrid;
    hipLaunchKernelGGL(row_merge_kernel, dim3((unsigned)grid), dim3(kMergeThreads), 0, s, src.f, src.c, src.n, n_query, n_in,
                       (int)k, plan.fan, n_out, dst.f, dst.c, dst.n, last ? out_cand : nullptr, out_logit, out_count,
                       out_info);
    if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
    if (last) break;
    n_in = n_out;
    in_a = !in_a;
  }
  return DGMI_OK;
}

}  // extern "C"

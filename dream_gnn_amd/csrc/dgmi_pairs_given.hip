// dgmi_pairs_given.hip — the decoder MLP on GIVEN (query, candidate) pairs (gfx950): the logit of every listed pair, and
// the pair's filtered position among all candidates of its query row.
//
// Same scorer as dgmi_pairs.hip / dgmi_pairs_rows.hip (dgmi_pair_score.h): the listed pairs sit on the lane columns
// (X[q_e] in VGPRs, 32 pairs per wave), the MFMA operand layout, step order and epilogue order are the shared ones, so
// every logit equals the ranking kernels' for the same pair, bit for bit.
//
// List scorer.  A wave takes 32 listed pairs; column j holds X[q_e] in registers and reads C[c_e] from its own LDS row
// (the wave stages its 32 candidate rows with coalesced loads).  One score per listed pair.
//
// Count scan.  A task is (32 listed pairs, a segment of the candidate axis); a persistent grid of one workgroup per CU
// takes them segment-major, as the per-row top-k does.  The four waves of a workgroup share the task's 32 pairs and split
// each chunk of up to 128 candidates evenly.  A lane keeps the key (order_key(logit_e), c_e) of its own pair, read from
// the list scorer's output, and two integer counters: `total` counts the streamed candidates c' != c_e with (q_e, c')
// not known, `above` those of them whose key is better (logit descending, ties by candidate id ascending, NaN last,
// -0 == +0).  Nothing is listed, sorted or merged.  A wave adds its partial counts to the pair's result with vector
// atomics; the sums are integers, so the result does not depend on scheduling.  n_pairs x n_cand scores.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dgmi.h"
#include "dgmi_given.h"
#include "dgmi_pair_stream.h"

namespace {

constexpr int kCols = kLaneRows;          // listed pairs per wave (one per lane column)
constexpr int kListBlock = 4 * kCols;     // listed pairs per workgroup of the list scorer

struct GivenArgs {
  const float* X;  // query side, on the lane columns
  int64_t ldx;
  const float* C;  // candidate side
  int64_t ldc;
  int n_query, n_cand;
  const float* W2;
  const float* b2;
  const float* w3;
  const float* b3;
  const int32_t* pair_query;
  const int32_t* pair_cand;
  int n_pairs;
  float* out_logit;
  int32_t* out_above;  // list scorer: nullptr when only logits are wanted, else initialised to 0 (-1: pair out of range)
  int32_t* out_total;
  int32_t* info;
  const uint32_t* bitmap;  // scan: nullptr: nothing known; else word (c, q / 32) at c * nwords + q / 32
  int64_t nwords;
  int n_groups, seg;
  int64_t n_tasks;
};

__global__ __launch_bounds__(kThreads) void pair_mlp_score_list_kernel(GivenArgs a) {
  __shared__ __attribute__((aligned(16))) float c_lds[kListBlock * kRowStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  float* const rows = c_lds + wave * kCols * kRowStride;  // this wave's 32 candidate rows

  PairDecoder dec;
  load_decoder(dec, a.W2, a.b2, a.w3, a.b3, half, col);

  const int n_blocks = (a.n_pairs + kListBlock - 1) / kListBlock;
  for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int e = b * kListBlock + wave * kCols + col;
    const bool listed = e < a.n_pairs;
    const int32_t q = listed ? a.pair_query[e] : 0, c = listed ? a.pair_cand[e] : 0;
    const bool ok = listed && q >= 0 && q < a.n_query && c >= 0 && c < a.n_cand;
    const int qr = ok ? q : 0, cr = ok ? c : 0;  // an id out of range reads row 0 and its score is dropped
    float x[kH1 / 2];
    load_lane_row(x, a.X + (int64_t)qr * a.ldx, half);
    __syncthreads();  // the previous block's readers of c_lds are done
    for (int it = 0; it < kCols * 32 / 64; ++it) {
      const int idx = it * 64 + lane, r = idx >> 5, c4 = idx & 31;
      const int src = __shfl(cr, r);  // the candidate row of column r
      const float4 v = *reinterpret_cast<const float4*>(a.C + (int64_t)src * a.ldc + 4 * c4);
      *reinterpret_cast<float4*>(rows + r * kRowStride + 68 * (c4 >> 4) + 4 * (c4 & 15)) = v;
    }
    __syncthreads();
    float logit;
    score_one(rows + col * kRowStride + 68 * half, x, dec, logit);
    if (half == 0 && listed) {
      a.out_logit[e] = ok ? logit : __uint_as_float(0x7fc00000u);
      if (a.out_above != nullptr) {
        a.out_above[e] = ok ? 0 : -1;
        a.out_total[e] = ok ? 0 : -1;
      }
      if (!ok) atomicOr(&a.info[0], 1);
    }
  }
}

__global__ __launch_bounds__(kThreads) void pair_count_scan_kernel(GivenArgs a) {
  __shared__ __attribute__((aligned(16))) float c_lds[kChunk * kRowStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;

  PairDecoder dec;
  load_decoder(dec, a.W2, a.b2, a.w3, a.b3, half, col);
  const bool words = a.bitmap != nullptr;

  for (int64_t task = blockIdx.x; task < a.n_tasks; task += gridDim.x) {
    const int g = (int)(task % a.n_groups), sidx = (int)(task / a.n_groups);
    const int c_begin = sidx * a.seg;
    const int c_end = a.n_cand - c_begin < a.seg ? a.n_cand : c_begin + a.seg;
    const int e = g * kCols + col;
    const bool listed = e < a.n_pairs;
    const int32_t q = listed ? a.pair_query[e] : 0, c = listed ? a.pair_cand[e] : 0;
    const bool ok = listed && q >= 0 && q < a.n_query && c >= 0 && c < a.n_cand;
    const int qr = ok ? q : 0;
    float x[kH1 / 2];
    load_lane_row(x, a.X + (int64_t)qr * a.ldx, half);
    const uint32_t ef = order_key(ok ? a.out_logit[e] : 0.f), ec = (uint32_t)c;  // the lane's own pair
    const uint32_t* bm = a.bitmap + (words ? (qr >> 5) : 0);
    const int qbit = qr & 31;
    int above = 0, total = 0;

    auto count = [&](bool valid, uint32_t known_word, float logit, uint32_t cand) {
      if (valid && cand != ec && !((known_word >> qbit) & 1u)) {
        ++total;
        if (RowKey::better(order_key(logit), cand, ef, ec)) ++above;
      }
    };

    for (int cc = c_begin; cc < c_end; cc += kChunk) {
      const int nc = c_end - cc < kChunk ? c_end - cc : kChunk;
      __syncthreads();  // the previous chunk's readers of c_lds are done
      for (int i = tid; i < nc * 32; i += kThreads) {
        const int r = i >> 5, c4 = i & 31;
        const float4 v = *reinterpret_cast<const float4*>(a.C + (int64_t)(cc + r) * a.ldc + 4 * c4);
        *reinterpret_cast<float4*>(c_lds + r * kRowStride + 68 * (c4 >> 4) + 4 * (c4 & 15)) = v;
      }
      __syncthreads();
      const int per = (nc + 7) / 8 * 2;  // an even share of the chunk per wave: a short segment still uses all four
      const int lo = wave * per;
      const int hi = nc < lo + per ? nc : lo + per;  // this wave's candidates [lo, hi) of the chunk
      for (int da = lo; da < hi; da += 2) {
        const bool has_b = da + 1 < hi;
        const int db = has_b ? da + 1 : da;
        const uint32_t kwa = words ? bm[(int64_t)(cc + da) * a.nwords] : 0u;
        const uint32_t kwb = words ? bm[(int64_t)(cc + db) * a.nwords] : 0u;
        float la, lb;
        score_two(c_lds + da * kRowStride + 68 * half, c_lds + db * kRowStride + 68 * half, x, dec, la, lb);
        count(ok, kwa, la, (uint32_t)(cc + da));
        count(ok && has_b, kwb, lb, (uint32_t)(cc + db));
      }
    }
    // lanes 32..63 hold the same pairs and counts; integer sums: the order of the adds does not matter
    if (half == 0 && ok) {
      if (above != 0) atomicAdd(&a.out_above[e], above);
      if (total != 0) atomicAdd(&a.out_total[e], total);
    }
  }
}

// no query rows or no candidate rows: every listed pair is out of range
__global__ __launch_bounds__(256) void given_empty_kernel(int64_t n_pairs, float* __restrict__ out_logit,
                                                          int32_t* __restrict__ out_above, int32_t* __restrict__ out_total,
                                                          int32_t* __restrict__ info) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_pairs; e += (int64_t)gridDim.x * 256) {
    out_logit[e] = __uint_as_float(0x7fc00000u);
    if (out_above != nullptr) {
      out_above[e] = -1;
      out_total[e] = -1;
    }
    if (e == 0) atomicOr(&info[0], 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

// Both entry points: out_above == nullptr scores the list only.
int given_launch(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc, int64_t n_cand, int32_t h1,
                 int32_t h2, const float* W2, const float* b2, const float* w3, const float* b3, const int32_t* pair_query,
                 const int32_t* pair_cand, int64_t n_pairs, const int32_t* known_query, const int32_t* known_cand,
                 int64_t n_known, bool rank, float* out_logit, int32_t* out_above, int32_t* out_total, int32_t* out_info,
                 void* workspace, size_t workspace_bytes, dgmi_stream_t stream) {
  if (!check_pair_extents(h1, h2, n_query, n_cand, n_known) || n_pairs < 0 || n_pairs > INT32_MAX) return DGMI_ERR_INVALID_ARG;
  if (n_pairs == 0) return DGMI_OK;
  if (pair_query == nullptr || pair_cand == nullptr || out_logit == nullptr || out_info == nullptr) return DGMI_ERR_INVALID_ARG;
  if (rank && (out_above == nullptr || out_total == nullptr)) return DGMI_ERR_INVALID_ARG;
  if (!check_known(known_query, known_cand, n_known)) return DGMI_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_query == 0 || n_cand == 0) {  // every listed pair is out of range, whatever the operands
    if (hipMemsetAsync(out_info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
    int64_t blocks = (n_pairs + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(given_empty_kernel, dim3((unsigned)blocks), dim3(256), 0, s, n_pairs, out_logit, out_above, out_total,
                       out_info);
    // every known id is out of range: flag it
    if (n_known > 0 && build_known_bitmap(known_cand, known_query, n_known, 0, 0, 0, nullptr, out_info, s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
    return hipGetLastError() == hipSuccess ? DGMI_OK : DGMI_ERR_LAUNCH;
  }
  if (!check_pair_operands(X, ldx, C, ldc, W2, b2, w3, b3)) return DGMI_ERR_INVALID_ARG;
  const SegmentPlan plan = segment_plan(n_pairs, n_cand, n_query);
  if (rank && (workspace == nullptr || workspace_bytes < bitmap_bytes(n_cand, plan.nwords))) return DGMI_ERR_WORKSPACE;

  if (hipMemsetAsync(out_info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  GivenArgs args{X, ldx, C, ldc, (int)n_query, (int)n_cand, W2, b2, w3, b3, pair_query, pair_cand, (int)n_pairs, out_logit,
                 out_above, out_total, out_info, nullptr, plan.nwords, plan.n_groups, plan.seg, plan.n_tasks};
  // the list scorer also sets the counters to 0 (-1 for a pair out of range) before the scan accumulates into them
  int64_t lgrid = (n_pairs + kListBlock - 1) / kListBlock;
  if (lgrid > 4 * kGrid) lgrid = 4 * kGrid;
  hipLaunchKernelGGL(pair_mlp_score_list_kernel, dim3((unsigned)lgrid), dim3(kThreads), 0, s, args);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
  if (!rank) return DGMI_OK;

  if (n_known > 0) {
    uint32_t* bitmap = static_cast<uint32_t*>(workspace);
    if (build_known_bitmap(known_cand, known_query, n_known, n_cand, n_query, plan.nwords, bitmap, out_info, s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
    args.bitmap = bitmap;
  }
  hipLaunchKernelGGL(pair_count_scan_kernel, dim3((unsigned)plan.grid), dim3(kThreads), 0, s, args);
  return hipGetLastError() == hipSuccess ? DGMI_OK : DGMI_ERR_LAUNCH;
}

}  // namespace

extern "C" {

DGMI_API size_t dgmi_pair_rank_workspace_bytes(int64_t n_query, int64_t n_cand, int64_t n_pairs) {
  if (n_query <= 0 || n_cand <= 0 || n_pairs <= 0 || n_query > INT32_MAX || n_cand > INT32_MAX || n_pairs > INT32_MAX) return 0;
  return bitmap_bytes(n_cand, segment_plan(n_pairs, n_cand, n_query).nwords);  // the known-pair bitmap, nothing else
}

DGMI_API int dgmi_pair_mlp_score_list_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                          int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                          const float* w3, const float* b3, const int32_t* pair_query,
                                          const int32_t* pair_cand, int64_t n_pairs, float* out_logit, int32_t* out_info,
                                          dgmi_stream_t stream) {
  return given_launch(X, ldx, n_query, C, ldc, n_cand, h1, h2, W2, b2, w3, b3, pair_query, pair_cand, n_pairs, nullptr, nullptr,
                      0, false, out_logit, nullptr, nullptr, out_info, nullptr, 0, stream);
}

DGMI_API int dgmi_pair_mlp_rank_list_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                         int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                         const float* w3, const float* b3, const int32_t* pair_query,
                                         const int32_t* pair_cand, int64_t n_pairs, const int32_t* known_query,
                                         const int32_t* known_cand, int64_t n_known, float* out_logit, int32_t* out_above,
                                         int32_t* out_total, int32_t* out_info, void* workspace, size_t workspace_bytes,
                                         dgmi_stream_t stream) {
  return given_launch(X, ldx, n_query, C, ldc, n_cand, h1, h2, W2, b2, w3, b3, pair_query, pair_cand, n_pairs, known_query,
                      known_cand, n_known, true, out_logit, out_above, out_total, out_info, workspace, workspace_bytes, stream);
}

}  // extern "C"

// dgmi_pairs.hip — all-pairs MLP decoder with an on-chip top-k (gfx950): the model's novel-pair ranking.
//
// Replaces the scoring loop of the reference's get_top_novel_predictions (train.py:26-151): every drug-disease pair
// (i, j) that is not a known association gets
//     logit(i, j) = b3 + sum_h w3[h] relu(b2[h] + sum_k W2[h, k] relu(P[i, k] + Q[j, k])),   h < 64, k < 128,
// where P = hd W1a^T + b1 and Q = hs W1b^T are the split first decoder layer (model.MLPDecoder.fuse_lin1), and the k
// best (logit desc, then (i, j) asc) are returned.  The n_drug x n_dis x 128 hidden layer is never written.
//
// Scorer.  A wave owns 32 diseases (one per lane column) and walks drugs two at a time.  For drug i the 64 x 32 block
// W2 . relu(P[i] + Q[j0:j0+32]) is 2 x 64 `v_mfma_f32_32x32x2_f32` (f32 in, f32 accumulate: exact f32 arithmetic):
// A = W2 rows (lane l: row l & 31 of the half, k = 64 (l >> 5) + s at step s), B = relu(P[i, k] + Q[j, k]) with the
// same k and the pair on the lane column.  The lane's 64 Q values and 128 W2 values stay in VGPRs for the whole kernel
// (Q: per task), P rows come from LDS as a two-address broadcast.  Two drugs x two row halves = 4 independent
// accumulators per wave, the condition for the 64-cycle f32 MFMA to issue back to back from one wave per SIMD.
// After the 64 steps each lane sums w3[h] relu(acc + b2[h]) over its 32 rows and adds its partner lane (l ^ 32).
// The scorer lives in dgmi_pair_score.h, shared by every pair kernel: same logits, same bits.  The ranking key, the
// ballot append, the task geometry and the host prologue are those of dgmi_pair_stream.h, shared with the emit kernel
// of dgmi_pairs_above.hip; the task loop and the sort stay here (that header says why).
//
// Top-k.  A persistent grid of one workgroup per CU takes (drug chunk, 128-disease group) tasks in drug-major order,
// so all workgroups read the same P rows at the same time.  Each keeps, in LDS, its best-k list followed by an append
// buffer: a lane whose pair beats the workgroup's threshold (the k-th key of its list) appends it at its ballot rank.
// Every 4 drugs the workgroup checks the fill; past 3/4 it sorts list + buffer (bitonic, on the full key) and raises
// the threshold.  A merge kernel reduces the workgroups' sorted lists in rounds of up to 64 lists to the result.
// Every comparison is on the full key (logit, i, j), so the result does not depend on scheduling.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dgmi.h"
#include "dgmi_pair_stream.h"
#include "dgmi_pairs.h"

namespace {

constexpr int kSortCap = 2048;           // LDS list + append buffer, entries
constexpr int kMergeThreads = 1024;      // this file's own: one list of up to kMergeCap entries per workgroup, dynamic LDS
constexpr int kMergeCap = 8192;          // entries one merge workgroup sorts (the per-row merge sorts 4096 in static LDS)

// Bitonic sort of n (a power of two) entries of the SoA list (f, i, j) into descending key order, all threads of the
// block.  Ends with a barrier.
__device__ void block_sort_desc(uint32_t* f, uint32_t* ii, uint32_t* jj, int n, int tid, int nthr) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (n >> 1); t += nthr) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const uint32_t fl = f[lo], fh = f[hi], il = ii[lo], ih = ii[hi], jl = jj[lo], jh = jj[hi];
        if (PairKey::better(fh, ih, jh, fl, il, jl) == desc) {
          f[lo] = fh;
          f[hi] = fl;
          ii[lo] = ih;
          ii[hi] = il;
          jj[lo] = jh;
          jj[hi] = jl;
        }
      }
      __syncthreads();
    }
  }
}

struct ScoreArgs {
  const float* P;
  int64_t ldp;
  const float* Q;
  int64_t ldq;
  int n_drug, n_dis;
  const float* W2;
  const float* b2;
  const float* w3;
  const float* b3;
  const uint32_t* bitmap;  // nullptr: nothing known
  int64_t nwords;
  int k, chunk, n_groups;
  int64_t n_tasks;
  uint32_t* list_f;  // [gridDim.x][k]
  uint32_t* list_i;
  uint32_t* list_j;
  int32_t* list_n;   // [gridDim.x]
};

__global__ __launch_bounds__(kThreads) void pair_mlp_topk_kernel(ScoreArgs a) {
  __shared__ __attribute__((aligned(16))) float p_lds[kMaxChunk * kRowStride];
  __shared__ uint32_t ef[kSortCap], ei[kSortCap], ej[kSortCap];
  __shared__ int s_used;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int k = a.k;

  PairDecoder dec;  // this lane's W2 operands and epilogue constants
  load_decoder(dec, a.W2, a.b2, a.w3, a.b3, half, col);

  if (tid == 0) s_used = 0;
  bool full = false;  // the list holds k entries: (tf, ti, tj) is its k-th key
  uint32_t tf = 0u, ti = 0xffffffffu, tj = 0xffffffffu;

  // sort list + buffer, keep the best k, raise the threshold.  Called by the whole block after a barrier.
  auto select = [&]() {
    const int n = s_used;
    int np = 1;
    while (np < n) np <<= 1;
    for (int e = n + tid; e < np; e += kThreads) PairKey{ef, ei, ej}.pad(e);
    __syncthreads();
    block_sort_desc(ef, ei, ej, np, tid, kThreads);
    const int keep = n < k ? n : k;
    full = keep == k;
    if (full) {
      tf = ef[k - 1];
      ti = ei[k - 1];
      tj = ej[k - 1];
    }
    __syncthreads();  // everyone has read s_used and the threshold
    if (tid == 0) s_used = keep;
    __syncthreads();
  };

  // offer lane `col`'s pair (i, j) of one drug; lanes 32..63 hold the same pairs and never append
  auto offer = [&](bool valid, float logit, uint32_t i, uint32_t j) {
    const uint32_t f = order_key(logit);
    const bool q = half == 0 && valid && (!full || PairKey::better(f, i, j, tf, ti, tj));
    ballot_append(q, f, i, j, lane, &s_used, ef, ei, ej, kSortCap);
  };

  for (int64_t task = blockIdx.x; task < a.n_tasks; task += gridDim.x) {
    const int g = (int)(task % a.n_groups);
    const int i0 = (int)(task / a.n_groups) * a.chunk;
    const int nd = a.n_drug - i0 < a.chunk ? a.n_drug - i0 : a.chunk;
    __syncthreads();  // the previous task's readers of p_lds are done
    for (int e = tid; e < a.chunk * 32; e += kThreads) {
      const int r = e >> 5, c4 = e & 31;
      const int row = r < nd ? i0 + r : a.n_drug - 1;
      const float4 v = *reinterpret_cast<const float4*>(a.P + (int64_t)row * a.ldp + 4 * c4);
      *reinterpret_cast<float4*>(p_lds + r * kRowStride + 68 * (c4 >> 4) + 4 * (c4 & 15)) = v;
    }
    const int j0 = g * kGroupCols + wave * 32;  // this wave's 32 diseases
    const int j = j0 + col;
    const bool col_ok = j < a.n_dis;
    const int jc = col_ok ? j : a.n_dis - 1;
    float q[kH1 / 2];
    load_lane_row(q, a.Q + (int64_t)jc * a.ldq, half);
    const bool words = a.bitmap != nullptr && j0 < a.n_dis;
    const uint32_t* bm = a.bitmap + (words ? (j0 >> 5) : 0);
    __syncthreads();

    for (int d0 = 0; d0 < nd; d0 += kSub) {
      const int d_end = d0 + kSub < nd ? d0 + kSub : nd;
      for (int da = d0; da < d_end; da += 2) {
        const bool has_b = da + 1 < d_end;
        const int db = has_b ? da + 1 : da;
        const uint32_t kwa = words ? bm[(int64_t)(i0 + da) * a.nwords] : 0u;
        const uint32_t kwb = words ? bm[(int64_t)(i0 + db) * a.nwords] : 0u;
        const float* pa = p_lds + da * kRowStride + 68 * half;
        const float* pb = p_lds + db * kRowStride + 68 * half;
        float la, lb;
        score_two(pa, pb, q, dec, la, lb);
        offer(col_ok && !((kwa >> col) & 1u), la, (uint32_t)(i0 + da), (uint32_t)j);
        offer(has_b && col_ok && !((kwb >> col) & 1u), lb, (uint32_t)(i0 + db), (uint32_t)j);
      }
      __syncthreads();  // this period's appends are in
      const int n = s_used;
      __syncthreads();  // everyone has read the fill before anyone appends again
      if (n > kSortCap - kSub * kGroupCols) select();
    }
  }

  __syncthreads();
  select();
  const int keep = s_used;
  uint32_t* of = a.list_f + (int64_t)blockIdx.x * k;
  uint32_t* oi = a.list_i + (int64_t)blockIdx.x * k;
  uint32_t* oj = a.list_j + (int64_t)blockIdx.x * k;
  for (int e = tid; e < keep; e += kThreads) {
    of[e] = ef[e];
    oi[e] = ei[e];
    oj[e] = ej[e];
  }
  if (tid == 0) a.list_n[blockIdx.x] = keep;
}

// One round of the final reduction: workgroup b merges lists [b fan, (b + 1) fan) of `n_lists` sorted lists into the
// best k.  The last round (one workgroup) writes the result and its count.
__global__ __launch_bounds__(kMergeThreads) void pair_merge_kernel(const uint32_t* __restrict__ in_f, const uint32_t* __restrict__ in_i,
                                                                  const uint32_t* __restrict__ in_j, const int32_t* __restrict__ in_n,
                                                                  int n_lists, int k, int fan, uint32_t* __restrict__ out_f,
                                                                  uint32_t* __restrict__ out_i, uint32_t* __restrict__ out_j,
                                                                  int32_t* __restrict__ out_n, int32_t* __restrict__ out_drug,
                                                                  int32_t* __restrict__ out_dis, float* __restrict__ out_logit,
                                                                  int32_t* __restrict__ out_info) {
  extern __shared__ uint32_t merge_lds[];
  __shared__ int s_total;
  const int tid = threadIdx.x;
  const int first = (int)blockIdx.x * fan;
  const int nl = n_lists - first < fan ? n_lists - first : fan;
  int np = 1;
  while (np < nl * k) np <<= 1;
  uint32_t* f = merge_lds;
  uint32_t* ii = merge_lds + np;
  uint32_t* jj = merge_lds + 2 * np;
  if (tid == 0) {
    int t = 0;
    for (int l = 0; l < nl; ++l) t += in_n[first + l];
    s_total = t;
  }
  for (int e = tid; e < np; e += kMergeThreads) {
    const int l = e / k, p = e - l * k;
    if (l < nl && p < in_n[first + l]) {
      const int64_t src = (int64_t)(first + l) * k + p;
      f[e] = in_f[src];
      ii[e] = in_i[src];
      jj[e] = in_j[src];
    } else {
      PairKey{f, ii, jj}.pad(e);
    }
  }
  __syncthreads();
  block_sort_desc(f, ii, jj, np, tid, kMergeThreads);
  const int keep = s_total < k ? s_total : k;
  if (out_drug != nullptr) {
    for (int e = tid; e < keep; e += kMergeThreads) {
      out_drug[e] = (int32_t)ii[e];
      out_dis[e] = (int32_t)jj[e];
      out_logit[e] = key_logit(f[e]);
    }
    if (tid == 0) out_info[0] = keep;
  } else {
    const int64_t o = (int64_t)blockIdx.x * k;
    for (int e = tid; e < keep; e += kMergeThreads) {
      out_f[o + e] = f[e];
      out_i[o + e] = ii[e];
      out_j[o + e] = jj[e];
    }
    if (tid == 0) out_n[blockIdx.x] = keep;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct Plan {
  LaneColumnPlan tasks;
  int fan;
  size_t bitmap, lists_a, lists_b, total;  // byte offsets / size
};

size_t lists_bytes(int64_t n_lists, int k) { return align_up((size_t)n_lists * (size_t)k * 12) + align_up((size_t)n_lists * 4); }

Plan make_plan(int64_t n_drug, int64_t n_dis, int k) {
  Plan p;
  p.tasks = lane_column_plan(n_drug, n_dis);
  p.fan = merge_fan(kMergeCap, k);
  if (p.fan < 2) p.fan = 2;
  p.bitmap = 0;
  p.lists_a = bitmap_bytes(n_drug, p.tasks.nwords);
  p.lists_b = p.lists_a + lists_bytes(p.tasks.grid, k);
  p.total = p.lists_b + lists_bytes((p.tasks.grid + p.fan - 1) / p.fan, k);
  return p;
}

struct Lists {
  uint32_t *f, *i, *j;
  int32_t* n;
};

Lists lists_at(void* ws, size_t off, int64_t n_lists, int k) {
  char* b = static_cast<char*>(ws) + off;
  const size_t m = (size_t)n_lists * (size_t)k;
  Lists l;
  l.f = reinterpret_cast<uint32_t*>(b);
  l.i = l.f + m;
  l.j = l.i + m;
  l.n = reinterpret_cast<int32_t*>(b + align_up(m * 12));
  return l;
}

}  // namespace

extern "C" {

DGMI_API size_t dgmi_pair_topk_workspace_bytes(int64_t n_drug, int64_t n_dis, int32_t k) {
  if (n_drug <= 0 || n_dis <= 0 || n_drug > INT32_MAX || n_dis > INT32_MAX || k < 1 || k > DGMI_PAIR_TOPK_MAX_K) return 0;
  return make_plan(n_drug, n_dis, k).total;
}

DGMI_API int dgmi_pair_mlp_topk_f32(const float* P, int64_t ldp, int64_t n_drug, const float* Q, int64_t ldq, int64_t n_dis,
                                    int32_t h1, int32_t h2, const float* W2, const float* b2, const float* w3, const float* b3,
                                    const int32_t* known_drug, const int32_t* known_dis, int64_t n_known, int32_t k,
                                    int32_t* out_drug, int32_t* out_dis, float* out_logit, int32_t* out_info, void* workspace,
                                    size_t workspace_bytes, dgmi_stream_t stream) {
  if (!check_pair_extents(h1, h2, n_drug, n_dis, n_known) || k < 1 || k > DGMI_PAIR_TOPK_MAX_K) return DGMI_ERR_INVALID_ARG;
  if (n_drug == 0 || n_dis == 0) return DGMI_OK;
  if (out_drug == nullptr || out_dis == nullptr || out_logit == nullptr || out_info == nullptr) return DGMI_ERR_INVALID_ARG;
  if (!check_known(known_drug, known_dis, n_known) || !check_pair_operands(P, ldp, Q, ldq, W2, b2, w3, b3))
    return DGMI_ERR_INVALID_ARG;
  const Plan plan = make_plan(n_drug, n_dis, k);
  if (workspace == nullptr || workspace_bytes < plan.total) return DGMI_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);

  if (hipMemsetAsync(out_info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  uint32_t* bitmap = nullptr;
  if (n_known > 0) {
    bitmap = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + plan.bitmap);
    if (build_known_bitmap(known_drug, known_dis, n_known, n_drug, n_dis, plan.tasks.nwords, bitmap, out_info, s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
  }

  Lists la = lists_at(workspace, plan.lists_a, plan.tasks.grid, k);
  ScoreArgs args{P, ldp, Q, ldq, (int)n_drug, (int)n_dis, W2, b2, w3, b3, bitmap, plan.tasks.nwords, k, plan.tasks.chunk,
                 plan.tasks.n_groups, plan.tasks.n_tasks, la.f, la.i, la.j, la.n};
  hipLaunchKernelGGL(pair_mlp_topk_kernel, dim3((unsigned)plan.tasks.grid), dim3(kThreads), 0, s, args);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;

  const size_t lds = (size_t)kMergeCap * 12;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(pair_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return DGMI_ERR_LAUNCH;
  // rounds: lists A -> B -> A ... until one workgroup merges what is left into the result
  int n_lists = plan.tasks.grid;
  bool in_a = true;
  for (;;) {
    const int out_lists = (n_lists + plan.fan - 1) / plan.fan;
    const Lists src = in_a ? la : lists_at(workspace, plan.lists_b, (plan.tasks.grid + plan.fan - 1) / plan.fan, k);
    const Lists dst = in_a ? lists_at(workspace, plan.lists_b, (plan.tasks.grid + plan.fan - 1) / plan.fan, k) : la;
    const bool last = out_lists == 1;
    int kp = 1;
    while (kp < (n_lists < plan.fan ? n_lists : plan.fan) * k) kp <<= 1;
    hipLaunchKernelGGL(pair_merge_kernel, dim3((unsigned)out_lists), dim3(kMergeThreads), (size_t)kp * 12, s, src.f, src.i,
                       src.j, src.n, n_lists, k, plan.fan, dst.f, dst.i, dst.j, dst.n, last ? out_drug : nullptr, out_dis,
                       out_logit, out_info);
    if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
    if (last) break;
    n_lists = out_lists;
    in_a = !in_a;
  }
  return DGMI_OK;
}

}  // extern "C"

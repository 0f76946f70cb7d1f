// dgmi_pairs_above.hip — all-pairs MLP decoder with a streaming emit of every novel pair at or above a cut (gfx950),
// and the record sort that puts the emitted buffer into the ranking order.
//
// The threshold sibling of dgmi_pairs.hip: the same persistent grid (one workgroup per CU), the same (drug chunk,
// 128-disease group) tasks in drug-major order, the same P staging in LDS and the same scorer (dgmi_pair_score.h), so
// every logit has the bits the two top-k kernels return for the pair.  Where pair_mlp_topk_kernel keeps a best-k list
// with a moving threshold, a sort and a merge, this kernel has a fixed cut and nothing to keep:
//   * a lane whose pair is novel and has order_key(logit) >= order_key(min_logit) appends (key, i, j) to the
//     workgroup's LDS staging buffer at its ballot rank (one LDS atomic per wave and drug);
//   * every kSub drugs the workgroup checks the fill; past 3/4 — and at the end of the kernel — it flushes: ONE lane
//     reserves n slots with a single 64-bit atomicAdd on the global counter, and the workgroup copies its records to
//     the reserved range with consecutive (coalesced) stores.  A record whose slot is >= capacity is dropped; the
//     counter keeps counting, so the total is exact whatever the capacity.
// The order of the buffer depends on which workgroup flushed first; dgmi_pair_records_sort_f32 removes that: three
// stable LSD stages of the record radix sort of dgmi_sort.hip (by disease, by drug, by the complemented logit key)
// leave logit descending, ties by (drug, disease) ascending, NaN last — a function of the record multiset alone.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dgmi.h"
#include "dgmi_above.h"
#include "dgmi_kernels.h"
#include "dgmi_pair_stream.h"

namespace {

constexpr int kStageCap = 2048;          // LDS staging buffer, records

struct EmitArgs {
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
  int chunk, n_groups;
  int64_t n_tasks;
  float min_logit;
  unsigned long long capacity;
  int32_t* out_drug;  // [capacity]
  int32_t* out_dis;
  float* out_logit;
  unsigned long long* count;  // [1], zeroed before the launch
};

__global__ __launch_bounds__(kThreads) void pair_mlp_emit_kernel(EmitArgs a) {
  __shared__ __attribute__((aligned(16))) float p_lds[kMaxChunk * kRowStride];
  __shared__ uint32_t ef[kStageCap], ei[kStageCap], ej[kStageCap];
  __shared__ int s_used;
  __shared__ unsigned long long s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const uint32_t cut = order_key(a.min_logit);  // NaN -> 0: every key qualifies

  PairDecoder dec;  // this lane's W2 operands and epilogue constants
  load_decoder(dec, a.W2, a.b2, a.w3, a.b3, half, col);

  if (tid == 0) s_used = 0;

  // write the n staged records to n freshly reserved slots of the output.  Called by the whole block with the same n,
  // after a barrier that follows the last append.
  auto flush = [&](int n) {
    if (n == 0) return;  // block-uniform
    if (tid == 0) {
      s_base = atomicAdd(a.count, (unsigned long long)n);
      s_used = 0;
    }
    __syncthreads();
    const unsigned long long base = s_base;
    for (int e = tid; e < n; e += kThreads) {
      const unsigned long long slot = base + (unsigned long long)e;
      if (slot < a.capacity) {
        a.out_drug[slot] = (int32_t)ei[e];
        a.out_dis[slot] = (int32_t)ej[e];
        a.out_logit[slot] = key_logit(ef[e]);
      }
    }
    __syncthreads();  // the staging buffer is free again
  };

  // offer lane `col`'s pair (i, j) of one drug; lanes 32..63 hold the same pairs and never append
  auto offer = [&](bool valid, float logit, uint32_t i, uint32_t j) {
    const uint32_t f = order_key(logit);
    const bool q = half == 0 && valid && f >= cut;
    ballot_append(q, f, i, j, lane, &s_used, ef, ei, ej, kStageCap);
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
      __syncthreads();  // everyone has read the fill before anyone appends (or the flush resets it)
      if (n > kStageCap - kSub * kGroupCols) flush(n);
    }
  }

  __syncthreads();
  const int n = s_used;
  __syncthreads();
  flush(n);
}

// logit -> the key the radix sort takes ascending: the complemented ranking key (largest logit first, NaN last)
__global__ __launch_bounds__(256) void records_to_key_kernel(const float* __restrict__ logit, int32_t* __restrict__ key, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) key[e] = (int32_t)~order_key(logit[e]);
}

__global__ __launch_bounds__(256) void records_from_key_kernel(const int32_t* __restrict__ key, float* __restrict__ logit, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) logit[e] = key_logit(~(uint32_t)key[e]);
}

constexpr int kIdBits = 31;   // ids are non-negative int32
constexpr int kKeyBits = 32;

}  // namespace

extern "C" {

DGMI_API size_t dgmi_pair_emit_workspace_bytes(int64_t n_drug, int64_t n_dis) {
  if (n_drug <= 0 || n_dis <= 0 || n_drug > INT32_MAX || n_dis > INT32_MAX) return 0;
  return bitmap_bytes(n_drug, lane_column_plan(n_drug, n_dis).nwords);  // the known-pair bitmap, nothing else
}

DGMI_API int dgmi_pair_mlp_emit_f32(const float* P, int64_t ldp, int64_t n_drug, const float* Q, int64_t ldq, int64_t n_dis,
                                    int32_t h1, int32_t h2, const float* W2, const float* b2, const float* w3, const float* b3,
                                    const int32_t* known_drug, const int32_t* known_dis, int64_t n_known, float min_logit,
                                    int64_t capacity, int32_t* out_drug, int32_t* out_dis, float* out_logit, int64_t* out_count,
                                    int32_t* out_info, void* workspace, size_t workspace_bytes, dgmi_stream_t stream) {
  if (!check_pair_extents(h1, h2, n_drug, n_dis, n_known) || capacity < 0 || capacity > DGMI_PAIR_EMIT_MAX_RECORDS)
    return DGMI_ERR_INVALID_ARG;
  if (out_count == nullptr || out_info == nullptr) return DGMI_ERR_INVALID_ARG;
  if (capacity > 0 && (out_drug == nullptr || out_dis == nullptr || out_logit == nullptr)) return DGMI_ERR_INVALID_ARG;
  // an empty problem takes any operands and no workspace: the two counters are all that is written
  const bool empty = n_drug == 0 || n_dis == 0;
  LaneColumnPlan plan{};
  if (!empty) {
    if (!check_known(known_drug, known_dis, n_known) || !check_pair_operands(P, ldp, Q, ldq, W2, b2, w3, b3))
      return DGMI_ERR_INVALID_ARG;
    plan = lane_column_plan(n_drug, n_dis);
    if (workspace == nullptr || workspace_bytes < bitmap_bytes(n_drug, plan.nwords)) return DGMI_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);

  if (hipMemsetAsync(out_count, 0, sizeof(int64_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  if (hipMemsetAsync(out_info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  if (empty) return DGMI_OK;
  uint32_t* bitmap = nullptr;
  if (n_known > 0) {
    bitmap = static_cast<uint32_t*>(workspace);
    if (build_known_bitmap(known_drug, known_dis, n_known, n_drug, n_dis, plan.nwords, bitmap, out_info, s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
  }
  EmitArgs args{P, ldp, Q, ldq, (int)n_drug, (int)n_dis, W2, b2, w3, b3, bitmap, plan.nwords, plan.chunk, plan.n_groups,
                plan.n_tasks, min_logit, (unsigned long long)capacity, out_drug, out_dis, out_logit,
                reinterpret_cast<unsigned long long*>(out_count)};
  hipLaunchKernelGGL(pair_mlp_emit_kernel, dim3((unsigned)plan.grid), dim3(kThreads), 0, s, args);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
  return DGMI_OK;
}

DGMI_API size_t dgmi_pair_records_sort_workspace_bytes(int64_t n) {
  if (n <= 0 || n > DGMI_PAIR_EMIT_MAX_RECORDS) return 0;
  return align_up((size_t)n * 4) + dgmi::radix_sort_workspace_bytes(n, kKeyBits);
}

DGMI_API int dgmi_pair_records_sort_f32(int32_t* drug, int32_t* dis, float* logit, int64_t n, void* workspace,
                                        size_t workspace_bytes, dgmi_stream_t stream) {
  if (n < 0 || n > DGMI_PAIR_EMIT_MAX_RECORDS) return DGMI_ERR_INVALID_ARG;
  if (n == 0) return DGMI_OK;
  if (drug == nullptr || dis == nullptr || logit == nullptr) return DGMI_ERR_INVALID_ARG;
  if (workspace == nullptr || workspace_bytes < dgmi_pair_records_sort_workspace_bytes(n)) return DGMI_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t* key = static_cast<int32_t*>(workspace);
  void* sort_ws = static_cast<char*>(workspace) + align_up((size_t)n * 4);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(records_to_key_kernel, dim3(blocks), dim3(256), 0, s, logit, key, n);
  // Three stable stages, least significant field first.  Each stage is several radix passes (31 or 32 bits in digits of
  // up to 9): its input is read by the first pass only and its output written by the last only, with the sort's own
  // buffers in between, so a stage sorts the three arrays in place.
  if (dgmi::radix_sort_records(dis, drug, key, n, 0, kIdBits, 0, 0, dis, drug, key, nullptr, sort_ws, s) != hipSuccess)
    return DGMI_ERR_LAUNCH;
  if (dgmi::radix_sort_records(drug, dis, key, n, 0, kIdBits, 0, 0, drug, dis, key, nullptr, sort_ws, s) != hipSuccess)
    return DGMI_ERR_LAUNCH;
  if (dgmi::radix_sort_records(key, drug, dis, n, 0, kKeyBits, 0, 0, key, drug, dis, nullptr, sort_ws, s) != hipSuccess)
    return DGMI_ERR_LAUNCH;
  hipLaunchKernelGGL(records_from_key_kernel, dim3(blocks), dim3(256), 0, s, key, logit, n);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
  return DGMI_OK;
}

}  // extern "C"

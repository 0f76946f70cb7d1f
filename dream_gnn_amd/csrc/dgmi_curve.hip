// dgmi_curve.hip — exact ROC / precision-recall areas of scored samples, overall or per segment (gfx950).
//
// The metric lines of evaluation.py:55-65 as a sort-scan on the device (definition: include/dgmi_curve.h):
//   K1  keys     key = ~order_key(score) (ascending sort = descending score, NaN last), label bit, segment id (an
//                out-of-range id goes to the trash segment S), the three flags                 reads 8-12 B, writes 12 B
//   --  sort     dgmi::radix_sort_records on the 32-bit key; with segments a second stable stage on the segment id
//   K2  counts   per 2048-record tile: the aggregate of the count scan below                   reads 8-12 B
//   K3  carry    exclusive scan of the tile aggregates (one workgroup)
//   K4  terms    the count scan inside the tile, the two terms of every tie group at its last record, P / N / the
//                threshold counts at the records that own them, and the segment sums inside the tile  reads 8-12 B
//   K5  close    scan of the tiles' term aggregates in tile order (one workgroup): closes the segments that cross tiles
//   K6  finish   one thread per segment: the two divisions and the NaN rules
//
// The count scan is ONE segmented scan (it restarts where the segment id changes) over (TP, FP, TP and FP at the last
// group end): its exclusive value at a group's last record holds TP_{g-1} and FP_{g-1}, so a tie group and a segment
// may each span any number of tiles and the carries cross them.  The terms (1, n_g (2 TP_{g-1} + p_g), p_g (pi_g +
// pi_{g-1})) are summed per segment by a second segmented scan: inside a tile by a fixed tree, across tiles in tile
// order, so the float64 sum depends on the sorted sequence alone — no floating-point atomics.  A segment's totals have
// exactly one writer: the tile that holds both its first and its last record, or K5 for one that started in an
// earlier tile.  The threshold counts need no pass of their own: inside a segment the records that reach the threshold
// are a prefix, and the last of them holds TPt and FPt.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dgmi.h"
#include "dgmi_curve.h"
#include "dgmi_kernels.h"
// order_key: the ranking key.  The header also carries the pair scorer, which is not used here.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "dgmi_pair_score.h"
#pragma clang diagnostic pop

namespace {

constexpr int kThreads = 256;  // 4 waves: at the terms kernel's ~150 VGPRs three workgroups share a CU
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;      // consecutive records per thread: two 16-B loads per field
constexpr int kTile = kThreads * kItems;
constexpr int kScanThreads = 512;  // the two one-workgroup scans over the tiles
constexpr int kKeyBits = 32;
constexpr size_t kAlign = 256;
constexpr uint32_t kNanKey = 0xffffffffu;  // ~order_key(NaN)

inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

inline int bits_for(int64_t n) {  // bits the ids 0 .. n - 1 take, at least 1
  int b = 1;
  while (b < 31 && ((int64_t)1 << b) < n) ++b;
  return b;
}

// ---- the two scan elements ------------------------------------------------------------------------------------------
// An interval of records of the sorted sequence.  flags bit 0: it holds a segment's first record; tp / fp: positives /
// negatives since then (since the interval's start without one); bit 1: a tie group ended since then, and gtp / gfp are
// tp / fp at the last such end (0 without one).
struct CountElem {
  int32_t flags, tp, fp, gtp, gfp;
  static __device__ __forceinline__ CountElem identity() { return CountElem{0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ CountElem combine(const CountElem& a, const CountElem& b) {
    if (b.flags & 1) return b;
    CountElem r;
    r.flags = a.flags | b.flags;
    r.tp = a.tp + b.tp;
    r.fp = a.fp + b.fp;
    const bool ge = (b.flags & 2) != 0;
    r.gtp = ge ? a.tp + b.gtp : a.gtp;
    r.gfp = ge ? a.fp + b.gfp : a.gfp;
    return r;
  }
};

// The terms of an interval: head as above; g groups ended, u2 and a are the sums of their terms since the head.
struct TermElem {
  int32_t head, g;
  int64_t u2;
  double a;
  static __device__ __forceinline__ TermElem identity() { return TermElem{0, 0, 0, 0.0}; }
  static __device__ __forceinline__ TermElem combine(const TermElem& x, const TermElem& y) {
    if (y.head) return y;
    return TermElem{x.head, x.g + y.g, x.u2 + y.u2, x.a + y.a};
  }
};

template <class T>
__device__ __forceinline__ T shfl_up_words(const T& v, int d) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); ++i) w[i] = __shfl_up(w[i], d, 64);
  T r;
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}

// Exclusive scan over the workgroup's threads in thread order (wave scans, then the waves' totals through LDS), in a
// fixed tree; *total = all threads combined.  Every thread calls it; s_wave is free again on return.
template <class T, int WAVES>
__device__ __forceinline__ T block_scan_excl(const T& mine, T* s_wave, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = shfl_up_words(incl, d);
    if (lane >= d) incl = T::combine(o, incl);
  }
  if (lane == 63) s_wave[wave] = incl;
  T ex = shfl_up_words(incl, 1);
  if (lane == 0) ex = T::identity();
  __syncthreads();
  T before = T::identity(), all = T::identity();
  for (int w = 0; w < WAVES; ++w) {
    const T x = s_wave[w];
    if (w < wave) before = T::combine(before, x);
    all = T::combine(all, x);
  }
  __syncthreads();
  *total = all;
  return T::combine(before, ex);
}

// ---- K1 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void curve_keys_kernel(const float* __restrict__ score, const float* __restrict__ label,
                                                         const int32_t* __restrict__ segment, int64_t n, int32_t n_seg,
                                                         int32_t* __restrict__ key, int32_t* __restrict__ lab,
                                                         int32_t* __restrict__ seg, int32_t* __restrict__ info) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float x = score[i], y = label[i];
    if (x != x) bad |= 1;
    if (!(y == 0.f || y == 1.f)) bad |= 2;
    int32_t s = 0;
    if (segment != nullptr) {
      s = segment[i];
      if (s < 0 || s >= n_seg) {
        s = n_seg;  // the trash segment
        bad |= 4;
      }
    }
    key[i] = (int32_t)~order_key(x);
    lab[i] = y != 0.f ? 1 : 0;  // a NaN label is != 0
    seg[i] = s;
  }
  // one integer atomic per wave that saw something
  const int any = (__ballot(bad & 1) ? 1 : 0) | (__ballot(bad & 2) ? 2 : 0) | (__ballot(bad & 4) ? 4 : 0);
  if (any != 0 && (threadIdx.x & 63) == 0) atomicOr(info, any);
}

// ---- a thread's records -----------------------------------------------------------------------------------------------
struct Items {
  uint32_t key[kItems];
  int32_t seg[kItems];
  uint32_t pos, head, ge, se, valid;  // bit j: record j is positive / first of its segment / last of its tie group /
                                      // last of its segment / inside the n records
  uint32_t next_key;                  // key of the record after the thread's last (when there is one)
};

struct Neighbours {
  uint32_t first_key[kThreads];
  int32_t first_seg[kThreads], last_seg[kThreads];
};

// The arrays hold whole tiles (the workspace pads them), so the loads need no bounds test; what lies past n is masked.
template <bool SEG>
__device__ __forceinline__ void load_items(Items& it, const int32_t* __restrict__ key, const int32_t* __restrict__ lab,
                                           const int32_t* __restrict__ seg, int64_t n, Neighbours& nb) {
  const int tid = threadIdx.x;
  const int64_t tile0 = (int64_t)blockIdx.x * kTile;
  const int64_t base = tile0 + (int64_t)tid * kItems;
  int32_t l[kItems];
#pragma unroll
  for (int h = 0; h < kItems / 4; ++h) {
    const int4 k4 = *reinterpret_cast<const int4*>(key + base + 4 * h);
    const int4 l4 = *reinterpret_cast<const int4*>(lab + base + 4 * h);
    it.key[4 * h + 0] = (uint32_t)k4.x, it.key[4 * h + 1] = (uint32_t)k4.y;
    it.key[4 * h + 2] = (uint32_t)k4.z, it.key[4 * h + 3] = (uint32_t)k4.w;
    l[4 * h + 0] = l4.x, l[4 * h + 1] = l4.y, l[4 * h + 2] = l4.z, l[4 * h + 3] = l4.w;
    if (SEG) {
      const int4 s4 = *reinterpret_cast<const int4*>(seg + base + 4 * h);
      it.seg[4 * h + 0] = s4.x, it.seg[4 * h + 1] = s4.y, it.seg[4 * h + 2] = s4.z, it.seg[4 * h + 3] = s4.w;
    } else {
      it.seg[4 * h + 0] = it.seg[4 * h + 1] = it.seg[4 * h + 2] = it.seg[4 * h + 3] = 0;
    }
  }
  nb.first_key[tid] = it.key[0];
  if (SEG) {
    nb.first_seg[tid] = it.seg[0];
    nb.last_seg[tid] = it.seg[kItems - 1];
  }
  __syncthreads();
  const int64_t tile_end = tile0 + kTile;
  int32_t next_seg = 0, prev_seg = 0;
  if (tid + 1 < kThreads) {
    it.next_key = nb.first_key[tid + 1];
    if (SEG) next_seg = nb.first_seg[tid + 1];
  } else {
    it.next_key = tile_end < n ? (uint32_t)key[tile_end] : 0u;
    if (SEG) next_seg = tile_end < n ? seg[tile_end] : 0;
  }
  if (SEG) prev_seg = tid > 0 ? nb.last_seg[tid - 1] : (tile0 > 0 ? seg[tile0 - 1] : 0);
  __syncthreads();  // the exchange arrays are free again
  it.pos = it.head = it.ge = it.se = it.valid = 0u;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int64_t i = base + j;
    const bool valid = i < n, has_next = i + 1 < n;
    const uint32_t nk = j + 1 < kItems ? it.key[j + 1 < kItems ? j + 1 : j] : it.next_key;
    const int32_t ns = j + 1 < kItems ? it.seg[j + 1 < kItems ? j + 1 : j] : next_seg;
    const int32_t ps = j > 0 ? it.seg[j > 0 ? j - 1 : 0] : prev_seg;
    const bool se = valid && (!has_next || ns != it.seg[j]);
    const bool ge = valid && (se || nk != it.key[j]);
    const bool head = valid && (i == 0 || ps != it.seg[j]);
    it.valid |= (valid ? 1u : 0u) << j;
    it.pos |= ((valid && l[j] != 0) ? 1u : 0u) << j;
    it.head |= (head ? 1u : 0u) << j;
    it.ge |= (ge ? 1u : 0u) << j;
    it.se |= (se ? 1u : 0u) << j;
  }
}

__device__ __forceinline__ CountElem count_leaf(const Items& it, int j) {
  if (!((it.valid >> j) & 1u)) return CountElem::identity();
  const int p = (int)((it.pos >> j) & 1u), ge = (int)((it.ge >> j) & 1u);
  return CountElem{(int32_t)((it.head >> j) & 1u) | (ge << 1), p, 1 - p, ge ? p : 0, ge ? 1 - p : 0};
}

// ---- K2 -------------------------------------------------------------------------------------------------------------
template <bool SEG>
__global__ __launch_bounds__(kThreads) void curve_tile_counts_kernel(const int32_t* __restrict__ key, const int32_t* __restrict__ lab,
                                                                     const int32_t* __restrict__ seg, int64_t n,
                                                                     CountElem* __restrict__ cagg) {
  __shared__ Neighbours nb;
  __shared__ CountElem s_wave[kWaves];
  Items it;
  load_items<SEG>(it, key, lab, seg, n, nb);
  CountElem mine = CountElem::identity();
#pragma unroll
  for (int j = 0; j < kItems; ++j) mine = CountElem::combine(mine, count_leaf(it, j));
  CountElem total;
  block_scan_excl<CountElem, kWaves>(mine, s_wave, &total);
  if (threadIdx.x == 0) cagg[blockIdx.x] = total;
}

// ---- K3 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void curve_count_carry_kernel(const CountElem* __restrict__ cagg, int n_tiles,
                                                                         CountElem* __restrict__ ccarry) {
  __shared__ CountElem s_wave[kScanThreads / 64];
  CountElem carry = CountElem::identity();  // the same in every thread
  for (int c0 = 0; c0 < n_tiles; c0 += kScanThreads) {
    const int t = c0 + threadIdx.x;
    const CountElem v = t < n_tiles ? cagg[t] : CountElem::identity();
    CountElem all;
    const CountElem ex = block_scan_excl<CountElem, kScanThreads / 64>(v, s_wave, &all);
    if (t < n_tiles) ccarry[t] = CountElem::combine(carry, ex);
    carry = CountElem::combine(carry, all);
  }
}

// ---- K4 -------------------------------------------------------------------------------------------------------------
struct TermArgs {
  const int32_t* key;
  const int32_t* lab;
  const int32_t* seg;
  int64_t n;
  int32_t n_out;  // S: segments with an output row (the trash segment S has none)
  uint32_t cut;   // ~order_key(threshold)
  int32_t cut_ok; // 0: the threshold is NaN, nothing qualifies
  const CountElem* ccarry;
  TermElem* tagg;     // [n_tiles] the tile's terms, as an interval
  TermElem* tpre;     // [n_tiles] the terms up to the end of the segment that was open at the tile's start, if it ends here
  int32_t* pre_seg;   // [n_tiles] that segment, or -1 (preset)
  int64_t* out_count; // [S][6]
  double* out_area;   // [S][2]; [.][1] holds the raw sum until K6
};

template <bool SEG>
__global__ __launch_bounds__(kThreads) void curve_tile_terms_kernel(TermArgs a) {
  __shared__ Neighbours nb;
  __shared__ CountElem s_cwave[kWaves];
  __shared__ TermElem s_twave[kWaves];
  Items it;
  load_items<SEG>(it, a.key, a.lab, a.seg, a.n, nb);
  CountElem mine = CountElem::identity();
#pragma unroll
  for (int j = 0; j < kItems; ++j) mine = CountElem::combine(mine, count_leaf(it, j));
  CountElem total;
  const CountElem ex = block_scan_excl<CountElem, kWaves>(mine, s_cwave, &total);
  CountElem run = CountElem::combine(a.ccarry[blockIdx.x], ex);

  auto reaches = [&](uint32_t k) { return a.cut_ok != 0 && k <= a.cut && k != kNanKey; };
  int64_t u2[kItems];
  double ar[kItems];
  TermElem tmine = TermElem::identity();
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    u2[j] = 0;
    ar[j] = 0.0;
    if (!((it.valid >> j) & 1u)) continue;
    const bool head = (it.head >> j) & 1u, ge = (it.ge >> j) & 1u, se = (it.se >> j) & 1u;
    const int32_t tp0 = head ? 0 : run.gtp, fp0 = head ? 0 : run.gfp;  // TP_{g-1}, FP_{g-1}
    run = CountElem::combine(run, count_leaf(it, j));
    const bool out = it.seg[j] < a.n_out;
    int64_t* cnt = a.out_count + (int64_t)(out ? it.seg[j] : 0) * 6;
    if (ge) {
      const int32_t pg = run.tp - tp0, ng = run.fp - fp0;
      u2[j] = (int64_t)ng * (2 * (int64_t)tp0 + pg);
      const double pi1 = (double)run.tp / ((double)run.tp + (double)run.fp);
      const double pi0 = tp0 + fp0 == 0 ? 1.0 : (double)tp0 / ((double)tp0 + (double)fp0);
      ar[j] = (double)pg * (pi1 + pi0);
    }
    if (se && out) {
      cnt[0] = run.tp;
      cnt[1] = run.fp;
    }
    const uint32_t nk = j + 1 < kItems ? it.key[j + 1 < kItems ? j + 1 : j] : it.next_key;
    if (out && reaches(it.key[j]) && (se || !reaches(nk))) {  // the last record of its segment that reaches the threshold
      cnt[2] = run.tp;
      cnt[3] = run.fp;
    }
    tmine = TermElem::combine(tmine, TermElem{head ? 1 : 0, ge ? 1 : 0, u2[j], ar[j]});
  }
  TermElem ttotal;
  TermElem r = block_scan_excl<TermElem, kWaves>(tmine, s_twave, &ttotal);
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    if (!((it.valid >> j) & 1u)) continue;
    r = TermElem::combine(r, TermElem{(int32_t)((it.head >> j) & 1u), (int32_t)((it.ge >> j) & 1u), u2[j], ar[j]});
    if ((it.se >> j) & 1u) {
      if (r.head) {  // the segment started in this tile: it is complete
        if (it.seg[j] < a.n_out) {
          a.out_count[(int64_t)it.seg[j] * 6 + 4] = r.g;
          a.out_count[(int64_t)it.seg[j] * 6 + 5] = r.u2;
          a.out_area[(int64_t)it.seg[j] * 2 + 1] = r.a;
        }
      } else {  // it started in an earlier tile (one such record per tile at most): K5 adds what came before
        a.tpre[blockIdx.x] = r;
        a.pre_seg[blockIdx.x] = it.seg[j];
      }
    }
  }
  if (threadIdx.x == 0) a.tagg[blockIdx.x] = ttotal;
}

// ---- K5 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void curve_close_segments_kernel(const TermElem* __restrict__ tagg,
                                                                            const TermElem* __restrict__ tpre,
                                                                            const int32_t* __restrict__ pre_seg, int n_tiles,
                                                                            int32_t n_out, int64_t* __restrict__ out_count,
                                                                            double* __restrict__ out_area) {
  __shared__ TermElem s_wave[kScanThreads / 64];
  TermElem carry = TermElem::identity();  // the same in every thread
  for (int c0 = 0; c0 < n_tiles; c0 += kScanThreads) {
    const int t = c0 + threadIdx.x;
    const TermElem v = t < n_tiles ? tagg[t] : TermElem::identity();
    TermElem all;
    const TermElem ex = block_scan_excl<TermElem, kScanThreads / 64>(v, s_wave, &all);
    if (t < n_tiles) {
      const int32_t s = pre_seg[t];
      if (s >= 0 && s < n_out) {
        const TermElem f = TermElem::combine(TermElem::combine(carry, ex), tpre[t]);
        out_count[(int64_t)s * 6 + 4] = f.g;
        out_count[(int64_t)s * 6 + 5] = f.u2;
        out_area[(int64_t)s * 2 + 1] = f.a;
      }
    }
    carry = TermElem::combine(carry, all);
  }
}

// ---- K6 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void curve_finish_kernel(const int64_t* __restrict__ out_count, double* __restrict__ out_area,
                                                           int64_t n_out) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_out) return;
  const int64_t P = out_count[s * 6 + 0], N = out_count[s * 6 + 1], U2 = out_count[s * 6 + 5];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double sum = out_area[s * 2 + 1];
  out_area[s * 2 + 0] = (P == 0 || N == 0) ? nan : (double)U2 / (double)(2 * P * N);
  out_area[s * 2 + 1] = P == 0 ? nan : sum / (double)(2 * P);
}

struct Plan {
  int64_t n_tiles;
  size_t arr;  // bytes of one padded record field
  size_t off_sort, off_cagg, off_ccarry, off_tagg, off_tpre, off_pre_seg, total;
};

Plan make_plan(int64_t n) {
  Plan p;
  p.n_tiles = (n + kTile - 1) / kTile;
  p.arr = align_up((size_t)p.n_tiles * kTile * 4);
  size_t off = 6 * p.arr;  // two sets of (key, label, segment): the sort's stages go from one to the other
  p.off_sort = off;
  off += align_up(dgmi::radix_sort_workspace_bytes(n, kKeyBits));  // the segment stage needs no more than the key stage
  p.off_cagg = off;
  off += align_up((size_t)p.n_tiles * sizeof(CountElem));
  p.off_ccarry = off;
  off += align_up((size_t)p.n_tiles * sizeof(CountElem));
  p.off_tagg = off;
  off += align_up((size_t)p.n_tiles * sizeof(TermElem));
  p.off_tpre = off;
  off += align_up((size_t)p.n_tiles * sizeof(TermElem));
  p.off_pre_seg = off;
  off += align_up((size_t)p.n_tiles * 4);
  p.total = off;
  return p;
}

inline bool sizes_ok(int64_t n, int64_t n_segments) {
  return n >= 0 && n <= INT32_MAX && n_segments >= 0 && n_segments <= DGMI_CURVE_MAX_SEGMENTS;
}

}  // namespace

extern "C" {

DGMI_API size_t dgmi_curve_areas_workspace_bytes(int64_t n, int64_t n_segments) {
  if (!sizes_ok(n, n_segments) || n == 0) return 0;
  return make_plan(n).total;
}

DGMI_API int dgmi_curve_areas_f32(const float* score, const float* label, const int32_t* segment, int64_t n, int64_t n_segments,
                                  float threshold, int64_t* out_count, double* out_area, int32_t* out_info, void* workspace,
                                  size_t workspace_bytes, dgmi_stream_t stream) {
  if (!sizes_ok(n, n_segments)) return DGMI_ERR_INVALID_ARG;
  if (out_count == nullptr || out_area == nullptr || out_info == nullptr) return DGMI_ERR_INVALID_ARG;
  if (n > 0 && (score == nullptr || label == nullptr)) return DGMI_ERR_INVALID_ARG;
  if (n_segments > 0 && segment == nullptr) return DGMI_ERR_INVALID_ARG;
  const bool segmented = n_segments > 0;
  const int64_t S = segmented ? n_segments : 1;
  Plan plan{};
  if (n > 0) {
    plan = make_plan(n);
    if (workspace == nullptr || workspace_bytes < plan.total) return DGMI_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  // a segment without samples keeps these zeros: P = N = 0, both areas NaN
  if (hipMemsetAsync(out_info, 0, sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  if (hipMemsetAsync(out_count, 0, (size_t)S * 6 * sizeof(int64_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  if (hipMemsetAsync(out_area, 0, (size_t)S * 2 * sizeof(double), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  const unsigned finish_blocks = (unsigned)((S + 255) / 256);
  if (n == 0) {
    hipLaunchKernelGGL(curve_finish_kernel, dim3(finish_blocks), dim3(256), 0, s, out_count, out_area, S);
    return hipGetLastError() == hipSuccess ? DGMI_OK : DGMI_ERR_LAUNCH;
  }
  char* ws = static_cast<char*>(workspace);
  int32_t* set[2][3];  // (key, label, segment) twice
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 3; ++j) set[i][j] = reinterpret_cast<int32_t*>(ws + (size_t)(3 * i + j) * plan.arr);
  void* sort_ws = ws + plan.off_sort;
  CountElem* cagg = reinterpret_cast<CountElem*>(ws + plan.off_cagg);
  CountElem* ccarry = reinterpret_cast<CountElem*>(ws + plan.off_ccarry);
  TermElem* tagg = reinterpret_cast<TermElem*>(ws + plan.off_tagg);
  TermElem* tpre = reinterpret_cast<TermElem*>(ws + plan.off_tpre);
  int32_t* pre_seg = reinterpret_cast<int32_t*>(ws + plan.off_pre_seg);
  const int n_tiles = (int)plan.n_tiles;
  if (hipMemsetAsync(pre_seg, 0xff, (size_t)n_tiles * 4, s) != hipSuccess) return DGMI_ERR_LAUNCH;  // -1: none

  int64_t key_blocks = (n + 255) / 256;
  if (key_blocks > 2048) key_blocks = 2048;
  hipLaunchKernelGGL(curve_keys_kernel, dim3((unsigned)key_blocks), dim3(256), 0, s, score, label, segmented ? segment : nullptr, n,
                     (int32_t)n_segments, set[0][0], set[0][1], set[0][2], out_info);
  // Stable stages, least significant field first, each from one record set to the other (a one-pass stage reads its
  // input while it writes its output, so the two must differ).
  if (dgmi::radix_sort_records(set[0][0], set[0][1], set[0][2], n, 0, kKeyBits, 0, 0, set[1][0], set[1][1], set[1][2], nullptr,
                               sort_ws, s) != hipSuccess)
    return DGMI_ERR_LAUNCH;
  int32_t** fin = set[1];
  if (segmented) {  // S + 1 ids: the trash segment sorts last.  (Also for S = 1: an out-of-range id must leave the segment.)
    if (dgmi::radix_sort_records(set[1][2], set[1][1], set[1][0], n, 0, bits_for(S + 1), 0, 0, set[0][2], set[0][1], set[0][0],
                                 nullptr, sort_ws, s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
    fin = set[0];
  }
  TermArgs ta{fin[0], fin[1], fin[2], n, (int32_t)S, ~0u, 0, ccarry, tagg, tpre, pre_seg, out_count, out_area};
  if (threshold == threshold) {  // the host restatement of order_key
    uint32_t u;
    __builtin_memcpy(&u, &threshold, 4);
    if (u == 0x80000000u) u = 0u;
    ta.cut = ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    ta.cut_ok = 1;
  }
  if (segmented) {
    hipLaunchKernelGGL(curve_tile_counts_kernel<true>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, fin[0], fin[1], fin[2], n, cagg);
    hipLaunchKernelGGL(curve_count_carry_kernel, dim3(1), dim3(kScanThreads), 0, s, cagg, n_tiles, ccarry);
    hipLaunchKernelGGL(curve_tile_terms_kernel<true>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, ta);
  } else {
    hipLaunchKernelGGL(curve_tile_counts_kernel<false>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, fin[0], fin[1], fin[2], n, cagg);
    hipLaunchKernelGGL(curve_count_carry_kernel, dim3(1), dim3(kScanThreads), 0, s, cagg, n_tiles, ccarry);
    hipLaunchKernelGGL(curve_tile_terms_kernel<false>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, ta);
  }
  hipLaunchKernelGGL(curve_close_segments_kernel, dim3(1), dim3(kScanThreads), 0, s, tagg, tpre, pre_seg, n_tiles, (int32_t)S,
                     out_count, out_area);
  hipLaunchKernelGGL(curve_finish_kernel, dim3(finish_blocks), dim3(256), 0, s, out_count, out_area, S);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
  return DGMI_OK;
}

}  // extern "C"

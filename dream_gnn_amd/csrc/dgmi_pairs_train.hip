// dgmi_pairs_train.hip — the decoder MLP on the training pair list (gfx950): logits with dropout in one kernel, every
// gradient from a recompute.  Nothing of size E x 128 is kept between forward and backward; the masks are a function
// (dgmi_pair_dropout.h), so the backward draws the forward's again.
//
// Forward.  pair_mlp_score_list_kernel's structure (dgmi_pairs_given.hip) and score_one's operand layout, step order and
// epilogue order (dgmi_pair_score.h): a wave takes 32 listed pairs on its lane columns, X[q_e] in VGPRs, C[c_e] staged
// to the wave's LDS rows, W2 as the A operand of 2 x 64 `v_mfma_f32_32x32x2_f32`.  The two differences: B =
// m1 relu(x + c) and the epilogue sums w3[h] m2 relu(acc + b2[h]).  With p = 0 both factors are exactly 1, so the logit
// is score_one's, bit for bit.  The scorer header is not touched (the ranking kernels' instructions are pinned).
//
// Backward, three launches:
//  1. pair_train_backward_kernel recomputes z2 as the forward does, then, per lane, in the accumulator layout
//     (row h = 32 hb + 8 (r >> 2) + 4 half + (r & 3) of pair `col`): dz2 = dlogit w3[h] m2 [z2 > 0], which it adds to its
//     db2 registers (dlogit h2 to its dw3 registers) and stores to the E x 64 workspace tensor dZ2.  The accumulator
//     layout IS a B operand with the pair on the column and K = h: 4 x 32 more MFMAs with A = W2[h, 32 kt + row] from a
//     padded LDS copy of W2 give W2^T dz2 as four 32 x 32 tiles, gated by m1 [x + c > 0] (x re-read from global, c
//     from the wave's LDS rows, the hash recomputed for the tile's k) and stored as dZ1 rows.
//  2. pair_train_dw2_kernel: dW2 = dZ2^T h1 with the PAIRS on the MFMA K axis: A = dZ2[e, 32 ht + row], B = h1[e, 32 kt
//     + col] recomputed from X, C and the hash: no MFMA recompute and no transpose.  8 accumulator tiles per wave for
//     the whole launch.  Why this is a kernel of its own (and dZ2 exists): DESIGN.md 4.15.
//  3. pair_train_reduce_kernel adds the workgroups' partial sums in a fixed order (sixteen runs in workgroup order).
// Sums.  List block b belongs to workgroup b mod grid, waves add their blocks in order, a workgroup adds its four waves
// in wave order, the reduce kernel adds workgroups in a fixed order; the column sums inside a wave are a fixed xor tree.  No
// float atomics: the same bits from run to run.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dgmi.h"
#include "dgmi_pair_dropout.h"
#include "dgmi_pair_stream.h"
#include "dgmi_train.h"

namespace {

using dgmi::PairDropout;
using dgmi::PairMask;

constexpr int kCols = kLaneRows;        // listed pairs per wave (one per lane column)
constexpr int kListBlock = 4 * kCols;   // listed pairs per workgroup and list block
constexpr int kW2Stride = kH1 + 8;      // a W2 row in LDS: rows h and h + 4 (the two lane halves of a step) 32 banks apart
constexpr int kSmall = 132;             // floats of a workgroup's small partial: db2 (64), dw3 (64), db3 (1), padding
constexpr int kW2Elems = kH2 * kH1;     // 8192
constexpr int kDw2Group = 8;            // MFMA steps of the dW2 kernel whose operands are in flight together

struct TrainArgs {
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
  PairDropout drop;
  const int64_t* seed;  // one int64 on the device
  float* out_logit;     // forward
  int32_t* info;
  const float* dlogit;  // backward
  float* dz1;
  int64_t ld_dz1;
  float* dz2;         // workspace: n_pairs x 64
  float* part_w2;     // workspace: [grid][64 x 128]
  float* part_small;  // workspace: [grid][kSmall]
};

__device__ __forceinline__ int list_blocks(int n_pairs) { return (int)(((int64_t)n_pairs + kListBlock - 1) / kListBlock); }

// The wave's 32 candidate rows into its LDS rows, coalesced; `cr` is the lane column's candidate row, -1: none (zeros).
__device__ __forceinline__ void stage_rows(float* rows, const float* C, int64_t ldc, int cr, int lane) {
  for (int it = 0; it < kCols * 32 / 64; ++it) {
    const int idx = it * 64 + lane, r = idx >> 5, c4 = idx & 31;
    const int src = __shfl(cr, r);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src >= 0) v = *reinterpret_cast<const float4*>(C + (int64_t)src * ldc + 4 * c4);
    *reinterpret_cast<float4*>(rows + r * kRowStride + 68 * (c4 >> 4) + 4 * (c4 & 15)) = v;
  }
}

// W2 . (m1 relu(pa + q)) of the lane column's pair: score_one's loop with the layer-1 factor on B.  he1 = m1.pair(e).
__device__ __forceinline__ void hidden2(const float* pa, const float (&q)[kH1 / 2], const PairDecoder& d, const PairMask& m1,
                                        uint32_t he1, int half, floatx16& c00, floatx16& c01) {
#pragma unroll
  for (int v = 0; v < 16; ++v) c00[v] = c01[v] = 0.f;
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) {
    const float4 xa = *reinterpret_cast<const float4*>(pa + 4 * s4);
    const float va[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = 4 * s4 + u;
      float ba = relu_nan(va[u] + q[s]);
      ba = m1.keep(he1, (uint32_t)(64 * half + s)) ? ba * m1.scale : 0.f;
      c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(d.wa[s], ba, c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(d.wb[s], ba, c01, 0, 0, 0);
    }
  }
}

struct ListedPair {
  int64_t e;
  bool listed, ok;
  int qr, cr;  // rows to read; -1: none (not listed, or an id out of range)
};

__device__ __forceinline__ ListedPair listed_pair(const TrainArgs& a, int64_t e) {
  ListedPair l;
  l.e = e;
  l.listed = e < a.n_pairs;
  const int32_t q = l.listed ? a.pair_query[e] : 0, c = l.listed ? a.pair_cand[e] : 0;
  l.ok = l.listed && q >= 0 && q < a.n_query && c >= 0 && c < a.n_cand;
  l.qr = l.ok ? q : -1;
  l.cr = l.ok ? c : -1;
  return l;
}

__device__ __forceinline__ void load_query_row(float (&x)[kH1 / 2], const TrainArgs& a, int qr, int half) {
  if (qr >= 0) {
    load_lane_row(x, a.X + (int64_t)qr * a.ldx, half);
  } else {
#pragma unroll
    for (int s = 0; s < kH1 / 2; ++s) x[s] = 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void pair_train_forward_kernel(TrainArgs a) {
  __shared__ __attribute__((aligned(16))) float c_lds[kListBlock * kRowStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  float* const rows = c_lds + wave * kCols * kRowStride;  // this wave's 32 candidate rows

  PairDecoder dec;
  load_decoder(dec, a.W2, a.b2, a.w3, a.b3, half, col);
  const uint64_t seed = (uint64_t)a.seed[0];
  const PairMask m1(seed, 1, a.drop), m2(seed, 2, a.drop);

  const int n_blocks = list_blocks(a.n_pairs);
  for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const ListedPair l = listed_pair(a, (int64_t)b * kListBlock + wave * kCols + col);
    float x[kH1 / 2];
    load_query_row(x, a, l.qr, half);
    __syncthreads();  // the previous block's readers of c_lds are done
    stage_rows(rows, a.C, a.ldc, l.cr, lane);
    __syncthreads();
    floatx16 c00, c01;
    hidden2(rows + col * kRowStride + 68 * half, x, dec, m1, m1.pair((uint32_t)l.e), half, c00, c01);
    const uint32_t he2 = m2.pair((uint32_t)l.e);
    float sa = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = relu_nan(c00[r] + dec.eb[0][r]);
      sa = fmaf(dec.ew[0][r], m2.keep(he2, (uint32_t)(8 * (r >> 2) + 4 * half + (r & 3))) ? v * m2.scale : 0.f, sa);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = relu_nan(c01[r] + dec.eb[1][r]);
      sa = fmaf(dec.ew[1][r], m2.keep(he2, (uint32_t)(32 + 8 * (r >> 2) + 4 * half + (r & 3))) ? v * m2.scale : 0.f, sa);
    }
    const float logit = (sa + __shfl_xor(sa, 32)) + dec.bias3;
    if (half == 0 && l.listed) {
      a.out_logit[l.e] = l.ok ? logit : __uint_as_float(0x7fc00000u);
      if (!l.ok) atomicOr(&a.info[0], 1);
    }
  }
}

// sum over the 32 lane columns of a half: a fixed xor tree, every lane of the half gets the sum
__device__ __forceinline__ float column_sum(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(kThreads) void pair_train_backward_kernel(TrainArgs a) {
  __shared__ __attribute__((aligned(16))) float c_lds[kListBlock * kRowStride];
  __shared__ __attribute__((aligned(16))) float w2_lds[kH2 * kW2Stride];
  __shared__ float red[4 * kSmall];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  float* const rows = c_lds + wave * kCols * kRowStride;

  PairDecoder dec;
  load_decoder(dec, a.W2, a.b2, a.w3, a.b3, half, col);
  for (int i = tid; i < kH2 * (kH1 / 4); i += kThreads) {
    const int h = i >> 5, c4 = i & 31;
    *reinterpret_cast<float4*>(w2_lds + h * kW2Stride + 4 * c4) = *reinterpret_cast<const float4*>(a.W2 + h * kH1 + 4 * c4);
  }
  const uint64_t seed = (uint64_t)a.seed[0];
  const PairMask m1(seed, 1, a.drop), m2(seed, 2, a.drop);

  float s_db2[2][16], s_dw3[2][16], s_db3 = 0.f;  // this lane's sums over its pairs, rows h of the accumulator layout
#pragma unroll
  for (int r = 0; r < 16; ++r) s_db2[0][r] = s_db2[1][r] = s_dw3[0][r] = s_dw3[1][r] = 0.f;

  const int n_blocks = list_blocks(a.n_pairs);
  for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const ListedPair l = listed_pair(a, (int64_t)b * kListBlock + wave * kCols + col);
    floatx16 c[2];
    const uint32_t he1 = m1.pair((uint32_t)l.e);
    {
      float x[kH1 / 2];
      load_query_row(x, a, l.qr, half);
      __syncthreads();  // the previous block's readers of c_lds are done (first block: w2_lds is written)
      stage_rows(rows, a.C, a.ldc, l.cr, lane);
      __syncthreads();
      hidden2(rows + col * kRowStride + 68 * half, x, dec, m1, he1, half, c[0], c[1]);
    }
    const float dl = l.ok ? a.dlogit[l.e] : 0.f;
    const uint32_t he2 = m2.pair((uint32_t)l.e);
    if (half == 0) s_db3 += dl;
    // z2 -> dz2 in place
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float z = c[hb][r] + dec.eb[hb][r];
        const bool kept = m2.keep(he2, (uint32_t)(32 * hb + 8 * (r >> 2) + 4 * half + (r & 3)));
        const float h2 = kept ? relu_nan(z) * m2.scale : 0.f;
        const float dz = (l.ok && kept && z > 0.f) ? (dl * dec.ew[hb][r]) * m2.scale : 0.f;
        if (l.ok) s_dw3[hb][r] += dl * h2;
        s_db2[hb][r] += dz;
        c[hb][r] = dz;
      }
    if (l.listed) {
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<float4*>(a.dz2 + l.e * kH2 + 32 * hb + 8 * j + 4 * half) =
              make_float4(c[hb][4 * j], c[hb][4 * j + 1], c[hb][4 * j + 2], c[hb][4 * j + 3]);
    }
    // dz1 = m1 [x + c > 0] W2^T dz2: the four 32-row tiles of k as four independent accumulators
    const float* crow = rows + col * kRowStride;
    floatx16 t[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int v = 0; v < 16; ++v) t[kt][v] = 0.f;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* w = w2_lds + (32 * hb + 8 * (r >> 2) + 4 * half + (r & 3)) * kW2Stride + col;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) t[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[32 * kt], c[hb][r], t[kt], 0, 0, 0);
      }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k0 = 32 * kt + 8 * j + 4 * half;  // rows k0 .. k0 + 3 of the tile are registers 4 j .. 4 j + 3
        float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l.ok) xv = *reinterpret_cast<const float4*>(a.X + (int64_t)l.qr * a.ldx + k0);
        const float4 cv = *reinterpret_cast<const float4*>(crow + 68 * (k0 >> 6) + (k0 & 63));
        const float zx[4] = {cv.x + xv.x, cv.y + xv.y, cv.z + xv.z, cv.w + xv.w};
        float o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          o[u] = (l.ok && zx[u] > 0.f && m1.keep(he1, (uint32_t)(k0 + u))) ? t[kt][4 * j + u] * m1.scale : 0.f;
        if (l.listed) *reinterpret_cast<float4*>(a.dz1 + l.e * a.ld_dz1 + k0) = make_float4(o[0], o[1], o[2], o[3]);
      }
    if (half == 0 && l.listed && !l.ok) atomicOr(&a.info[0], 1);
  }

  // this workgroup's partial sums: columns (xor tree), then the four waves in order
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int h = 32 * hb + 8 * (r >> 2) + 4 * half + (r & 3);
      const float sb = column_sum(s_db2[hb][r]), sw = column_sum(s_dw3[hb][r]);
      if (col == 0) {
        red[wave * kSmall + h] = sb;
        red[wave * kSmall + kH2 + h] = sw;
      }
    }
  const float s3 = column_sum(s_db3);
  if (lane == 0) red[wave * kSmall + 2 * kH2] = s3;
  __syncthreads();
  if (tid <= 2 * kH2)
    a.part_small[(int64_t)blockIdx.x * kSmall + tid] =
        ((red[tid] + red[kSmall + tid]) + red[2 * kSmall + tid]) + red[3 * kSmall + tid];
}

__global__ __launch_bounds__(kThreads) void pair_train_dw2_kernel(TrainArgs a) {
  __shared__ float acc_lds[kW2Elems];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const uint64_t seed = (uint64_t)a.seed[0];
  const PairMask m1(seed, 1, a.drop);

  floatx16 acc[2][4];  // tile (ht, kt): dW2[32 ht + 8 (r >> 2) + 4 half + (r & 3), 32 kt + col]
#pragma unroll
  for (int ht = 0; ht < 2; ++ht)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ht][kt][v] = 0.f;

  const int n_blocks = list_blocks(a.n_pairs);
  for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t base = (int64_t)b * kListBlock + wave * kCols;
    const ListedPair l = listed_pair(a, base + col);  // pair `col` of the wave's 32, on both halves
    // MFMA step t: K = pairs 2 t (lanes 0..31) and 2 t + 1 (lanes 32..63).  The operands of kDw2Group steps are loaded
    // before the first of them is used: the loads of a step depend on nothing but the ids, and one step's MFMAs are
    // shorter than a trip to L2.
#pragma unroll 1
    for (int t0 = 0; t0 < kCols / 2; t0 += kDw2Group) {
      float a0[kDw2Group], a1[kDw2Group], xs[kDw2Group][4], cs[kDw2Group][4];
      bool valid[kDw2Group];
#pragma unroll
      for (int u = 0; u < kDw2Group; ++u) {
        const int src = 2 * (t0 + u) + half;
        const int qe = __shfl(l.qr, src), ce = __shfl(l.cr, src);
        const int64_t e = base + src;
        valid[u] = qe >= 0;
        a0[u] = a1[u] = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) xs[u][kt] = cs[u][kt] = 0.f;
        if (valid[u]) {
          a0[u] = a.dz2[e * kH2 + col];
          a1[u] = a.dz2[e * kH2 + 32 + col];
          const float* xr = a.X + (int64_t)qe * a.ldx + col;
          const float* cr = a.C + (int64_t)ce * a.ldc + col;
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) xs[u][kt] = xr[32 * kt], cs[u][kt] = cr[32 * kt];
        }
      }
#pragma unroll
      for (int u = 0; u < kDw2Group; ++u) {
        const uint32_t he1 = m1.pair((uint32_t)(base + 2 * (t0 + u) + half));
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const float z = relu_nan(cs[u][kt] + xs[u][kt]);
          const float bk = (valid[u] && m1.keep(he1, (uint32_t)(32 * kt + col))) ? z * m1.scale : 0.f;
          acc[0][kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], bk, acc[0][kt], 0, 0, 0);
          acc[1][kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], bk, acc[1][kt], 0, 0, 0);
        }
      }
    }
  }

  // the four waves in order; every element is held by the same lane and register in each wave
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ht = 0; ht < 2; ++ht)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int idx = (32 * ht + 8 * (r >> 2) + 4 * half + (r & 3)) * kH1 + 32 * kt + col;
            acc_lds[idx] = w == 0 ? acc[ht][kt][r] : acc_lds[idx] + acc[ht][kt][r];
          }
    }
    __syncthreads();
  }
  for (int i = tid; i < kW2Elems; i += kThreads) a.part_w2[(int64_t)blockIdx.x * kW2Elems + i] = acc_lds[i];
}

// out = the sum of the workgroups' partials in a fixed order: a workgroup owns kReduceOuts outputs, thread (run, o) adds
// the run-th sixteenth of output o's partials in workgroup order (the loads of a run are independent: all in flight),
// then one thread per output adds the sixteen runs in order.  Output i < 8192 is dW2[i], then db2, dw3, db3.
constexpr int kReduceOuts = 16, kReduceRuns = 16, kReduceTotal = kW2Elems + 2 * kH2 + 1;

__global__ __launch_bounds__(kReduceOuts* kReduceRuns) void pair_train_reduce_kernel(
    const float* __restrict__ part_w2, const float* __restrict__ part_small, int n_parts, float* __restrict__ dW2,
    float* __restrict__ db2, float* __restrict__ dw3, float* __restrict__ db3) {
  __shared__ float red[kReduceRuns][kReduceOuts];
  const int o = threadIdx.x % kReduceOuts, run = threadIdx.x / kReduceOuts;
  const int i = (int)blockIdx.x * kReduceOuts + o;
  const bool small = i >= kW2Elems;
  const float* src = small ? part_small + (i - kW2Elems) : part_w2 + i;
  const int64_t stride = small ? kSmall : kW2Elems;
  const int per = (n_parts + kReduceRuns - 1) / kReduceRuns;
  const int g0 = run * per, g1 = g0 + per < n_parts ? g0 + per : n_parts;
  float s = 0.f;
  if (i < kReduceTotal) {
    int g = g0;
    for (; g + 16 <= g1; g += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = src[(int64_t)(g + u) * stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; g < g1; ++g) s += src[(int64_t)g * stride];
  }
  red[run][o] = s;
  __syncthreads();
  if (run == 0 && i < kReduceTotal) {
    float sum = red[0][o];
    for (int r = 1; r < kReduceRuns; ++r) sum += red[r][o];
    if (!small) dW2[i] = sum;
    else if (i < kW2Elems + kH2) db2[i - kW2Elems] = sum;
    else if (i < kW2Elems + 2 * kH2) dw3[i - kW2Elems - kH2] = sum;
    else db3[0] = sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct TrainPlan {
  int grid;                               // workgroups of every launch over the list: list block b goes to b mod grid
  size_t dz2, part_w2, part_small, total;  // byte offsets / size
};

TrainPlan train_plan(int64_t n_pairs) {
  TrainPlan p;
  const int64_t n_blocks = (n_pairs + kListBlock - 1) / kListBlock;
  p.grid = (int)(n_blocks < kGrid ? n_blocks : kGrid);
  p.dz2 = 0;
  p.part_w2 = align_up((size_t)n_pairs * kH2 * sizeof(float));
  p.part_small = p.part_w2 + align_up((size_t)p.grid * kW2Elems * sizeof(float));
  p.total = p.part_small + align_up((size_t)p.grid * kSmall * sizeof(float));
  return p;
}

// extents, widths and p; the rest is checked once the list is known not to be empty
bool check_train_extents(int32_t h1, int32_t h2, int64_t n_query, int64_t n_cand, int64_t n_pairs, float p) {
  return check_pair_extents(h1, h2, n_query, n_cand, 0) && n_pairs >= 0 && n_pairs <= INT32_MAX && p >= 0.f && p < 1.f;
}

}  // namespace

extern "C" {

DGMI_API size_t dgmi_pair_mlp_train_workspace_bytes(int64_t n_pairs) {
  if (n_pairs <= 0 || n_pairs > INT32_MAX) return 0;
  return train_plan(n_pairs).total;
}

DGMI_API int dgmi_pair_mlp_train_forward_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                             int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                             const float* w3, const float* b3, const int32_t* pair_query,
                                             const int32_t* pair_cand, int64_t n_pairs, float p, const int64_t* seed_dev,
                                             float* out_logit, int32_t* out_info, dgmi_stream_t stream) {
  if (!check_train_extents(h1, h2, n_query, n_cand, n_pairs, p)) return DGMI_ERR_INVALID_ARG;
  if (n_pairs == 0) return DGMI_OK;
  if (pair_query == nullptr || pair_cand == nullptr || seed_dev == nullptr || out_logit == nullptr || out_info == nullptr)
    return DGMI_ERR_INVALID_ARG;
  if (!check_pair_operands(X, ldx, C, ldc, W2, b2, w3, b3)) return DGMI_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(out_info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  const TrainPlan plan = train_plan(n_pairs);
  TrainArgs args{X, ldx, C, ldc, (int)n_query, (int)n_cand, W2, b2, w3, b3, pair_query, pair_cand, (int)n_pairs,
                 dgmi::pair_dropout_of(p), seed_dev, out_logit, out_info, nullptr, nullptr, 0, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(pair_train_forward_kernel, dim3((unsigned)plan.grid), dim3(kThreads), 0, s, args);
  return hipGetLastError() == hipSuccess ? DGMI_OK : DGMI_ERR_LAUNCH;
}

DGMI_API int dgmi_pair_mlp_train_backward_f32(const float* X, int64_t ldx, int64_t n_query, const float* C, int64_t ldc,
                                              int64_t n_cand, int32_t h1, int32_t h2, const float* W2, const float* b2,
                                              const float* w3, const float* b3, const int32_t* pair_query,
                                              const int32_t* pair_cand, int64_t n_pairs, float p, const int64_t* seed_dev,
                                              const float* dlogit, float* out_dz1, int64_t ld_dz1, float* out_dW2,
                                              float* out_db2, float* out_dw3, float* out_db3, int32_t* out_info,
                                              void* workspace, size_t workspace_bytes, dgmi_stream_t stream) {
  if (!check_train_extents(h1, h2, n_query, n_cand, n_pairs, p)) return DGMI_ERR_INVALID_ARG;
  if (out_dW2 == nullptr || out_db2 == nullptr || out_dw3 == nullptr || out_db3 == nullptr) return DGMI_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_pairs == 0) {
    if (hipMemsetAsync(out_dW2, 0, kW2Elems * sizeof(float), s) != hipSuccess || hipMemsetAsync(out_db2, 0, kH2 * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(out_dw3, 0, kH2 * sizeof(float), s) != hipSuccess || hipMemsetAsync(out_db3, 0, sizeof(float), s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
    return DGMI_OK;
  }
  if (pair_query == nullptr || pair_cand == nullptr || seed_dev == nullptr || dlogit == nullptr || out_dz1 == nullptr ||
      out_info == nullptr)
    return DGMI_ERR_INVALID_ARG;
  if (!check_pair_operands(X, ldx, C, ldc, W2, b2, w3, b3)) return DGMI_ERR_INVALID_ARG;
  if (ld_dz1 < kH1 || ld_dz1 % 4 != 0 || misaligned(out_dz1)) return DGMI_ERR_INVALID_ARG;
  const TrainPlan plan = train_plan(n_pairs);
  if (workspace == nullptr || workspace_bytes < plan.total || misaligned(workspace)) return DGMI_ERR_WORKSPACE;
  if (hipMemsetAsync(out_info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return DGMI_ERR_LAUNCH;
  char* ws = static_cast<char*>(workspace);
  TrainArgs args{X, ldx, C, ldc, (int)n_query, (int)n_cand, W2, b2, w3, b3, pair_query, pair_cand, (int)n_pairs,
                 dgmi::pair_dropout_of(p), seed_dev, nullptr, out_info, dlogit, out_dz1, ld_dz1,
                 reinterpret_cast<float*>(ws + plan.dz2), reinterpret_cast<float*>(ws + plan.part_w2),
                 reinterpret_cast<float*>(ws + plan.part_small)};
  hipLaunchKernelGGL(pair_train_backward_kernel, dim3((unsigned)plan.grid), dim3(kThreads), 0, s, args);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
  hipLaunchKernelGGL(pair_train_dw2_kernel, dim3((unsigned)plan.grid), dim3(kThreads), 0, s, args);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
  hipLaunchKernelGGL(pair_train_reduce_kernel, dim3((kReduceTotal + kReduceOuts - 1) / kReduceOuts), dim3(kReduceOuts * kReduceRuns),
                     0, s, args.part_w2, args.part_small, plan.grid, out_dW2, out_db2, out_dw3, out_db3);
  return hipGetLastError() == hipSuccess ? DGMI_OK : DGMI_ERR_LAUNCH;
}

}  // extern "C"

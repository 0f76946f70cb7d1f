// dgmi_pair_score.h — the decoder-MLP pair scorer shared by every pair kernel (gfx950): the global top-k of
// dgmi_pairs.hip, the per-row top-k of dgmi_pairs_rows.hip, the emit of dgmi_pairs_above.hip and the list scorer and
// count scan of dgmi_pairs_given.hip.  One place for the arithmetic, so that all return the same bits for the same pair.
// What else they share is in dgmi_pair_stream.h.
//
// A wave holds 32 "lane" rows (one per lane column; lane l keeps k = 64 (l >> 5) + s of row l & 31) and streams
// "stream" rows two at a time.  For stream row i the 64 x 32 block W2 . relu(S[i] + L[j0:j0+32]) is 2 x 64
// `v_mfma_f32_32x32x2_f32` (f32 in, f32 accumulate): A = W2 rows (lane l: row l & 31 of the half, k = 64 (l >> 5) + s
// at step s), B = relu(S[i, k] + L[j, k]).  Two stream rows x two row halves = 4 independent accumulators.  Epilogue:
// each lane sums w3[h] relu(acc + b2[h]) over its hb = 0 rows, then its hb = 1 rows, adds its partner lane (l ^ 32),
// then b3.  relu(S + L) is symmetric and f32 addition commutes, so which side streams does not change a logit's bits.
#ifndef DGMI_PAIR_SCORE_H_
#define DGMI_PAIR_SCORE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kH1 = 128;  // decoder hidden width 1 (layers.py:349)
constexpr int kH2 = 64;   // decoder hidden width 2 (layers.py:350)

typedef float floatx16 __attribute__((ext_vector_type(16)));

// order-preserving key of a logit: larger logit -> larger key; NaN -> 0, below every number; -0 == +0
__device__ __forceinline__ uint32_t order_key(float x) {
  if (x != x) return 0u;
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_logit(uint32_t f) {
  if (f == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((f & 0x80000000u) ? (f & 0x7fffffffu) : ~f);
}

// relu that keeps NaN (torch.relu does; fmaxf would drop it)
__device__ __forceinline__ float relu_nan(float x) { return x < 0.f ? 0.f : x; }

// The lane's constant operands: W2 rows col and 32 + col at k = 64 half + s, and its epilogue rows
// h = 32 hb + 8 (r >> 2) + 4 half + (r & 3).
struct PairDecoder {
  float wa[kH1 / 2], wb[kH1 / 2];
  float eb[2][16], ew[2][16];
  float bias3;
};

__device__ __forceinline__ void load_decoder(PairDecoder& d, const float* W2, const float* b2, const float* w3,
                                             const float* b3, int half, int col) {
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) {
    const float4 x = *reinterpret_cast<const float4*>(W2 + col * kH1 + 64 * half + 4 * s4);
    const float4 y = *reinterpret_cast<const float4*>(W2 + (32 + col) * kH1 + 64 * half + 4 * s4);
    d.wa[4 * s4] = x.x, d.wa[4 * s4 + 1] = x.y, d.wa[4 * s4 + 2] = x.z, d.wa[4 * s4 + 3] = x.w;
    d.wb[4 * s4] = y.x, d.wb[4 * s4 + 1] = y.y, d.wb[4 * s4 + 2] = y.z, d.wb[4 * s4 + 3] = y.w;
  }
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int h = 32 * hb + 8 * (r >> 2) + 4 * half + (r & 3);
      d.eb[hb][r] = b2[h];
      d.ew[hb][r] = w3[h];
    }
  d.bias3 = b3[0];
}

// The lane row's 64 values (k = 64 half + s) from global memory.
__device__ __forceinline__ void load_lane_row(float (&q)[kH1 / 2], const float* row, int half) {
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) {
    const float4 x = *reinterpret_cast<const float4*>(row + 64 * half + 4 * s4);
    q[4 * s4] = x.x, q[4 * s4 + 1] = x.y, q[4 * s4 + 2] = x.z, q[4 * s4 + 3] = x.w;
  }
}

// Logits of two stream rows against the wave's 32 lane rows: pa / pb point at this lane's 64-float half of each stream
// row (LDS, 16-B aligned), q holds the lane row's half.  Every lane of a column pair (l, l ^ 32) returns the same logit.
__device__ __forceinline__ void score_two(const float* pa, const float* pb, const float (&q)[kH1 / 2], const PairDecoder& d,
                                          float& la, float& lb) {
  floatx16 c00, c01, c10, c11;
#pragma unroll
  for (int v = 0; v < 16; ++v) c00[v] = c01[v] = c10[v] = c11[v] = 0.f;
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) {
    const float4 xa = *reinterpret_cast<const float4*>(pa + 4 * s4);
    const float4 xb = *reinterpret_cast<const float4*>(pb + 4 * s4);
    const float va[4] = {xa.x, xa.y, xa.z, xa.w}, vb[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = 4 * s4 + u;
      const float ba = relu_nan(va[u] + q[s]);
      const float bb = relu_nan(vb[u] + q[s]);
      c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(d.wa[s], ba, c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(d.wb[s], ba, c01, 0, 0, 0);
      c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(d.wa[s], bb, c10, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(d.wb[s], bb, c11, 0, 0, 0);
    }
  }
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    sa = fmaf(d.ew[0][r], relu_nan(c00[r] + d.eb[0][r]), sa);
    sb = fmaf(d.ew[0][r], relu_nan(c10[r] + d.eb[0][r]), sb);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    sa = fmaf(d.ew[1][r], relu_nan(c01[r] + d.eb[1][r]), sa);
    sb = fmaf(d.ew[1][r], relu_nan(c11[r] + d.eb[1][r]), sb);
  }
  la = (sa + __shfl_xor(sa, 32)) + d.bias3;
  lb = (sb + __shfl_xor(sb, 32)) + d.bias3;
}

// Logit of ONE stream row per call, two accumulators: score_two's row a, step for step (the same MFMA order per
// accumulator, the same epilogue order), so the bits are the same.  pa may differ from lane column to lane column: the
// operand B = relu(pa[k] + q[k]) is the lane's own, and column j's logit depends on column j's B alone.
__device__ __forceinline__ void score_one(const float* pa, const float (&q)[kH1 / 2], const PairDecoder& d, float& la) {
  floatx16 c00, c01;
#pragma unroll
  for (int v = 0; v < 16; ++v) c00[v] = c01[v] = 0.f;
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) {
    const float4 xa = *reinterpret_cast<const float4*>(pa + 4 * s4);
    const float va[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = 4 * s4 + u;
      const float ba = relu_nan(va[u] + q[s]);
      c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(d.wa[s], ba, c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(d.wb[s], ba, c01, 0, 0, 0);
    }
  }
  float sa = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) sa = fmaf(d.ew[0][r], relu_nan(c00[r] + d.eb[0][r]), sa);
#pragma unroll
  for (int r = 0; r < 16; ++r) sa = fmaf(d.ew[1][r], relu_nan(c01[r] + d.eb[1][r]), sa);
  la = (sa + __shfl_xor(sa, 32)) + d.bias3;
}

// known[(s, l)] -> bit l & 31 of word s * nwords + l / 32 (s: the streamed id, l: the lane id); an id outside its
// range sets info[1] and is skipped.  Vector atomics only.
__global__ __launch_bounds__(256) void known_bitmap_kernel(const int32_t* __restrict__ ks, const int32_t* __restrict__ kl,
                                                           int64_t n_known, int n_stream, int n_lane, int64_t nwords,
                                                           uint32_t* __restrict__ bitmap, int32_t* __restrict__ info) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_known; e += (int64_t)gridDim.x * 256) {
    const int32_t i = ks[e], j = kl[e];
    if (i < 0 || i >= n_stream || j < 0 || j >= n_lane) {
      atomicOr(&info[1], 1);
      continue;
    }
    atomicOr(&bitmap[(int64_t)i * nwords + (j >> 5)], 1u << (j & 31));
  }
}

}  // namespace

#endif  // DGMI_PAIR_SCORE_H_

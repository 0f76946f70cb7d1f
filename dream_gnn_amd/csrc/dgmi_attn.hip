// dgmi_attn.hip — the two-channel attention fusion of the encoder in training (gfx950): out = beta'_0 A + beta'_1 B in
// one kernel, every gradient from a recompute.  Contract: include/dgmi_attn.h; design: DESIGN.md 4.16.
//
// Layout.  A wave takes a TILE of 16 rows; lane = (n, g) = (lane & 15, lane >> 4) holds, of row n of BOTH tables, the
// float4 at columns 16 j + 4 g, j < ceil(F / 16): one 16-byte load per table and j.  The projection W1 z is
// `v_mfma_f32_16x16x4_f32` with the hidden units on M, the tile's rows on N and K over the columns, one accumulator tile
// per channel: A = W1[m = lane & 15][16 j + 4 g + u], B = z_c[n][16 j + 4 g + u], u = 0..3 (the K order is a permutation
// of the columns, the same on both operands).  The result has row n on the lane and hidden unit 4 g + r in register r, so
// tanh, * w2 and the sum over hidden units are 4 fmaf and two xor steps (16, 32); both channels of a row are in the same
// lane, so softmax and the weighted sum need nothing else.
//
// Backward, two launches:
//  1. attn_backward_kernel.  Pass 1 over j loads A, B and dout as above, runs the forward's projection and gate (the same
//     device functions, so h and beta are the forward's bits) and the two dots dout . z_c.  dpre_c (hidden 4 g + r of row
//     n in register r) IS the B operand of W1^T dpre_c with K = hidden: with A = W1[4 g + s][16 j + i] (a second LDS copy
//     of W1) the result tile holds columns 16 j + 4 g + r of row n, the float4 that pass 2 stores to dA / dB after adding
//     beta'_c dout.  dW1 += dpre_c^T z_c puts the ROWS on K: A = dpre_c[m][row 4 s + k] (through 2 KiB of LDS per wave),
//     B = z_c[row 4 s + k][16 j + i] re-read from cache in that layout; ceil(F / 16) accumulator tiles per wave live for
//     the whole launch.  db1 / dw2 are 8 registers per lane.
//  2. attn_reduce_kernel adds the workgroups' partials in workgroup order (sixteen runs, as pair_train_reduce_kernel).
// Sums.  Block b of 64 rows belongs to workgroup b mod grid; a wave adds its tiles in block order, the 16 rows of a tile
// are the MFMA's k chain (dW1) or a fixed xor tree (db1, dw2), a workgroup adds its four waves in wave order.  No float
// atomics: the same bits from run to run, the order a function of n_rows and F alone.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dgmi.h"
#include "dgmi_attn.h"

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kH = 16;            // hidden units of the projection
constexpr int kThreads = 256;     // four waves
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 16;         // rows of a wave's tile
constexpr int kBlockRows = DGMI_ATTN_BLOCK_ROWS;
constexpr int kMaxGrid = DGMI_ATTN_MAX_WORKGROUPS;
constexpr int kMaxF = 512;
static_assert(kBlockRows == kWaves * kTile, "a block is one tile per wave");

struct AttnArgs {
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  int n_rows, F;
  const float* W1;
  const float* b1;
  const float* w2;
  const float* M;  // (n_rows, 2) or null
  float* out;      // forward
  int64_t ldo;
  float* out_beta;
  const float* g;  // backward
  int64_t ldg;
  float* dA;
  int64_t ld_da;
  float* dB;
  int64_t ld_db;
  float* part;  // workspace: [grid][16 F + 32]
};

__device__ __forceinline__ int row_blocks(int n_rows) { return (int)(((int64_t)n_rows + kBlockRows - 1) / kBlockRows); }

__device__ __forceinline__ float4 load4(const float* p, bool ok) {
  return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// W1 as the A operand of the projection: entry (j, lane) = W1[lane & 15][16 j + 4 (lane >> 4) .. + 3], zeros past F
template <int NJ>
__device__ __forceinline__ void stage_w1(float4* w_lds, const float* W1, int F, int tid) {
  for (int idx = tid; idx < NJ * 64; idx += kThreads) {
    const int j = idx >> 6, l = idx & 63, col = 16 * j + 4 * (l >> 4);
    w_lds[idx] = load4(W1 + (int64_t)(l & 15) * F + col, col < F);
  }
}

// W1 as the A operand of W1^T dpre: entry (j, lane), component s = W1[4 (lane >> 4) + s][16 j + (lane & 15)]
template <int NJ>
__device__ __forceinline__ void stage_w1t(float4* wt_lds, const float* W1, int F, int tid) {
  for (int idx = tid; idx < NJ * 64; idx += kThreads) {
    const int j = idx >> 6, l = idx & 63, col = 16 * j + (l & 15), h = 4 * (l >> 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col < F) v = make_float4(W1[(h + 0) * F + col], W1[(h + 1) * F + col], W1[(h + 2) * F + col], W1[(h + 3) * F + col]);
    wt_lds[idx] = v;
  }
}

// four k steps of both channels' projections: columns 16 j + 4 g + u of W1 (w) and of the two rows (za, zb)
__device__ __forceinline__ void project_step(floatx4& acc0, floatx4& acc1, const float4 w, const float4 za, const float4 zb) {
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, za.x, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, zb.x, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, za.y, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, zb.y, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, za.z, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, zb.z, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, za.w, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, zb.w, acc1, 0, 0, 0);
}

struct Gate {
  float h[2][4];  // tanh of hidden unit 4 g + r, per channel
  float beta[2];  // softmax
  float bm[2];    // beta * M
};

// from the two projections to the weights of row n: every lane of the row gets the same bits (the xor sums are
// commutative pairs).  One sequence of single operations, shared by forward and backward.
__device__ __forceinline__ Gate gate(const floatx4 acc0, const floatx4 acc1, const float (&b1r)[4], const float (&w2r)[4],
                                     float m0, float m1) {
  Gate q;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    q.h[0][r] = tanhf(acc0[r] + b1r[r]);
    q.h[1][r] = tanhf(acc1[r] + b1r[r]);
    s0 = fmaf(w2r[r], q.h[0][r], s0);
    s1 = fmaf(w2r[r], q.h[1][r], s1);
  }
  s0 += __shfl_xor(s0, 16);
  s1 += __shfl_xor(s1, 16);
  s0 += __shfl_xor(s0, 32);
  s1 += __shfl_xor(s1, 32);
  const float mx = fmaxf(s0, s1);
  const float e0 = expf(s0 - mx), e1 = expf(s1 - mx);
  const float den = e0 + e1;
  q.beta[0] = e0 / den;
  q.beta[1] = e1 / den;
  q.bm[0] = q.beta[0] * m0;
  q.bm[1] = q.beta[1] * m1;
  return q;
}

__device__ __forceinline__ float4 weighted(float b0, const float4 a, float b1, const float4 b) {
  return make_float4(fmaf(b1, b.x, b0 * a.x), fmaf(b1, b.y, b0 * a.y), fmaf(b1, b.z, b0 * a.z), fmaf(b1, b.w, b0 * a.w));
}

template <int NJ>
__global__ __launch_bounds__(kThreads) void attn_forward_kernel(AttnArgs a) {
  __shared__ float4 w_lds[NJ * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  stage_w1<NJ>(w_lds, a.W1, a.F, tid);
  float b1r[4], w2r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) b1r[r] = a.b1[4 * g + r], w2r[r] = a.w2[4 * g + r];
  __syncthreads();

  const int n_blocks = row_blocks(a.n_rows);
  for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t row = (int64_t)b * kBlockRows + wave * kTile + n;
    const bool valid = row < a.n_rows;
    const float* pa = a.A + row * a.lda + 4 * g;
    const float* pb = a.B + row * a.ldb + 4 * g;
    float4 za[NJ], zb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const bool ok = valid && 16 * j + 4 * g < a.F;
      za[j] = load4(pa + 16 * j, ok);
      zb[j] = load4(pb + 16 * j, ok);
    }
    float m0 = 1.f, m1 = 1.f;
    if (valid && a.M != nullptr) m0 = a.M[2 * row], m1 = a.M[2 * row + 1];
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (16 * j < a.F) project_step(acc0, acc1, w_lds[j * 64 + lane], za[j], zb[j]);
    }
    const Gate q = gate(acc0, acc1, b1r, w2r, m0, m1);
    float* po = a.out + row * a.ldo + 4 * g;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (valid && 16 * j + 4 * g < a.F) *reinterpret_cast<float4*>(po + 16 * j) = weighted(q.bm[0], za[j], q.bm[1], zb[j]);
    if (valid && g == 0) *reinterpret_cast<float2*>(a.out_beta + 2 * row) = make_float2(q.bm[0], q.bm[1]);
  }
}

// sum over the 16 rows of a tile (the lanes of one g): a fixed xor tree
__device__ __forceinline__ float tile_sum(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

template <int NJ>
__global__ __launch_bounds__(kThreads) void attn_backward_kernel(AttnArgs a) {
  __shared__ float4 w_lds[NJ * 64];
  __shared__ float4 wt_lds[NJ * 64];            // after the row loop: the workgroup's dW1, [16][16 NJ]
  __shared__ float dp_lds[kWaves][2][kH][kTile + 1];  // dpre_c[hidden][row of the tile], per wave
  __shared__ float red[kWaves][2 * kH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  stage_w1<NJ>(w_lds, a.W1, a.F, tid);
  stage_w1t<NJ>(wt_lds, a.W1, a.F, tid);
  float b1r[4], w2r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) b1r[r] = a.b1[4 * g + r], w2r[r] = a.w2[4 * g + r];

  floatx4 acc_w[NJ];  // dW1[4 g + r][16 j + n], this wave's rows
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc_w[j] = floatx4{0.f, 0.f, 0.f, 0.f};
  float s_db1[4] = {0.f, 0.f, 0.f, 0.f}, s_dw2[4] = {0.f, 0.f, 0.f, 0.f};  // hidden 4 g + r, this lane's rows

  const int n_blocks = row_blocks(a.n_rows);
  for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t row0 = (int64_t)b * kBlockRows + wave * kTile, row = row0 + n;
    const bool valid = row < a.n_rows;
    const float* pa = a.A + row * a.lda + 4 * g;
    const float* pb = a.B + row * a.ldb + 4 * g;
    const float* pg = a.g + row * a.ldg + 4 * g;
    float m0 = 1.f, m1 = 1.f;
    if (valid && a.M != nullptr) m0 = a.M[2 * row], m1 = a.M[2 * row + 1];
    __syncthreads();  // first block: the LDS copies of W1 are written; later: the previous block's readers of dp_lds are done

    // pass 1: the forward's projection and gate, and dout . z_c
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (16 * j >= a.F) continue;
      const bool ok = valid && 16 * j + 4 * g < a.F;
      const float4 za = load4(pa + 16 * j, ok), zb = load4(pb + 16 * j, ok), gg = load4(pg + 16 * j, ok);
      d0 = fmaf(gg.w, za.w, fmaf(gg.z, za.z, fmaf(gg.y, za.y, fmaf(gg.x, za.x, d0))));
      d1 = fmaf(gg.w, zb.w, fmaf(gg.z, zb.z, fmaf(gg.y, zb.y, fmaf(gg.x, zb.x, d1))));
      project_step(acc0, acc1, w_lds[j * 64 + lane], za, zb);
    }
    const Gate q = gate(acc0, acc1, b1r, w2r, m0, m1);
    d0 += __shfl_xor(d0, 16);
    d1 += __shfl_xor(d1, 16);
    d0 += __shfl_xor(d0, 32);
    d1 += __shfl_xor(d1, 32);
    const float db0 = m0 * d0, db1 = m1 * d1;
    const float dot = fmaf(q.beta[1], db1, q.beta[0] * db0);
    const float ds0 = valid ? q.beta[0] * (db0 - dot) : 0.f, ds1 = valid ? q.beta[1] * (db1 - dot) : 0.f;
    float dp0[4], dp1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dp0[r] = (ds0 * w2r[r]) * fmaf(-q.h[0][r], q.h[0][r], 1.f);
      dp1[r] = (ds1 * w2r[r]) * fmaf(-q.h[1][r], q.h[1][r], 1.f);
      s_db1[r] += dp0[r] + dp1[r];
      s_dw2[r] += fmaf(ds1, q.h[1][r], ds0 * q.h[0][r]);
      dp_lds[wave][0][4 * g + r][n] = dp0[r];
      dp_lds[wave][1][4 * g + r][n] = dp1[r];
    }
    __syncthreads();
    float ta[2][4];  // dpre_c[hidden n][row 4 s + g of the tile]: the A operand of dW1's step s
#pragma unroll
    for (int s = 0; s < 4; ++s) ta[0][s] = dp_lds[wave][0][n][4 * s + g], ta[1][s] = dp_lds[wave][1][n][4 * s + g];

    // pass 2: dA / dB rows and the dW1 tiles
    float* pda = a.dA + row * a.ld_da + 4 * g;
    float* pdb = a.dB + row * a.ld_db + 4 * g;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (16 * j >= a.F) continue;
      const bool ok = valid && 16 * j + 4 * g < a.F;
      const float4 gg = load4(pg + 16 * j, ok);
      const float4 wt = wt_lds[j * 64 + lane];
      floatx4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
      t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt.x, dp0[0], t0, 0, 0, 0);
      t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt.x, dp1[0], t1, 0, 0, 0);
      t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt.y, dp0[1], t0, 0, 0, 0);
      t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt.y, dp1[1], t1, 0, 0, 0);
      t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt.z, dp0[2], t0, 0, 0, 0);
      t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt.z, dp1[2], t1, 0, 0, 0);
      t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt.w, dp0[3], t0, 0, 0, 0);
      t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt.w, dp1[3], t1, 0, 0, 0);
      if (ok) {
        *reinterpret_cast<float4*>(pda + 16 * j) =
            make_float4(fmaf(q.bm[0], gg.x, t0[0]), fmaf(q.bm[0], gg.y, t0[1]), fmaf(q.bm[0], gg.z, t0[2]), fmaf(q.bm[0], gg.w, t0[3]));
        *reinterpret_cast<float4*>(pdb + 16 * j) =
            make_float4(fmaf(q.bm[1], gg.x, t1[0]), fmaf(q.bm[1], gg.y, t1[1]), fmaf(q.bm[1], gg.z, t1[2]), fmaf(q.bm[1], gg.w, t1[3]));
      }
      // rows on K: lane (i, k) = (n, g) reads column 16 j + i of row 4 s + k of the tile
      const int col = 16 * j + n;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int64_t r2 = row0 + 4 * s + g;
        const bool okz = r2 < a.n_rows && col < a.F;
        const float z0 = okz ? a.A[r2 * a.lda + col] : 0.f, z1 = okz ? a.B[r2 * a.ldb + col] : 0.f;
        acc_w[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[0][s], z0, acc_w[j], 0, 0, 0);
        acc_w[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[1][s], z1, acc_w[j], 0, 0, 0);
      }
    }
  }

  // this workgroup's partial: rows of a tile (xor tree), then the four waves in order
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float sb = tile_sum(s_db1[r]), sw = tile_sum(s_dw2[r]);
    if (n == 0) red[wave][4 * g + r] = sb, red[wave][kH + 4 * g + r] = sw;
  }
  __syncthreads();  // every wave has left the row loop: wt_lds is free
  float* const part_lds = reinterpret_cast<float*>(wt_lds);
  for (int w = 0; w < kWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int idx = (4 * g + r) * (16 * NJ) + 16 * j + n;
          part_lds[idx] = w == 0 ? acc_w[j][r] : part_lds[idx] + acc_w[j][r];
        }
    }
    __syncthreads();
  }
  float* const dst = a.part + (int64_t)blockIdx.x * (kH * a.F + 2 * kH);
  for (int i = tid; i < kH * a.F; i += kThreads) dst[i] = part_lds[(i / a.F) * (16 * NJ) + i % a.F];
  if (tid < 2 * kH) dst[kH * a.F + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// out = the sum of the workgroups' partials in workgroup order, as pair_train_reduce_kernel: a workgroup owns
// kReduceOuts outputs, thread (run, o) adds the run-th sixteenth of output o's partials in order, then one thread per
// output adds the sixteen runs in order.  Output i < 16 F is dW1[i], then db1, then dw2.
constexpr int kReduceOuts = 16, kReduceRuns = 16;

__global__ __launch_bounds__(kReduceOuts* kReduceRuns) void attn_reduce_kernel(const float* __restrict__ part, int n_parts, int F,
                                                                              float* __restrict__ dW1, float* __restrict__ db1,
                                                                              float* __restrict__ dw2) {
  __shared__ float red[kReduceRuns][kReduceOuts];
  const int o = threadIdx.x % kReduceOuts, run = threadIdx.x / kReduceOuts;
  const int i = (int)blockIdx.x * kReduceOuts + o;
  const int total = kH * F + 2 * kH;
  const float* src = part + i;
  const int per = (n_parts + kReduceRuns - 1) / kReduceRuns;
  const int g0 = run * per < n_parts ? run * per : n_parts, g1 = g0 + per < n_parts ? g0 + per : n_parts;
  float s = 0.f;
  if (i < total) {
    int g = g0;
    for (; g + 16 <= g1; g += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = src[(int64_t)(g + u) * total];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; g < g1; ++g) s += src[(int64_t)g * total];
  }
  red[run][o] = s;
  __syncthreads();
  if (run == 0 && i < total) {
    float sum = red[0][o];
    for (int r = 1; r < kReduceRuns; ++r) sum += red[r][o];
    if (i < kH * F) dW1[i] = sum;
    else if (i < kH * F + kH) db1[i - kH * F] = sum;
    else dw2[i - kH * F - kH] = sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
bool bad_ld(int64_t ld, int32_t F) { return ld < F || ld % 4 != 0; }

int grid_of(int64_t n_rows) {
  const int64_t n_blocks = (n_rows + kBlockRows - 1) / kBlockRows;
  return (int)(n_blocks < kMaxGrid ? n_blocks : kMaxGrid);
}

bool check_extents(int64_t n_rows, int32_t F, int32_t H) {
  return H == kH && F >= 4 && F <= kMaxF && F % 4 == 0 && n_rows >= 0 && n_rows <= INT32_MAX;
}

// the bytes [p, p + extent of an (n_rows, F) table with leading dimension ld) against the same of q
bool overlaps(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t n_rows, int32_t F) {
  if (p == q) return true;
  if (n_rows == 0) return false;
  const float* pe = p + (n_rows - 1) * ldp + F;
  const float* qe = q + (n_rows - 1) * ldq + F;
  return reinterpret_cast<uintptr_t>(p) < reinterpret_cast<uintptr_t>(qe) && reinterpret_cast<uintptr_t>(q) < reinterpret_cast<uintptr_t>(pe);
}

bool check_operands(const float* A, int64_t lda, const float* B, int64_t ldb, int32_t F, const float* W1, const float* b1,
                    const float* w2) {
  if (A == nullptr || B == nullptr || W1 == nullptr || b1 == nullptr || w2 == nullptr) return false;
  if (bad_ld(lda, F) || bad_ld(ldb, F)) return false;
  return !misaligned(A) && !misaligned(B) && !misaligned(W1);
}

template <template <int> class Launch, typename... Args>
void by_width(int F, Args&&... args) {
  if (F <= 32) Launch<2>::run(args...);
  else if (F <= 128) Launch<8>::run(args...);
  else if (F <= 256) Launch<16>::run(args...);
  else Launch<32>::run(args...);
}

template <int NJ>
struct LaunchForward {
  static void run(int grid, hipStream_t s, const AttnArgs& args) {
    hipLaunchKernelGGL(attn_forward_kernel<NJ>, dim3((unsigned)grid), dim3(kThreads), 0, s, args);
  }
};

template <int NJ>
struct LaunchBackward {
  static void run(int grid, hipStream_t s, const AttnArgs& args) {
    hipLaunchKernelGGL(attn_backward_kernel<NJ>, dim3((unsigned)grid), dim3(kThreads), 0, s, args);
  }
};

}  // namespace

extern "C" {

DGMI_API size_t dgmi_attn_fuse_workspace_bytes(int64_t n_rows, int32_t F) {
  if (n_rows <= 0 || n_rows > INT32_MAX || F < 4 || F > kMaxF || F % 4 != 0) return 0;
  return align_up((size_t)grid_of(n_rows) * (size_t)(kH * F + 2 * kH) * sizeof(float));
}

DGMI_API int dgmi_attn_fuse_forward_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n_rows, int32_t F,
                                        int32_t H, const float* W1, const float* b1, const float* w2, const float* M,
                                        float* out, int64_t ldo, float* out_beta, dgmi_stream_t stream) {
  if (!check_extents(n_rows, F, H) || !check_operands(A, lda, B, ldb, F, W1, b1, w2)) return DGMI_ERR_INVALID_ARG;
  if (out == nullptr || out_beta == nullptr || bad_ld(ldo, F) || misaligned(out)) return DGMI_ERR_INVALID_ARG;
  if (overlaps(out, ldo, A, lda, n_rows, F) || overlaps(out, ldo, B, ldb, n_rows, F)) return DGMI_ERR_INVALID_ARG;
  if (n_rows == 0) return DGMI_OK;
  AttnArgs args{A, lda, B, ldb, (int)n_rows, F, W1, b1, w2, M, out, ldo, out_beta, nullptr, 0, nullptr, 0, nullptr, 0, nullptr};
  by_width<LaunchForward>(F, grid_of(n_rows), static_cast<hipStream_t>(stream), args);
  return hipGetLastError() == hipSuccess ? DGMI_OK : DGMI_ERR_LAUNCH;
}

DGMI_API int dgmi_attn_fuse_backward_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n_rows, int32_t F,
                                         int32_t H, const float* W1, const float* b1, const float* w2, const float* M,
                                         const float* dout, int64_t ldg, float* out_dA, int64_t ld_da, float* out_dB,
                                         int64_t ld_db, float* out_dW1, float* out_db1, float* out_dw2, void* workspace,
                                         size_t workspace_bytes, dgmi_stream_t stream) {
  if (!check_extents(n_rows, F, H) || !check_operands(A, lda, B, ldb, F, W1, b1, w2)) return DGMI_ERR_INVALID_ARG;
  if (dout == nullptr || out_dA == nullptr || out_dB == nullptr || out_dW1 == nullptr || out_db1 == nullptr || out_dw2 == nullptr)
    return DGMI_ERR_INVALID_ARG;
  if (bad_ld(ldg, F) || bad_ld(ld_da, F) || bad_ld(ld_db, F) || misaligned(dout) || misaligned(out_dA) || misaligned(out_dB))
    return DGMI_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_rows == 0) {
    if (hipMemsetAsync(out_dW1, 0, (size_t)kH * F * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(out_db1, 0, kH * sizeof(float), s) != hipSuccess || hipMemsetAsync(out_dw2, 0, kH * sizeof(float), s) != hipSuccess)
      return DGMI_ERR_LAUNCH;
    return DGMI_OK;
  }
  const int grid = grid_of(n_rows);
  if (workspace == nullptr || workspace_bytes < dgmi_attn_fuse_workspace_bytes(n_rows, F) || misaligned(workspace))
    return DGMI_ERR_WORKSPACE;
  AttnArgs args{A, lda, B, ldb, (int)n_rows, F, W1, b1, w2, M, nullptr, 0, nullptr, dout, ldg, out_dA, ld_da, out_dB, ld_db,
                static_cast<float*>(workspace)};
  by_width<LaunchBackward>(F, grid, s, args);
  if (hipGetLastError() != hipSuccess) return DGMI_ERR_LAUNCH;
  const int total = kH * F + 2 * kH;
  hipLaunchKernelGGL(attn_reduce_kernel, dim3((unsigned)((total + kReduceOuts - 1) / kReduceOuts)), dim3(kReduceOuts * kReduceRuns),
                     0, s, static_cast<const float*>(workspace), grid, (int)F, out_dW1, out_db1, out_dw2);
  return hipGetLastError() == hipSuccess ? DGMI_OK : DGMI_ERR_LAUNCH;
}

}  // extern "C"

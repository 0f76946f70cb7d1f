// dgmi_sliced_bf16.hip — the bf16 copy of a feature table that the XCD-local SpMM (dgmi_sliced.hip, dgmi_owned.hip) may
// gather from instead of the fp32 one.  The table is made by ONE streaming pass (rows_to_bf16_kernel) that also applies
// the source scale, in fp32, before the single round-to-nearest-even:
//
//   xb[j]  = bf16_rne(src_scale[j] * X[j])
//   Y[i]   = dst_scale[i] * sum_{e: dst(e) = i} w_e * float(xb[src(e)])          (products, sums, planes, Y: fp32)
//
// The gather kernels have no source-scale form for such a table: the scale belongs to this pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dgmi_sliced_common.h"

namespace dgmi {
namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));

// two fp32 -> one dword of two bf16, round-to-nearest-even (v_cvt_pk_bf16_f32); element 0 in the low half
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
  const v2f f = {lo, hi};
  const v2bf b = __builtin_convertvector(f, v2bf);
  return __builtin_bit_cast(uint32_t, b);
}

// out[r, :] = bf16_rne(scale[r] * X[r, :]); one thread per 8 columns: two 16-B loads, one 16-B store
template <bool HAS_SCALE>
__global__ __launch_bounds__(256) void rows_to_bf16_kernel(const float* __restrict__ X, int64_t ldx,
                                                           const float* __restrict__ scale, int64_t n, int F8,
                                                           uint16_t* __restrict__ out, int64_t ldo) {
  const int64_t total = n * F8;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const int64_t row = t / F8;
    const int c = (int)(t - row * F8) * 8;
    const float* src = X + row * ldx + c;
    float4 a = ld4(src), b = ld4(src + 4);
    if (HAS_SCALE) {
      const float s = scale[row];
      a.x *= s, a.y *= s, a.z *= s, a.w *= s;
      b.x *= s, b.y *= s, b.z *= s, b.w *= s;
    }
    const v4u o = {pack_bf16(a.x, a.y), pack_bf16(a.z, a.w), pack_bf16(b.x, b.y), pack_bf16(b.z, b.w)};
    *reinterpret_cast<v4u*>(out + row * ldo + c) = o;
  }
}

}  // namespace

hipError_t rows_to_bf16(const float* X, int64_t ldx, const float* scale, int64_t n, int64_t F, uint16_t* out, int64_t ldo,
                        hipStream_t s) {
  if (n == 0 || F == 0) return hipSuccess;
  const int F8 = (int)(F / 8);
  int64_t blocks = (n * F8 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (scale != nullptr)
    hipLaunchKernelGGL(rows_to_bf16_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, X, ldx, scale, n, F8, out, ldo);
  else
    hipLaunchKernelGGL(rows_to_bf16_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, X, ldx, scale, n, F8, out, ldo);
  return hipGetLastError();
}

}  // namespace dgmi

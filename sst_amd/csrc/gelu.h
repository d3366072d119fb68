// The epilogues of the tall linear layers (csrc/dense_f32.hip, dense_f32x3.hip, dense_f32x6.hip, dense_bf16.hip) and of the
// one-kernel encoder tails (csrc/layer_tail_x6.hip, layer_tail_bf16.hip): their codes and the GELU they all evaluate the same way.
#pragma once
#include <math.h>
#include "common.h"

namespace {

// the `epilogue` argument of the C ABI (include/sst_amd.h): the values must not move.  Not every kernel builds every epilogue.
// kEpiAddRows: + aux_in[row_index[row]] (ln.pos_idx; negative -> row 0): the split-weight VFE layer (csrc/dense_f32x6.hip)
enum { kEpiBias = 0, kEpiGelu = 1, kEpiRelu = 2, kEpiMulGeluGrad = 3, kEpiMulReluGrad = 4, kEpiAdd = 5, kEpiAddLN = 6,
       kEpiAddRows = 7 };

// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far below the bf16 resolution of every reduced-precision consumer):
// one reciprocal, one exponential and five FMAs instead of the ~40 instructions of the library's erff.
// e = exp(-z^2) is returned too: the GELU derivative needs exp(-x^2 / 2) = e at z = x / sqrt(2).
__device__ __forceinline__ float erf_as(float z, float& e) {
  const float az = fabsf(z);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.f));
  e = __expf(-az * az);
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  return copysignf(fmaf(-poly, e, 1.f), z);
}
__device__ __forceinline__ float gelu_f(float x) {
  float e;
  return 0.5f * x * (1.f + erf_as(x * 0.70710678118654752f, e));
}
__device__ __forceinline__ float gelu_grad_f(float x) {
  float e;
  const float phi = 0.5f * (1.f + erf_as(x * 0.70710678118654752f, e));
  return fmaf(x * 0.3989422804014327f, e, phi);
}
// gelu_f(x) (returned) and gelu_grad_f(x) (grad) from ONE erf_as evaluation, each with the bits of its own function: both are
// formed from the same s = 1 + erf by the operations those functions apply to it - (0.5 x) s and fma(x / sqrt(2 pi), e, 0.5 s).
// The products are rounded on their own (__fmul_rn is never contracted), the one fused operation is spelled out, so the
// combined expression leaves the compiler nothing to contract differently from the two separate ones.
__device__ __forceinline__ float gelu_with_grad_f(float x, float& grad) {
  float e;
  const float s = 1.f + erf_as(x * 0.70710678118654752f, e);
  grad = fmaf(__fmul_rn(x, 0.3989422804014327f), e, __fmul_rn(0.5f, s));
  return __fmul_rn(__fmul_rn(0.5f, x), s);
}

}  // namespace

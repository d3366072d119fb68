// torch's fp32 floor division (c10::div_floor_floating) restated operation by operation, shared by the incremental point
// stage (incremental.hip) and the class-batched cluster keys (cluster_classes.hip).  The files that include it are built
// without floating-point contraction (Makefile): every operation below is rounded on its own.
#pragma once
#include <math.h>
#include "common.h"

namespace {

// torch.div(p - lo, vs, rounding_mode='floor').int() of one fp32 element (vs > 0)
__device__ __forceinline__ int32_t floor_div_coor(float p, float lo, float vs) {
  const float a = __fsub_rn(p, lo);
  const float mod = fmodf(a, vs);
  float div = __fdiv_rn(__fsub_rn(a, mod), vs);
  if (mod != 0.f && ((vs < 0.f) != (mod < 0.f))) div = __fsub_rn(div, 1.f);
  float fd;
  if (div != 0.f) {
    fd = floorf(div);
    if (__fsub_rn(div, fd) > 0.5f) fd = __fadd_rn(fd, 1.f);
  } else {
    fd = copysignf(0.f, __fdiv_rn(a, vs));
  }
  return (int32_t)fd;
}

}  // namespace

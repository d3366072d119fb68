// The point-in-box test of the reference's points-in-boxes kernels (ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-50),
// shared by the dynamic point pool (point_pool.hip) and the points-in-boxes entry point (box_ops.hip): both must answer
// the same question with the same operations, and point_pool.hip's results are pinned to the reference's compiled
// points_in_boxes_cpu.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct DppBox {
  float cx, cy, cz;  // centre (cz lifted from the bottom face)
  float w, l, h;
  float cosa, sina;
  float lw, ll, lh;  // enlarged extents
};

__device__ __forceinline__ DppBox dpp_box(const float* __restrict__ roi, float ew, float el, float eh) {
  DppBox b;
  b.cx = roi[0];
  b.cy = roi[1];
  b.w = roi[3];
  b.l = roi[4];
  b.h = roi[5];
  b.cz = __fadd_rn(roi[2], __fmul_rn(b.h, 0.5f));
  // points_in_boxes_cuda.cu:28-29: the angle is formed in double (M_PI), then used as a float
  const float rot = (float)((double)roi[6] + 1.57079632679489661923);
  b.cosa = cosf(rot);
  b.sina = sinf(rot);
  b.lw = __fadd_rn(b.w, ew);
  b.ll = __fadd_rn(b.l, el);
  b.lh = __fadd_rn(b.h, eh);
  return b;
}

// 0 = outside the enlarged box, 1 = inside the box proper, 2 = only inside the enlarged box (the margin).
// No fused multiply-add: the products and sums round one by one, as a restatement in numpy does.
__device__ __forceinline__ int dpp_classify(const DppBox& b, float x, float y, float z, float& lx, float& ly,
                                            float& lz) {
  lz = __fsub_rn(z, b.cz);
  const float sx = __fsub_rn(x, b.cx), sy = __fsub_rn(y, b.cy);
  lx = __fadd_rn(__fmul_rn(sx, b.cosa), __fmul_rn(sy, -b.sina));  // points_in_boxes_cuda.cu:30-31
  ly = __fadd_rn(__fmul_rn(sx, b.sina), __fmul_rn(sy, b.cosa));
  const float hl = __fmul_rn(b.ll, 0.5f), hw = __fmul_rn(b.lw, 0.5f), hh = __fmul_rn(b.lh, 0.5f);
  if (fabsf(lz) > hh || !(lx > -hl && lx < hl && ly > -hw && ly < hw)) return 0;
  const float sl = __fmul_rn(b.l, 0.5f), sw = __fmul_rn(b.w, 0.5f), sh = __fmul_rn(b.h, 0.5f);
  const bool inner = !(fabsf(lz) > sh) && lx > -sl && lx < sl && ly > -sw && ly < sw;  // :45-48
  return inner ? 1 : 2;
}

}  // namespace

// The regression target of one positive RoI and the 3-D IoU of one box pair, shared by the RoI head (roi_head.hip) and the
// tracklet targets (tracklet.hip).  Every file that includes this header is built without floating-point contraction
// (Makefile): the IoU has to equal that of the box ops bit for bit, and the target follows the reference's fp32 operation order.
#pragma once
#include "bev_clip.h"
#include "head_math.h"

namespace {

// torch.remainder(x, m) for m > 0
__device__ __forceinline__ float py_mod(float x, float m) {
  float r = fmodf(x, m);
  if (r != 0.f && r < 0.f) r += m;
  return r;
}

// _get_target_single for one positive RoI and its box (fsd_bbox_head.py:420-447)
__device__ __forceinline__ void roi_target_row(const float* roi, const float* g, float* t) {
  const float roi_ry = py_mod(roi[6], kTwoPi);
  const float cx = g[0] - roi[0], cy = g[1] - roi[1], cz = g[2] - roi[2];
  const float cr = g[6] - roi_ry;
  const float ang = -(roi_ry + kHalfPi);
  const float sn = sinf(ang), cs = cosf(ang);
  const float x = cx * cs + cy * sn, y = cy * cs - cx * sn;
  float ry = py_mod(cr, kTwoPi);
  if (ry > kHalfPi && ry < kPi * 1.5f) ry = py_mod(ry + kPi, kTwoPi);
  if (ry > kPi) ry = ry - kTwoPi;
  ry = fminf(fmaxf(ry, -kHalfPi), kHalfPi);
  // DeltaXYZWLHRBBoxCoder.encode against the anchor (0, 0, 0, w, l, h, 0)
  const float wa = roi[3], la = roi[4], ha = roi[5];
  const float za = ha / 2, zg = cz + g[5] / 2;
  const float diag = sqrtf(la * la + wa * wa);
  t[0] = x / diag;
  t[1] = y / diag;
  t[2] = (zg - za) / ha;
  t[3] = logf(g[3] / wa);
  t[4] = logf(g[4] / la);
  t[5] = logf(g[5] / ha);
  t[6] = ry;
}

// LiDARInstance3DBoxes.aligned_iou_3d of one pair of [x, y, z_bottom, w, l, h, ry] boxes (lidar_box3d.py:404-450): the BEV
// overlap of bev_clip.h on xywhr2xyxyr(bev) x the clamped height overlap, over the clamped union of the volumes.  The same
// operation sequence as the rows of sst_roi_assign_f32 and as box_ops.boxes3d_overlaps_lidar.  lx / ly / lk: this thread's
// column of a [kPolyCap][kPolyBlock] LDS polygon array.
__device__ __forceinline__ float lidar_iou3d_pair(const float* a, const float* b, float* lx, float* ly, float* lk) {
  float pa[5], pb[5];
  const float ahw = a[3] / 2, ahl = a[4] / 2, bhw = b[3] / 2, bhl = b[4] / 2;
  pa[0] = a[0] - ahw;
  pa[1] = a[1] - ahl;
  pa[2] = a[0] + ahw;
  pa[3] = a[1] + ahl;
  pa[4] = a[6];
  pb[0] = b[0] - bhw;
  pb[1] = b[1] - bhl;
  pb[2] = b[0] + bhw;
  pb[3] = b[1] + bhl;
  pb[4] = b[6];
  const float oh = fmaxf(fminf(a[2] + a[5], b[2] + b[5]) - fmaxf(a[2], b[2]), 0.f);
  const float o3 = bev_overlap(pa, pb, lx, ly, lk) * oh;
  const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
  return o3 / fmaxf(va + vb - o3, 1e-8f);
}

}  // namespace

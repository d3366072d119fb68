// The rotated BEV overlap of two boxes [x1, y1, x2, y2, ry]: the polygon arithmetic shared by the box ops (box_ops.hip) and
// the RoI head's assignment (roi_head.hip).  It restates the reference's iou3d kernels (ops/iou3d/src/iou3d_kernel.cu:54-251):
// corners rotated about the centre (rotate_around_center), edge intersections with strict sign tests and the EPS fallback
// (intersection), corners of one box inside the other with a 1e-5 margin (check_in_box2d), points sorted by atan2 about their
// mean, area as a fan from vertex 0.  The polygon points live in LDS (per-thread columns of a [slot][lane] array of kPolyBlock
// lanes), so the dynamically indexed lists never spill to scratch.  Every translation unit that includes this header is built
// without floating-point contraction (Makefile), so that every product and sum rounds on its own.
#pragma once

namespace {

constexpr float kIouEps = 1e-8f;      // iou3d_kernel.cu:15
constexpr float kInBoxMargin = 1e-5f; // check_in_box2d
constexpr int kPolyCap = 16;          // the reference's cross_points[16]; a 17th point (only from rounding at a vertex) is dropped
constexpr int kPolyBlock = 64;        // threads of every polygon kernel: one wave, 64 x 16 x 12 B = 12 KB of LDS

struct Pt {
  float x, y;
};

__device__ __forceinline__ float cross3(const Pt& p1, const Pt& p2, const Pt& p0) {
  return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__device__ __forceinline__ bool rect_cross(const Pt& p1, const Pt& p2, const Pt& q1, const Pt& q2) {
  return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
         fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

// edge p0 -> p1 against edge q0 -> q1 (iou3d_kernel.cu:79-109)
__device__ __forceinline__ bool edge_cross(const Pt& p1, const Pt& p0, const Pt& q1, const Pt& q0, Pt& ans) {
  if (!rect_cross(p0, p1, q0, q1)) return false;
  const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0);
  const float s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
  const float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > kIouEps) {
    ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float d = a0 * b1 - a1 * b0;
    ans.x = (b0 * c1 - b1 * c0) / d;
    ans.y = (a1 * c0 - a0 * c1) / d;
  }
  return true;
}

// rotate_around_center (iou3d_kernel.cu:111-119): x' = dx cos + dy sin + cx, y' = -dx sin + dy cos + cy
__device__ __forceinline__ Pt rotate_about(const Pt& c, float cs, float sn, float x, float y) {
  const float dx = x - c.x, dy = y - c.y;
  Pt r;
  r.x = dx * cs + dy * sn + c.x;
  r.y = -dx * sn + dy * cs + c.y;
  return r;
}

// check_in_box2d (iou3d_kernel.cu:54-77); cs / sn = cos / sin of -angle
__device__ __forceinline__ bool in_box(const float* b, const Pt& c, float cs, float sn, const Pt& p) {
  const Pt r = rotate_about(c, cs, sn, p.x, p.y);
  return r.x > b[0] - kInBoxMargin && r.x < b[2] + kInBoxMargin && r.y > b[1] - kInBoxMargin &&
         r.y < b[3] + kInBoxMargin;
}

// Overlap area of two boxes [x1, y1, x2, y2, ry] (box_overlap, iou3d_kernel.cu:127-242).  lx / ly / lk: this
// thread's column of the LDS polygon arrays (slot s at [s * kPolyBlock]).
__device__ __forceinline__ float bev_overlap(const float* a, const float* b, float* lx, float* ly, float* lk) {
  const Pt ca = {(a[0] + a[2]) / 2, (a[1] + a[3]) / 2};
  const Pt cb = {(b[0] + b[2]) / 2, (b[1] + b[3]) / 2};
  const float wa = a[2] - a[0], ha = a[3] - a[1], wb = b[2] - b[0], hb = b[3] - b[1];
  // Early out: boxes whose circumscribed circles are apart by more than 1 cm (+0.1 % of the radii) have no crossing
  // edges and no corner within the 1e-5 margin of the other box, so the full algorithm returns 0 for them as well.
  {
    const float r = 0.5f * (sqrtf(wa * wa + ha * ha) + sqrtf(wb * wb + hb * hb));
    const float reach = r * 1.001f + 1e-2f;
    const float dx = ca.x - cb.x, dy = ca.y - cb.y;
    if (dx * dx + dy * dy > reach * reach) return 0.f;
  }
  const float acs = cosf(a[4]), asn = sinf(a[4]);
  const float bcs = cosf(b[4]), bsn = sinf(b[4]);
  Pt pa[5], pb[5];
  pa[0] = rotate_about(ca, acs, asn, a[0], a[1]);
  pa[1] = rotate_about(ca, acs, asn, a[2], a[1]);
  pa[2] = rotate_about(ca, acs, asn, a[2], a[3]);
  pa[3] = rotate_about(ca, acs, asn, a[0], a[3]);
  pa[4] = pa[0];
  pb[0] = rotate_about(cb, bcs, bsn, b[0], b[1]);
  pb[1] = rotate_about(cb, bcs, bsn, b[2], b[1]);
  pb[2] = rotate_about(cb, bcs, bsn, b[2], b[3]);
  pb[3] = rotate_about(cb, bcs, bsn, b[0], b[3]);
  pb[4] = pb[0];

  int cnt = 0;
  Pt ctr = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Pt q;
      if (edge_cross(pa[i + 1], pa[i], pb[j + 1], pb[j], q) && cnt < kPolyCap) {
        ctr.x = ctr.x + q.x;
        ctr.y = ctr.y + q.y;
        lx[cnt * kPolyBlock] = q.x;
        ly[cnt * kPolyBlock] = q.y;
        ++cnt;
      }
    }
  }
  const float nacs = cosf(-a[4]), nasn = sinf(-a[4]);
  const float nbcs = cosf(-b[4]), nbsn = sinf(-b[4]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (in_box(a, ca, nacs, nasn, pb[k]) && cnt < kPolyCap) {
      ctr.x = ctr.x + pb[k].x;
      ctr.y = ctr.y + pb[k].y;
      lx[cnt * kPolyBlock] = pb[k].x;
      ly[cnt * kPolyBlock] = pb[k].y;
      ++cnt;
    }
    if (in_box(b, cb, nbcs, nbsn, pa[k]) && cnt < kPolyCap) {
      ctr.x = ctr.x + pa[k].x;
      ctr.y = ctr.y + pa[k].y;
      lx[cnt * kPolyBlock] = pa[k].x;
      ly[cnt * kPolyBlock] = pa[k].y;
      ++cnt;
    }
  }
  if (cnt < 3) return 0.f;  // the fan of fewer than three points is empty (the reference sums 0 or 1 zero term)
  ctr.x /= (float)cnt;
  ctr.y /= (float)cnt;
  for (int s = 0; s < cnt; ++s) lk[s * kPolyBlock] = atan2f(ly[s * kPolyBlock] - ctr.y, lx[s * kPolyBlock] - ctr.x);
  // the reference's bubble sort: swap while the left angle is strictly larger (a stable ascending sort)
  for (int j = 0; j < cnt - 1; ++j) {
    for (int i = 0; i < cnt - j - 1; ++i) {
      const float k0 = lk[i * kPolyBlock], k1 = lk[(i + 1) * kPolyBlock];
      if (k0 > k1) {
        const float x0 = lx[i * kPolyBlock], y0 = ly[i * kPolyBlock];
        lk[i * kPolyBlock] = k1;
        lx[i * kPolyBlock] = lx[(i + 1) * kPolyBlock];
        ly[i * kPolyBlock] = ly[(i + 1) * kPolyBlock];
        lk[(i + 1) * kPolyBlock] = k0;
        lx[(i + 1) * kPolyBlock] = x0;
        ly[(i + 1) * kPolyBlock] = y0;
      }
    }
  }
  const float x0 = lx[0], y0 = ly[0];
  float area = 0.f;
  float ux = lx[kPolyBlock] - x0, uy = ly[kPolyBlock] - y0;
  for (int k = 1; k < cnt - 1; ++k) {
    const float vx = lx[(k + 1) * kPolyBlock] - x0, vy = ly[(k + 1) * kPolyBlock] - y0;
    area += ux * vy - uy * vx;
    ux = vx;
    uy = vy;
  }
  // The one deliberate departure from the reference: an overlap cannot exceed either box.  The fan of a box with
  // (nearly) itself carries the rounding of corners at up to 75 m and came out up to 1e-5 (relative) above the box's
  // own area, an IoU of up to 1.00002; the cap only ever moves the result towards the exact value.  NaN passes.
  const float s = fabsf(area) / 2;
  const float cap = fminf(fabsf(wa * ha), fabsf(wb * hb));
  return s > cap ? cap : s;
}

__device__ __forceinline__ float bev_iou(const float* a, const float* b, float* lx, float* ly, float* lk) {
  const float sa = (a[2] - a[0]) * (a[3] - a[1]);
  const float sb = (b[2] - b[0]) * (b[3] - b[1]);
  const float s = bev_overlap(a, b, lx, ly, lk);
  return s / fmaxf(sa + sb - s, kIouEps);
}

}  // namespace

// The second stage of FSD / FSDv2 (GroupCorrectionHead with FullySparseBboxHead) around its network: IoU assignment of all
// samples and classes in one launch, the assigner's finish + IoUNegPiecewiseSampler + the regression targets in one launch (one
// workgroup per sample), the class / box / corner losses in two launches forward and one backward, and the box decoding.
// fp32 data, no float atomics, no host read-back, bit-reproducible.
//
// Reference (mmdet3d/models/roi_heads, mmdet3d/core/bbox):
//   sst_roi_assign_f32          fsd_roi_head.py:213-296 (_assign_and_sample: the per-sample, per-class mask compactions and
//                               assigner calls), BboxOverlaps3D / BaseInstance3DBoxes.overlaps (structures/base_box3d.py:395-450)
//   sst_roi_sample_targets_f32  mmdet's MaxIoUAssigner.assign_wrt_overlaps (with gt_max_assign_all), samplers/
//                               iou_neg_piecewise_sampler.py:46-164, bbox_heads/fsd_bbox_head.py:343-543 (get_targets,
//                               _get_target_single, get_multi_class_soft_label), coders/delta_xyzwhlr_bbox_coder.py:20-56 (encode)
//   sst_roi_loss_fwd_f32 / bwd  fsd_bbox_head.py:207-341 (loss, filter_pos_assigned_but_empty_rois) and :546-579
//                               (get_corner_loss_lidar), LiDARInstance3DBoxes.corners (structures/lidar_box3d.py:54-92),
//                               rotation_3d_in_axis (structures/utils.py:21-61), and what autograd derives from them
//   sst_roi_decode_f32          fsd_bbox_head.py:634-653 (the decode of get_bboxes), :609 (sigmoid), xywhr2xyxyr of the BEV rows
//
// PARITY.  The IoU is the operation sequence of box_ops.boxes3d_overlaps_lidar: the BEV overlap of bev_clip.h (the box ops'
// own device function) x the clamped height overlap, divided by the clamped union; this file is built without floating-point
// contraction (Makefile), so the matrix is bit-equal to that of the box ops.  Targets, losses and decoded boxes follow the
// reference's fp32 operation order; sin / cos / log / exp are the device library's.
#include "common.h"
#include "bev_clip.h"
#include "head_math.h"
#include "roi_target.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGtTile = 64;          // ground-truth boxes per LDS tile of the assignment
constexpr int kMaxCls = SST_ROI_MAX_CLASSES;
constexpr int kMaxPieces = SST_ROI_MAX_PIECES;
constexpr int kMaxProps = 8192;      // proposals of one sample the sampler holds in LDS (keys 32 KB + 2 x 8 KB of flags)
constexpr int kRec = 5;              // 8-byte slots of a loss record: cls, reg, corner sums (double), num_pos, corner rows (int64)

// ------------------------------------------------------------------------------------------------------------------
// assignment: IoU of every proposal with the boxes of its sample (and class)
// ------------------------------------------------------------------------------------------------------------------

struct GtTile {
  float bev[kGtTile][5];
  float bottom[kGtTile], top[kGtTile], volume[kGtTile];
  int label[kGtTile];
};

__global__ __launch_bounds__(kPolyBlock) void roi_assign_k(sst_roi_assign_args a) {
  __shared__ float poly_x[kPolyCap * kPolyBlock];
  __shared__ float poly_y[kPolyCap * kPolyBlock];
  __shared__ float poly_k[kPolyCap * kPolyBlock];
  __shared__ GtTile gt;
  const int tid = threadIdx.x;
  float* lx = poly_x + tid;
  float* ly = poly_y + tid;
  float* lk = poly_k + tid;
  const int64_t p = (int64_t)blockIdx.x * kPolyBlock + tid;
  const bool live = p < a.n_props;
  int mine = -1, label = -1;
  float pb[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, bottom = 0.f, top = 0.f, volume = 0.f;
  if (live) {
    for (int s = 0; s < a.batch; ++s)
      if (p >= a.prop_offsets[s] && p < a.prop_offsets[s + 1]) mine = s;
    const int64_t l = a.prop_labels[p];
    label = (l >= 0 && l < a.num_classes) ? (int)l : -1;
    const float* b = a.props + p * a.prop_cols;
    // xywhr2xyxyr(LiDARInstance3DBoxes.bev): (x - w / 2, y - l / 2, x + w / 2, y + l / 2, ry)
    const float hw = b[3] / 2, hl = b[4] / 2;
    pb[0] = b[0] - hw;
    pb[1] = b[1] - hl;
    pb[2] = b[0] + hw;
    pb[3] = b[1] + hl;
    pb[4] = b[6];
    bottom = b[2];
    top = b[2] + b[5];
    volume = b[3] * b[4] * b[5];
  }
  float best = -1.f;
  int best_at = -1;
  float* row = a.iou + (live ? p : 0) * a.ld;
  int64_t written = 0;  // columns of this proposal's row written so far
  for (int s = 0; s < a.batch; ++s) {
    if (!__syncthreads_or(mine == s ? 1 : 0)) continue;
    const int64_t g0 = max((int64_t)a.gt_offsets[s], (int64_t)0), g1 = min((int64_t)a.gt_offsets[s + 1], a.n_gts);
    for (int64_t t0 = g0; t0 < g1; t0 += kGtTile) {
      const int nt = (int)min((int64_t)kGtTile, g1 - t0);
      __syncthreads();
      if (tid < nt) {
        const float* b = a.gts + (t0 + tid) * a.gt_cols;
        const float hw = b[3] / 2, hl = b[4] / 2;
        gt.bev[tid][0] = b[0] - hw;
        gt.bev[tid][1] = b[1] - hl;
        gt.bev[tid][2] = b[0] + hw;
        gt.bev[tid][3] = b[1] + hl;
        gt.bev[tid][4] = b[6];
        gt.bottom[tid] = b[2];
        gt.top[tid] = b[2] + b[5];
        gt.volume[tid] = b[3] * b[4] * b[5];
        const int64_t l = a.gt_labels[t0 + tid];
        gt.label[tid] = (l >= 0 && l < a.num_classes) ? (int)l : -1;
      }
      __syncthreads();
      if (mine == s) {
        for (int k = 0; k < nt; ++k) {
          const int gl = gt.label[k];
          float v = -1.f;  // masked: another class, an invalid label on either side
          if (gl >= 0 && label >= 0 && (!a.class_mask || gl == label)) {
            const float oh = fmaxf(fminf(top, gt.top[k]) - fmaxf(bottom, gt.bottom[k]), 0.f);
            const float o3 = bev_overlap(pb, gt.bev[k], lx, ly, lk) * oh;
            v = o3 / fmaxf(volume + gt.volume[k] - o3, 1e-8f);
            if (v > best || best_at < 0) {  // the first maximum; a NaN never replaces a number
              best = v;
              best_at = (int)(t0 + k);
            }
          }
          const int64_t col = t0 - g0 + k;
          if (col < a.ld) row[col] = v;
        }
        written = min(g1 - g0, a.ld);
      }
    }
  }
  if (!live) return;
  for (int64_t c = written; c < a.ld; ++c) row[c] = -1.f;  // every element is written
  a.max_iou[p] = best_at < 0 ? 0.f : best;
  a.argmax[p] = best_at;
}

// ------------------------------------------------------------------------------------------------------------------
// the assigner's finish, the sampler, the targets: one workgroup per sample
// ------------------------------------------------------------------------------------------------------------------

struct SampleLds {
  float key[kMaxProps];
  uint8_t pool[kMaxProps];  // 0 positives, 1 + piece negatives, 255 in no pool
  uint8_t sel[kMaxProps];   // 1 chosen positive, 2 chosen negative
  float part[kWaves][kGtTile];
  float colmax[kGtTile];
  int colok[kGtTile];
  int cnt[1 + kMaxPieces];
  int take[1 + kMaxPieces];
  int wave_p[kWaves], wave_n[kWaves];
};

__global__ __launch_bounds__(kThreads) void roi_sample_k(sst_roi_sample_args a) {
  __shared__ SampleLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const int64_t p0 = max((int64_t)a.prop_offsets[s], (int64_t)0);
  const int64_t p1 = min((int64_t)a.prop_offsets[s + 1], a.n_props);
  const int64_t g0 = max((int64_t)a.gt_offsets[s], (int64_t)0);
  const int64_t g1 = min(min((int64_t)a.gt_offsets[s + 1], a.n_gts), g0 + a.ld);
  const bool fits = p1 - p0 <= kMaxProps;
  const int n = fits ? (int)max(p1 - p0, (int64_t)0) : 0;  // a sample beyond the LDS limit is reported, not sampled
  const int rc = 1 + a.prop_cols;

  // A. assign_wrt_overlaps on the row maxima: -1 background, -2 ignored, else the box
  for (int i = tid; i < n; i += kThreads) {
    const int64_t p = p0 + i;
    const int64_t l = a.prop_labels[p];
    const int am = a.argmax[p];
    const float mx = a.max_iou[p];
    int as = -2;
    if (l < 0 || l >= a.num_classes || am < 0) {
      as = -1;  // no box of its class: the reference's zero overlaps, background
    } else {
      const int c = a.class_mask ? (int)l : 0;
      if (mx >= 0.f && mx < a.neg_iou_thr[c]) as = -1;
      if (mx >= a.pos_iou_thr[c]) as = am;
    }
    a.assigned[p] = as;
  }
  if (tid <= kMaxPieces) {
    L.cnt[tid] = 0;
    L.take[tid] = 0;
  }
  __syncthreads();

  // B. low-quality matching with gt_max_assign_all, boxes in index order: the last box wins
  for (int64_t c0 = g0; c0 < g1; c0 += kGtTile) {
    const int nt = (int)min((int64_t)kGtTile, g1 - c0);
    float cm = -1.f;
    if (lane < nt)
      for (int i = wave; i < n; i += kWaves) cm = fmaxf(cm, a.iou[(p0 + i) * a.ld + (c0 - g0) + lane]);
    L.part[wave][lane] = cm;
    __syncthreads();
    if (tid < kGtTile) {
      float m = L.part[0][tid];
      for (int w = 1; w < kWaves; ++w) m = fmaxf(m, L.part[w][tid]);
      int ok = 0;
      if (tid < nt && m >= 0.f) {
        const int64_t gl = a.gt_labels[c0 + tid];
        if (gl >= 0 && gl < a.num_classes) ok = m >= a.min_pos_iou[a.class_mask ? (int)gl : 0] ? 1 : 0;
      }
      L.colmax[tid] = m;
      L.colok[tid] = ok;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      const float* row = a.iou + (p0 + i) * a.ld + (c0 - g0);
      int as = a.assigned[p0 + i];
      for (int k = 0; k < nt; ++k)
        if (L.colok[k] && row[k] == L.colmax[k]) as = (int)(c0 + k);
      a.assigned[p0 + i] = as;
    }
    __syncthreads();
  }

  // C. the pools and their sizes
  int my_p = 0, my_n = 0;
  for (int i = tid; i < n; i += kThreads) {
    const int as = a.assigned[p0 + i];
    L.key[i] = a.keys[p0 + i];
    L.pool[i] = as >= 0 ? 0 : as == -1 ? 1 : 255;
    L.sel[i] = 0;
    my_p += as >= 0;
    my_n += as == -1;
  }
  if (my_p) atomicAdd(&L.cnt[0], my_p);  // integer LDS atomics: the sums do not depend on their order
  if (my_n) atomicAdd(&L.cnt[1], my_n);
  __syncthreads();
  const int n_pos = L.cnt[0], n_neg = L.cnt[1];
  const int k_pos = min(n_pos, a.num_expected_pos);
  const int expected_neg = a.num - k_pos;
  const bool pieces = n_neg > expected_neg;
  __syncthreads();
  if (pieces) {
    if (tid == 0) L.cnt[1] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      if (L.pool[i] != 1) continue;
      const float ov = a.max_iou[p0 + i];
      int q = 255;
      for (int k = 0; k < a.n_pieces; ++k) {
        const float lo = k == a.n_pieces - 1 ? 0.f : a.piece_thr[k + 1];
        if (ov >= lo && ov < a.piece_thr[k]) {
          q = 1 + k;
          break;
        }
      }
      L.pool[i] = (uint8_t)q;
      if (q != 255) atomicAdd(&L.cnt[q], 1);
    }
    __syncthreads();
  }
  if (tid == 0) {
    L.take[0] = k_pos;
    if (!pieces) {
      L.take[1] = n_neg;
    } else {
      int chosen = 0, extend = 0;
      for (int k = 0; k < a.n_pieces; ++k) {
        int want = k == a.n_pieces - 1 ? expected_neg - chosen : (int)((double)expected_neg * a.piece_frac[k]) + extend;
        want = max(want, 0);
        const int have = L.cnt[1 + k];
        if (have < want) {
          L.take[1 + k] = have;
          extend += want - have;
        } else {
          L.take[1 + k] = want;
          extend = 0;
        }
        chosen += L.take[1 + k];
      }
    }
  }
  __syncthreads();
  // "k of a pool" = its k smallest (key, index)
  for (int i = tid; i < n; i += kThreads) {
    const int q = L.pool[i];
    if (q == 255) continue;
    const int k = L.take[q];
    bool in = L.cnt[q] <= k;
    if (!in && k > 0) {
      const float mine = L.key[i];
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const float kj = L.key[j];
        rank += (L.pool[j] == q && (kj < mine || (kj == mine && j < i))) ? 1 : 0;
      }
      in = rank < k;
    }
    if (in) L.sel[i] = q == 0 ? 1 : 2;
  }
  __syncthreads();
  int total_neg = 0;
  for (int k = 1; k <= kMaxPieces; ++k) total_neg += L.take[k];
  total_neg = min(total_neg, a.num - k_pos);
  if (tid == 0) {
    a.counts[2 * s] = fits ? k_pos : -1;
    a.counts[2 * s + 1] = fits ? total_neg : -1;
  }

  // D. the rows: positives, then negatives, each in ascending proposal index; then the padding
  const int64_t out0 = (int64_t)s * a.num;
  int base_p = 0, base_n = 0;
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int i = i0 + tid;
    const int sel = i < n ? L.sel[i] : 0;
    const unsigned long long bp = __ballot(sel == 1), bn = __ballot(sel == 2);
    if (lane == 0) {
      L.wave_p[wave] = __popcll(bp);
      L.wave_n[wave] = __popcll(bn);
    }
    __syncthreads();
    int off_p = base_p, off_n = base_n, all_p = 0, all_n = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) {
        off_p += L.wave_p[w];
        off_n += L.wave_n[w];
      }
      all_p += L.wave_p[w];
      all_n += L.wave_n[w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int r = -1;
    if (sel == 1) r = off_p + __popcll(bp & below);
    if (sel == 2) r = k_pos + off_n + __popcll(bn & below);
    if (r >= 0 && r < a.num) {
      const int64_t p = p0 + i, o = out0 + r;
      const float* roi = a.props + p * a.prop_cols;
      float* orow = a.rois + o * rc;
      orow[0] = (float)s;
      for (int c = 0; c < a.prop_cols; ++c) orow[1 + c] = roi[c];
      const int as = a.assigned[p];
      const float ov = a.max_iou[p];
      float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float soft = 0.f;
      int64_t lab = -1;
      if (sel == 1) {
        roi_target_row(roi, a.gts + (int64_t)as * a.gt_cols, t);
        lab = a.gt_labels[as];
        if (lab >= 0 && lab < a.num_classes) {  // get_multi_class_soft_label
          const float pos = (float)a.cls_pos_thr[lab], neg = (float)a.cls_neg_thr[lab];
          soft = ov > pos ? 1.f : ov < neg ? 0.f : (ov - neg) / (float)(a.cls_pos_thr[lab] - a.cls_neg_thr[lab]);
        }
      }
      a.src[o] = (int32_t)p;
      a.gt_index[o] = sel == 1 ? as : -1;
      a.labels[o] = lab;
      a.iou_out[o] = ov;
      a.soft_label[o] = soft;
      a.reg_mask[o] = sel == 1 ? 1 : 0;
      for (int c = 0; c < 7; ++c) a.targets[o * 7 + c] = t[c];
    }
    base_p += all_p;
    base_n += all_n;
    __syncthreads();
  }
  for (int r = k_pos + total_neg + tid; r < a.num; r += kThreads) {
    const int64_t o = out0 + r;
    for (int c = 0; c < rc; ++c) a.rois[o * rc + c] = 0.f;
    a.src[o] = -1;
    a.gt_index[o] = -1;
    a.labels[o] = -1;
    a.iou_out[o] = 0.f;
    a.soft_label[o] = 0.f;
    a.reg_mask[o] = 0;
    for (int c = 0; c < 7; ++c) a.targets[o * 7 + c] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// losses
// ------------------------------------------------------------------------------------------------------------------

// corner k of LiDARInstance3DBoxes.corners in units of (w, l, h): unravel_index(k, [2, 2, 2])[[0, 1, 3, 2, 4, 5, 7, 6]] - (.5, .5, 0)
__device__ __forceinline__ void corner_norm(int k, float& nx, float& ny, float& nz) {
  const int y = (k >> 1) & 1;
  nx = (k & 4) ? 0.5f : -0.5f;
  ny = y ? 0.5f : -0.5f;
  nz = (float)((k & 1) ^ y);
}

// The corner loss of one row (fsd_bbox_head.py:293-311, :546-577): the sum of its 8 Huber terms.  bp: the 7 predictions, roi:
// the RoI box, gt: the assigned box.  With g != nullptr also the gradient of that sum in bp.
__device__ __forceinline__ float corner_row(const float* bp, const float* roi, const float* gt, float* g) {
  const float wa = roi[3], la = roi[4], ha = roi[5], ra = roi[6];
  // DeltaXYZWLHRBBoxCoder.decode against the anchor (0, 0, 0, w, l, h, ry)
  const float diag = sqrtf(la * la + wa * wa);
  const float X = bp[0] * diag, Y = bp[1] * diag;
  const float za = ha / 2;
  const float lg = expf(bp[4]) * la, wg = expf(bp[3]) * wa, hg = expf(bp[5]) * ha;
  const float Z = (bp[2] * ha + za) - hg / 2;
  const float r = bp[6] + ra;
  // rotation_3d_in_axis by roi_ry + pi / 2 about z, then the RoI centre
  const float th = ra + kHalfPi;
  const float tc = cosf(th), ts = sinf(th);
  const float px = (X * tc + Y * ts) + roi[0], py = (Y * tc - X * ts) + roi[1], pz = Z + roi[2];
  const float c = cosf(r), s = sinf(r);
  const float gc = cosf(gt[6]), gs = sinf(gt[6]);
  const float gf = gt[6] + kPi;
  const float fc = cosf(gf), fs = sinf(gf);
  float sum = 0.f;
  float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f, al = 0.f, ah = 0.f, ar = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float nx, ny, nz;
    corner_norm(k, nx, ny, nz);
    const float lx = wg * nx, ly = lg * ny, lz = hg * nz;
    const float cx = (lx * c + ly * s) + px, cy = (ly * c - lx * s) + py, cz = lz + pz;
    const float qx = gt[3] * nx, qy = gt[4] * ny, qz = gt[5] * nz;
    const float dz = cz - (qz + gt[2]);
    const float d0x = cx - ((qx * gc + qy * gs) + gt[0]), d0y = cy - ((qy * gc - qx * gs) + gt[1]);
    const float d1x = cx - ((qx * fc + qy * fs) + gt[0]), d1y = cy - ((qy * fc - qx * fs) + gt[1]);
    const float n0 = sqrtf(d0x * d0x + d0y * d0y + dz * dz), n1 = sqrtf(d1x * d1x + d1y * d1y + dz * dz);
    const bool first = n0 <= n1;
    const float d = first ? n0 : n1;
    const float q = fminf(d, 1.f);
    sum += 0.5f * q * q + (d - q);
    if (g) {
      // d Huber / d corner = (d < 1 ? 1 : 1 / d) * (corner - target): no division below the knee, 0 at d = 0
      const float sc = d < 1.f ? 1.f : 1.f / d;
      const float gx = sc * (first ? d0x : d1x), gy = sc * (first ? d0y : d1y), gz = sc * dz;
      ax += gx;
      ay += gy;
      az += gz;
      aw += nx * (gx * c - gy * s);
      al += ny * (gx * s + gy * c);
      ah += nz * gz;
      ar += gx * (ly * c - lx * s) - gy * (lx * c + ly * s);
    }
  }
  if (g) {
    g[0] = (ax * tc - ay * ts) * diag;
    g[1] = (ax * ts + ay * tc) * diag;
    g[2] = az * ha;
    g[3] = aw * wg;
    g[4] = al * lg;
    g[5] = (ah - 0.5f * az) * hg;
    g[6] = ar;
  }
  return sum;
}

__device__ __forceinline__ float bce_elem(float z, float t) { return fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z))); }

struct RowFlags {
  bool cls, reg, corner;
};
__device__ __forceinline__ RowFlags row_flags(const sst_roi_loss_args& a, int64_t r) {
  RowFlags f;
  f.cls = a.nonempty[r] != 0;
  f.reg = f.cls && a.reg_mask[r] != 0;
  f.corner = f.reg && a.with_corner && a.gt_index[r] >= 0 && a.gt_index[r] < a.n_gts &&
             (a.car_index < 0 || a.labels[r] == a.car_index);
  return f;
}

__global__ __launch_bounds__(kThreads) void roi_loss_partial_k(sst_roi_loss_args a, unsigned long long* __restrict__ partials) {
  __shared__ double wsum[3][kWaves];
  __shared__ long long wcnt[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = (int64_t)blockIdx.x * kThreads + tid;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  bool reg = false, corner = false;
  if (r < a.n) {
    const RowFlags f = row_flags(a, r);
    reg = f.reg;
    corner = f.corner;
    if (f.cls) s0 = (double)bce_elem(a.cls_score[r], a.soft_label[r]);
    if (f.reg) {
      const float* bp = a.bbox_pred + r * 7;
      const float* tg = a.targets + r * 7;
#pragma unroll
      for (int k = 0; k < 7; ++k) s1 += (double)(sst_reg_elem(bp[k] - tg[k], a.beta) * a.code_weight[k]);
      if (f.corner) s2 = (double)corner_row(bp, a.rois + r * a.roi_cols + 1, a.gts + (int64_t)a.gt_index[r] * a.gt_cols, nullptr);
    }
  }
  const long long n_reg = __popcll(__ballot(reg)), n_corner = __popcll(__ballot(corner));
  s0 = sst_wave_sum(s0);
  s1 = sst_wave_sum(s1);
  s2 = sst_wave_sum(s2);
  if (lane == 0) {
    wsum[0][wave] = s0;
    wsum[1][wave] = s1;
    wsum[2][wave] = s2;
    wcnt[0][wave] = n_reg;
    wcnt[1][wave] = n_corner;
  }
  __syncthreads();
  unsigned long long* rec = partials + (int64_t)blockIdx.x * kRec;
  sst_write_record<kWaves, 3>(wsum, rec);
  if (tid >= 3 && tid < kRec) {
    long long v = 0;
    for (int w = 0; w < kWaves; ++w) v += wcnt[tid - 3][w];
    rec[tid] = (unsigned long long)v;
  }
}

// one workgroup: thread q < 5 adds slot q of the records in index order; thread 0 writes the results.  Phases as in
// cluster_head.hip: COUNTS writes counts (averaging factors at their defaults), FINISH reads the factors from counts.
__global__ __launch_bounds__(64) void roi_loss_final_k(int64_t n, int nb, int phase, float w_cls, float w_reg, float w_corner,
                                                       const unsigned long long* __restrict__ partials, float* __restrict__ out,
                                                       double* __restrict__ counts) {
  __shared__ double tot[kRec];
  const int tid = threadIdx.x;
  if (tid < 3) {
    double v = 0.0;
    for (int b = 0; b < nb; ++b) v += __longlong_as_double((long long)partials[(int64_t)b * kRec + tid]);
    tot[tid] = v;
  } else if (tid < kRec) {
    long long v = 0;
    for (int b = 0; b < nb; ++b) v += (long long)partials[(int64_t)b * kRec + tid];
    tot[tid] = (double)v;
  }
  __syncthreads();
  if (tid != 0) return;
  const double n_pos = tot[3], n_corner = tot[4];
  double cls_avg = (double)n, reg_avg = n_pos;
  if (phase & SST_ROI_LOSS_COUNTS) {
    counts[0] = n_pos;
    counts[1] = n_corner;
    counts[2] = cls_avg;
    counts[3] = reg_avg;
  } else {
    cls_avg = counts[2];
    reg_avg = counts[3];
  }
  if (!(phase & SST_ROI_LOSS_FINISH)) return;
  out[0] = (float)((double)w_cls * tot[0] / cls_avg);
  out[1] = n_pos > 0.0 && reg_avg > 0.0 ? (float)((double)w_reg * tot[1] / reg_avg) : 0.f;
  out[2] = n_corner > 0.0 ? (float)((double)w_corner * tot[2] / (8.0 * n_corner)) : 0.f;
  out[3] = (float)n_pos;
  out[4] = (float)((double)n - n_pos);
}

__global__ __launch_bounds__(kThreads) void roi_loss_bwd_k(sst_roi_loss_args a, const float* __restrict__ g,
                                                           const double* __restrict__ counts, float* __restrict__ d_cls,
                                                           float* __restrict__ d_bbox) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n) return;
  const double n_pos = counts[0], n_corner = counts[1], cls_avg = counts[2], reg_avg = counts[3];
  const float k_cls = (float)((double)g[0] * (double)a.w_cls / cls_avg);
  const float k_reg = n_pos > 0.0 && reg_avg > 0.0 ? (float)((double)g[1] * (double)a.w_reg / reg_avg) : 0.f;
  const float k_cor = n_corner > 0.0 ? (float)((double)g[2] * (double)a.w_corner / (8.0 * n_corner)) : 0.f;
  const RowFlags f = row_flags(a, r);
  float dc = 0.f;
  float db[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (f.cls) {
    // d bce / dz = sigmoid(z) - t, the sigmoid from exp(-|z|)
    const float z = a.cls_score[r];
    const float e = expf(-fabsf(z));
    const float sg = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    dc = k_cls * (sg - a.soft_label[r]);
  }
  if (f.reg) {
    const float* bp = a.bbox_pred + r * 7;
    const float* tg = a.targets + r * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) db[k] = sst_reg_grad(bp[k] - tg[k], a.beta) * (a.code_weight[k] * k_reg);
    if (f.corner) {
      float gc[7];
      corner_row(bp, a.rois + r * a.roi_cols + 1, a.gts + (int64_t)a.gt_index[r] * a.gt_cols, gc);
#pragma unroll
      for (int k = 0; k < 7; ++k) db[k] += k_cor * gc[k];
    }
  }
  d_cls[r] = dc;
#pragma unroll
  for (int k = 0; k < 7; ++k) d_bbox[r * 7 + k] = db[k];
}

// ------------------------------------------------------------------------------------------------------------------
// decoding
// ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void roi_decode_k(const float* __restrict__ rois, int roi_cols,
                                                         const float* __restrict__ bbox_pred, const float* __restrict__ cls_score,
                                                         int64_t n, float* __restrict__ boxes, float* __restrict__ scores,
                                                         float* __restrict__ bev) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  const float* roi = rois + r * roi_cols + 1;
  const float* bp = bbox_pred + r * 7;
  const int cols = roi_cols - 1;
  const float wa = roi[3], la = roi[4], ha = roi[5], ra = roi[6];
  const float diag = sqrtf(la * la + wa * wa);
  const float X = bp[0] * diag, Y = bp[1] * diag;
  const float za = ha / 2;
  const float lg = expf(bp[4]) * la, wg = expf(bp[3]) * wa, hg = expf(bp[5]) * ha;
  const float Z = (bp[2] * ha + za) - hg / 2;
  const float th = ra + kHalfPi;
  const float tc = cosf(th), ts = sinf(th);
  const float x = (X * tc + Y * ts) + roi[0], y = (Y * tc - X * ts) + roi[1], z = Z + roi[2];
  const float ry = bp[6] + ra;
  float* o = boxes + r * cols;
  o[0] = x;
  o[1] = y;
  o[2] = z;
  o[3] = wg;
  o[4] = lg;
  o[5] = hg;
  o[6] = ry;
  for (int c = 7; c < cols; ++c) o[c] = roi[c];  // the padded zero deltas: the head does not refine the velocity
  if (scores) scores[r] = (float)(1.0 / (1.0 + exp(-(double)cls_score[r])));
  if (bev) {
    const float hw = wg / 2, hl = lg / 2;
    float* b = bev + r * 5;
    b[0] = x - hw;
    b[1] = y - hl;
    b[2] = x + hw;
    b[3] = y + hl;
    b[4] = ry;
  }
}

int check_loss_args(const sst_roi_loss_args* a) {
  if (!a || a->n < 1) return SST_ERR_ARG;
  if (!a->cls_score || !a->bbox_pred || !a->nonempty || !a->rois || !a->soft_label || !a->reg_mask || !a->targets) return SST_ERR_ARG;
  if (a->roi_cols != 8 && a->roi_cols != 10) return SST_ERR_UNSUPPORTED;
  if (!(a->beta >= 0.f)) return SST_ERR_ARG;
  if (a->with_corner && (!a->gt_index || !a->labels || a->n_gts < 0 || (a->n_gts > 0 && !a->gts) || a->gt_cols < 7)) return SST_ERR_ARG;
  if (sst_div_up(a->n, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  return SST_OK;
}

}  // namespace

extern "C" int sst_roi_assign_gt_tile(void) { return kGtTile; }
extern "C" int sst_roi_assign_block(void) { return kPolyBlock; }
extern "C" int sst_roi_sample_max_proposals(void) { return kMaxProps; }

extern "C" int sst_roi_assign_f32(const sst_roi_assign_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_roi_assign_args& a = *args;
  if (a.n_props < 0 || a.n_gts < 0 || a.batch < 1 || a.ld < 0) return SST_ERR_ARG;
  if ((a.prop_cols != 7 && a.prop_cols != 9) || a.gt_cols < 7) return SST_ERR_UNSUPPORTED;
  if (a.num_classes < 1 || a.num_classes > kMaxCls || a.batch > 65535) return SST_ERR_UNSUPPORTED;
  if (a.n_props == 0) return SST_OK;
  if (!a.props || !a.prop_labels || !a.prop_offsets || !a.gt_offsets || !a.max_iou || !a.argmax) return SST_ERR_ARG;
  if (a.n_gts > 0 && (!a.gts || !a.gt_labels)) return SST_ERR_ARG;
  if (a.ld > 0 && !a.iou) return SST_ERR_ARG;
  if (sst_div_up(a.n_props, kPolyBlock) > 0x7fffffff || a.n_gts > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(roi_assign_k, dim3((unsigned)sst_div_up(a.n_props, kPolyBlock)), dim3(kPolyBlock), 0, (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_roi_sample_targets_f32(const sst_roi_sample_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_roi_sample_args& a = *args;
  if (a.n_props < 0 || a.n_gts < 0 || a.batch < 1 || a.ld < 0 || a.num < 1 || a.num_expected_pos < 0) return SST_ERR_ARG;
  if ((a.prop_cols != 7 && a.prop_cols != 9) || a.gt_cols < 7) return SST_ERR_UNSUPPORTED;
  if (a.num_classes < 1 || a.num_classes > kMaxCls || a.n_pieces < 1 || a.n_pieces > kMaxPieces) return SST_ERR_UNSUPPORTED;
  if (a.max_props_per_sample > kMaxProps || a.batch > 65535) return SST_ERR_UNSUPPORTED;
  if (!a.prop_offsets || !a.gt_offsets || !a.rois || !a.src || !a.gt_index || !a.labels || !a.iou_out || !a.soft_label ||
      !a.reg_mask || !a.targets || !a.counts)
    return SST_ERR_ARG;
  if (a.n_props > 0 && (!a.props || !a.prop_labels || !a.max_iou || !a.argmax || !a.keys || !a.assigned)) return SST_ERR_ARG;
  if (a.n_gts > 0 && (!a.gts || !a.gt_labels || (a.n_props > 0 && a.ld > 0 && !a.iou))) return SST_ERR_ARG;
  hipLaunchKernelGGL(roi_sample_k, dim3(a.batch), dim3(kThreads), 0, (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int64_t sst_roi_loss_workspace_bytes(int64_t n) {
  if (n < 1) return 256;
  return sst_align_up(sst_div_up(n, kThreads) * kRec * 8, 256);
}

extern "C" int sst_roi_loss_fwd_f32(const sst_roi_loss_args* args, int phases, float* d_out, double* d_counts, void* d_workspace,
                                    void* stream) {
  const int rc = check_loss_args(args);
  if (rc != SST_OK) return rc;
  if (!d_counts || !d_workspace || !(phases & (SST_ROI_LOSS_COUNTS | SST_ROI_LOSS_FINISH))) return SST_ERR_ARG;
  if ((phases & SST_ROI_LOSS_FINISH) && !d_out) return SST_ERR_ARG;
  const int nb = (int)sst_div_up(args->n, kThreads);
  hipStream_t s = (hipStream_t)stream;
  if (phases & SST_ROI_LOSS_COUNTS) {
    hipLaunchKernelGGL(roi_loss_partial_k, dim3(nb), dim3(kThreads), 0, s, *args, (unsigned long long*)d_workspace);
    SST_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(roi_loss_final_k, dim3(1), dim3(64), 0, s, args->n, nb, phases, args->w_cls, args->w_reg, args->w_corner,
                     (const unsigned long long*)d_workspace, d_out, d_counts);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_roi_loss_bwd_f32(const sst_roi_loss_args* args, const float* d_g, const double* d_counts, float* d_dcls,
                                    float* d_dbbox, void* stream) {
  const int rc = check_loss_args(args);
  if (rc != SST_OK) return rc;
  if (!d_g || !d_counts || !d_dcls || !d_dbbox) return SST_ERR_ARG;
  hipLaunchKernelGGL(roi_loss_bwd_k, dim3((unsigned)sst_div_up(args->n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, *args,
                     d_g, d_counts, d_dcls, d_dbbox);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_roi_decode_f32(const float* d_rois, int roi_cols, const float* d_bbox_pred, const float* d_cls_score, int64_t n,
                                  float* d_boxes, float* d_scores, float* d_bev, void* stream) {
  if (n < 0) return SST_ERR_ARG;
  if (roi_cols != 8 && roi_cols != 10) return SST_ERR_UNSUPPORTED;
  if (n == 0) return SST_OK;
  if (!d_rois || !d_bbox_pred || !d_boxes || (d_scores && !d_cls_score)) return SST_ERR_ARG;
  if (sst_div_up(n, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(roi_decode_k, dim3((unsigned)sst_div_up(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, d_rois, roi_cols,
                     d_bbox_pred, d_cls_score, n, d_boxes, d_scores, d_bev);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

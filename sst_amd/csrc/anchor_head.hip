// Training and decoding side of Anchor3DHead: the MaxIoU assignment of every anchor of a whole batch and of every anchor size in
// one memset and two launches, the focal / box / direction losses straight from the NCHW maps in two launches forward and one
// backward, and the box decoding of the kept anchors in one launch.  fp32 data, no float atomics, no host read-back,
// bit-reproducible.  No anchor tensor exists: an anchor is (cell, size index, rotation index); its centre comes from three small
// per-axis tables, its size and rotation from the arguments.
//
// Reference:
//   sst_anchor_targets_f32   AnchorTrainMixin.anchor_target_3d_single / anchor_target_single_assigner, mmdet3d/models/
//                            dense_heads/train_mixins.py:101-314 (the list of per-size assigners), bbox_overlaps_nearest_3d of
//                            mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py:94-140, LiDARInstance3DBoxes.nearest_bev of
//                            mmdet3d/core/bbox/structures/lidar_box3d.py:123-141, limit_period, mmdet 2.x bbox_overlaps and
//                            MaxIoUAssigner.assign_wrt_overlaps (match_low_quality, gt_max_assign_all), PseudoSampler
//   sst_anchor_loss_fwd_f32  Anchor3DHead.loss / loss_single / add_sin_difference, dense_heads/anchor3d_head.py:197-379,
//                            DeltaXYZWLHRBBoxCoder.encode (core/bbox/coders/delta_xyzwhlr_bbox_coder.py:20-54),
//                            get_direction_target (train_mixins.py:317-346), mmdet's sigmoid FocalLoss, L1Loss / SmoothL1Loss
//                            and softmax CrossEntropyLoss with mean reduction and avg_factor
//   sst_anchor_loss_bwd_f32  what autograd derives from the above
//   sst_anchor_decode_f32    Anchor3DHead.get_bboxes_single :465-530 after its topk: the three permuted gathers,
//                            DeltaXYZWLHRBBoxCoder.decode :57-90, the zero background column, xywhr2xyxyr(bev)
//
// PARITY.  The nearest-BEV IoU is performed operation by operation as the reference's float32 tensor arithmetic is: every
// subtraction, product, sum and the division rounded once (this file is compiled with -ffp-contract=off, and the division is the
// compiler's IEEE one), because gt_max_assign_all compares IoUs for equality and the thresholds compare them exactly.  Python
// scalars (pi, thresholds, dir_offset) are rounded to fp32 once, as torch does with a Python scalar operand.  Square roots go
// through fp64 (correct rounding whatever the build flags).  log / sin / cos are the device library's; the decoder's exp and
// sigmoid are evaluated in fp64 and rounded once.
#include "common.h"
#include "head_math.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTileW = 32, kTileH = 8;   // cells per workgroup of the assignment: one lane per cell, consecutive lanes along w
constexpr int kThreads = kTileW * kTileH;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 128;               // ground-truth boxes per LDS pass
constexpr int kMaxSizes = SST_ANCHOR_MAX_SIZES, kMaxRots = SST_ANCHOR_MAX_ROTS;
constexpr int kFinalThreads = 1024;

struct Grid {
  const float* xs;  // [n_sizes, W]
  const float* ys;  // [n_sizes, H]
  const float* zs;  // [n_sizes]
  int H, W, ns, nr;
  float sizes[kMaxSizes][3];
  float rots[kMaxRots];
};

// limit_period(val, offset, period) = val - floor(val / period + offset) * period
__device__ __forceinline__ float limit_period(float val, float offset, float period) {
  return val - floorf(val / period + offset) * period;
}

// the extents along x and y of LiDARInstance3DBoxes.nearest_bev: (w, l), swapped when |limit_period(rz, 0.5, pi)| > pi / 4
__device__ __forceinline__ void nearest_dims(float rz, float w, float l, float& dx, float& dy) {
  const bool swap = fabsf(limit_period(rz, 0.5f, kPi)) > kQuarterPi;
  dx = swap ? l : w;
  dy = swap ? w : l;
}

// mmdet 2.x bbox_overlaps(gt, anchor, 'iou'), one pair
__device__ __forceinline__ float iou_pair(float gx1, float gy1, float gx2, float gy2, float garea, float ax1, float ay1,
                                          float ax2, float ay2, float aarea) {
  const float iw = fmaxf(fminf(gx2, ax2) - fmaxf(gx1, ax1), 0.f);
  const float ih = fmaxf(fminf(gy2, ay2) - fmaxf(gy1, ay1), 0.f);
  const float overlap = iw * ih;
  const float uni = fmaxf(garea + aarea - overlap, 1e-6f);
  return overlap / uni;
}

// ------------------------------------------------------------------------------------------------------------------
// targets
// ------------------------------------------------------------------------------------------------------------------

struct TargetsArgs {
  Grid g;
  const float* gts;
  const int64_t* labels;
  const int32_t* off;
  int64_t n_gts;
  int cols, batch, per_class, tiles_w;
  float pos[kMaxSizes], neg[kMaxSizes], min_pos[kMaxSizes];
  int32_t* assigned;  // [B, H * W * ns * nr]
  unsigned* gt_max;   // [ns, n_gts] float bits
  int* counts;        // [B]
};

// One workgroup: a kTileW x kTileH tile of cells of one sample for one anchor type (size, rotation), a lane per anchor.  The
// sample's boxes pass through LDS in chunks of kChunk; a box that cannot meet the tile's anchors at all is skipped by the whole
// workgroup (its IoU with every anchor of the tile is exactly 0: the clamped extents are).
// kSecond == false: the lane's maximum IoU and its first arg-max -> the code of assign_wrt_overlaps before the low-quality
// matches; the maximum per box over the tile's anchors is formed in LDS and merged into gt_max with an integer atomic max on the
// bit pattern (IoUs are non-negative floats, which order as unsigned integers), so the result does not depend on arrival order.
// kSecond == true: the same lanes recompute the same IoUs (same function, same inputs, same bits) against the boxes whose
// maximum reaches min_pos_iou, apply `assigned[overlaps[i] == gt_max[i]] = i` in box order, and count the sample's positives.
template <bool kSecond>
__global__ __launch_bounds__(kThreads) void anchor_assign_k(TargetsArgs a) {
  __shared__ float s_x1[kChunk], s_y1[kChunk], s_x2[kChunk], s_y2[kChunk], s_area[kChunk];
  __shared__ unsigned s_max[kChunk];
  __shared__ int s_hit[kChunk];
  __shared__ int s_cnt[kWaves];
  const int tid = threadIdx.x;
  const int tw = blockIdx.x % a.tiles_w, th = blockIdx.x / a.tiles_w;
  const int t = blockIdx.y, s = t / a.g.nr, r = t - s * a.g.nr, b = blockIdx.z;
  const int w = tw * kTileW + (tid & (kTileW - 1)), h = th * kTileH + tid / kTileW;
  const bool active = w < a.g.W && h < a.g.H;
  float dx, dy;
  nearest_dims(a.g.rots[r], a.g.sizes[s][0], a.g.sizes[s][1], dx, dy);
  const float hx = dx / 2.f, hy = dy / 2.f;
  const float* xs = a.g.xs + (int64_t)s * a.g.W;
  const float* ys = a.g.ys + (int64_t)s * a.g.H;
  const float cx = xs[min(w, a.g.W - 1)], cy = ys[min(h, a.g.H - 1)];
  const float ax1 = cx - hx, ay1 = cy - hy, ax2 = cx + hx, ay2 = cy + hy;
  const float aarea = (ax2 - ax1) * (ay2 - ay1);
  // the tile's anchors lie within [bx1, bx2] x [by1, by2]: the tables are monotone and fp32 addition is
  const float xa = xs[tw * kTileW], xb = xs[min(tw * kTileW + kTileW - 1, a.g.W - 1)];
  const float ya = ys[th * kTileH], yb = ys[min(th * kTileH + kTileH - 1, a.g.H - 1)];
  const float bx1 = fminf(xa, xb) - hx, bx2 = fmaxf(xa, xb) + hx, by1 = fminf(ya, yb) - hy, by2 = fmaxf(ya, yb) + hy;
  const int64_t g0 = max((int64_t)a.off[b], (int64_t)0), g1 = min((int64_t)a.off[b + 1], a.n_gts);
  const int na = a.g.ns * a.g.nr;
  const int64_t at = ((int64_t)b * a.g.H * a.g.W + (int64_t)h * a.g.W + w) * na + t;
  float best = 0.f;
  int arg = 0;
  int code = (kSecond && active) ? a.assigned[at] : -1;
  const int code0 = code;
  const float min_pos = a.min_pos[s];
  for (int64_t c0 = g0; c0 < g1; c0 += kChunk) {
    const int n = (int)min((int64_t)kChunk, g1 - c0);
    __syncthreads();
    if (tid < n) {
      const int64_t j = c0 + tid;
      const float* bx = a.gts + j * a.cols;
      float gdx, gdy;
      nearest_dims(bx[6], bx[3], bx[4], gdx, gdy);
      const float x1 = bx[0] - gdx / 2.f, y1 = bx[1] - gdy / 2.f, x2 = bx[0] + gdx / 2.f, y2 = bx[1] + gdy / 2.f;
      s_x1[tid] = x1;
      s_y1[tid] = y1;
      s_x2[tid] = x2;
      s_y2[tid] = y2;
      s_area[tid] = (x2 - x1) * (y2 - y1);
      bool hit = (!a.per_class || a.labels[j] == (int64_t)s) && x2 > bx1 && x1 < bx2 && y2 > by1 && y1 < by2;
      unsigned m = 0;
      if (kSecond) {
        m = a.gt_max[(int64_t)s * a.n_gts + j];
        hit = hit && __uint_as_float(m) >= min_pos;
      }
      s_max[tid] = m;
      s_hit[tid] = hit ? 1 : 0;
    }
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      if (!s_hit[i]) continue;  // uniform over the workgroup
      if (!active) continue;
      const float iou = iou_pair(s_x1[i], s_y1[i], s_x2[i], s_y2[i], s_area[i], ax1, ay1, ax2, ay2, aarea);
      if (kSecond) {
        if (__float_as_uint(iou) == s_max[i]) code = (int)(c0 - g0) + i;
      } else {
        if (iou > best) {
          best = iou;
          arg = (int)(c0 - g0) + i;
        }
        if (iou > 0.f) atomicMax(&s_max[i], __float_as_uint(iou));
      }
    }
    if (!kSecond) {
      __syncthreads();
      if (tid < n && s_max[tid] != 0) atomicMax(a.gt_max + (int64_t)s * a.n_gts + c0 + tid, s_max[tid]);
    }
  }
  if (!kSecond) {
    if (active) a.assigned[at] = best >= a.pos[s] ? arg : (best < a.neg[s] ? -1 : -2);
    return;
  }
  if (active && code != code0) a.assigned[at] = code;
  const unsigned long long pos = __ballot(active && code >= 0);
  __syncthreads();
  if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(pos);
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int k = 0; k < kWaves; ++k) total += s_cnt[k];
    if (total) atomicAdd(a.counts + b, total);  // integer: the sum does not depend on the order
  }
}

// ------------------------------------------------------------------------------------------------------------------
// losses
// ------------------------------------------------------------------------------------------------------------------

struct LossArgs {
  Grid g;
  const float* cls;   // [B, na * C, H, W]
  const float* box;   // [B, na * 7, H, W]
  const float* dir;   // [B, na * 2, H, W] or null
  const int32_t* assigned;
  const float* gts;
  const int64_t* labels;
  const int32_t* off;
  const int32_t* counts;
  int64_t n_gts;
  int cols, batch, C, smooth_l1, sin_diff;
  float gamma, alpha, w_cls, w_bbox, w_dir, beta, pos_weight, dir_offset;
  float cw[7];
};

// One logit z against the 0 / 1 target of mmdet's py_sigmoid_focal_loss:
//   pt = sigmoid(z) (target 0) or 1 - sigmoid(z) (target 1) = sigmoid(u), u = z or -z
//   e = (alpha or 1 - alpha) pt^gamma softplus(u);  de/du = (...) pt^gamma (gamma (1 - pt) softplus(u) + pt)
// Not sst_focal_elem: this one forms (aw * pt^gamma) * softplus where that forms (bce * aw) * mod, and calls powf for every gamma
// other than 2, so the last bit can differ.
__device__ __forceinline__ void focal_term(float z, bool target, float alpha, float gamma, float& loss, float& dz) {
  const float u = target ? -z : z;
  float pt, qt;
  const float e = sst_sigmoid_pair(u, pt, qt);
  const float sp = fmaxf(u, 0.f) + log1pf(e);
  const float ptg = gamma == 2.f ? pt * pt : powf(pt, gamma);
  const float aw = target ? alpha : 1.f - alpha;
  loss = aw * ptg * sp;
  const float du = aw * ptg * (gamma * qt * sp + pt);
  dz = target ? -du : du;
}

// DeltaXYZWLHRBBoxCoder.encode(anchor, gt) and get_direction_target
__device__ __forceinline__ int encode_box(const float* an, const float* gt, float dir_offset, float* tg) {
  const float za = an[2] + an[5] / 2.f, zg = gt[2] + gt[5] / 2.f;
  const float diagonal = sst_sqrt_rn(an[4] * an[4] + an[3] * an[3]);
  tg[0] = (gt[0] - an[0]) / diagonal;
  tg[1] = (gt[1] - an[1]) / diagonal;
  tg[2] = (zg - za) / an[5];
  tg[3] = logf(gt[3] / an[3]);
  tg[4] = logf(gt[4] / an[4]);
  tg[5] = logf(gt[5] / an[5]);
  tg[6] = gt[6] - an[6];
  const float rot_gt = tg[6] + an[6];
  const float offset_rot = limit_period(rot_gt - dir_offset, 0.f, kTwoPi);
  const float bin = floorf(offset_rot / kPi);
  return bin >= 1.f ? 1 : 0;  // .long() then clamp(0, 1); a NaN lands in 0
}

__device__ __forceinline__ void anchor_of(const Grid& g, int h, int w, int s, int r, float* an) {
  an[0] = g.xs[(int64_t)s * g.W + w];
  an[1] = g.ys[(int64_t)s * g.H + h];
  an[2] = g.zs[s];
  an[3] = g.sizes[s][0];
  an[4] = g.sizes[s][1];
  an[5] = g.sizes[s][2];
  an[6] = g.rots[r];
}

// box and direction terms of one positive anchor: the loss values and the derivatives in its 7 + 2 predictions
__device__ __forceinline__ void positive_terms(const LossArgs& a, const float* an, const float* gt, const float* pred,
                                               bool has_dir, float dir0, float dir1, float& l_box, float& l_dir, float* d_pred,
                                               float& d_dir0, float& d_dir1) {
  float tg[7];
  const int dir_t = encode_box(an, gt, a.dir_offset, tg);
  l_box = 0.f;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    float p = pred[c], q = tg[c], chain = 1.f;
    if (c == 6 && a.sin_diff) {
      const float sp = sinf(pred[6]), cp = cosf(pred[6]), st = sinf(tg[6]), ct = cosf(tg[6]);
      p = sp * ct;
      q = cp * st;
      chain = cp * ct + sp * st;  // d(p - q) / d pred
    }
    // sst_reg_elem / sst_reg_grad of (diff, smooth_l1 ? beta : 0), written out: through the helpers this kernel needs more VGPRs
    const float diff = p - q, ad = fabsf(diff);
    float e, de;
    if (a.smooth_l1 && ad < a.beta) {
      e = 0.5f * ad * ad / a.beta;
      de = diff / a.beta;
    } else {
      e = a.smooth_l1 ? ad - 0.5f * a.beta : ad;
      de = diff > 0.f ? 1.f : diff < 0.f ? -1.f : 0.f;
    }
    l_box += e * a.cw[c];
    d_pred[c] = de * chain * a.cw[c];
  }
  l_dir = 0.f;
  d_dir0 = d_dir1 = 0.f;
  if (has_dir) {
    // softmax cross entropy of two logits: softplus(z_other - z_target)
    const float u = dir_t ? dir0 - dir1 : dir1 - dir0;
    float p_other, p_target;
    const float e = sst_sigmoid_pair(u, p_other, p_target);
    l_dir = fmaxf(u, 0.f) + log1pf(e);
    d_dir0 = dir_t ? p_other : -p_other;
    d_dir1 = dir_t ? -p_other : p_other;
  }
}

// A lane per (sample, cell): its ns * nr anchors in turn.  The logits, box codes and direction logits are read where they lie
// in the NCHW maps (consecutive lanes read consecutive cells of one plane).  kBackward == false: the three sums of the
// workgroup -> partials[3 * block ..]; kBackward == true: every element of the three gradient maps.
template <bool kBackward>
__global__ __launch_bounds__(kThreads) void anchor_loss_k(LossArgs a, double* __restrict__ partials,
                                                          const float* __restrict__ g_cls, const float* __restrict__ g_box,
                                                          const float* __restrict__ g_dir, const float* __restrict__ out,
                                                          float* __restrict__ d_cls, float* __restrict__ d_box,
                                                          float* __restrict__ d_dir) {
  __shared__ double wsum[kWaves];
  const int64_t hw = (int64_t)a.g.H * a.g.W;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool active = i < (int64_t)a.batch * hw;
  const int na = a.g.ns * a.g.nr;
  double sum_cls = 0.0, sum_box = 0.0, sum_dir = 0.0;
  float k_cls = 0.f, k_box = 0.f, k_dir = 0.f;
  if (kBackward) {
    const double avg = (double)out[3];
    k_cls = g_cls ? (float)((double)g_cls[0] * (double)a.w_cls / avg) : 0.f;
    k_box = g_box ? (float)((double)g_box[0] * (double)a.w_bbox / avg) : 0.f;
    k_dir = g_dir ? (float)((double)g_dir[0] * (double)a.w_dir / avg) : 0.f;
  }
  if (active) {
    const int b = (int)(i / hw);
    const int64_t cell = i - (int64_t)b * hw;
    const int h = (int)(cell / a.g.W), w = (int)(cell - (int64_t)h * a.g.W);
    const int64_t g0 = a.off[b], ng = (int64_t)a.off[b + 1] - g0;
    const int32_t* codes = a.assigned + i * na;
    const float* cls = a.cls + (int64_t)b * na * a.C * hw + cell;
    const float* box = a.box + (int64_t)b * na * 7 * hw + cell;
    const float* dir = a.dir ? a.dir + (int64_t)b * na * 2 * hw + cell : nullptr;
    for (int t = 0; t < na; ++t) {
      const int code = codes[t];
      const bool positive = code >= 0 && code < ng;
      int label = a.C;  // background: no target column
      float weight = code == -2 ? 0.f : 1.f;
      if (positive) {
        label = (int)a.labels[g0 + code];
        weight = a.pos_weight > 0.f ? a.pos_weight : 1.f;
      }
      for (int k = 0; k < a.C; ++k) {
        const int64_t ch = ((int64_t)t * a.C + k) * hw;
        float e, dz;
        focal_term(cls[ch], k == label, a.alpha, a.gamma, e, dz);
        if (kBackward)
          d_cls[(cls - a.cls) + ch] = k_cls * weight * dz;
        else
          sum_cls += (double)(e * weight);
      }
      float dp[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dd0 = 0.f, dd1 = 0.f;
      if (positive) {
        const int s = t / a.g.nr, r = t - s * a.g.nr;
        float an[7], gt[7], pred[7];
        anchor_of(a.g, h, w, s, r, an);
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          gt[c] = a.gts[(g0 + code) * a.cols + c];
          pred[c] = box[((int64_t)t * 7 + c) * hw];
        }
        const float dir0 = dir ? dir[((int64_t)t * 2) * hw] : 0.f, dir1 = dir ? dir[((int64_t)t * 2 + 1) * hw] : 0.f;
        float l_box, l_dir;
        positive_terms(a, an, gt, pred, dir != nullptr, dir0, dir1, l_box, l_dir, dp, dd0, dd1);
        sum_box += (double)l_box;
        sum_dir += (double)l_dir;
      }
      if (kBackward) {
#pragma unroll
        for (int c = 0; c < 7; ++c) d_box[(box - a.box) + ((int64_t)t * 7 + c) * hw] = k_box * dp[c];
        if (dir) {
          d_dir[(dir - a.dir) + ((int64_t)t * 2) * hw] = k_dir * dd0;
          d_dir[(dir - a.dir) + ((int64_t)t * 2 + 1) * hw] = k_dir * dd1;
        }
      }
    }
  }
  if (!kBackward) {
    sum_cls = sst_block_sum(sum_cls, wsum);
    sum_box = sst_block_sum(sum_box, wsum);
    sum_dir = sst_block_sum(sum_dir, wsum);
    if (threadIdx.x == 0) {
      partials[3 * (int64_t)blockIdx.x] = sum_cls;
      partials[3 * (int64_t)blockIdx.x + 1] = sum_box;
      partials[3 * (int64_t)blockIdx.x + 2] = sum_dir;
    }
  }
}

// one workgroup: the records in index order; avg_factor = sum over the samples of max(positives, 1)
__global__ __launch_bounds__(kFinalThreads) void anchor_loss_final_k(const double* __restrict__ partials, int nb,
                                                                     const int32_t* __restrict__ counts, int batch, float w_cls,
                                                                     float w_bbox, float w_dir, float* __restrict__ out) {
  __shared__ double wsum[kFinalThreads / 64];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int r = threadIdx.x; r < nb; r += kFinalThreads) {
    s0 += partials[3 * (int64_t)r];
    s1 += partials[3 * (int64_t)r + 1];
    s2 += partials[3 * (int64_t)r + 2];
  }
  s0 = sst_block_sum(s0, wsum);
  s1 = sst_block_sum(s1, wsum);
  s2 = sst_block_sum(s2, wsum);
  if (threadIdx.x == 0) {
    double avg = 0.0;
    for (int b = 0; b < batch; ++b) avg += (double)max(counts[b], 1);
    out[0] = (float)(s0 / avg * (double)w_cls);
    out[1] = (float)(s1 / avg * (double)w_bbox);
    out[2] = (float)(s2 / avg * (double)w_dir);
    out[3] = (float)avg;  // an integer below 2^24 for any map that fits the device
  }
}

// ------------------------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void anchor_decode_k(Grid g, const float* __restrict__ cls, const float* __restrict__ box,
                                                            const float* __restrict__ dir, const int64_t* __restrict__ inds,
                                                            int64_t n, int C, float* __restrict__ boxes,
                                                            float* __restrict__ scores, int64_t* __restrict__ dir_out,
                                                            float* __restrict__ bev) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int na = g.ns * g.nr;
  const int64_t hw = (int64_t)g.H * g.W, total = hw * na;
  const int64_t idx = inds ? inds[i] : i;
  float* o = boxes + i * 7;
  if (idx < 0 || idx >= total) {  // not an anchor of the map: no box
    for (int c = 0; c < 7; ++c) o[c] = 0.f;
    for (int k = 0; k <= C; ++k) scores[i * (C + 1) + k] = 0.f;
    for (int c = 0; c < 5; ++c) bev[i * 5 + c] = 0.f;
    dir_out[i] = 0;
    return;
  }
  const int64_t cell = idx / na;
  const int t = (int)(idx - cell * na), s = t / g.nr, r = t - s * g.nr;
  const int h = (int)(cell / g.W), w = (int)(cell - (int64_t)h * g.W);
  float an[7], d[7];
  anchor_of(g, h, w, s, r, an);
#pragma unroll
  for (int c = 0; c < 7; ++c) d[c] = box[((int64_t)t * 7 + c) * hw + cell];
  const float za = an[2] + an[5] / 2.f;
  const float diagonal = sst_sqrt_rn(an[4] * an[4] + an[3] * an[3]);
  const float xg = d[0] * diagonal + an[0], yg = d[1] * diagonal + an[1];
  float zg = d[2] * an[5] + za;
  const float lg = (float)exp((double)d[4]) * an[4], wg = (float)exp((double)d[3]) * an[3];
  const float hg = (float)exp((double)d[5]) * an[5];
  const float rg = d[6] + an[6];
  zg = zg - hg / 2.f;
  o[0] = xg;
  o[1] = yg;
  o[2] = zg;
  o[3] = wg;
  o[4] = lg;
  o[5] = hg;
  o[6] = rg;
  for (int k = 0; k < C; ++k)
    scores[i * (C + 1) + k] = (float)(1.0 / (1.0 + exp(-(double)cls[((int64_t)t * C + k) * hw + cell])));
  scores[i * (C + 1) + C] = 0.f;
  dir_out[i] = dir ? (dir[((int64_t)t * 2 + 1) * hw + cell] > dir[((int64_t)t * 2) * hw + cell] ? 1 : 0) : 0;
  const float half_w = wg / 2.f, half_l = lg / 2.f;
  float* v = bev + i * 5;
  v[0] = xg - half_w;
  v[1] = yg - half_l;
  v[2] = xg + half_w;
  v[3] = yg + half_l;
  v[4] = rg;
}

int make_grid(Grid& g, const sst_anchor_grid* grid) {
  if (!grid || !grid->centers) return SST_ERR_ARG;
  if (grid->H < 1 || grid->W < 1 || grid->n_sizes < 1 || grid->n_rots < 1) return SST_ERR_ARG;
  if (grid->n_sizes > kMaxSizes || grid->n_rots > kMaxRots) return SST_ERR_UNSUPPORTED;
  if ((int64_t)grid->H * grid->W * grid->n_sizes * grid->n_rots > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  g.H = grid->H;
  g.W = grid->W;
  g.ns = grid->n_sizes;
  g.nr = grid->n_rots;
  g.xs = grid->centers;
  g.ys = g.xs + (int64_t)g.ns * g.W;
  g.zs = g.ys + (int64_t)g.ns * g.H;
  for (int s = 0; s < kMaxSizes; ++s)
    for (int c = 0; c < 3; ++c) g.sizes[s][c] = s < g.ns ? grid->sizes[s][c] : 1.f;
  for (int r = 0; r < kMaxRots; ++r) g.rots[r] = r < g.nr ? grid->rots[r] : 0.f;
  return SST_OK;
}

int make_loss_args(LossArgs& a, const sst_anchor_grid* grid, const sst_anchor_loss_args* in) {
  const int rc = make_grid(a.g, grid);
  if (rc != SST_OK) return rc;
  if (!in || !in->cls_score || !in->bbox_pred || !in->assigned || !in->gt_offsets || !in->pos_counts) return SST_ERR_ARG;
  if (in->batch < 1 || in->num_classes < 1 || in->n_gts < 0 || in->gt_cols < 7) return SST_ERR_ARG;
  if (in->n_gts > 0 && (!in->gts || !in->gt_labels)) return SST_ERR_ARG;
  if (in->smooth_l1 && !(in->beta > 0.f)) return SST_ERR_ARG;
  const int64_t cells = (int64_t)in->batch * a.g.H * a.g.W;
  if (sst_div_up(cells, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  a.cls = in->cls_score;
  a.box = in->bbox_pred;
  a.dir = in->dir_pred;
  a.assigned = in->assigned;
  a.gts = in->gts;
  a.labels = in->gt_labels;
  a.off = in->gt_offsets;
  a.counts = in->pos_counts;
  a.n_gts = in->n_gts;
  a.cols = in->gt_cols;
  a.batch = in->batch;
  a.C = in->num_classes;
  a.smooth_l1 = in->smooth_l1;
  a.sin_diff = in->sin_diff;
  a.gamma = in->gamma;
  a.alpha = in->alpha;
  a.w_cls = in->w_cls;
  a.w_bbox = in->w_bbox;
  a.w_dir = in->w_dir;
  a.beta = in->beta;
  a.pos_weight = in->pos_weight;
  a.dir_offset = in->dir_offset;
  for (int c = 0; c < 7; ++c) a.cw[c] = in->code_weight[c];
  return SST_OK;
}

}  // namespace

extern "C" int sst_anchor_targets_gt_chunk(void) { return kChunk; }

extern "C" int sst_anchor_block(void) { return kThreads; }

extern "C" int sst_anchor_targets_f32(const sst_anchor_grid* grid, const float* d_gts, int gt_cols, const int64_t* d_gt_labels,
                                      const int32_t* d_gt_offsets, int64_t n_gts, int batch, int assign_per_class,
                                      const float* pos_iou_thr, const float* neg_iou_thr, const float* min_pos_iou,
                                      int32_t* d_assigned, int32_t* d_state, void* stream) {
  TargetsArgs a;
  const int rc = make_grid(a.g, grid);
  if (rc != SST_OK) return rc;
  if (batch < 1 || n_gts < 0 || gt_cols < 7 || !d_gt_offsets || !pos_iou_thr || !neg_iou_thr || !min_pos_iou || !d_assigned ||
      !d_state)
    return SST_ERR_ARG;
  if (n_gts > 0 && (!d_gts || (assign_per_class && !d_gt_labels))) return SST_ERR_ARG;
  if (batch > 65535 || a.g.ns * a.g.nr > 65535 || n_gts > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  for (int s = 0; s < kMaxSizes; ++s) {
    a.pos[s] = s < a.g.ns ? pos_iou_thr[s] : 1.f;
    a.neg[s] = s < a.g.ns ? neg_iou_thr[s] : 0.f;
    a.min_pos[s] = s < a.g.ns ? min_pos_iou[s] : 1.f;
    if (s < a.g.ns && (!(a.min_pos[s] > 0.f) || !(a.pos[s] > 0.f))) return SST_ERR_UNSUPPORTED;
  }
  a.gts = d_gts;
  a.labels = d_gt_labels;
  a.off = d_gt_offsets;
  a.n_gts = n_gts;
  a.cols = gt_cols;
  a.batch = batch;
  a.per_class = assign_per_class;
  a.tiles_w = (int)sst_div_up(a.g.W, kTileW);
  a.assigned = d_assigned;
  a.gt_max = (unsigned*)d_state;
  a.counts = d_state + (int64_t)a.g.ns * n_gts;
  hipStream_t s = (hipStream_t)stream;
  SST_HIP(hipMemsetAsync(d_state, 0, (size_t)((int64_t)a.g.ns * n_gts + batch) * sizeof(int32_t), s));
  const int64_t tiles = (int64_t)a.tiles_w * sst_div_up(a.g.H, kTileH);
  if (tiles > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  const dim3 grid_dim((unsigned)tiles, a.g.ns * a.g.nr, batch);
  hipLaunchKernelGGL(anchor_assign_k<false>, grid_dim, dim3(kThreads), 0, s, a);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(anchor_assign_k<true>, grid_dim, dim3(kThreads), 0, s, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int64_t sst_anchor_loss_workspace_bytes(int batch, int grid_h, int grid_w) {
  if (batch < 1 || grid_h < 1 || grid_w < 1) return 256;
  return sst_align_up(sst_div_up((int64_t)batch * grid_h * grid_w, kThreads) * 3 * (int64_t)sizeof(double), 256);
}

extern "C" int sst_anchor_loss_fwd_f32(const sst_anchor_grid* grid, const sst_anchor_loss_args* args, float* d_out,
                                       void* d_workspace, void* stream) {
  LossArgs a;
  const int rc = make_loss_args(a, grid, args);
  if (rc != SST_OK) return rc;
  if (!d_out || !d_workspace) return SST_ERR_ARG;
  const int nb = (int)sst_div_up((int64_t)a.batch * a.g.H * a.g.W, kThreads);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(anchor_loss_k<false>, dim3(nb), dim3(kThreads), 0, s, a, (double*)d_workspace, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(anchor_loss_final_k, dim3(1), dim3(kFinalThreads), 0, s, (const double*)d_workspace, nb, a.counts, a.batch,
                     a.w_cls, a.w_bbox, a.w_dir, d_out);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_anchor_loss_bwd_f32(const sst_anchor_grid* grid, const sst_anchor_loss_args* args, const float* d_out,
                                       const float* d_g_cls, const float* d_g_bbox, const float* d_g_dir, float* d_dcls,
                                       float* d_dbbox, float* d_ddir, void* stream) {
  LossArgs a;
  const int rc = make_loss_args(a, grid, args);
  if (rc != SST_OK) return rc;
  if (!d_out || !d_dcls || !d_dbbox || (a.dir && !d_ddir)) return SST_ERR_ARG;
  const int nb = (int)sst_div_up((int64_t)a.batch * a.g.H * a.g.W, kThreads);
  hipLaunchKernelGGL(anchor_loss_k<true>, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, a, (double*)nullptr, d_g_cls,
                     d_g_bbox, d_g_dir, d_out, d_dcls, d_dbbox, d_ddir);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_anchor_decode_f32(const sst_anchor_grid* grid, const float* d_cls_score, const float* d_bbox_pred,
                                     const float* d_dir_pred, const int64_t* d_inds, int64_t n, int num_classes, float* d_boxes,
                                     float* d_scores, int64_t* d_dir, float* d_bev, void* stream) {
  Grid g;
  const int rc = make_grid(g, grid);
  if (rc != SST_OK) return rc;
  if (n < 0 || num_classes < 1) return SST_ERR_ARG;
  if (n == 0) return SST_OK;
  if (!d_cls_score || !d_bbox_pred || !d_boxes || !d_scores || !d_dir || !d_bev) return SST_ERR_ARG;
  if (sst_div_up(n, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(anchor_decode_k, dim3((unsigned)sst_div_up(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, g,
                     d_cls_score, d_bbox_pred, d_dir_pred, d_inds, n, num_classes, d_boxes, d_scores, d_dir, d_bev);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

// The CTRL tracklet family (TrackletRoIHead with TrackletAssigner and FullySparseBboxHead): the training targets of a whole
// batch of tracklets in one launch, and the input rows of the box head in one launch forward and one backward.
// fp32 data, no float atomics, no host read-back, bit-reproducible.
//
// Reference (mmdet3d/models/roi_heads, mmdet3d/core/bbox):
//   sst_tracklet_targets_f32     tracklet_roi_head.py:333-347 (_select_one2one_candidates), :287-331 (_assign_and_sample),
//                                assigners/tracklet_assigner.py:14-55, structures/lidar_tracklet.py:278-299 (self_ious,
//                                intersection_ious), mmdet's PseudoSampler, bbox_heads/fsd_bbox_head.py:343-543 (get_targets)
//   sst_tracklet_rows_fwd / bwd  tracklet_roi_head.py:247-258 (_bbox_forward: the gathers and the two cats) and their autograd
//
// PARITY.  The IoU is lidar_iou3d_pair of roi_target.h: the BEV overlap of bev_clip.h (the box ops' own device function) x the
// clamped height overlap over the clamped union; this file is built without floating-point contraction (Makefile), so the value
// is bit-equal to LiDARInstance3DBoxes.aligned_iou_3d built on sst_boxes_overlap_aligned_f32.  The regression target is
// roi_target_row, the RoI head's own.
#include "common.h"
#include "roi_target.h"
#include "tracklet_ts.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxCls = SST_ROI_MAX_CLASSES;

// ------------------------------------------------------------------------------------------------------------------
// targets: one workgroup per tracklet
// ------------------------------------------------------------------------------------------------------------------

// integer sum over the workgroup (order does not matter); every thread must call
__device__ __forceinline__ int block_count(int v, int* wcnt) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  for (int w = 0; w < kWaves; ++w) r += wcnt[w];
  return r;
}

__global__ __launch_bounds__(kThreads) void tracklet_targets_k(sst_tracklet_targets_args a) {
  // one polygon array per wave: bev_overlap strides its slots by kPolyBlock (= 64 lanes)
  __shared__ float poly_x[kWaves][kPolyCap * kPolyBlock];
  __shared__ float poly_y[kWaves][kPolyCap * kPolyBlock];
  __shared__ float poly_k[kWaves][kPolyCap * kPolyBlock];
  __shared__ int wcnt[kWaves];
  __shared__ int wave_p[kWaves], wave_n[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* lx = poly_x[wave] + lane;
  float* ly = poly_y[wave] + lane;
  float* lk = poly_k[wave] + lane;
  const int t = blockIdx.x;
  const int64_t r0 = min(max(a.trk_offsets[t], (int64_t)0), a.n_rows);
  const int n = (int)(min(max(a.trk_offsets[t + 1], r0), a.n_rows) - r0);
  const int64_t c0 = min(max(a.trk_cand_offsets[t], (int64_t)0), a.n_cands);
  const int64_t c1 = min(max(a.trk_cand_offsets[t + 1], c0), a.n_cands);
  const int64_t* ts = a.ts + r0;
  const float* boxes = a.boxes + r0 * 7;

  // A. the chosen candidate: the first one with the most shared timestamps of IoU > candidate_thresh
  int best = -1, best_cnt = -1;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t g0 = min(max(a.cand_offsets[c], (int64_t)0), a.n_cand_rows);
    const int m = (int)(min(max(a.cand_offsets[c + 1], g0), a.n_cand_rows) - g0);
    int cnt = 0;
    for (int i = tid; i < n; i += kThreads) {
      const int j = find_ts(a.cand_ts + g0, m, ts[i]);
      if (j >= 0 && lidar_iou3d_pair(boxes + (int64_t)i * 7, a.cand_boxes + (g0 + j) * 7, lx, ly, lk) > a.candidate_thresh) ++cnt;
    }
    cnt = block_count(cnt, wcnt);
    if (cnt > best_cnt) {
      best_cnt = cnt;
      best = (int)c;
    }
  }
  int64_t g0 = 0;
  int m = 0;
  if (best >= 0) {
    g0 = min(max(a.cand_offsets[best], (int64_t)0), a.n_cand_rows);
    m = (int)(min(max(a.cand_offsets[best + 1], g0), a.n_cand_rows) - g0);
  }
  const int64_t cls = a.trk_class[t];
  const bool cls_ok = cls >= 0 && cls < a.num_classes;

  // B. TrackletAssigner.assign in frame order
  int my_pos = 0;
  for (int i = tid; i < n; i += kThreads) {
    const int j = m > 0 ? find_ts(a.cand_ts + g0, m, ts[i]) : -1;
    const float iou = j >= 0 ? lidar_iou3d_pair(boxes + (int64_t)i * 7, a.cand_boxes + (g0 + j) * 7, lx, ly, lk) : 0.f;
    int64_t as = j + 1;
    if (a.object_centric && !(iou > a.iou_thr)) as = 0;
    a.matched[r0 + i] = j;
    a.overlaps[r0 + i] = iou;
    a.assigned_gt_inds[r0 + i] = as;
    my_pos += as > 0;
  }
  const int n_pos = block_count(my_pos, wcnt);
  if (tid == 0) {
    a.chosen[t] = best;
    a.counts[2 * t] = n_pos;
    a.counts[2 * t + 1] = n - n_pos;
  }

  // C. PseudoSampler's order (positives in frame order, then negatives in frame order) and get_targets in that order.  Thread
  // tid reads back the rows it wrote in B.
  int base_p = 0, base_n = 0;
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int i = i0 + tid;
    const bool live = i < n;
    const int64_t as = live ? a.assigned_gt_inds[r0 + i] : -1;
    const unsigned long long bp = __ballot(live && as > 0), bn = __ballot(live && as == 0);
    __syncthreads();
    if (lane == 0) {
      wave_p[wave] = __popcll(bp);
      wave_n[wave] = __popcll(bn);
    }
    __syncthreads();
    int off_p = base_p, off_n = base_n, all_p = 0, all_n = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) {
        off_p += wave_p[w];
        off_n += wave_n[w];
      }
      all_p += wave_p[w];
      all_n += wave_n[w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (live) {
      const bool pos = as > 0;
      const int r = pos ? off_p + __popcll(bp & below) : n_pos + off_n + __popcll(bn & below);
      const int64_t o = r0 + r;
      const float* roi = boxes + (int64_t)i * 7;
      float* orow = a.rois + o * 8;
      orow[0] = (float)t;
#pragma unroll
      for (int c = 0; c < 7; ++c) orow[1 + c] = roi[c];
      const float ov = a.overlaps[r0 + i];
      float tg[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float gb[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float soft = 0.f;
      if (pos) {
        const float* g = a.cand_boxes + (g0 + (as - 1)) * 7;
#pragma unroll
        for (int c = 0; c < 7; ++c) gb[c] = g[c];
        roi_target_row(roi, g, tg);
        if (cls_ok) {  // get_multi_class_soft_label
          const float pt = (float)a.cls_pos_thr[cls], nt = (float)a.cls_neg_thr[cls];
          soft = ov > pt ? 1.f : ov < nt ? 0.f : (ov - nt) / (float)(a.cls_pos_thr[cls] - a.cls_neg_thr[cls]);
        }
      }
      a.src[o] = (int32_t)(r0 + i);
      a.frame_inds[o] = i;
      a.gt_index[o] = pos ? (int32_t)(g0 + (as - 1)) : -1;
      a.labels[o] = pos ? cls : -1;
      a.iou_out[o] = ov;
      a.scores_out[o] = a.scores[r0 + i];
      a.soft_label[o] = soft;
      a.reg_mask[o] = pos ? 1 : 0;
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        a.targets[o * 7 + c] = tg[c];
        a.pos_gt_bboxes[o * 7 + c] = gb[c];
      }
    }
    base_p += all_p;
    base_n += all_n;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// the input rows of the box head
// ------------------------------------------------------------------------------------------------------------------

// Python's indexing of a tensor of n rows: -n <= i < 0 counts from the end; anything else outside names no row (-1)
__device__ __forceinline__ int64_t py_index(int64_t i, int64_t n) {
  if (i < 0) i += n;
  return i >= 0 && i < n ? i : -1;
}

constexpr int kRowLanes = 16;                  // lanes that read one source row
constexpr int kRowsPerBlock = kThreads / kRowLanes;
constexpr int kRowsLds = 12 * 1024;            // floats of the staged output rows of a workgroup (48 KB)

// out[i] = (feats[p_i, 0 : F] | is_cur_frame_i | roi_score[r_i]), xyz_out[i] = xyz[p_i].  A workgroup makes kRowsPerBlock
// consecutive output rows.  Reading: 16 lanes per source row; the row's 16-byte-aligned middle is read as float4 (a row of F =
// 67 floats starts on any 4-byte boundary), its head and tail float by float.  Writing: the rows are staged in LDS, and the
// workgroup's rows - one contiguous span of the output, whatever its alignment - leave with consecutive lanes on consecutive
// floats.  W floats per row; rows too wide for the LDS stage are written directly (staged == 0).
__global__ __launch_bounds__(kThreads) void tracklet_rows_fwd_k(sst_tracklet_rows_args a, int W, int staged) {
  extern __shared__ float stage[];
  const int sub = threadIdx.x % kRowLanes, local = threadIdx.x / kRowLanes;
  const int64_t i0 = (int64_t)blockIdx.x * kRowsPerBlock;
  const int64_t i = i0 + local;
  const int F = a.feat_cols;
  const bool live = i < a.m;
  float* __restrict__ orow = staged ? stage + local * W : a.out + (live ? i : 0) * W;
  if (live) {
    const int64_t p = py_index(a.pts_inds[i], a.n_points);
    if (p < 0) {
      for (int k = sub; k < F; k += kRowLanes) orow[k] = 0.f;
    } else {
      const float* __restrict__ src = a.feats + p * a.ld_feats;
      const int head = min(F, (int)((4 - (((uintptr_t)src >> 2) & 3)) & 3));
      const int body = (F - head) >> 2;
      if (sub < head) orow[sub] = src[sub];
      for (int q = sub; q < body; q += kRowLanes) {
        const float4 v = *(const float4*)(src + head + 4 * q);
        float* o = orow + head + 4 * q;
        o[0] = v.x;
        o[1] = v.y;
        o[2] = v.z;
        o[3] = v.w;
      }
      for (int k = head + 4 * body + sub; k < F; k += kRowLanes) orow[k] = src[k];
    }
    if (sub == 0) {
      const int64_t r = (a.combined || a.with_roi_scores) ? py_index(a.roi_inds[i], a.n_rois) : -1;
      int c = F;
      if (a.combined) orow[c++] = (p >= 0 && r >= 0 && a.pts_frame_inds[p] == a.roi_frame_inds[r]) ? 1.f : 0.f;
      if (a.with_roi_scores) orow[c++] = r >= 0 ? a.roi_scores[r] : 0.f;
    }
    if (a.xyz_out != nullptr && sub < a.xyz_cols) a.xyz_out[i * a.xyz_cols + sub] = p >= 0 ? a.xyz[p * a.ld_xyz + sub] : 0.f;
  }
  if (!staged) return;
  __syncthreads();
  const int64_t span = min((int64_t)kRowsPerBlock, a.m - i0) * W;
  float* __restrict__ dst = a.out + i0 * W;
  for (int64_t e = threadIdx.x; e < span; e += kThreads) dst[e] = stage[e];
}

constexpr int64_t kNoPoint = INT64_MAX;

// key[i] = p_i * m + i (p_i: the source point of output row i, Python's indexing): sorted, the rows of a point are one run in
// ascending row order.  A row that names no point sorts behind every run.
__global__ __launch_bounds__(kThreads) void tracklet_rows_keys_k(const int64_t* __restrict__ pts_inds, int64_t m, int64_t n,
                                                                 int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const int64_t p = py_index(pts_inds[i], n);
  keys[i] = p < 0 ? kNoPoint : p * m + i;
}

// d_feats[p][f] = the sum over the output rows of point p, in ascending row order, of d_out[row][f]; d_feats is zero on entry.
// 16 lanes per position of the sorted keys; the lanes at the first key of a run walk the run (a point of a parked object lies in
// every box of its tracklet: runs of up to ~200 rows) and write the point's row once: no float atomic, one order of the additions.
__global__ __launch_bounds__(kThreads) void tracklet_rows_bwd_k(const float* __restrict__ d_out, int64_t m, int64_t ld_out, int F,
                                                                const int64_t* __restrict__ keys, int64_t n,
                                                                float* __restrict__ d_feats) {
  const int sub = threadIdx.x % kRowLanes;
  const int64_t s = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kRowLanes;
  if (s >= m) return;
  const int64_t key = keys[s];
  if (key == kNoPoint) return;
  const int64_t p = key / m;
  if (p < 0 || p >= n) return;
  const int64_t lo = p * m, hi = lo + m;      // the keys of point p
  if (s > 0 && keys[s - 1] >= lo) return;     // not the first row of its run
  for (int f = sub; f < F; f += kRowLanes) {
    float acc = 0.f;
    for (int64_t t = s; t < m; ++t) {
      const int64_t k = keys[t];
      if (k >= hi) break;
      acc += d_out[(k - lo) * ld_out + f];
    }
    d_feats[p * F + f] = acc;
  }
}

}  // namespace

extern "C" int sst_tracklet_targets_block(void) { return kThreads; }

extern "C" int sst_tracklet_targets_f32(const sst_tracklet_targets_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_tracklet_targets_args& a = *args;
  if (a.n_rows < 0 || a.n_cand_rows < 0 || a.n_cands < 0 || a.n_tracklets < 0) return SST_ERR_ARG;
  if (a.num_classes < 1 || a.num_classes > kMaxCls || a.n_tracklets > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  if (a.n_rows > 0x7fffffff || a.n_cand_rows > 0x7fffffff || a.n_cands > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  if (a.n_tracklets == 0) return SST_OK;
  if (!a.trk_offsets || !a.trk_cand_offsets || !a.trk_class || !a.chosen || !a.counts) return SST_ERR_ARG;
  if (a.n_cands > 0 && !a.cand_offsets) return SST_ERR_ARG;
  if (a.n_cand_rows > 0 && (!a.cand_boxes || !a.cand_ts)) return SST_ERR_ARG;
  if (a.n_rows > 0 && (!a.boxes || !a.ts || !a.scores || !a.matched || !a.overlaps || !a.assigned_gt_inds || !a.rois || !a.src ||
                       !a.frame_inds || !a.gt_index || !a.labels || !a.iou_out || !a.scores_out || !a.soft_label || !a.reg_mask ||
                       !a.targets || !a.pos_gt_bboxes))
    return SST_ERR_ARG;
  hipLaunchKernelGGL(tracklet_targets_k, dim3((unsigned)a.n_tracklets), dim3(kThreads), 0, (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

static int check_rows(const sst_tracklet_rows_args& a) {
  if (a.m < 0 || a.n_points < 0 || a.n_rois < 0 || a.feat_cols < 0 || a.xyz_cols < 0 || a.xyz_cols > kRowLanes) return SST_ERR_ARG;
  if (a.ld_feats < a.feat_cols || a.ld_xyz < a.xyz_cols) return SST_ERR_ARG;
  if (sst_div_up(a.m, kRowsPerBlock) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  return SST_OK;
}

extern "C" int sst_tracklet_rows_fwd_f32(const sst_tracklet_rows_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_tracklet_rows_args& a = *args;
  const int rc = check_rows(a);
  if (rc != SST_OK) return rc;
  if (a.m == 0) return SST_OK;
  if (!a.pts_inds || !a.out) return SST_ERR_ARG;
  if (a.n_points > 0 && a.feat_cols > 0 && !a.feats) return SST_ERR_ARG;
  if (a.xyz_out && a.n_points > 0 && a.xyz_cols > 0 && !a.xyz) return SST_ERR_ARG;
  if ((a.combined || a.with_roi_scores) && !a.roi_inds) return SST_ERR_ARG;
  if (a.combined && ((a.n_points > 0 && !a.pts_frame_inds) || (a.n_rois > 0 && !a.roi_frame_inds))) return SST_ERR_ARG;
  if (a.with_roi_scores && a.n_rois > 0 && !a.roi_scores) return SST_ERR_ARG;
  const int W = a.feat_cols + (a.combined ? 1 : 0) + (a.with_roi_scores ? 1 : 0);
  const int staged = (int64_t)kRowsPerBlock * W <= kRowsLds ? 1 : 0;
  hipLaunchKernelGGL(tracklet_rows_fwd_k, dim3((unsigned)sst_div_up(a.m, kRowsPerBlock)), dim3(kThreads),
                     staged ? sizeof(float) * kRowsPerBlock * W : 0, (hipStream_t)stream, a, W, staged);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_tracklet_rows_keys_i64(const int64_t* d_pts_inds, int64_t m, int64_t n_points, int64_t* d_keys, void* stream) {
  if (m < 0 || n_points < 0) return SST_ERR_ARG;
  if (m == 0) return SST_OK;
  if (!d_pts_inds || !d_keys) return SST_ERR_ARG;
  if (sst_div_up(m, kThreads) > 0x7fffffff || (n_points > 0 && m > INT64_MAX / n_points - 1)) return SST_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(tracklet_rows_keys_k, dim3((unsigned)sst_div_up(m, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, d_pts_inds,
                     m, n_points, d_keys);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_tracklet_rows_bwd_f32(const float* d_out_grad, int64_t m, int64_t ld_out, int feat_cols, const int64_t* d_sorted_keys,
                                         int64_t n_points, float* d_feats_grad, void* stream) {
  if (m < 0 || n_points < 0 || feat_cols < 0 || ld_out < feat_cols) return SST_ERR_ARG;
  if (n_points == 0 || feat_cols == 0) return SST_OK;
  if (!d_feats_grad || (m > 0 && (!d_sorted_keys || !d_out_grad))) return SST_ERR_ARG;
  if (sst_div_up(m, kRowsPerBlock) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  SST_HIP(hipMemsetAsync(d_feats_grad, 0, sizeof(float) * (size_t)n_points * (size_t)feat_cols, (hipStream_t)stream));
  if (m == 0) return SST_OK;
  hipLaunchKernelGGL(tracklet_rows_bwd_k, dim3((unsigned)sst_div_up(m, kRowsPerBlock)), dim3(kThreads), 0, (hipStream_t)stream,
                     d_out_grad, m, ld_out, feat_cols, d_sorted_keys, n_points, d_feats_grad);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

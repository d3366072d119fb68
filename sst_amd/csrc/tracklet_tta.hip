// Test-time augmentation of the CTRL tracklet family on the device: the K views that the reference's
// MultiScaleFlipAug3D (mmdet3d/datasets/pipelines/test_time_aug.py:88-109) makes by deep-copying a sample and running
// TrackletGlobalRotScaleTrans (tracklet_pipelines.py:329-355), TrackletRandomFlip (:414-439), PointsRangeFilter and PointShuffle
// once per view in a data-loader worker, and what happens behind the network: TrackletRoIHead.inverse_aug
// (mmdet3d/models/roi_heads/tracklet_roi_head.py:168-179), LiDARTracklet.update_from_prediction
// (mmdet3d/core/bbox/structures/lidar_tracklet.py:403-445) and LiDARTracklet.merge_augs (:548-602).
//
// Views.  One classify launch (a lane per INPUT row: the row is read once, its frame found once by the binary search over the
// sample's frame offsets staged in LDS, the frame's 3 x 4 matrix applied once, the posed row with its copied columns and the
// frame's decoration values written once to the workspace; then per view the transform, the strict range test, one 64-bit key
// and an integer count), ONE sst_sort_pairs_u64 over (dropped | view | sample | key32), one gather launch that writes every
// survivor of every view through LDS as contiguous spans.  The output is view-major: the rows of (view v, sample s) are one run,
// so what follows sees a batch of n_views * batch samples.  The boxes of every view come from one more launch.
//
// Inside a view the steps are the reference's: rotation, scale, translation (TrackletGlobalRotScaleTrans), THEN flip h, flip v
// (TrackletRandomFlip) - not the order of augment_common.h's transform_point, which flips first.
//
// Finish.  One launch, a lane per tracklet row: the view's flips and rotation undone, the row's matrix inv(pose_i) @ shared_pose
// applied (centre by the full matrix, heading by its rotation, atan2), the old box and score where the RoI was invalid, and the
// merge over the views in fp64 in the fixed order k = 0 .. K - 1.
//
// PARITY.  Built without floating-point contraction (Makefile).  Integer atomics only; two runs are bit-equal.
#include "augment_common.h"
#include "roi_target.h"

namespace {

using sst_aug::kBlock;
using sst_aug::sample_bits;
using sst_aug::sample_of_block;
using sst_aug::shuffle_key;
constexpr int kMaxCols = SST_AUG_MAX_COLS;
constexpr int kMaxDeco = SST_TRK_AUG_MAX_DECO;
constexpr int kMaxFrames = SST_TRK_AUG_MAX_FRAMES;
constexpr int kMaxViews = SST_TRK_TTA_MAX_VIEWS;
constexpr int kMatFloats = 12;
constexpr uint64_t kViewSeed = 0xD6E8FEB86659FD93ull;   // view v shuffles with seed + v * this: view 0 keeps the sample's seed

struct Work {
  uint64_t* keys_in;
  uint64_t* keys_out;
  uint32_t* perm;
  int32_t* row_frame;            // the frame (index into `frames`) of every input row
  float* base;                   // [n_total, cols + deco]: the posed row, its copied columns, its frame's decoration values
  void* sort_ws;
  int64_t bytes;
};

Work carve(void* base, int64_t n, int views, int width) {
  sst_carver c(base);
  Work w;
  w.keys_in = c.take<uint64_t>(n * views);
  w.keys_out = c.take<uint64_t>(n * views);
  w.perm = c.take<uint32_t>(n * views);
  w.row_frame = c.take<int32_t>(n);
  w.base = c.take<float>(n * width);
  w.sort_ws = c.take<char>(sst_sort_workspace_bytes(n * views));
  w.bytes = c.off;
  return w;
}

// rows 0..2 of the frame's 4 x 4 matrix applied to (x, y, z, 1): ((m0 x + m1 y) + m2 z) + m3, every operation rounded
__device__ __forceinline__ void pose_point(const float* __restrict__ m, float& x, float& y, float& z) {
  const float xn = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
  const float yn = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[4], x), __fmul_rn(m[5], y)), __fmul_rn(m[6], z)), m[7]);
  const float zn = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[8], x), __fmul_rn(m[9], y)), __fmul_rn(m[10], z)), m[11]);
  x = xn;
  y = yn;
  z = zn;
}

// one view of one point: rotation, scale, translation, flip h, flip v; -> inside the range (strict; a NaN fails)
__device__ __forceinline__ bool view_point(const sst_augment_params& p, float& x, float& y, float& z) {
  if (p.rotate) {
    const float xr = __fadd_rn(__fmul_rn(x, p.cos), __fmul_rn(y, p.sin));
    const float yr = __fadd_rn(__fmul_rn(x, -p.sin), __fmul_rn(y, p.cos));
    x = xr;
    y = yr;
  }
  x = __fadd_rn(__fmul_rn(x, p.scale), p.trans[0]);
  y = __fadd_rn(__fmul_rn(y, p.scale), p.trans[1]);
  z = __fadd_rn(__fmul_rn(z, p.scale), p.trans[2]);
  if (p.flip_h) y = -y;
  if (p.flip_v) x = -x;
  return x > p.range[0] && y > p.range[1] && z > p.range[2] && x < p.range[3] && y < p.range[4] && z < p.range[5];
}

__global__ __launch_bounds__(kBlock) void tta_classify_kernel(sst_tracklet_tta_views_args a, uint64_t* __restrict__ keys,
                                                              int32_t* __restrict__ row_frame, float* __restrict__ base,
                                                              int sbits, int vbits) {
  __shared__ int32_t frame_at[kMaxFrames + 1];        // the sample's frame offsets, relative to its first row
  __shared__ int32_t view_cnt[kMaxViews];
  const int s = sample_of_block(a.block_offsets, a.batch, (int)blockIdx.x);
  if (s < 0) return;
  const int f0 = a.sample_frames[s];
  int nf = a.sample_frames[s + 1] - f0;
  if (f0 < 0 || nf < 0 || nf > kMaxFrames || (int64_t)f0 + nf > a.n_frames) nf = 0;   // a table that disagrees reads nothing
  const int64_t row0 = nf > 0 ? (int64_t)a.frame_rows[f0] : 0;
  for (int k = threadIdx.x; k <= nf; k += kBlock) frame_at[k] = nf > 0 ? (int32_t)((int64_t)a.frame_rows[f0 + k] - row0) : 0;
  if (threadIdx.x < kMaxViews) view_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t n_s = frame_at[nf];
  const int64_t r = (int64_t)((int)blockIdx.x - a.block_offsets[s]) * kBlock + threadIdx.x;
  const bool active = nf > 0 && r < n_s && row0 >= 0 && row0 + r < a.n_total;
  const int W = a.cols + a.deco;
  float bx = 0.f, by = 0.f, bz = 0.f;
  if (active) {
    int lo = 0, hi = nf - 1;                            // the first frame k with frame_at[k + 1] > r: empty frames own no row
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)frame_at[mid + 1] > r) hi = mid;
      else lo = mid + 1;
    }
    const int f = f0 + lo;
    const float* src = a.points + (row0 + r) * a.cols;
    const float* rec = a.frames + (int64_t)f * (kMatFloats + a.deco);
    bx = src[0];
    by = src[1];
    bz = src[2];
    pose_point(rec, bx, by, bz);
    float* dst = base + (row0 + r) * W;
    dst[0] = bx;
    dst[1] = by;
    dst[2] = bz;
    for (int k = 3; k < a.cols; ++k) dst[k] = src[k];
    for (int k = 0; k < a.deco; ++k) dst[a.cols + k] = rec[kMatFloats + k];
    row_frame[row0 + r] = f;
  }
  for (int v = 0; v < a.n_views; ++v) {                 // uniform: every lane of the workgroup takes part in the ballot
    bool keep = false;
    if (active) {
      const sst_augment_params p = a.params[(int64_t)v * a.batch + s];
      float x = bx, y = by, z = bz;
      keep = view_point(p, x, y, z);
      const uint32_t key32 = p.shuffle ? shuffle_key(p.seed + kViewSeed * (uint64_t)v, (uint32_t)s, (uint32_t)r) : (uint32_t)r;
      keys[(int64_t)v * a.n_total + row0 + r] = ((uint64_t)(keep ? 0 : 1) << (32 + sbits + vbits)) |
                                                ((uint64_t)(uint32_t)v << (32 + sbits)) | ((uint64_t)(uint32_t)s << 32) | key32;
    }
    const int cnt = __popcll(__ballot(keep));
    if (sst_lane() == 0 && cnt > 0) atomicAdd(&view_cnt[v], cnt);
  }
  __syncthreads();
  if ((int)threadIdx.x < a.n_views && view_cnt[threadIdx.x] > 0)
    atomicAdd(&a.counts[(int64_t)threadIdx.x * a.batch + s], view_cnt[threadIdx.x]);
}

// one lane per output row; the rows of a workgroup leave as one contiguous span.  WT: the output width at compile time (the
// shipped widths), or 0: read from the arguments (the stage then holds the widest row)
template <int WT>
__global__ __launch_bounds__(kBlock) void tta_gather_kernel(sst_tracklet_tta_views_args a, const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ perm,
                                                            const int32_t* __restrict__ row_frame,
                                                            const float* __restrict__ base, int sbits, int vbits) {
  constexpr int kStageCols = WT ? WT : kMaxCols + kMaxDeco;
  __shared__ __attribute__((aligned(16))) float stage[kBlock * kStageCols];
  const int W = WT ? WT : a.cols + a.deco;
  const int64_t n_keys = a.n_total * a.n_views;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool valid = false;
  if (j < n_keys) {
    const uint64_t key = keys[j];
    const int s = (int)((key >> 32) & ((1ull << sbits) - 1));
    const int v = (int)((key >> (32 + sbits)) & ((1ull << vbits) - 1));
    const int64_t g = (int64_t)perm[j] - (int64_t)v * a.n_total;
    valid = (key >> (32 + sbits + vbits)) == 0 && s < a.batch && v < a.n_views && g >= 0 && g < a.n_total;
    if (valid) {
      const int f = row_frame[g];
      valid = f >= 0 && f < a.n_frames;
      if (valid) {
        const float* src = base + g * W;
        float* dst = stage + threadIdx.x * W;
        float x = src[0], y = src[1], z = src[2];
        const sst_augment_params p = a.params[(int64_t)v * a.batch + s];
        view_point(p, x, y, z);
        dst[0] = x;
        dst[1] = y;
        dst[2] = z;
        if constexpr (WT != 0) {
#pragma unroll
          for (int k = 3; k < WT; ++k) dst[k] = src[k];
        } else {
          for (int k = 3; k < W; ++k) dst[k] = src[k];
        }
        a.out_frame_inds[j] = a.frame_values[f];          // position j of the sorted rows IS the output row: a contiguous span
      }
    }
  }
  const int rows = __syncthreads_count(valid);            // the survivors are a prefix of the sorted rows
  const int total = rows * W;
  float* dst = a.out + (int64_t)blockIdx.x * kBlock * W;   // 16-byte aligned: kBlock * W * 4 bytes per workgroup
  const int quads = total >> 2;
  for (int e = threadIdx.x; e < quads; e += kBlock) ((float4*)dst)[e] = ((const float4*)stage)[e];
  for (int e = (quads << 2) + threadIdx.x; e < total; e += kBlock) dst[e] = stage[e];
}

template <int WT>
void launch_gather(const sst_tracklet_tta_views_args& a, const Work& w, int sbits, int vbits, hipStream_t st) {
  hipLaunchKernelGGL((tta_gather_kernel<WT>), dim3((unsigned)sst_div_up(a.n_total * a.n_views, kBlock)), dim3(kBlock), 0, st, a,
                     w.keys_out, w.perm, w.row_frame, w.base, sbits, vbits);
}

// a lane per (view, box): rotation, scale, translation, flip h, flip v -> boxes_out [n_views, n_boxes, cols]
__global__ __launch_bounds__(kBlock) void tta_boxes_kernel(sst_tracklet_tta_box_args a) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= (int64_t)a.n_views * a.n_boxes) return;
  const int v = (int)(t / a.n_boxes), i = (int)(t % a.n_boxes);
  int lo = 0, hi = a.batch - 1;                           // the first sample s with box_offsets[s + 1] > i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.box_offsets[mid + 1] > i) hi = mid;
    else lo = mid + 1;
  }
  const sst_augment_params p = a.params[(int64_t)v * a.batch + lo];
  const int D = a.cols;
  const float* src = a.boxes + (int64_t)i * D;
  float b[9];
  for (int k = 0; k < 9; ++k) b[k] = k < D ? src[k] : 0.f;
  if (p.rotate) {
    const float xr = __fadd_rn(__fmul_rn(b[0], p.cos), __fmul_rn(b[1], p.sin));
    const float yr = __fadd_rn(__fmul_rn(b[0], -p.sin), __fmul_rn(b[1], p.cos));
    b[0] = xr;
    b[1] = yr;
    b[6] = __fadd_rn(b[6], p.angle);
    const float vx = __fadd_rn(__fmul_rn(b[7], p.cos), __fmul_rn(b[8], p.sin));
    const float vy = __fadd_rn(__fmul_rn(b[7], -p.sin), __fmul_rn(b[8], p.cos));
    b[7] = vx;
    b[8] = vy;
  }
  for (int k = 0; k < 6; ++k) b[k] = __fmul_rn(b[k], p.scale);
  b[7] = __fmul_rn(b[7], p.scale);
  b[8] = __fmul_rn(b[8], p.scale);
  for (int k = 0; k < 3; ++k) b[k] = __fadd_rn(b[k], p.trans[k]);
  if (p.flip_h) {
    b[1] = -b[1];
    b[8] = -b[8];
    b[6] = __fadd_rn(-b[6], 3.14159274101257324f);         // -yaw + (float)pi
  }
  if (p.flip_v) {
    b[0] = -b[0];
    b[7] = -b[7];
    b[6] = -b[6];
  }
  float* dst = a.boxes_out + t * D;
  for (int k = 0; k < D; ++k) dst[k] = b[k];
}

// LiDARTracklet._apply_poses of one box: the centre by the full matrix, the heading (sin yaw, cos yaw, 0) by its rotation
__device__ __forceinline__ void ego_box(const float* __restrict__ m, const float* b, float* o) {
  float x = b[0], y = b[1], z = b[2];
  pose_point(m, x, y, z);
  const float sn = sinf(b[6]), cs = cosf(b[6]);
  const float hx = __fadd_rn(__fmul_rn(m[0], sn), __fmul_rn(m[1], cs));
  const float hy = __fadd_rn(__fmul_rn(m[4], sn), __fmul_rn(m[5], cs));
  o[0] = x;
  o[1] = y;
  o[2] = z;
  o[3] = b[3];
  o[4] = b[4];
  o[5] = b[5];
  o[6] = atan2f(hx, hy);
}

constexpr int kFinishBlock = kPolyBlock;                  // one wave: bev_overlap strides its LDS slots by kPolyBlock

__global__ __launch_bounds__(kFinishBlock) void tta_finish_kernel(sst_tracklet_tta_finish_args a, float* __restrict__ vb,
                                                                  double* __restrict__ vs) {
  __shared__ float poly_x[kPolyCap * kPolyBlock];
  __shared__ float poly_y[kPolyCap * kPolyBlock];
  __shared__ float poly_k[kPolyCap * kPolyBlock];
  const int64_t r = (int64_t)blockIdx.x * kFinishBlock + threadIdx.x;
  if (r >= a.n_rows) return;                              // no barrier below: a lane owns its row and its LDS column
  const int K = a.n_views;
  const int64_t n = a.n_rows;
  const float* m = a.mats + r * kMatFloats;

  // per view: the flips and the rotation undone, the box in its own frame's pose; the old box and score off the valid RoIs
  for (int k = 0; k < K; ++k) {
    float b[7], o[7];
    double sc;
    if (a.valid[k * n + r]) {
      const float* src = a.boxes + (k * n + r) * 7;
      for (int c = 0; c < 7; ++c) b[c] = src[c];
      const sst_tracklet_tta_view& vw = a.views[k];
      if (vw.flip_h) {
        b[1] = -b[1];
        b[6] = __fadd_rn(-b[6], 3.14159274101257324f);
      }
      if (vw.flip_v) {
        b[0] = -b[0];
        b[6] = -b[6];
      }
      if (vw.rotate) {                                    // rotate(-angle): cos(-angle) = cos, sin(-angle) = -sin
        const float xr = __fadd_rn(__fmul_rn(b[0], vw.cos), __fmul_rn(b[1], -vw.sin));
        const float yr = __fadd_rn(__fmul_rn(b[0], vw.sin), __fmul_rn(b[1], vw.cos));
        b[0] = xr;
        b[1] = yr;
        b[6] = __fadd_rn(b[6], -vw.angle);
      }
      sc = (double)a.scores[k * n + r];
    } else {
      const float* src = a.old_boxes + r * 7;
      for (int c = 0; c < 7; ++c) b[c] = src[c];
      sc = a.old_scores[r];
    }
    ego_box(m, b, o);
    float* dst = vb + (k * n + r) * 7;
    for (int c = 0; c < 7; ++c) dst[c] = o[c];
    vs[k * n + r] = sc;
  }

  if (a.mode == SST_TRK_TTA_MERGE_IOU_CLAMPED) {          // scores off the views that left view 0's box: times 0.0
    float b0[7];
    for (int c = 0; c < 7; ++c) b0[c] = vb[r * 7 + c];
    for (int k = 0; k < K; ++k) {
      float bk[7];
      for (int c = 0; c < 7; ++c) bk[c] = vb[(k * n + r) * 7 + c];
      const float iou = k == 0 ? 1.f : lidar_iou3d_pair(b0, bk, poly_x + threadIdx.x, poly_y + threadIdx.x, poly_k + threadIdx.x);
      vs[k * n + r] = __dmul_rn(vs[k * n + r], iou > a.iou_merge_thresh ? 1.0 : 0.0);
    }
  }

  double* mb = a.merged_boxes + r * 7;
  if (a.mode == SST_TRK_TTA_MERGE_MAX) {                  // numpy's argmax: the first maximum, a NaN counts as one
    int best = 0;
    double bs = vs[r];
    for (int k = 1; k < K; ++k) {
      const double s = vs[k * n + r];
      if (bs == bs && (s > bs || s != s)) {
        best = k;
        bs = s;
      }
    }
    for (int c = 0; c < 7; ++c) mb[c] = (double)vb[(best * n + r) * 7 + c];
    a.merged_scores[r] = bs;
    return;
  }
  double den = vs[r];
  for (int k = 1; k < K; ++k) den = __dadd_rn(den, vs[k * n + r]);
  for (int c = 0; c < 6; ++c) {
    double num = __dmul_rn((double)vb[r * 7 + c], vs[r]);
    for (int k = 1; k < K; ++k) num = __dadd_rn(num, __dmul_rn((double)vb[(k * n + r) * 7 + c], vs[k * n + r]));
    mb[c] = __ddiv_rn(num, den);
  }
  // np.median of the float32 yaws: the middle one, or (lower + upper) / 2 in float32; a NaN anywhere gives NaN.  Ranks by
  // counting: view k's rank is the number of views below it, ties in view order
  float lower = 0.f, upper = 0.f;
  bool nan = false;
  for (int k = 0; k < K; ++k) {
    const float yk = vb[(k * n + r) * 7 + 6];
    if (yk != yk) nan = true;
    int rank = 0;
    for (int q = 0; q < K; ++q) {
      const float yq = vb[(q * n + r) * 7 + 6];
      rank += (yq < yk || (yq == yk && q < k)) ? 1 : 0;
    }
    if (rank == (K - 1) / 2) lower = yk;
    if (rank == K / 2) upper = yk;
  }
  const float med = (K & 1) ? lower : __fdiv_rn(__fadd_rn(lower, upper), 2.f);
  mb[6] = nan ? (double)__builtin_nanf("") : (double)med;
  a.merged_scores[r] = __ddiv_rn(den, (double)K);
}

}  // namespace

extern "C" {

int64_t sst_tracklet_tta_views_workspace_bytes(int64_t n_total, int batch, int n_views, int width) {
  if (n_total < 0 || batch < 1 || n_views < 1 || n_views > kMaxViews || width < 3 || width > kMaxCols + kMaxDeco) return 0;
  if (n_total * n_views > (int64_t)INT32_MAX - kBlock) return 0;
  return carve(nullptr, n_total > 0 ? n_total : 1, n_views, width).bytes;
}

int sst_tracklet_tta_views_f32(const sst_tracklet_tta_views_args* args, void* stream) {
  if (args == nullptr) return SST_ERR_ARG;
  const sst_tracklet_tta_views_args& a = *args;
  if (a.cols < 3 || a.cols > kMaxCols || a.deco < 0 || a.deco > kMaxDeco) return SST_ERR_UNSUPPORTED;
  if (a.max_frames > kMaxFrames || a.n_views > kMaxViews) return SST_ERR_UNSUPPORTED;
  if (a.n_total < 0 || a.batch < 1 || a.n_views < 1 || a.n_blocks < 0 || a.n_frames < 0 || a.max_frames < 0 ||
      a.counts == nullptr)
    return SST_ERR_ARG;
  if (a.n_total * a.n_views > (int64_t)INT32_MAX - kBlock) return SST_ERR_UNSUPPORTED;
  const int sbits = sample_bits(a.batch), vbits = sample_bits(a.n_views);
  if (33 + sbits + vbits > 64) return SST_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int W = a.cols + a.deco;
  Work w = {};
  if (a.n_total > 0) {                                    // every check comes before the first byte is written
    if (a.points == nullptr || a.frame_rows == nullptr || a.sample_frames == nullptr || a.block_offsets == nullptr ||
        a.frames == nullptr || a.frame_values == nullptr || a.params == nullptr || a.out == nullptr ||
        a.out_frame_inds == nullptr || a.workspace == nullptr || a.n_blocks < 1 || a.n_frames < 1)
      return SST_ERR_ARG;
    if (((uintptr_t)a.points | (uintptr_t)a.out | (uintptr_t)a.workspace) & 15) return SST_ERR_ARG;
    w = carve(a.workspace, a.n_total, a.n_views, W);
    if (a.workspace_bytes < w.bytes) return SST_ERR_ARG;
  }
  SST_HIP(hipMemsetAsync(a.counts, 0, sizeof(int32_t) * a.batch * a.n_views, st));
  if (a.n_total == 0) return SST_OK;
  hipLaunchKernelGGL(tta_classify_kernel, dim3((unsigned)a.n_blocks), dim3(kBlock), 0, st, a, w.keys_in, w.row_frame, w.base,
                     sbits, vbits);
  SST_LAUNCH_CHECK();
  const int rc = sst_sort_pairs_u64(w.keys_in, w.keys_out, w.perm, a.n_total * a.n_views, 33 + sbits + vbits, w.sort_ws, stream);
  if (rc != SST_OK) return rc;
  if (W == 10) launch_gather<10>(a, w, sbits, vbits, st);           // 5 columns + yaw, size, score
  else if (W == 11) launch_gather<11>(a, w, sbits, vbits, st);      // ... and length
  else launch_gather<0>(a, w, sbits, vbits, st);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int sst_tracklet_tta_boxes_f32(const sst_tracklet_tta_box_args* args, void* stream) {
  if (args == nullptr) return SST_ERR_ARG;
  const sst_tracklet_tta_box_args& a = *args;
  if (a.cols != 7 && a.cols != 9) return SST_ERR_UNSUPPORTED;
  if (a.n_views > kMaxViews) return SST_ERR_UNSUPPORTED;
  if (a.batch < 1 || a.n_views < 1 || a.n_boxes < 0 || a.box_offsets == nullptr || a.params == nullptr) return SST_ERR_ARG;
  if ((int64_t)a.n_boxes * a.n_views > (int64_t)INT32_MAX - kBlock) return SST_ERR_UNSUPPORTED;
  if (a.n_boxes == 0) return SST_OK;
  if (a.boxes == nullptr || a.boxes_out == nullptr) return SST_ERR_ARG;
  hipLaunchKernelGGL(tta_boxes_kernel, dim3((unsigned)sst_div_up((int64_t)a.n_boxes * a.n_views, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int64_t sst_tracklet_tta_finish_workspace_bytes(int64_t n_rows, int n_views) {
  if (n_rows < 0 || n_views < 1 || n_views > kMaxViews) return 0;
  const int64_t rows = (n_rows > 0 ? n_rows : 1) * n_views;
  return sst_align_up(rows * 8, 16) + sst_align_up(rows * 7 * 4, 16);
}

int sst_tracklet_tta_finish(const sst_tracklet_tta_finish_args* args, void* stream) {
  if (args == nullptr) return SST_ERR_ARG;
  const sst_tracklet_tta_finish_args& a = *args;
  if (a.n_views > kMaxViews) return SST_ERR_UNSUPPORTED;
  if (a.mode != SST_TRK_TTA_MERGE_MAX && a.mode != SST_TRK_TTA_MERGE_WEIGHTED && a.mode != SST_TRK_TTA_MERGE_IOU_CLAMPED)
    return SST_ERR_UNSUPPORTED;
  if (a.n_rows < 0 || a.n_views < 1) return SST_ERR_ARG;
  if (a.n_rows * a.n_views > (int64_t)INT32_MAX) return SST_ERR_UNSUPPORTED;
  if (a.n_rows == 0) return SST_OK;
  if (a.boxes == nullptr || a.scores == nullptr || a.valid == nullptr || a.old_boxes == nullptr || a.old_scores == nullptr ||
      a.mats == nullptr || a.merged_boxes == nullptr || a.merged_scores == nullptr)
    return SST_ERR_ARG;
  if ((a.view_boxes == nullptr) != (a.view_scores == nullptr)) return SST_ERR_ARG;
  float* vb = a.view_boxes;
  double* vs = a.view_scores;
  if (vb == nullptr) {                                    // nobody asked for the per-view boxes: they live in the workspace
    if (a.workspace == nullptr || ((uintptr_t)a.workspace & 15) ||
        a.workspace_bytes < sst_tracklet_tta_finish_workspace_bytes(a.n_rows, a.n_views))
      return SST_ERR_ARG;
    vs = (double*)a.workspace;
    vb = (float*)((char*)a.workspace + sst_align_up(a.n_rows * a.n_views * 8, 16));
  }
  hipLaunchKernelGGL(tta_finish_kernel, dim3((unsigned)sst_div_up(a.n_rows, kFinishBlock)), dim3(kFinishBlock), 0,
                     (hipStream_t)stream, a, vb, vs);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

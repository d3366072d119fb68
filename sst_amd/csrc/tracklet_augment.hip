// The point side of a CTRL tracklet pipeline on the device: what the reference's TrackletPoseTransform
// (mmdet3d/datasets/pipelines/tracklet_pipelines.py:149-208), PointDecoration (:455-506), TrackletRandomFlip (:414-439),
// TrackletGlobalRotScaleTrans (:329-355), PointsRangeFilter and PointShuffle do to the points of a batch of tracklets, whose
// rows lie sample after sample and frame after frame.
//
// One classify launch (a lane per input row: the row's frame by a binary search over the sample's frame offsets staged in
// LDS, the frame's 3 x 4 matrix, the per-sample record, the range, one 64-bit key per row, an integer count per sample), ONE
// sst_sort_pairs_u64 of the keys of augment.hip (dropped | sample | key32), and one gather launch that reads every survivor's
// input row again through the permutation, applies the same two transforms (so the bits are the classify launch's), appends
// the D decoration values of the row's frame and writes rows and frame-index values through LDS as contiguous spans.  The
// survivors sort in front of the dropped rows, sample after sample: the output row of a survivor IS its sorted position.
//
// The boxes of the tracklets and candidates go through sst_augment_boxes_f32 (augment.hip) as they are.
//
// PARITY.  Built without floating-point contraction (Makefile).  Integer atomics only; two runs are bit-equal.
#include "augment_common.h"

namespace {

using sst_aug::kBlock;
using sst_aug::sample_bits;
using sst_aug::sample_of_block;
using sst_aug::shuffle_key;
using sst_aug::transform_point;
constexpr int kMaxCols = SST_AUG_MAX_COLS;
constexpr int kMaxDeco = SST_TRK_AUG_MAX_DECO;
constexpr int kMaxFrames = SST_TRK_AUG_MAX_FRAMES;
constexpr int kMatFloats = 12;

struct Work {
  uint64_t* keys_in;
  uint64_t* keys_out;
  uint32_t* perm;
  int32_t* row_frame;            // the frame (index into `frames`) of every input row, written by the classify launch
  void* sort_ws;
  int64_t bytes;
};

Work carve(void* base, int64_t n) {
  sst_carver c(base);
  Work w;
  w.keys_in = c.take<uint64_t>(n);
  w.keys_out = c.take<uint64_t>(n);
  w.perm = c.take<uint32_t>(n);
  w.row_frame = c.take<int32_t>(n);
  w.sort_ws = c.take<char>(sst_sort_workspace_bytes(n));
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

__global__ __launch_bounds__(kBlock) void trk_classify_kernel(sst_tracklet_augment_args a, uint64_t* __restrict__ keys,
                                                              int32_t* __restrict__ row_frame, int sbits) {
  __shared__ int32_t frame_at[kMaxFrames + 1];        // the sample's frame offsets, relative to its first row
  const int s = sample_of_block(a.block_offsets, a.batch, (int)blockIdx.x);
  if (s < 0) return;
  const int f0 = a.sample_frames[s];
  int nf = a.sample_frames[s + 1] - f0;
  if (f0 < 0 || nf < 0 || nf > kMaxFrames || (int64_t)f0 + nf > a.n_frames) nf = 0;   // a table that disagrees reads nothing
  const int64_t row0 = nf > 0 ? (int64_t)a.frame_rows[f0] : 0;
  for (int k = threadIdx.x; k <= nf; k += kBlock) frame_at[k] = nf > 0 ? (int32_t)((int64_t)a.frame_rows[f0 + k] - row0) : 0;
  __syncthreads();
  const int64_t n_s = frame_at[nf];
  const int64_t r = (int64_t)((int)blockIdx.x - a.block_offsets[s]) * kBlock + threadIdx.x;
  const bool active = nf > 0 && r < n_s && row0 >= 0 && row0 + r < a.n_total;
  bool keep = false;
  if (active) {
    int lo = 0, hi = nf - 1;                            // the first frame k with frame_at[k + 1] > r: empty frames own no row
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)frame_at[mid + 1] > r) hi = mid;
      else lo = mid + 1;
    }
    const int f = f0 + lo;
    const sst_augment_params p = a.params[s];
    const float* src = a.points + (row0 + r) * a.cols;
    float x = src[0], y = src[1], z = src[2];
    pose_point(a.frames + (int64_t)f * (kMatFloats + a.deco), x, y, z);
    keep = transform_point(p, x, y, z);
    const uint32_t key32 = p.shuffle ? shuffle_key(p.seed, (uint32_t)s, (uint32_t)r) : (uint32_t)r;
    keys[row0 + r] = ((uint64_t)(keep ? 0 : 1) << (32 + sbits)) | ((uint64_t)(uint32_t)s << 32) | key32;
    row_frame[row0 + r] = f;
  }
  const int cnt = __popcll(__ballot(keep));
  if (sst_lane() == 0 && cnt > 0) atomicAdd(&a.counts[s], cnt);
}

// one lane per output row; the rows of a workgroup leave as one contiguous span.  CT, DT: the input columns and decoration
// values at compile time (the shipped widths), or 0, 0: read from the arguments (the stage then holds the widest row)
template <int CT, int DT>
__global__ __launch_bounds__(kBlock) void trk_gather_kernel(sst_tracklet_augment_args a, const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ perm,
                                                            const int32_t* __restrict__ row_frame, int sbits) {
  constexpr int kStageCols = CT ? CT + DT : kMaxCols + kMaxDeco;
  __shared__ __attribute__((aligned(16))) float stage[kBlock * kStageCols];
  const int C = CT ? CT : a.cols;
  const int D = CT ? DT : a.deco;
  const int W = C + D;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool valid = false;
  if (j < a.n_total) {
    const uint64_t key = keys[j];
    const int s = (int)((key >> 32) & ((1ull << sbits) - 1));
    const uint32_t g = perm[j];
    valid = (key >> (32 + sbits)) == 0 && s < a.batch && (int64_t)g < a.n_total;
    if (valid) {
      const int f = row_frame[g];
      valid = f >= 0 && f < a.n_frames;
      if (valid) {
        const float* src = a.points + (int64_t)g * C;
        const float* rec = a.frames + (int64_t)f * (kMatFloats + D);
        float* dst = stage + threadIdx.x * W;
        float x = src[0], y = src[1], z = src[2];
        pose_point(rec, x, y, z);
        const sst_augment_params p = a.params[s];
        transform_point(p, x, y, z);
        dst[0] = x;
        dst[1] = y;
        dst[2] = z;
        if constexpr (CT != 0) {
#pragma unroll
          for (int k = 3; k < CT; ++k) dst[k] = src[k];
#pragma unroll
          for (int k = 0; k < DT; ++k) dst[CT + k] = rec[kMatFloats + k];
        } else {
          for (int k = 3; k < C; ++k) dst[k] = src[k];
          for (int k = 0; k < D; ++k) dst[C + k] = rec[kMatFloats + k];
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

template <int CT, int DT>
void launch_gather(const sst_tracklet_augment_args& a, const Work& w, int sbits, hipStream_t st) {
  hipLaunchKernelGGL((trk_gather_kernel<CT, DT>), dim3((unsigned)sst_div_up(a.n_total, kBlock)), dim3(kBlock), 0, st, a,
                     w.keys_out, w.perm, w.row_frame, sbits);
}

}  // namespace

extern "C" {

int64_t sst_tracklet_augment_workspace_bytes(int64_t n_total, int batch) {
  if (n_total < 0 || batch < 1 || n_total > (int64_t)INT32_MAX - kBlock) return 0;
  return carve(nullptr, n_total > 0 ? n_total : 1).bytes;
}

int sst_tracklet_augment_points_f32(const sst_tracklet_augment_args* args, void* stream) {
  if (args == nullptr) return SST_ERR_ARG;
  const sst_tracklet_augment_args& a = *args;
  if (a.cols < 3 || a.cols > kMaxCols || a.deco < 0 || a.deco > kMaxDeco) return SST_ERR_UNSUPPORTED;
  if (a.max_frames > kMaxFrames) return SST_ERR_UNSUPPORTED;
  if (a.n_total < 0 || a.batch < 1 || a.n_blocks < 0 || a.n_frames < 0 || a.max_frames < 0 || a.counts == nullptr)
    return SST_ERR_ARG;
  if (a.n_total > (int64_t)INT32_MAX - kBlock) return SST_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  SST_HIP(hipMemsetAsync(a.counts, 0, sizeof(int32_t) * a.batch, st));
  if (a.n_total == 0) return SST_OK;
  if (a.points == nullptr || a.frame_rows == nullptr || a.sample_frames == nullptr || a.block_offsets == nullptr ||
      a.frames == nullptr || a.frame_values == nullptr || a.params == nullptr || a.out == nullptr ||
      a.out_frame_inds == nullptr || a.workspace == nullptr || a.n_blocks < 1 || a.n_frames < 1)
    return SST_ERR_ARG;
  if (((uintptr_t)a.points | (uintptr_t)a.out | (uintptr_t)a.workspace) & 15) return SST_ERR_ARG;
  const Work w = carve(a.workspace, a.n_total);
  if (a.workspace_bytes < w.bytes) return SST_ERR_ARG;
  const int sbits = sample_bits(a.batch);
  hipLaunchKernelGGL(trk_classify_kernel, dim3((unsigned)a.n_blocks), dim3(kBlock), 0, st, a, w.keys_in, w.row_frame, sbits);
  SST_LAUNCH_CHECK();
  const int rc = sst_sort_pairs_u64(w.keys_in, w.keys_out, w.perm, a.n_total, 33 + sbits, w.sort_ws, stream);
  if (rc != SST_OK) return rc;
  if (a.cols == 5 && a.deco == 5) launch_gather<5, 5>(a, w, sbits, st);            // yaw, size, score
  else if (a.cols == 5 && a.deco == 6) launch_gather<5, 6>(a, w, sbits, st);       // ... and length
  else launch_gather<0, 0>(a, w, sbits, st);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

// Training augmentation of points and boxes on the device: what a shipped train_pipeline does between
// db_sampler.sample_all and the collate - ObjectSample's removal of the points inside the pasted boxes
// (mmdet3d/datasets/pipelines/transforms_3d.py:262-279, :332-334), RandomFlip3D (:95-172), GlobalRotScaleTrans (:564-676),
// PointsRangeFilter / ObjectRangeFilter (:745-851) and PointShuffle (:679-700) - for a whole packed batch.
//
// Points.  One classify launch (a lane per input row: six plane tests per pasted box with the planes staged in LDS, the
// transform, the range, one 64-bit key per row and an integer count per sample), ONE sst_sort_pairs_u64 of
//   key = dropped << (32 + sample_bits) | sample << 32 | key32,    key32 = the row's index in its sample, or with `shuffle`
//   the high word of splitmix64(seed + 0x9E3779B97F4A7C15 * ((sample << 32 | row) + 1)),
// and one gather launch that reads the input row of every survivor again through the permutation, transforms it with the same
// function (so the bits are the classify launch's) and writes the packed output through LDS as contiguous spans.  The sort is
// stable: equal keys keep their input order.  Survivors sort in front of the dropped rows, sample after sample, so the output
// row of a survivor IS its position after the sort.
//
// Boxes.  One workgroup per sample; the kept boxes and labels keep their order (ranks by wave ballots).
//
// PARITY.  Built without floating-point contraction (Makefile): every product and sum below is rounded on its own, in the
// order include/sst_amd.h states.  Integer atomics only; two runs with the same inputs are bit-equal.
#include "augment_common.h"

namespace {

using sst_aug::kBlock;
using sst_aug::sample_bits;
using sst_aug::sample_of_block;
using sst_aug::shuffle_key;
using sst_aug::transform_point;   // one definition for this file and tracklet_augment.hip
constexpr int kWaves = kBlock / 64;
constexpr int kPlaneChunk = 64;            // pasted boxes staged in LDS at a time: 64 * 24 floats = 6 KiB
constexpr int kMaxCols = SST_AUG_MAX_COLS;

struct Work {
  uint64_t* keys_in;
  uint64_t* keys_out;
  uint32_t* perm;
  void* sort_ws;
  int64_t bytes;
};

Work carve(void* base, int64_t n) {
  sst_carver c(base);
  Work w;
  w.keys_in = c.take<uint64_t>(n);
  w.keys_out = c.take<uint64_t>(n);
  w.perm = c.take<uint32_t>(n);
  w.sort_ws = c.take<char>(sst_sort_workspace_bytes(n));
  w.bytes = c.off;
  return w;
}

__global__ __launch_bounds__(kBlock) void aug_classify_kernel(sst_augment_args a, uint64_t* __restrict__ keys, int sbits) {
  __shared__ float planes[kPlaneChunk * 24];
  const int s = sample_of_block(a.block_offsets, a.batch, (int)blockIdx.x);
  if (s < 0) return;
  const int64_t row0 = a.row_offsets[s];
  const int64_t n_s = a.row_offsets[s + 1] - row0;
  const int64_t r = (int64_t)((int)blockIdx.x - a.block_offsets[s]) * kBlock + threadIdx.x;
  const bool active = r < n_s && row0 >= 0 && row0 + r < a.n_total;   // a table that disagrees with n_total reads nothing
  const sst_augment_params p = a.params[s];
  float x = 0.f, y = 0.f, z = 0.f;
  if (active) {
    const float* src = a.points + (row0 + r) * a.cols;
    x = src[0];
    y = src[1];
    z = src[2];
  }
  // removal: the sample's own rows (not the pasted ones) that lie inside a pasted box
  bool inside = false;
  const bool tested = active && r >= (int64_t)a.n_pasted[s];
  const int box0 = a.plane_offsets[s];
  const int n_box = box0 >= 0 && a.plane_offsets[s + 1] <= a.n_planes ? a.plane_offsets[s + 1] - box0 : 0;
  for (int c0 = 0; c0 < n_box; c0 += kPlaneChunk) {
    const int nc = min(kPlaneChunk, n_box - c0);
    __syncthreads();
    for (int k = threadIdx.x; k < nc * 24; k += kBlock) planes[k] = a.planes[(int64_t)(box0 + c0) * 24 + k];
    __syncthreads();
    if (tested && !inside) {
      for (int j = 0; j < nc; ++j) {
        const float* q = planes + j * 24;
        bool in = true;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const float sgn = __fadd_rn(
              __fadd_rn(__fadd_rn(__fmul_rn(x, q[4 * k]), __fmul_rn(y, q[4 * k + 1])), __fmul_rn(z, q[4 * k + 2])), q[4 * k + 3]);
          in = in && sgn < 0.f;
        }
        inside = inside || in;
      }
    }
  }
  bool keep = false;
  if (active && !inside) keep = transform_point(p, x, y, z);
  if (active) {
    const uint32_t key32 = p.shuffle ? shuffle_key(p.seed, (uint32_t)s, (uint32_t)r) : (uint32_t)r;
    keys[row0 + r] = ((uint64_t)(keep ? 0 : 1) << (32 + sbits)) | ((uint64_t)(uint32_t)s << 32) | key32;
  }
  const int cnt = __popcll(__ballot(keep));
  if (sst_lane() == 0 && cnt > 0) atomicAdd(&a.counts[s], cnt);
}

// one lane per output row; the rows of a workgroup leave as one contiguous span
template <int C>
__global__ __launch_bounds__(kBlock) void aug_gather_kernel(sst_augment_args a, const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ perm, int sbits) {
  __shared__ __attribute__((aligned(16))) float stage[kBlock * C];
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool valid = false;
  if (j < a.n_total) {
    const uint64_t key = keys[j];
    valid = (key >> (32 + sbits)) == 0;
    if (valid) {
      const int s = (int)((key >> 32) & ((1ull << sbits) - 1));
      const float* src = a.points + (int64_t)perm[j] * C;
      __attribute__((aligned(16))) float v[C];
      if constexpr (C % 4 == 0) {
#pragma unroll
        for (int k = 0; k < C; k += 4) *(float4*)(v + k) = *(const float4*)(src + k);
      } else if constexpr (C % 2 == 0) {
#pragma unroll
        for (int k = 0; k < C; k += 2) *(float2*)(v + k) = *(const float2*)(src + k);
      } else {
#pragma unroll
        for (int k = 0; k < C; ++k) v[k] = src[k];
      }
      const sst_augment_params p = a.params[s];
      transform_point(p, v[0], v[1], v[2]);
      // NormalizePoints (mmdet3d/datasets/pipelines/loading.py:1044-1048) on the attribute columns it names: (v - mean) / std
#pragma unroll
      for (int k = 3; k < C; ++k)
        if ((a.norm_mask >> k) & 1) v[k] = __fdiv_rn(__fsub_rn(v[k], a.norm_mean[k]), a.norm_std[k]);
#pragma unroll
      for (int k = 0; k < C; ++k) stage[threadIdx.x * C + k] = v[k];
    }
  }
  const int rows = __syncthreads_count(valid);          // the survivors are a prefix of the sorted rows
  const int total = rows * C;
  float* dst = a.out + (int64_t)blockIdx.x * kBlock * C;   // 16-byte aligned: kBlock * C * 4 bytes per workgroup
  const int quads = total >> 2;
  for (int e = threadIdx.x; e < quads; e += kBlock) ((float4*)dst)[e] = ((const float4*)stage)[e];
  for (int e = (quads << 2) + threadIdx.x; e < total; e += kBlock) dst[e] = stage[e];
}

// one workgroup per sample: flips, rotation, scale, translation, the BEV range, limit_yaw; kept rows keep their order
__global__ __launch_bounds__(kBlock) void aug_boxes_kernel(sst_augment_box_args a) {
  __shared__ int32_t wcnt[kWaves];
  const int s = blockIdx.x;
  const int D = a.cols;
  const int b0 = a.box_offsets[s];
  const int n = b0 >= 0 && a.box_offsets[s + 1] <= a.n_boxes ? a.box_offsets[s + 1] - b0 : 0;
  const sst_augment_params p = a.params[s];
  const bool rotate = a.always_rotate ? true : p.rotate != 0;
  const int wave = threadIdx.x >> 6, lane = sst_lane();
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += kBlock) {
    const int i = c0 + threadIdx.x;
    const bool active = i < n;
    float v[9];
    bool keep = false;
    if (active) {
      const float* src = a.boxes + (int64_t)(b0 + i) * D;
      for (int k = 0; k < 9; ++k) v[k] = k < D ? src[k] : 0.f;
      if (p.flip_h) {
        v[1] = -v[1];
        v[8] = -v[8];
        v[6] = __fadd_rn(-v[6], 3.14159274101257324f);   // -yaw + (float)pi
      }
      if (p.flip_v) {
        v[0] = -v[0];
        v[7] = -v[7];
        v[6] = -v[6];
      }
      if (rotate) {
        const float xr = __fadd_rn(__fmul_rn(v[0], p.cos), __fmul_rn(v[1], p.sin));
        const float yr = __fadd_rn(__fmul_rn(v[0], -p.sin), __fmul_rn(v[1], p.cos));
        v[0] = xr;
        v[1] = yr;
        v[6] = __fadd_rn(v[6], p.angle);
        const float vx = __fadd_rn(__fmul_rn(v[7], p.cos), __fmul_rn(v[8], p.sin));
        const float vy = __fadd_rn(__fmul_rn(v[7], -p.sin), __fmul_rn(v[8], p.cos));
        v[7] = vx;
        v[8] = vy;
      }
      for (int k = 0; k < 6; ++k) v[k] = __fmul_rn(v[k], p.scale);
      v[7] = __fmul_rn(v[7], p.scale);
      v[8] = __fmul_rn(v[8], p.scale);
      for (int k = 0; k < 3; ++k) v[k] = __fadd_rn(v[k], p.trans[k]);
      keep = true;
      if (a.filter) {
        keep = v[0] > p.range[0] && v[1] > p.range[1] && v[0] < p.range[3] && v[1] < p.range[4];
        // limit_period(yaw, 0.5, 2 pi): yaw - floor(yaw / period + offset) * period, each operation in fp32
        const float period = 6.28318548202514648f;
        v[6] = __fsub_rn(v[6], __fmul_rn(floorf(__fadd_rn(__fdiv_rn(v[6], period), 0.5f)), period));
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int rank = base + __popcll(m & ((1ull << lane) - 1ull));
    int chunk = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) rank += wcnt[w];
      chunk += wcnt[w];
    }
    if (keep) {
      float* dst = a.boxes_out + (int64_t)(b0 + rank) * D;
      for (int k = 0; k < D; ++k) dst[k] = v[k];
      if (a.labels != nullptr) a.labels_out[b0 + rank] = a.labels[b0 + i];
    }
    base += chunk;
    __syncthreads();
  }
  if (threadIdx.x == 0) a.counts[s] = base;
}

template <int C>
void launch_gather(const sst_augment_args& a, const Work& w, int sbits, hipStream_t st) {
  hipLaunchKernelGGL(aug_gather_kernel<C>, dim3((unsigned)sst_div_up(a.n_total, kBlock)), dim3(kBlock), 0, st, a, w.keys_out,
                     w.perm, sbits);
}

}  // namespace

extern "C" {

int sst_augment_plane_chunk(void) { return kPlaneChunk; }

int64_t sst_augment_workspace_bytes(int64_t n_total, int batch) {
  if (n_total < 0 || batch < 1 || n_total > (int64_t)INT32_MAX - kBlock) return 0;
  return carve(nullptr, n_total > 0 ? n_total : 1).bytes;
}

int sst_augment_points_f32(const sst_augment_args* args, void* stream) {
  if (args == nullptr) return SST_ERR_ARG;
  const sst_augment_args& a = *args;
  if (a.cols < 3 || a.cols > kMaxCols) return SST_ERR_UNSUPPORTED;
  if (a.n_total < 0 || a.batch < 1 || a.n_blocks < 0 || a.counts == nullptr) return SST_ERR_ARG;
  if (a.n_total > (int64_t)INT32_MAX - kBlock) return SST_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  SST_HIP(hipMemsetAsync(a.counts, 0, sizeof(int32_t) * a.batch, st));
  if (a.n_total == 0) return SST_OK;
  if (a.points == nullptr || a.row_offsets == nullptr || a.n_pasted == nullptr || a.block_offsets == nullptr ||
      a.params == nullptr || a.plane_offsets == nullptr || a.n_planes < 0 || (a.n_planes > 0 && a.planes == nullptr) || a.out == nullptr || a.workspace == nullptr || a.n_blocks < 1)
    return SST_ERR_ARG;
  if (((uintptr_t)a.points | (uintptr_t)a.out | (uintptr_t)a.workspace) & 15) return SST_ERR_ARG;
  const Work w = carve(a.workspace, a.n_total);
  if (a.workspace_bytes < w.bytes) return SST_ERR_ARG;
  const int sbits = sample_bits(a.batch);
  hipLaunchKernelGGL(aug_classify_kernel, dim3((unsigned)a.n_blocks), dim3(kBlock), 0, st, a, w.keys_in, sbits);
  SST_LAUNCH_CHECK();
  const int rc = sst_sort_pairs_u64(w.keys_in, w.keys_out, w.perm, a.n_total, 33 + sbits, w.sort_ws, stream);
  if (rc != SST_OK) return rc;
  switch (a.cols) {
    case 3: launch_gather<3>(a, w, sbits, st); break;
    case 4: launch_gather<4>(a, w, sbits, st); break;
    case 5: launch_gather<5>(a, w, sbits, st); break;
    case 6: launch_gather<6>(a, w, sbits, st); break;
    case 7: launch_gather<7>(a, w, sbits, st); break;
    default: launch_gather<8>(a, w, sbits, st); break;
  }
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int sst_augment_boxes_f32(const sst_augment_box_args* args, void* stream) {
  if (args == nullptr) return SST_ERR_ARG;
  const sst_augment_box_args& a = *args;
  if (a.cols != 7 && a.cols != 9) return SST_ERR_UNSUPPORTED;
  if (a.batch < 1 || a.n_boxes < 0 || a.box_offsets == nullptr || a.params == nullptr || a.counts == nullptr) return SST_ERR_ARG;
  if (a.n_boxes > 0 && (a.boxes == nullptr || a.boxes_out == nullptr || (a.labels != nullptr && a.labels_out == nullptr)))
    return SST_ERR_ARG;
  hipLaunchKernelGGL(aug_boxes_kernel, dim3((unsigned)a.batch), dim3(kBlock), 0, (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

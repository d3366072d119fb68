// Rotated-box operations of the detection heads and the FSD training step: BEV overlap / IoU of box pairs (matrix and
// aligned), NMS over score-sorted boxes with a device-side sweep, and points in boxes.
//
// The BEV polygon arithmetic (bev_clip.h, shared with roi_head.hip) restates the reference's iou3d kernels
// (ops/iou3d/src/iou3d_kernel.cu:54-251, 335-343):
// boxes [x1, y1, x2, y2, ry], corners rotated about the centre (rotate_around_center), edge intersections with strict
// sign tests and the EPS fallback (intersection), corners of one box inside the other with a 1e-5 margin
// (check_in_box2d), points sorted by atan2 about their mean, area as a fan from vertex 0.  The polygon points go to
// LDS (per-thread columns of a [slot][lane] array), so the dynamically indexed lists never spill to scratch.  This
// file is built without floating-point contraction (Makefile) so that every product and sum rounds on its own, as
// in the reference and in the float32 restatement of the tests (tests/box_ops_ref.py).
//
// Points in boxes uses dpp_classify of pib_test.h, the membership test of the dynamic point pool.
#include "common.h"
#include "pib_test.h"
#include "bev_clip.h"

namespace {

// iou_normal (iou3d_kernel.cu:335-343): the angle is ignored
__device__ __forceinline__ float axis_iou(const float* a, const float* b) {
  const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
  const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
  const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
  const float inter = w * h;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]);
  const float sb = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / fmaxf(sa + sb - inter, kIouEps);
}

__device__ __forceinline__ float pair_value(const float* a, const float* b, int mode, float* lx, float* ly, float* lk) {
  if (mode == SST_BOX_OVERLAP) return bev_overlap(a, b, lx, ly, lk);
  if (mode == SST_BOX_IOU) return bev_iou(a, b, lx, ly, lk);
  return axis_iou(a, b);
}

__device__ __forceinline__ void load_box5(const float* __restrict__ src, float (&dst)[5]) {
#pragma unroll
  for (int k = 0; k < 5; ++k) dst[k] = src[k];
}

#define SST_POLY_LDS                                   \
  __shared__ float poly_x[kPolyCap * kPolyBlock];      \
  __shared__ float poly_y[kPolyCap * kPolyBlock];      \
  __shared__ float poly_k[kPolyCap * kPolyBlock];      \
  float* lx = poly_x + threadIdx.x;                    \
  float* ly = poly_y + threadIdx.x;                    \
  float* lk = poly_k + threadIdx.x

// out[i, j] = value(a_i, b_j), flat grid-stride over n_a * n_b (row-major: consecutive lanes write consecutive j)
__global__ __launch_bounds__(kPolyBlock) void box_pairs_k(const float* __restrict__ ba, int64_t n_a,
                                                          const float* __restrict__ bb, int64_t n_b, int mode,
                                                          float* __restrict__ out) {
  SST_POLY_LDS;
  const int64_t total = n_a * n_b;
  for (int64_t idx = (int64_t)blockIdx.x * kPolyBlock + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * kPolyBlock) {
    const int64_t i = idx / n_b, j = idx - i * n_b;
    float a[5], b[5];
    load_box5(ba + i * 5, a);
    load_box5(bb + j * 5, b);
    out[idx] = pair_value(a, b, mode, lx, ly, lk);
  }
}

// out[i] = value(a_i, b_i): the same device function as box_pairs_k, hence bit-identical to its diagonal
__global__ __launch_bounds__(kPolyBlock) void box_aligned_k(const float* __restrict__ ba, const float* __restrict__ bb,
                                                            int64_t n, int mode, float* __restrict__ out) {
  SST_POLY_LDS;
  for (int64_t i = (int64_t)blockIdx.x * kPolyBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPolyBlock) {
    float a[5], b[5];
    load_box5(ba + i * 5, a);
    load_box5(bb + i * 5, b);
    out[i] = pair_value(a, b, mode, lx, ly, lk);
  }
}

constexpr int kNmsMaxGroups = 64;
struct NmsGroupThr {  // per-group thresholds, passed by value (no host-to-device copy per call)
  float t[kNmsMaxGroups];
};

// NMS suppression mask (nms_kernel / nms_normal_kernel, iou3d_kernel.cu:284-333 / :345-): one workgroup per 64 x 64
// tile (row block r = blockIdx.y, column block c = blockIdx.x); bit k of mask[i * col_blocks + c] = box i suppresses
// box c * 64 + k (same group, IoU strictly above the group's threshold).  Tiles below the diagonal are neither
// computed nor written: the sweep never reads them.
__global__ __launch_bounds__(kPolyBlock) void nms_mask_k(const float* __restrict__ boxes,
                                                         const int32_t* __restrict__ group, int n, int col_blocks,
                                                         float thresh, NmsGroupThr group_thr, int n_groups, int rotated,
                                                         unsigned long long* __restrict__ mask) {
  const int r = blockIdx.y, c = blockIdx.x;
  if (c < r) return;
  SST_POLY_LDS;
  __shared__ float cbox[kPolyBlock][5];
  __shared__ int cgroup[kPolyBlock];
  const int tid = threadIdx.x;
  const int row_size = min(n - r * kPolyBlock, kPolyBlock);
  const int col_size = min(n - c * kPolyBlock, kPolyBlock);
  if (tid < col_size) {
    const int j = c * kPolyBlock + tid;
#pragma unroll
    for (int k = 0; k < 5; ++k) cbox[tid][k] = boxes[(int64_t)j * 5 + k];
    cgroup[tid] = group ? group[j] : 0;
  }
  __syncthreads();
  if (tid >= row_size) return;
  const int i = r * kPolyBlock + tid;
  const int g = group ? group[i] : 0;
  // a group id outside [0, n_groups) suppresses nothing (and, having no partner in its group, is never suppressed)
  const float thr = !group ? thresh : (g >= 0 && g < n_groups) ? group_thr.t[g] : __builtin_inff();
  unsigned long long t = 0;
  if (thr < __builtin_inff()) {  // +inf (no suppression) or NaN: no IoU can pass, none is computed
    float cur[5];
    load_box5(boxes + (int64_t)i * 5, cur);
    for (int k = (r == c ? tid + 1 : 0); k < col_size; ++k) {
      if (cgroup[k] != g) continue;
      const float v = rotated ? bev_iou(cur, cbox[k], lx, ly, lk) : axis_iou(cur, cbox[k]);
      if (v > thr) t |= 1ull << k;
    }
  }
  mask[(int64_t)i * col_blocks + c] = t;
}

constexpr int kSweepThreads = 256;
constexpr int kFoldRows = kPolyBlock / (kSweepThreads / 64);  // rows of a 64-row block folded by each wave: 16

// The reference's host loop (iou3d.cpp:116-133) on the device, one workgroup of four waves; the removal bit vector
// lives in LDS.  Per 64-row block r:
//   1. every wave issues the loads of its 16 rows' words for the first 64 column blocks right of r.  They do not depend
//      on which rows survive, so they are in flight while the block is resolved;
//   2. every wave resolves the block itself (identically: lane t holds row t's diagonal word, the next block's words
//      are already loaded), serially over the 64 rows with readlane; wave 0 appends the kept rows to the keep list;
//   3. each wave ORs the words of its kept rows (a mask select, no branch) and merges them into the removal vector with
//      an LDS atomic OR; further column chunks load their 16 words at once, then OR.
// No load waits on another load of the same block: one round trip per column chunk, not one per kept row.
__global__ __launch_bounds__(kSweepThreads) void nms_sweep_k(const unsigned long long* __restrict__ mask, int n,
                                                             int col_blocks, int64_t* __restrict__ keep,
                                                             int32_t* __restrict__ num_keep) {
  extern __shared__ unsigned long long remv[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ld = col_blocks;
  for (int j = tid; j < col_blocks; j += kSweepThreads) remv[j] = 0ull;
  unsigned long long diag_next = lane < n ? mask[(int64_t)lane * ld] : 0ull;
  int num = 0;
  __syncthreads();
  for (int r = 0; r < col_blocks; ++r) {
    const int64_t row0 = (int64_t)r * kPolyBlock;
    const int rows_in = (int)min((int64_t)n - row0, (int64_t)kPolyBlock);
    // 1. fold loads of the first column chunk; rows past n and columns past the end are clamped to valid words and
    //    masked out below
    const int j0 = r + 1 + lane;
    const int64_t jc0 = min(j0, col_blocks - 1);
    unsigned long long w[kFoldRows];
#pragma unroll
    for (int i = 0; i < kFoldRows; ++i) w[i] = mask[(row0 + min(wave * kFoldRows + i, rows_in - 1)) * ld + jc0];
    const unsigned long long diag = diag_next;
    if (r + 1 < col_blocks) {
      const int64_t row = row0 + kPolyBlock + lane;
      diag_next = row < n ? mask[row * ld + r + 1] : 0ull;
    }
    // 2. resolve the block
    const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
    unsigned long long cur = remv[r], kb = 0ull;
    for (int t = 0; t < rows_in; ++t) {
      const unsigned long long d = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)dhi, t) << 32) |
                                   (unsigned)__builtin_amdgcn_readlane((int)dlo, t);
      if (!((cur >> t) & 1ull)) {
        kb |= 1ull << t;
        cur |= d;
      }
    }
    if (wave == 0 && ((kb >> lane) & 1ull)) keep[num + __popcll(kb & ((1ull << lane) - 1ull))] = row0 + lane;
    num += __popcll(kb);
    // 3. fold the kept rows into the removal vector
    const unsigned long long wkb = kb >> (wave * kFoldRows);
    if (j0 < col_blocks) {
      unsigned long long acc = 0ull;
#pragma unroll
      for (int i = 0; i < kFoldRows; ++i) acc |= w[i] & (0ull - ((wkb >> i) & 1ull));
      if (acc) atomicOr(&remv[j0], acc);
    }
    if (wkb & ((1ull << kFoldRows) - 1ull)) {
      for (int jb = r + 1 + kPolyBlock; jb < col_blocks; jb += kPolyBlock) {
        const int j = jb + lane;
        const int64_t jc = min(j, col_blocks - 1);
#pragma unroll
        for (int i = 0; i < kFoldRows; ++i) w[i] = mask[(row0 + min(wave * kFoldRows + i, rows_in - 1)) * ld + jc];
        unsigned long long acc = 0ull;
#pragma unroll
        for (int i = 0; i < kFoldRows; ++i) acc |= w[i] & (0ull - ((wkb >> i) & 1ull));
        if (j < col_blocks && acc) atomicOr(&remv[j], acc);
      }
    }
    __syncthreads();
  }
  if (tid == 0) *num_keep = num;
}

constexpr int kPibFirstBoxes = 256;  // boxes per LDS tile of the first-box kernel (256 x 44 B)
constexpr int kPibRows = 64;         // points per workgroup of the membership kernel

// first box containing each point: out[b, p] = smallest box index, else -1 (points_in_boxes_kernel, :52-77)
__global__ __launch_bounds__(256) void pib_first_k(const float* __restrict__ boxes, const float* __restrict__ pts,
                                                   int64_t n_boxes, int64_t n_pts, int32_t* __restrict__ out) {
  __shared__ DppBox sb[kPibFirstBoxes];
  const int b = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  if (p < n_pts) {
    const float* q = pts + ((int64_t)b * n_pts + p) * 3;
    x = q[0];
    y = q[1];
    z = q[2];
  }
  int found = -1;
  for (int64_t t0 = 0; t0 < n_boxes; t0 += kPibFirstBoxes) {
    const int nt = (int)min((int64_t)kPibFirstBoxes, n_boxes - t0);
    __syncthreads();
    if ((int)threadIdx.x < nt) sb[threadIdx.x] = dpp_box(boxes + ((int64_t)b * n_boxes + t0 + threadIdx.x) * 7, 0.f, 0.f, 0.f);
    __syncthreads();
    if (found < 0 && p < n_pts) {
      for (int k = 0; k < nt; ++k) {
        float lx, ly, lz;
        if (dpp_classify(sb[k], x, y, z, lx, ly, lz) != 0) {
          found = (int)(t0 + k);
          break;
        }
      }
    }
  }
  if (p < n_pts) out[(int64_t)b * n_pts + p] = found;
}

// membership: out[b, p, t] = 1 if point p lies in box t (points_in_boxes_batch_kernel, :79-105).  Lane = box within a
// 64-box column tile, so a wave stores one point's 64 flags as 256 contiguous bytes; the 4 waves take every 4th point.
__global__ __launch_bounds__(256) void pib_batch_k(const float* __restrict__ boxes, const float* __restrict__ pts,
                                                   int64_t n_boxes, int64_t n_pts, int32_t* __restrict__ out) {
  __shared__ DppBox sb[64];
  const int b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.y * 64 + lane;
  if (threadIdx.x < 64 && t < n_boxes) sb[lane] = dpp_box(boxes + ((int64_t)b * n_boxes + t) * 7, 0.f, 0.f, 0.f);
  __syncthreads();
  if (t >= n_boxes) return;
  const DppBox box = sb[lane];
  const int64_t p0 = (int64_t)blockIdx.x * kPibRows;
  for (int i = wave; i < kPibRows; i += 4) {
    const int64_t p = p0 + i;
    if (p >= n_pts) break;
    const float* q = pts + ((int64_t)b * n_pts + p) * 3;
    float lx, ly, lz;
    out[((int64_t)b * n_pts + p) * n_boxes + t] = dpp_classify(box, q[0], q[1], q[2], lx, ly, lz) != 0 ? 1 : 0;
  }
}

}  // namespace

// compute-bound polygon launches: one item per lane up to 8192 one-wave workgroups (32 per CU), grid-stride beyond
static int poly_grid(int64_t items) {
  const int64_t g = sst_div_up(items, kPolyBlock);
  return (int)(g < 8192 ? g : 8192);
}

extern "C" int sst_boxes_overlap_bev_f32(const float* d_a, int64_t n_a, const float* d_b, int64_t n_b, int mode,
                                         float* d_out, void* stream) {
  if (n_a < 0 || n_b < 0 || mode < SST_BOX_OVERLAP || mode > SST_BOX_IOU_AXIS) return SST_ERR_ARG;
  if (n_a == 0 || n_b == 0) return SST_OK;
  if (!d_a || !d_b || !d_out) return SST_ERR_ARG;
  hipLaunchKernelGGL(box_pairs_k, dim3(poly_grid(n_a * n_b)), dim3(kPolyBlock), 0,
                     (hipStream_t)stream, d_a, n_a, d_b, n_b, mode, d_out);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_boxes_overlap_aligned_f32(const float* d_a, const float* d_b, int64_t n, int mode, float* d_out,
                                             void* stream) {
  if (n < 0 || mode < SST_BOX_OVERLAP || mode > SST_BOX_IOU_AXIS) return SST_ERR_ARG;
  if (n == 0) return SST_OK;
  if (!d_a || !d_b || !d_out) return SST_ERR_ARG;
  hipLaunchKernelGGL(box_aligned_k, dim3(poly_grid(n)), dim3(kPolyBlock), 0, (hipStream_t)stream,
                     d_a, d_b, n, mode, d_out);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

static const int64_t kNmsMaxBoxes = 64 * 8064;  // removal vector of the sweep: <= 8064 words, within 64 KB of LDS

extern "C" int64_t sst_nms_bev_workspace_bytes(int64_t n) {
  if (n <= 0) return 256;
  return sst_align_up(n * sst_div_up(n, 64) * 8, 256);
}

extern "C" int sst_nms_bev_f32(const float* d_sorted_boxes, const int32_t* d_group, int64_t n, float thresh,
                               const float* h_group_thresh, int n_groups, int rotated, int64_t* d_keep,
                               int32_t* d_num_keep, void* d_workspace, void* stream) {
  if (n < 0 || !d_num_keep || (d_group && (!h_group_thresh || n_groups <= 0))) return SST_ERR_ARG;
  if (n > kNmsMaxBoxes || (d_group && n_groups > kNmsMaxGroups)) return SST_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    SST_HIP(hipMemsetAsync(d_num_keep, 0, sizeof(int32_t), s));
    return SST_OK;
  }
  if (!d_sorted_boxes || !d_keep || !d_workspace) return SST_ERR_ARG;
  NmsGroupThr gt;
  for (int k = 0; k < kNmsMaxGroups; ++k) gt.t[k] = (d_group && k < n_groups) ? h_group_thresh[k] : __builtin_inff();
  const int cb = (int)sst_div_up(n, 64);
  unsigned long long* mask = (unsigned long long*)d_workspace;
  hipLaunchKernelGGL(nms_mask_k, dim3(cb, cb), dim3(kPolyBlock), 0, s, d_sorted_boxes, d_group, (int)n, cb, thresh, gt,
                     d_group ? n_groups : 0, rotated, mask);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(nms_sweep_k, dim3(1), dim3(kSweepThreads), (size_t)cb * 8, s, mask, (int)n, cb, d_keep,
                     d_num_keep);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_points_in_boxes_f32(const float* d_boxes, const float* d_pts, int batch, int64_t n_boxes,
                                       int64_t n_pts, int mode, int32_t* d_out, void* stream) {
  if (batch < 0 || n_boxes < 0 || n_pts < 0 || (mode != SST_PIB_FIRST && mode != SST_PIB_MEMBERSHIP)) return SST_ERR_ARG;
  if (batch > 65535) return SST_ERR_UNSUPPORTED;
  if (batch == 0 || n_pts == 0) return SST_OK;
  if (mode == SST_PIB_MEMBERSHIP && n_boxes == 0) return SST_OK;
  if (!d_pts || !d_out || (n_boxes > 0 && !d_boxes)) return SST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (mode == SST_PIB_FIRST) {
    hipLaunchKernelGGL(pib_first_k, dim3((unsigned)sst_div_up(n_pts, 256), batch), dim3(256), 0, s, d_boxes, d_pts,
                       n_boxes, n_pts, d_out);
  } else {
    if (sst_div_up(n_boxes, 64) > 65535) return SST_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pib_batch_k, dim3((unsigned)sst_div_up(n_pts, kPibRows), (unsigned)sst_div_up(n_boxes, 64), batch),
                       dim3(256), 0, s, d_boxes, d_pts, n_boxes, n_pts, d_out);
  }
  SST_LAUNCH_CHECK();
  return SST_OK;
}

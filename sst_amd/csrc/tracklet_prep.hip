// CTRL's offline stage: the compute loops of the reference's tools/ctrl/ scripts, each for a whole batch in one launch.
// fp32 data, int64 timestamps, integer atomics only, one host read per call, bit-reproducible.
//
// Reference (tools/ctrl, mmdet3d/core/bbox/structures):
//   sst_tracklet_affinity_f32    generate_candidates.py:39-66 (tracklet_assign: predicted x ground-truth tracklets of a segment),
//                                lidar_tracklet.py:210-229 (max_iou: set intersection, two cats, two copies, one aligned_iou_3d
//                                launch and one .item() per pair)
//   sst_box_crops_count / fill   generate_track_input.py:88-101 (extract_and_save_point: per frame and box points_in_boxes on the
//                                whole cloud, a mask, an index, a copy), remove_empty.py:82-134 (process_single_frame with
//                                box_grouping and group_size 1: does the box hold a point)
//
// PARITY.  The IoU is lidar_iou3d_pair of roi_target.h with the arguments in max_iou's order (predicted, ground truth); this file
// is built without floating-point contraction (Makefile), so a pair's value is bit-equal to the maximum of
// sst_amd.aligned_iou_3d over its shared frames.  bev_overlap's own early out (circumscribed circles apart by more than 1 cm +
// 0.1 % of the radii, where the full clip returns 0 as well) is the only reject in front of the polygon clip: it is part of the
// value the box ops compute, so nothing is added here that could change a bit.  The inside test is dpp_box(roi, 0, 0, 0) /
// dpp_classify == 1 of pib_test.h - with no enlargement the margin class 2 cannot occur, so this is sst_points_in_boxes_f32's
// "!= 0" - built from __f*_rn operations that no flag can fuse.
#include "common.h"
#include "pib_test.h"
#include "roi_target.h"
#include "tracklet_ts.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// the segment s in [0, n) with off[s] <= v < off[s + 1] of ascending offsets off[0 .. n] (empty segments are passed over)
__device__ __forceinline__ int find_segment(const int64_t* __restrict__ off, int n, int64_t v) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return min(max(v, lo), hi); }

// ------------------------------------------------------------------------------------------------------------------
// affinity: one wave per (predicted, ground-truth) pair, kWaves ground-truth tracklets of one predicted tracklet per workgroup
// ------------------------------------------------------------------------------------------------------------------

constexpr int kTsLds = 1024;  // timestamps of the predicted tracklet staged in LDS (8 KB); a longer tracklet is searched in memory

// torch.max's maximum: a NaN wins
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

__global__ __launch_bounds__(kThreads) void tracklet_affinity_k(sst_tracklet_affinity_args a) {
  // one polygon array per wave: bev_overlap strides its slots by kPolyBlock (= 64 lanes)
  __shared__ float poly_x[kWaves][kPolyCap * kPolyBlock];
  __shared__ float poly_y[kWaves][kPolyCap * kPolyBlock];
  __shared__ float poly_k[kWaves][kPolyCap * kPolyBlock];
  __shared__ int64_t s_ts[kTsLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* lx = poly_x[wave] + lane;
  float* ly = poly_y[wave] + lane;
  float* lk = poly_k[wave] + lane;
  const int p = find_segment(a.block_offsets, (int)a.n_pd, (int64_t)blockIdx.x);
  const int64_t group = (int64_t)blockIdx.x - a.block_offsets[p];
  const int64_t r0 = clamp_i64(a.pd_offsets[p], 0, a.n_pd_rows);
  const int n = (int)(clamp_i64(a.pd_offsets[p + 1], r0, a.n_pd_rows) - r0);
  const int64_t gb = clamp_i64(a.pd_gt_begin[p], 0, a.n_gt);
  const int64_t ge = clamp_i64(a.pd_gt_end[p], gb, a.n_gt);
  const bool staged = n <= kTsLds;
  if (staged)
    for (int i = tid; i < n; i += kThreads) s_ts[i] = a.pd_ts[r0 + i];
  __syncthreads();
  if (group < 0 || group > (ge - gb) / kWaves) return;
  const int64_t g = gb + group * kWaves + wave;
  if (g >= ge) return;                                  // the tail of the range: wave-uniform
  const int64_t o = a.out_offsets[p] + (g - gb);
  if (o < 0 || o >= a.n_out) return;
  const int64_t g0 = clamp_i64(a.gt_offsets[g], 0, a.n_gt_rows);
  const int m = (int)(clamp_i64(a.gt_offsets[g + 1], g0, a.n_gt_rows) - g0);
  const int64_t* __restrict__ gts = a.gt_ts + g0;
  const int64_t* pts = staged ? s_ts : a.pd_ts + r0;
  float best = 0.f;                                     // max_iou without a shared timestamp
  // the two timestamp ranges do not meet: nothing is shared (wave-uniform)
  if (n > 0 && m > 0 && !(pts[n - 1] < gts[0] || gts[m - 1] < pts[0])) {
    const float* __restrict__ pb = a.pd_boxes + r0 * 7;
    const float* __restrict__ gbx = a.gt_boxes + g0 * 7;
    for (int j = lane; j < m; j += 64) {
      const int i = staged ? find_ts(s_ts, n, gts[j]) : find_ts(a.pd_ts + r0, n, gts[j]);
      if (i >= 0) best = nan_max(best, lidar_iou3d_pair(pb + (int64_t)i * 7, gbx + (int64_t)j * 7, lx, ly, lk));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best = nan_max(best, __shfl_xor(best, d, 64));
  }
  if (lane == 0) a.affinity[o] = best;
}

// ------------------------------------------------------------------------------------------------------------------
// crops: a workgroup takes a tile of kTile consecutive points of one frame; wave w its kTile / kWaves consecutive points, a
// lane every 64th of them - so that (wave, k, lane) is the ascending point index
// ------------------------------------------------------------------------------------------------------------------

constexpr int kPerLane = 16;
constexpr int kWavePoints = 64 * kPerLane;       // 1024
constexpr int kTile = kWaves * kWavePoints;      // 4096
constexpr int kBoxChunk = 128;                   // DppBox staged at a time: 5.5 KB

struct TilePoints {
  float x[kPerLane], y[kPerLane], z[kPerLane];
  uint32_t valid;       // bit k: point k of this lane exists
  int64_t first;        // index in the frame of this lane's point 0; point k is first + 64 k
};

struct TileOf {
  int64_t p0, b0, cell0, t, T;
  int N, B;
  bool ok;
};

__device__ __forceinline__ TileOf locate_tile(const sst_box_crops_args& a) {
  TileOf o;
  const int f = find_segment(a.tile_offsets, a.n_frames, (int64_t)blockIdx.x);
  o.t = (int64_t)blockIdx.x - a.tile_offsets[f];
  o.T = a.tile_offsets[f + 1] - a.tile_offsets[f];
  o.p0 = clamp_i64(a.pt_offsets[f], 0, a.n_points);
  o.N = (int)(clamp_i64(a.pt_offsets[f + 1], o.p0, a.n_points) - o.p0);
  o.b0 = clamp_i64(a.box_offsets[f], 0, a.n_boxes);
  o.B = (int)(clamp_i64(a.box_offsets[f + 1], o.b0, a.n_boxes) - o.b0);
  o.cell0 = a.cell_offsets[f];
  o.ok = o.t >= 0 && o.t < o.T && o.B > 0 && o.t * kTile < o.N;
  return o;
}

__device__ __forceinline__ void load_tile(const sst_box_crops_args& a, const TileOf& o, TilePoints& q) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  q.first = o.t * kTile + (int64_t)wave * kWavePoints + lane;
  q.valid = 0;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int64_t i = q.first + 64 * k;
    q.x[k] = q.y[k] = q.z[k] = 0.f;
    if (i < o.N) {
      const float* __restrict__ s = a.points + (o.p0 + i) * a.cols;
      q.x[k] = s[0];
      q.y[k] = s[1];
      q.z[k] = s[2];
      q.valid |= 1u << k;
    }
  }
}

__device__ __forceinline__ bool inside(const DppBox& b, const TilePoints& q, int k) {
  float lx, ly, lz;
  return ((q.valid >> k) & 1u) && dpp_classify(b, q.x[k], q.y[k], q.z[k], lx, ly, lz) == 1;
}

__global__ __launch_bounds__(kThreads) void box_crops_count_k(sst_box_crops_args a) {
  __shared__ DppBox s_box[kBoxChunk];
  __shared__ int s_wcnt[kBoxChunk][kWaves];
  const TileOf o = locate_tile(a);
  if (!o.ok) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  TilePoints q;
  load_tile(a, o, q);
  for (int c0 = 0; c0 < o.B; c0 += kBoxChunk) {
    const int nb = min(kBoxChunk, o.B - c0);
    __syncthreads();        // the previous chunk's boxes and wave counts have been read
    if (tid < nb) s_box[tid] = dpp_box(a.boxes + (o.b0 + c0 + tid) * 7, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
      const DppBox bx = s_box[b];     // a broadcast read
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) cnt += __popcll(__ballot(inside(bx, q, k)));
      if (lane == 0) s_wcnt[b][wave] = cnt;
    }
    __syncthreads();
    if (tid < nb) {
      int c = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) c += s_wcnt[tid][w];
      if (a.tile_counts != nullptr) {
        const int64_t cell = o.cell0 + (int64_t)(c0 + tid) * o.T + o.t;
        if (cell >= 0 && cell < a.n_cells) a.tile_counts[cell] = c;
      }
      if (c != 0) atomicAdd(a.counts + o.b0 + c0 + tid, c);   // an integer sum over the tiles: any order, one result
    }
  }
}

__global__ __launch_bounds__(kThreads) void box_crops_fill_k(sst_box_crops_args a) {
  __shared__ int s_wsum[2][kWaves];
  const TileOf o = locate_tile(a);
  if (!o.ok) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  TilePoints q;
  load_tile(a, o, q);
  int parity = 0;
  for (int b = 0; b < o.B; ++b) {
    const int64_t cell = o.cell0 + (int64_t)b * o.T + o.t;
    if (cell < 0 || cell >= a.n_cells) continue;
    if (a.tile_counts[cell] == 0) continue;         // workgroup-uniform: most boxes hold no point of most tiles
    const DppBox bx = dpp_box(a.boxes + (o.b0 + b) * 7, 0.f, 0.f, 0.f);
    uint32_t mine = 0;
    int wtot = 0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const bool in = inside(bx, q, k);
      wtot += __popcll(__ballot(in));
      mine |= (in ? 1u : 0u) << k;
    }
    if (lane == 0) s_wsum[parity][wave] = wtot;
    __syncthreads();
    int64_t slot = a.tile_starts[cell];
    for (int w = 0; w < wave; ++w) slot += s_wsum[parity][w];
    parity ^= 1;            // the next box writes the other half: one barrier per box
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const bool in = (mine >> k) & 1u;
      const unsigned long long bal = __ballot(in);
      if (in) {
        const int64_t r = slot + __popcll(bal & below);
        if (r >= 0 && r < a.n_rows) {
          const int64_t i = q.first + 64 * k;
          const float* __restrict__ s = a.points + (o.p0 + i) * a.cols;
          float* __restrict__ d = a.rows + r * a.cols;
          for (int c = 0; c < a.cols; ++c) d[c] = s[c];   // any width: a 24-byte row is not 16-byte aligned
          a.src[r] = i;
        }
      }
      slot += __popcll(bal);
    }
  }
}

int check_crops(const sst_box_crops_args& a) {
  if (a.n_frames < 0 || a.n_points < 0 || a.n_boxes < 0 || a.n_tiles < 0 || a.n_cells < 0 || a.n_rows < 0 || a.cols < 3)
    return SST_ERR_ARG;
  if (a.n_points > 0x7fffffffLL || a.n_boxes > 0x7fffffffLL || a.n_tiles > 0x7fffffffLL || a.n_cells > (1ll << 31) - 2 ||
      a.n_rows > 0x7fffffffLL)
    return SST_ERR_UNSUPPORTED;
  return SST_OK;
}

}  // namespace

extern "C" int sst_tracklet_affinity_pairs_per_block(void) { return kWaves; }

extern "C" int sst_tracklet_affinity_f32(const sst_tracklet_affinity_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_tracklet_affinity_args& a = *args;
  if (a.n_pd_rows < 0 || a.n_gt_rows < 0 || a.n_pd < 0 || a.n_gt < 0 || a.n_out < 0 || a.n_blocks < 0) return SST_ERR_ARG;
  if (a.n_pd_rows > 0x7fffffffLL || a.n_gt_rows > 0x7fffffffLL || a.n_pd > 0x7fffffffLL || a.n_gt > 0x7fffffffLL ||
      a.n_blocks > 0x7fffffffLL)
    return SST_ERR_UNSUPPORTED;
  if (a.n_pd == 0 || a.n_blocks == 0) return SST_OK;
  if (!a.pd_offsets || !a.pd_gt_begin || !a.pd_gt_end || !a.out_offsets || !a.block_offsets || !a.affinity) return SST_ERR_ARG;
  if (a.n_gt > 0 && !a.gt_offsets) return SST_ERR_ARG;
  if ((a.n_pd_rows > 0 && (!a.pd_boxes || !a.pd_ts)) || (a.n_gt_rows > 0 && (!a.gt_boxes || !a.gt_ts))) return SST_ERR_ARG;
  hipLaunchKernelGGL(tracklet_affinity_k, dim3((unsigned)a.n_blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_box_crops_tile(void) { return kTile; }

extern "C" int sst_box_crops_box_chunk(void) { return kBoxChunk; }

extern "C" int64_t sst_box_crops_workspace_bytes(int64_t n_cells) { return sst_scan_workspace_bytes(n_cells > 0 ? n_cells : 1) + 256; }

extern "C" int sst_box_crops_count_f32(const sst_box_crops_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_box_crops_args& a = *args;
  const int rc = check_crops(a);
  if (rc != SST_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool with_cells = a.tile_counts != nullptr;
  if (with_cells && (!a.total || (a.n_cells > 0 && (!a.tile_starts || !a.workspace)))) return SST_ERR_ARG;
  if (with_cells && a.n_cells > 0 && a.workspace_bytes < sst_box_crops_workspace_bytes(a.n_cells)) return SST_ERR_ARG;
  if (a.n_boxes > 0 && !a.counts) return SST_ERR_ARG;
  const bool work = a.n_frames > 0 && a.n_tiles > 0 && a.n_boxes > 0;
  if (work && (!a.points || !a.boxes || !a.pt_offsets || !a.box_offsets || !a.tile_offsets || !a.cell_offsets)) return SST_ERR_ARG;
  if (a.n_boxes > 0) SST_HIP(hipMemsetAsync(a.counts, 0, sizeof(int32_t) * (size_t)a.n_boxes, st));
  if (with_cells) SST_HIP(hipMemsetAsync(a.total, 0, sizeof(int32_t), st));
  if (!work) return SST_OK;
  hipLaunchKernelGGL(box_crops_count_k, dim3((unsigned)a.n_tiles), dim3(kThreads), 0, st, a);
  SST_LAUNCH_CHECK();
  if (with_cells && a.n_cells > 0) return sst_exclusive_scan_i32(a.tile_counts, a.tile_starts, a.n_cells, a.total, a.workspace, stream);
  return SST_OK;
}

extern "C" int sst_box_crops_fill_f32(const sst_box_crops_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_box_crops_args& a = *args;
  const int rc = check_crops(a);
  if (rc != SST_OK) return rc;
  if (a.n_rows == 0 || a.n_frames == 0 || a.n_tiles == 0 || a.n_boxes == 0 || a.n_cells == 0) return SST_OK;
  if (!a.points || !a.boxes || !a.pt_offsets || !a.box_offsets || !a.tile_offsets || !a.cell_offsets || !a.tile_counts ||
      !a.tile_starts || !a.rows || !a.src)
    return SST_ERR_ARG;
  hipLaunchKernelGGL(box_crops_fill_k, dim3((unsigned)a.n_tiles), dim3(kThreads), 0, (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

// The FSD++ incremental point stage (TwoStageFSDPP's input stage): seed-box crops of the previous frames, capped per box, and
// the delta points of the current frame and of frame -1, for every sample of a batch; the points-level delta mask, the
// coordinate and mask ops it is made of, and the frame transform of up to 8 clouds in one launch.
// fp32 points, integer atomics only (bitmap bits, list cursors, box counts: order-free), no float atomics, bit-reproducible.
//
// Reference (mmdet3d/models/detectors):
//   sst_incr_voxel_coors_f32          incremental_ops.py:14-18 (voxelize_single)
//   sst_incr_mask_i32                 torchex.incremental_points_mask (incremental_ops.py:62, :121), semantics of :20-34, :83-97
//   sst_incr_delta_mask_f32           incremental_ops.py:45-63, :99-123
//   sst_incr_plan_f32 / _rows_f32     two_stage_fsdpp.py:460-503, :592-635, :637-678, :738-745
//   sst_points_frame_transform_f32    incremental_ops.py:175-186
//
// PARITY.  This file is built without floating-point contraction (Makefile).  The voxel coordinate restates torch's floor
// division (c10::div_floor_floating) operation by operation; the inside test is pib_test.h's, the one sst_points_in_boxes_f32
// answers with; the transform rounds every product and sum on its own in the order the header states.
#include "common.h"
#include "floor_div.h"
#include "pib_test.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBins = SST_INCR_MAX_FRAMES + SST_INCR_MAX_QUERIES;
constexpr int kMaxW = SST_INCR_MAX_COLS + 1;

struct Grid3 {
  int32_t x, y, z;
};

// linear cell of a triple, -1 outside the grid
__device__ __forceinline__ int64_t cell_of(const Grid3& g, int32_t cx, int32_t cy, int32_t cz) {
  if (cx < 0 || cy < 0 || cz < 0 || cx >= g.x || cy >= g.y || cz >= g.z) return -1;
  return ((int64_t)cx * g.y + cy) * g.z + cz;
}

// a base point: its bit, or a slot of the overflow list (cap entries: one per base point at the most, so it cannot overflow)
__device__ __forceinline__ void occupy(uint32_t* __restrict__ bits, int32_t* __restrict__ ovf_n, int32_t* __restrict__ ovf,
                                       int64_t cap, const Grid3& g, int32_t cx, int32_t cy, int32_t cz) {
  const int64_t c = cell_of(g, cx, cy, cz);
  if (c >= 0) {
    uint32_t* w = bits + (c >> 5);
    const uint32_t bit = 1u << (c & 31);
    if ((*(volatile const uint32_t*)w & bit) == 0) atomicOr(w, bit);  // most points share their voxel with an earlier one
    return;
  }
  const int pos = atomicAdd(ovf_n, 1);
  if (pos >= 0 && pos < cap) {
    ovf[3 * (int64_t)pos] = cx;
    ovf[3 * (int64_t)pos + 1] = cy;
    ovf[3 * (int64_t)pos + 2] = cz;
  }
}

// a queried point: new iff no base point has its triple.  Outside the grid: a linear walk of the overflow list (arrival order,
// the membership answer does not depend on it).
__device__ __forceinline__ bool is_new(const uint32_t* __restrict__ bits, const int32_t* __restrict__ ovf_n,
                                       const int32_t* __restrict__ ovf, int64_t cap, const Grid3& g, int32_t cx, int32_t cy,
                                       int32_t cz) {
  const int64_t c = cell_of(g, cx, cy, cz);
  if (c >= 0) return ((bits[c >> 5] >> (c & 31)) & 1u) == 0;
  const int64_t n = min((int64_t)max(*ovf_n, 0), cap);
  for (int64_t i = 0; i < n; ++i)
    if (ovf[3 * i] == cx && ovf[3 * i + 1] == cy && ovf[3 * i + 2] == cz) return false;
  return true;
}

__device__ __forceinline__ bool above_lo(const float* lo, float x, float y, float z) { return x > lo[0] && y > lo[1] && z > lo[2]; }

// exclusive scan of in[i * stride], i < n, by one workgroup -> out[i * stride]; returns the total (to every thread)
__device__ int block_excl_scan(const int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t n, int64_t stride, int* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int64_t i0 = 0; i0 < n; i0 += kThreads) {
    const int64_t i = i0 + threadIdx.x;
    const int v = i < n ? in[i * stride] : 0;
    const int incl = sst_wave_incl_scan(v);
    __syncthreads();
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int off = carry, all = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) off += wsum[w];
      all += wsum[w];
    }
    if (i < n) out[i * stride] = off + incl - v;
    carry += all;
  }
  return carry;
}

// ------------------------------------------------------------------------------------------------------------------
// coordinates, the integer mask, the points-level mask
// ------------------------------------------------------------------------------------------------------------------

struct F3 {
  float v[3];
};

__global__ __launch_bounds__(kThreads) void voxel_coors_k(const float* __restrict__ pts, int64_t n, int64_t ld, F3 lo, F3 vs,
                                                          int32_t* __restrict__ coors) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float* p = pts + i * ld;
#pragma unroll
  for (int c = 0; c < 3; ++c) coors[i * 3 + c] = floor_div_coor(p[c], lo.v[c], vs.v[c]);
}

__global__ __launch_bounds__(kThreads) void mask_occupy_k(const int32_t* __restrict__ coors, int64_t n, Grid3 g,
                                                          uint32_t* __restrict__ bits, int32_t* __restrict__ ovf_n,
                                                          int32_t* __restrict__ ovf) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  occupy(bits, ovf_n, ovf, n, g, coors[i * 3], coors[i * 3 + 1], coors[i * 3 + 2]);
}

__global__ __launch_bounds__(kThreads) void mask_query_k(const int32_t* __restrict__ coors, int64_t n, int64_t cap, Grid3 g,
                                                         const uint32_t* __restrict__ bits, const int32_t* __restrict__ ovf_n,
                                                         const int32_t* __restrict__ ovf, uint8_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  mask[i] = is_new(bits, ovf_n, ovf, cap, g, coors[i * 3], coors[i * 3 + 1], coors[i * 3 + 2]) ? 1 : 0;
}

// the workgroups of cloud c follow those of cloud c - 1; -> the cloud and the point of this thread (cloud == n_clouds: none)
__device__ __forceinline__ int64_t locate_cloud(const int64_t* n_of, int n_clouds, int& cloud) {
  int64_t blk = blockIdx.x;
  for (cloud = 0; cloud < n_clouds; ++cloud) {
    const int64_t nb = (n_of[cloud] + kThreads - 1) / kThreads;
    if (blk < nb) break;
    blk -= nb;
  }
  return blk * kThreads + threadIdx.x;
}

__global__ __launch_bounds__(kThreads) void delta_occupy_k(sst_incr_delta_args a, int64_t cap, uint32_t* __restrict__ bits,
                                                           int32_t* __restrict__ ovf_n, int32_t* __restrict__ ovf) {
  int c;
  const int64_t i = locate_cloud(a.n_base, a.n_clouds, c);
  if (c >= a.n_clouds || i >= a.n_base[c]) return;
  const float* p = a.base[c] + i * a.ld_base[c];
  const float x = p[0], y = p[1], z = p[2];
  if (a.lower_bound && !above_lo(a.lo, x, y, z)) return;
  const Grid3 g = {a.grid[0], a.grid[1], a.grid[2]};
  occupy(bits, ovf_n, ovf, cap, g, floor_div_coor(x, a.lo[0], a.vs[0]), floor_div_coor(y, a.lo[1], a.vs[1]),
         floor_div_coor(z, a.lo[2], a.vs[2]));
}

__global__ __launch_bounds__(kThreads) void delta_query_k(sst_incr_delta_args a, int64_t cap, const uint32_t* __restrict__ bits,
                                                          const int32_t* __restrict__ ovf_n, const int32_t* __restrict__ ovf) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n_query) return;
  const float* p = a.query + i * a.ld_query;
  const float x = p[0], y = p[1], z = p[2];
  bool fresh = false;
  if (!a.lower_bound || above_lo(a.lo, x, y, z)) {
    const Grid3 g = {a.grid[0], a.grid[1], a.grid[2]};
    fresh = is_new(bits, ovf_n, ovf, cap, g, floor_div_coor(x, a.lo[0], a.vs[0]), floor_div_coor(y, a.lo[1], a.vs[1]),
                   floor_div_coor(z, a.lo[2], a.vs[2]));
  }
  a.mask[i] = fresh ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------
// the fused stage
// ------------------------------------------------------------------------------------------------------------------

// what the stage's launches share: slices of the caller's one workspace
struct IncrWs {
  uint32_t* bits;       // [S * Q][words]                  zeroed
  int32_t* ovf_n;       // [S * Q]                         zeroed
  int32_t* has_base;    // [S * Q]                         zeroed; 1 once a base point was seen (get_delta_points: an EMPTY
                        //                                 base cloud yields no delta points, :740-743)
  int32_t* box_count;   // [n_boxes + 1]                   zeroed
  int32_t* ovf;         // [Q][total points][3]
  int32_t* box_start;   // [n_boxes + 1]
  uint8_t* flags;       // [total points]: bit 0 = kept crop row, bit 1 = delta row
  uint64_t* keys_in;    // [total points]
  uint64_t* keys_out;
  uint32_t* perm;
  void* sort_ws;
  int32_t* blk_count;   // [workgroups][bins]
  int32_t* blk_base;
  int64_t words, total, blocks, zero_bytes, bytes;
};

int64_t grid_words(const int32_t* grid) {
  const int64_t vol = (int64_t)grid[0] * grid[1] * grid[2];
  return (vol + 31) / 32;
}

IncrWs carve(const sst_incr_args& a) {
  IncrWs w;
  w.total = 0;
  w.blocks = 0;
  for (int s = 0; s < a.n_samples; ++s) {
    w.total += a.n_points[s];
    w.blocks += sst_div_up(a.n_points[s], kThreads);
  }
  w.words = a.n_queries > 0 ? grid_words(a.grid) : 0;
  const int nb = a.n_frames + a.n_queries;
  const int64_t sq = (int64_t)a.n_samples * a.n_queries;
  sst_carver c(a.workspace);
  w.bits = c.take<uint32_t>(sq * w.words);
  w.ovf_n = c.take<int32_t>(sq);
  w.has_base = c.take<int32_t>(sq);
  w.box_count = c.take<int32_t>((int64_t)a.n_boxes + 1);
  w.zero_bytes = c.off;
  w.ovf = c.take<int32_t>((int64_t)a.n_queries * w.total * 3);
  w.box_start = c.take<int32_t>((int64_t)a.n_boxes + 1);
  w.flags = c.take<uint8_t>(w.total);
  const bool sorted = a.max_crop_points > 0 && a.n_boxes > 0 && a.n_frames > 0;
  w.keys_in = c.take<uint64_t>(sorted ? w.total : 0);
  w.keys_out = c.take<uint64_t>(sorted ? w.total : 0);
  w.perm = c.take<uint32_t>(sorted ? w.total : 0);
  w.sort_ws = c.take<char>(sorted ? sst_sort_workspace_bytes(w.total) : 0);
  w.blk_count = c.take<int32_t>(w.blocks * nb);
  w.blk_base = c.take<int32_t>(w.blocks * nb);
  w.bytes = c.off;
  return w;
}

struct Loc {
  int s;        // sample (n_samples: none)
  int64_t blk;  // workgroup among all of the launch
  int64_t p;    // point within the sample
  int64_t g;    // point within the batch
  int64_t g0;   // first point of the sample within the batch
};

__device__ __forceinline__ Loc locate(const sst_incr_args& a) {
  Loc l;
  l.blk = blockIdx.x;
  l.g0 = 0;
  int64_t blk = blockIdx.x;
  for (l.s = 0; l.s < a.n_samples; ++l.s) {
    const int64_t nb = (a.n_points[l.s] + kThreads - 1) / kThreads;
    if (blk < nb) break;
    blk -= nb;
    l.g0 += a.n_points[l.s];
  }
  l.p = blk * kThreads + threadIdx.x;
  l.g = l.g0 + l.p;
  return l;
}

// mark: the bits and lists of every query, the first box of the point's own (sample, frame), the box counts, the sort keys
__global__ __launch_bounds__(kThreads) void incr_mark_k(sst_incr_args a, IncrWs w, int sorted) {
  __shared__ DppBox sb[kThreads];
  const Loc l = locate(a);
  if (l.s >= a.n_samples) return;  // uniform over the workgroup
  const bool live = l.p < a.n_points[l.s];
  float x = 0.f, y = 0.f, z = 0.f;
  int64_t fi = 1;  // names no frame
  if (live) {
    const float* q = a.points[l.s] + l.p * a.cols;
    x = q[0];
    y = q[1];
    z = q[2];
    fi = a.frame_inds[l.s][l.p];
  }
  if (live && a.n_queries > 0) {
    const Grid3 g = {a.grid[0], a.grid[1], a.grid[2]};
    const bool valid = !a.lower_bound || above_lo(a.lo, x, y, z);
    bool have = false;
    int32_t cx = 0, cy = 0, cz = 0;
    for (int q = 0; q < a.n_queries; ++q) {
      if (fi < a.q_lo[q] || fi > a.q_hi[q]) continue;
      if (w.has_base[(int64_t)l.s * a.n_queries + q] == 0) w.has_base[(int64_t)l.s * a.n_queries + q] = 1;  // every writer writes 1
      if (!valid) continue;
      if (!have) {
        cx = floor_div_coor(x, a.lo[0], a.vs[0]);
        cy = floor_div_coor(y, a.lo[1], a.vs[1]);
        cz = floor_div_coor(z, a.lo[2], a.vs[2]);
        have = true;
      }
      const int64_t sq = (int64_t)l.s * a.n_queries + q;
      occupy(w.bits + sq * w.words, w.ovf_n + sq, w.ovf + ((int64_t)q * w.total + l.g0) * 3, a.n_points[l.s], g, cx, cy, cz);
    }
  }
  if (a.n_frames <= 0) return;
  // the boxes of this sample, chunk by chunk through LDS; a point tests those of its own frame only
  const int F = a.n_frames;
  const int nbx = a.n_boxes;
  int B0 = 0, B1 = 0, b0 = 0, b1 = 0;
  if (nbx > 0) {
    B0 = min(max(a.box_offsets[l.s * F], 0), nbx);
    B1 = min(max(a.box_offsets[(l.s + 1) * F], B0), nbx);
    if (live && fi <= -1 && fi >= -(int64_t)F) {
      const int i = (int)(-fi) - 1;
      b0 = min(max(a.box_offsets[l.s * F + i], B0), B1);
      b1 = min(max(a.box_offsets[l.s * F + i + 1], b0), B1);
    }
  }
  int found = -1;
  for (int t0 = B0; t0 < B1; t0 += kThreads) {
    const int nt = min(kThreads, B1 - t0);
    __syncthreads();
    if ((int)threadIdx.x < nt) sb[threadIdx.x] = dpp_box(a.boxes + (int64_t)(t0 + threadIdx.x) * 7, 0.f, 0.f, 0.f);
    __syncthreads();
    if (found < 0) {
      const int k0 = max(b0, t0), k1 = min(b1, t0 + nt);
      for (int k = k0; k < k1; ++k) {
        float lx, ly, lz;
        if (dpp_classify(sb[k - t0], x, y, z, lx, ly, lz) != 0) {
          found = k;
          break;
        }
      }
    }
  }
  if (!live) return;
  if (sorted) {
    w.flags[l.g] = 0;
    const uint32_t key = a.keys != nullptr ? a.keys[l.g] : (uint32_t)l.g;
    w.keys_in[l.g] = found >= 0 ? ((uint64_t)found << 32) | key : (uint64_t)nbx << 32;
    if (found >= 0) atomicAdd(w.box_count + found, 1);
  } else {
    w.flags[l.g] = found >= 0 ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads) void incr_box_scan_k(IncrWs w, int n_boxes) {
  __shared__ int wsum[kWaves];
  block_excl_scan(w.box_count, w.box_start, n_boxes, 1, wsum);
}

// sorted position -> rank within its box = position - first position of the box; the first max_crop_points stay
__global__ __launch_bounds__(kThreads) void incr_rank_k(IncrWs w, int n_boxes, int max_n) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= w.total) return;
  const uint64_t b = w.keys_out[p] >> 32;
  if (b >= (uint64_t)n_boxes) return;
  const uint32_t src = w.perm[p];
  if (p - w.box_start[b] < max_n && src < w.total) w.flags[src] = 1;
}

// the segments a point contributes a row to: crop segment (its frame's, if kept) and delta segment (its query's, if new)
__device__ __forceinline__ void bins_of(const sst_incr_args& a, int64_t fi, uint8_t fl, int& crop_bin, int& delta_bin) {
  crop_bin = ((fl & 1) && fi <= -1 && fi >= -(int64_t)a.n_frames) ? (int)(-fi) - 1 : -1;
  delta_bin = -1;
  if (fl & 2)
    for (int q = 0; q < a.n_queries; ++q)
      if (fi == a.q_inc[q]) {
        delta_bin = a.n_frames + q;
        break;
      }
}

// flags (the delta bit) and the rows of every segment per workgroup
__global__ __launch_bounds__(kThreads) void incr_count_k(sst_incr_args a, IncrWs w) {
  __shared__ int wc[kWaves][kMaxBins];
  const Loc l = locate(a);
  if (l.s >= a.n_samples) return;
  const bool live = l.p < a.n_points[l.s];
  const int nb = a.n_frames + a.n_queries;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int crop_bin = -1, delta_bin = -1;
  if (live) {
    const int64_t fi = a.frame_inds[l.s][l.p];
    uint8_t fl = a.n_frames > 0 ? (w.flags[l.g] & 1) : 0;
    for (int q = 0; q < a.n_queries; ++q) {
      if (fi != a.q_inc[q]) continue;
      const float* pt = a.points[l.s] + l.p * a.cols;
      const float x = pt[0], y = pt[1], z = pt[2];
      const int64_t sq = (int64_t)l.s * a.n_queries + q;
      if (w.has_base[sq] != 0 && (!a.lower_bound || above_lo(a.lo, x, y, z))) {
        const Grid3 g = {a.grid[0], a.grid[1], a.grid[2]};
        if (is_new(w.bits + sq * w.words, w.ovf_n + sq, w.ovf + ((int64_t)q * w.total + l.g0) * 3, a.n_points[l.s], g,
                   floor_div_coor(x, a.lo[0], a.vs[0]), floor_div_coor(y, a.lo[1], a.vs[1]), floor_div_coor(z, a.lo[2], a.vs[2])))
          fl |= 2;
      }
      break;
    }
    w.flags[l.g] = fl;
    bins_of(a, fi, fl, crop_bin, delta_bin);
  }
  for (int b = 0; b < nb; ++b) {
    const unsigned long long m = __ballot(crop_bin == b || delta_bin == b);
    if (lane == 0) wc[wave][b] = __popcll(m);
  }
  __syncthreads();
  if ((int)threadIdx.x < nb) {
    int t = 0;
    for (int v = 0; v < kWaves; ++v) t += wc[v][threadIdx.x];
    w.blk_count[l.blk * nb + threadIdx.x] = t;
  }
}

// one workgroup per (sample, segment): the offsets of the sample's workgroups within the segment, and its row count
__global__ __launch_bounds__(kThreads) void incr_scan_k(sst_incr_args a, IncrWs w) {
  __shared__ int wsum[kWaves];
  const int nb = a.n_frames + a.n_queries;
  const int s = blockIdx.x / nb, b = blockIdx.x % nb;
  int64_t blk0 = 0;
  for (int t = 0; t < s; ++t) blk0 += (a.n_points[t] + kThreads - 1) / kThreads;
  const int64_t n = (a.n_points[s] + kThreads - 1) / kThreads;
  const int total = block_excl_scan(w.blk_count + blk0 * nb + b, w.blk_base + blk0 * nb + b, n, nb, wsum);
  if (threadIdx.x == 0) a.counts[s * nb + b] = total;
}

// rows: staged in LDS by (segment, rank), then every segment's rows of the workgroup leave as one contiguous span
__global__ __launch_bounds__(kThreads) void incr_rows_k(sst_incr_args a, IncrWs w) {
  __shared__ int wc[kWaves][kMaxBins];
  __shared__ int bin_off[kMaxBins + 1];
  __shared__ float stage[2 * kThreads * kMaxW];
  const Loc l = locate(a);
  if (l.s >= a.n_samples) return;
  const bool live = l.p < a.n_points[l.s];
  const int nb = a.n_frames + a.n_queries;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.cols, W = C + 1;
  int crop_bin = -1, delta_bin = -1;
  if (live) bins_of(a, a.frame_inds[l.s][l.p], w.flags[l.g], crop_bin, delta_bin);
  const unsigned long long below = (1ull << lane) - 1ull;
  int crop_rank = 0, delta_rank = 0;
  for (int b = 0; b < nb; ++b) {
    const unsigned long long m = __ballot(crop_bin == b || delta_bin == b);
    if (lane == 0) wc[wave][b] = __popcll(m);
    if (crop_bin == b) crop_rank = __popcll(m & below);
    if (delta_bin == b) delta_rank = __popcll(m & below);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int o = 0;
    for (int b = 0; b < nb; ++b) {
      bin_off[b] = o;
      for (int v = 0; v < kWaves; ++v) o += wc[v][b];
    }
    bin_off[nb] = o;
  }
  __syncthreads();
  if (live && (crop_bin >= 0 || delta_bin >= 0)) {
    const float* src = a.points[l.s] + l.p * C;
    for (int t = 0; t < 2; ++t) {
      const int b = t == 0 ? crop_bin : delta_bin;
      if (b < 0) continue;
      int pos = bin_off[b] + (t == 0 ? crop_rank : delta_rank);
      for (int v = 0; v < wave; ++v) pos += wc[v][b];
      float* o = stage + pos * W;
      for (int c = 0; c < C; ++c) o[c] = src[c];
      o[C] = t == 0 ? (float)((double)(-b - 1) / 10.0) : a.q_tag[b - a.n_frames];
    }
  }
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int cnt = bin_off[b + 1] - bin_off[b];
    if (cnt == 0) continue;
    float* __restrict__ dst = a.out + (a.seg_base[l.s * nb + b] + w.blk_base[l.blk * nb + b]) * W;
    const float* from = stage + bin_off[b] * W;
    for (int e = threadIdx.x; e < cnt * W; e += kThreads) dst[e] = from[e];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// frame transform
// ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void frame_transform_k(sst_frame_transform_args a) {
  int c;
  const int64_t i = locate_cloud(a.n, a.n_clouds, c);
  if (c >= a.n_clouds || i >= a.n[c]) return;
  const float* __restrict__ s = a.src[c] + i * a.cols;
  float* __restrict__ d = a.dst[c] + i * a.cols;
  const float* m = a.mat[c];
  const float x = s[0], y = s[1], z = s[2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    d[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, m[4 * r]), __fmul_rn(y, m[4 * r + 1])), __fmul_rn(z, m[4 * r + 2])), m[4 * r + 3]);
  for (int k = 3; k < a.cols; ++k) d[k] = s[k];
}

int check_grid(const float* vs, const int32_t* grid) {
  for (int c = 0; c < 3; ++c) {
    if (!(vs[c] > 0.f) || grid[c] < 1) return SST_ERR_ARG;
  }
  if ((double)grid[0] * (double)grid[1] * (double)grid[2] > 8589934592.0) return SST_ERR_UNSUPPORTED;
  return SST_OK;
}

struct MaskWs {
  uint32_t* bits;
  int32_t* ovf_n;
  int32_t* ovf;
  int64_t zero_bytes, bytes;
};

MaskWs carve_mask(void* p, int64_t n_base, const int32_t* grid) {
  MaskWs m;
  sst_carver c(p);
  m.bits = c.take<uint32_t>(grid_words(grid));
  m.ovf_n = c.take<int32_t>(1);
  m.zero_bytes = c.off;
  m.ovf = c.take<int32_t>(n_base * 3);
  m.bytes = c.off;
  return m;
}

int check_stage(const sst_incr_args& a) {
  if (a.n_samples < 0 || a.n_frames < 0 || a.n_queries < 0 || a.n_boxes < 0) return SST_ERR_ARG;
  if (a.n_samples > SST_INCR_MAX_SAMPLES || a.n_frames > SST_INCR_MAX_FRAMES || a.n_queries > SST_INCR_MAX_QUERIES)
    return SST_ERR_UNSUPPORTED;
  if (a.cols < 3 || a.cols > SST_INCR_MAX_COLS) return SST_ERR_UNSUPPORTED;
  int64_t total = 0, blocks = 0;
  for (int s = 0; s < a.n_samples; ++s) {
    if (a.n_points[s] < 0) return SST_ERR_ARG;
    if (a.n_points[s] > 0 && (!a.points[s] || !a.frame_inds[s])) return SST_ERR_ARG;
    total += a.n_points[s];
    blocks += sst_div_up(a.n_points[s], kThreads);
  }
  if (total > 0x7fffffff || blocks > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  if (a.n_queries > 0) {
    const int rc = check_grid(a.vs, a.grid);
    if (rc != SST_OK) return rc;
  }
  if (a.n_boxes > 0 && a.n_frames > 0 && (!a.boxes || !a.box_offsets)) return SST_ERR_ARG;
  return SST_OK;
}

}  // namespace

extern "C" int sst_incr_voxel_coors_f32(const float* d_points, int64_t n, int64_t ld, const float* lo3, const float* vs3,
                                        int32_t* d_coors, void* stream) {
  if (n < 0 || ld < 3 || !lo3 || !vs3) return SST_ERR_ARG;
  for (int c = 0; c < 3; ++c)
    if (!(vs3[c] > 0.f)) return SST_ERR_ARG;
  if (n == 0) return SST_OK;
  if (!d_points || !d_coors) return SST_ERR_ARG;
  if (sst_div_up(n, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  F3 lo, vs;
  for (int c = 0; c < 3; ++c) {
    lo.v[c] = lo3[c];
    vs.v[c] = vs3[c];
  }
  hipLaunchKernelGGL(voxel_coors_k, dim3((unsigned)sst_div_up(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, d_points, n, ld,
                     lo, vs, d_coors);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int64_t sst_incr_mask_workspace_bytes(int64_t n_base, const int32_t* spatial3) {
  if (n_base < 0 || !spatial3) return SST_ERR_ARG;
  const float one[3] = {1.f, 1.f, 1.f};
  const int rc = check_grid(one, spatial3);
  if (rc != SST_OK) return rc;
  return carve_mask(nullptr, n_base, spatial3).bytes;
}

extern "C" int sst_incr_mask_i32(const int32_t* d_coors1, int64_t n1, const int32_t* d_coors2, int64_t n2, const int32_t* spatial3,
                                 void* d_workspace, int64_t workspace_bytes, uint8_t* d_mask, void* stream) {
  if (n1 < 0 || n2 < 0 || !spatial3) return SST_ERR_ARG;
  const float one[3] = {1.f, 1.f, 1.f};
  const int rc = check_grid(one, spatial3);
  if (rc != SST_OK) return rc;
  if (sst_div_up(n1, kThreads) > 0x7fffffff || sst_div_up(n2, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  if (n2 == 0) return SST_OK;
  if (!d_coors2 || !d_mask || !d_workspace || (n1 > 0 && !d_coors1)) return SST_ERR_ARG;
  const MaskWs m = carve_mask(d_workspace, n1, spatial3);
  if (workspace_bytes < m.bytes) return SST_ERR_ARG;
  const Grid3 g = {spatial3[0], spatial3[1], spatial3[2]};
  hipStream_t s = (hipStream_t)stream;
  SST_HIP(hipMemsetAsync(d_workspace, 0, (size_t)m.zero_bytes, s));
  if (n1 > 0) {
    hipLaunchKernelGGL(mask_occupy_k, dim3((unsigned)sst_div_up(n1, kThreads)), dim3(kThreads), 0, s, d_coors1, n1, g, m.bits, m.ovf_n,
                       m.ovf);
    SST_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mask_query_k, dim3((unsigned)sst_div_up(n2, kThreads)), dim3(kThreads), 0, s, d_coors2, n2, n1, g, m.bits,
                     m.ovf_n, m.ovf, d_mask);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_incr_delta_mask_f32(const sst_incr_delta_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_incr_delta_args& a = *args;
  if (a.n_clouds < 0 || a.n_query < 0 || a.ld_query < 3) return SST_ERR_ARG;
  if (a.n_clouds > SST_INCR_MAX_CLOUDS) return SST_ERR_UNSUPPORTED;
  const int rc = check_grid(a.vs, a.grid);
  if (rc != SST_OK) return rc;
  int64_t n_base = 0, blocks = 0;
  for (int c = 0; c < a.n_clouds; ++c) {
    if (a.n_base[c] < 0 || a.ld_base[c] < 3 || (a.n_base[c] > 0 && !a.base[c])) return SST_ERR_ARG;
    n_base += a.n_base[c];
    blocks += sst_div_up(a.n_base[c], kThreads);
  }
  if (n_base > 0x7fffffff || blocks > 0x7fffffff || sst_div_up(a.n_query, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  if (a.n_query == 0) return SST_OK;
  if (!a.query || !a.mask || !a.workspace) return SST_ERR_ARG;
  const MaskWs m = carve_mask(a.workspace, n_base, a.grid);
  if (a.workspace_bytes < m.bytes) return SST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  SST_HIP(hipMemsetAsync(a.workspace, 0, (size_t)m.zero_bytes, s));
  if (blocks > 0) {
    hipLaunchKernelGGL(delta_occupy_k, dim3((unsigned)blocks), dim3(kThreads), 0, s, a, n_base, m.bits, m.ovf_n, m.ovf);
    SST_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(delta_query_k, dim3((unsigned)sst_div_up(a.n_query, kThreads)), dim3(kThreads), 0, s, a, n_base, m.bits, m.ovf_n,
                     m.ovf);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int64_t sst_incr_workspace_bytes(const sst_incr_args* args) {
  if (!args) return SST_ERR_ARG;
  const int rc = check_stage(*args);
  if (rc != SST_OK) return rc;
  sst_incr_args a = *args;
  a.workspace = nullptr;
  return carve(a).bytes;
}

extern "C" int sst_incr_plan_f32(const sst_incr_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_incr_args& a = *args;
  const int rc = check_stage(a);
  if (rc != SST_OK) return rc;
  const int nb = a.n_frames + a.n_queries;
  if (a.n_samples == 0 || nb == 0) return SST_OK;
  if (!a.counts || !a.workspace) return SST_ERR_ARG;
  for (int q = 0; q < a.n_queries; ++q)
    if (a.q_lo[q] <= a.q_inc[q] && a.q_inc[q] <= a.q_hi[q]) return SST_ERR_ARG;  // a frame is not its own base
  const IncrWs w = carve(a);
  if (a.workspace_bytes < w.bytes) return SST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (w.total == 0) {
    SST_HIP(hipMemsetAsync(a.counts, 0, sizeof(int32_t) * (size_t)a.n_samples * nb, s));
    return SST_OK;
  }
  const int sorted = (a.max_crop_points > 0 && a.n_boxes > 0 && a.n_frames > 0) ? 1 : 0;
  SST_HIP(hipMemsetAsync(a.workspace, 0, (size_t)w.zero_bytes, s));
  hipLaunchKernelGGL(incr_mark_k, dim3((unsigned)w.blocks), dim3(kThreads), 0, s, a, w, sorted);
  SST_LAUNCH_CHECK();
  if (sorted) {
    hipLaunchKernelGGL(incr_box_scan_k, dim3(1), dim3(kThreads), 0, s, w, a.n_boxes);
    SST_LAUNCH_CHECK();
    int bits = 1;
    while (bits < 31 && (1ll << bits) <= a.n_boxes) ++bits;
    const int src = sst_sort_pairs_u64(w.keys_in, w.keys_out, w.perm, w.total, 32 + bits, w.sort_ws, stream);
    if (src != SST_OK) return src;
    hipLaunchKernelGGL(incr_rank_k, dim3((unsigned)sst_div_up(w.total, kThreads)), dim3(kThreads), 0, s, w, a.n_boxes,
                       a.max_crop_points);
    SST_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(incr_count_k, dim3((unsigned)w.blocks), dim3(kThreads), 0, s, a, w);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(incr_scan_k, dim3((unsigned)(a.n_samples * nb)), dim3(kThreads), 0, s, a, w);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_incr_rows_f32(const sst_incr_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_incr_args& a = *args;
  const int rc = check_stage(a);
  if (rc != SST_OK) return rc;
  const int nb = a.n_frames + a.n_queries;
  if (a.n_samples == 0 || nb == 0) return SST_OK;
  if (!a.workspace) return SST_ERR_ARG;
  const IncrWs w = carve(a);
  if (a.workspace_bytes < w.bytes) return SST_ERR_ARG;
  if (w.total == 0) return SST_OK;
  if (!a.out) return SST_ERR_ARG;
  for (int i = 0; i < a.n_samples * nb; ++i)
    if (a.seg_base[i] < 0) return SST_ERR_ARG;
  hipLaunchKernelGGL(incr_rows_k, dim3((unsigned)w.blocks), dim3(kThreads), 0, (hipStream_t)stream, a, w);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_points_frame_transform_f32(const sst_frame_transform_args* args, void* stream) {
  if (!args) return SST_ERR_ARG;
  const sst_frame_transform_args& a = *args;
  if (a.n_clouds < 0) return SST_ERR_ARG;
  if (a.n_clouds > SST_INCR_MAX_CLOUDS || a.cols < 3 || a.cols > 64) return SST_ERR_UNSUPPORTED;
  int64_t blocks = 0;
  for (int c = 0; c < a.n_clouds; ++c) {
    if (a.n[c] < 0 || (a.n[c] > 0 && (!a.src[c] || !a.dst[c]))) return SST_ERR_ARG;
    blocks += sst_div_up(a.n[c], kThreads);
  }
  if (blocks > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  if (blocks == 0) return SST_OK;
  hipLaunchKernelGGL(frame_transform_k, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

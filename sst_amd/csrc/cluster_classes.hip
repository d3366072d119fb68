// ClusterAssigner.forward for ALL classes of a step in one pass (include/sst_amd.h "Class-batched cluster assignment").
//
// Reference: mmdet3d/models/detectors/single_stage_fsd.py:922-999 runs, class after class, the cluster-voxel grouping of the
// voted centres, filter_almost_empty with the "nothing survives, so keep every point" rule (:968-970), the centroids, their
// connected components (:45-84) and the point -> component map.  sst_amd/cluster.py's per-class path does the same with one
// sorted-unique, one segmented mean, one union-find launch sequence and one host read PER CLASS; here the votes of all classes
// are keyed (class, sample, cell) in one launch, grouped once, and everything behind the grouping stays on the device:
//   ccl_keys_k      the key rows; the cell is torch's fp32 floor division restated (floor_div.h)
//   ccl_groups_k    occupancy per cluster voxel, and per class: votes in crowded voxels, voxels, crowded voxels
//   ccl_decide_k    per class the keep-everything rule, the two sizes of the host read, and the running bases (ONE wave)
//   ccl_flags_k     surviving voxel / surviving vote flags (scanned: centroid rows, output rows)
//   ccl_centroids_k the surviving voxels' centroids compacted with their partition id, union-find initialised
//   ccl_pairs_k     the edge test of cluster.hip (same partition && sst_xy_dist < dist[class]) over 256 x 256 tile pairs.  The
//                   centroids are sorted by partition ((class, sample) in training, (class) in eval), so the partitions of tile
//                   tj <= ti can meet those of ti only if part[last of tj] >= part[first of ti]: every other pair leaves
//                   before it stages anything.  (The further criterion the sorted x cells would allow inside a partition is
//                   not built: DESIGN.md 3.29.)
//   ccl_flatten_k   roots; their exclusive scan numbers the components of all classes by smallest member
//   ccl_points_k    (class, sample, component - first component of the class) of every surviving vote, compacted
// Integer atomics only (counters; hooks of the larger root under the smaller one): whatever the execution order the root of a
// component is its smallest centroid, so two runs are bit-equal.
#include "common.h"
#include "exact_math.h"
#include "floor_div.h"

namespace {

constexpr int kTile = 256;
constexpr int kMaxCls = SST_CCL_MAX_CLASSES;
// fixed key layout of the rows: no read-back sizes it.  62 bits with 32 classes.
constexpr int kCellXY = 1 << 16;   // cell x, y in [-65536, 65536)
constexpr int kCellZ = 1 << 14;    // cell z in [-16384, 16384)

// words of the zeroed header of the workspace
enum {
  kHdrPtsValid = 0,                 // [32] votes in crowded voxels per class
  kHdrGroups = kMaxCls,             // [32] voxels per class
  kHdrCrowded = 2 * kMaxCls,        // [32] crowded voxels per class
  kHdrNumCent = 3 * kMaxCls,        // surviving voxels of all classes (scan total)
  kHdrNumRoots = 3 * kMaxCls + 1,   // components of all classes (scan total)
  kHdrNumKept = 3 * kMaxCls + 2,    // surviving votes of all classes (scan total)
  kHdrTilesRun = 3 * kMaxCls + 3,
  kHdrTilesSkipped = 3 * kMaxCls + 4,
  kHdrRule = 3 * kMaxCls + 8,       // [32] keep-everything rule per class
  kHdrCentStart = 4 * kMaxCls + 8,  // [33] first centroid row per class
  kHdrWords = 6 * kMaxCls           // 192 words = 768 bytes
};
static_assert(kHdrCentStart + kMaxCls + 1 <= kHdrWords, "header layout");

__device__ __forceinline__ int class_of_row(const sst_cluster_classes_params& P, int64_t i) {
  int c = 0;
  while (c + 1 < P.n_classes && i >= P.class_off[c + 1]) ++c;   // <= 31 steps over kernel arguments
  return c;
}

__global__ __launch_bounds__(256) void ccl_keys_k(const float* __restrict__ pts, int64_t ld, const int32_t* __restrict__ batch,
                                                  int64_t n, const sst_cluster_classes_params P, int32_t* __restrict__ rows,
                                                  int32_t* __restrict__ status) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = class_of_row(P, i);
    int32_t s = batch[i];
    int32_t cx = floor_div_coor(pts[i * ld], P.origin[0], P.cell[c][0]);
    int32_t cy = floor_div_coor(pts[i * ld + 1], P.origin[1], P.cell[c][1]);
    int32_t cz = floor_div_coor(pts[i * ld + 2], P.origin[2], P.cell[c][2]);
    if (s < 0 || s >= SST_CCL_MAX_SAMPLES) bad |= SST_CCL_STATUS_SAMPLE_RANGE, s = s < 0 ? 0 : SST_CCL_MAX_SAMPLES - 1;
    if (cx < -kCellXY || cx >= kCellXY) bad |= SST_CCL_STATUS_CELL_RANGE, cx = cx < 0 ? -kCellXY : kCellXY - 1;
    if (cy < -kCellXY || cy >= kCellXY) bad |= SST_CCL_STATUS_CELL_RANGE, cy = cy < 0 ? -kCellXY : kCellXY - 1;
    if (cz < -kCellZ || cz >= kCellZ) bad |= SST_CCL_STATUS_CELL_RANGE, cz = cz < 0 ? -kCellZ : kCellZ - 1;
    int32_t* r = rows + i * 5;
    r[0] = c, r[1] = s, r[2] = cx, r[3] = cy, r[4] = cz;
  }
  if (bad) atomicOr(status, bad);
}

// one thread per group of the sorted-unique: occupancy -> crowded flag, partition id, the per-class counters (LDS first)
__global__ __launch_bounds__(256) void ccl_groups_k(const int32_t* __restrict__ rows, const uint32_t* __restrict__ perm,
                                                    const int32_t* __restrict__ offsets, const int32_t* __restrict__ d_m,
                                                    const sst_cluster_classes_params P, int32_t* __restrict__ gpart,
                                                    int32_t* __restrict__ gcrowded, int32_t* __restrict__ hdr) {
  __shared__ int bins[3 * kMaxCls];
  if (threadIdx.x < 3 * kMaxCls) bins[threadIdx.x] = 0;
  __syncthreads();
  const int64_t m = *d_m;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < m; g += (int64_t)gridDim.x * blockDim.x) {
    const int beg = offsets[g], cnt = offsets[g + 1] - beg;
    const int32_t* r = rows + (int64_t)perm[beg] * 5;
    const int c = r[0];
    const int crowded = cnt >= P.min_points ? 1 : 0;
    gpart[g] = P.per_sample ? c * SST_CCL_MAX_SAMPLES + r[1] : c;
    gcrowded[g] = crowded;
    atomicAdd(&bins[kMaxCls + c], 1);
    if (crowded) {
      atomicAdd(&bins[c], cnt);
      atomicAdd(&bins[2 * kMaxCls + c], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 * kMaxCls && bins[threadIdx.x] != 0) atomicAdd(&hdr[threadIdx.x], bins[threadIdx.x]);
}

// ONE wave: the rule and the sizes per class, the first centroid row per class (the scan of the per-class bases)
__global__ __launch_bounds__(64) void ccl_decide_k(const sst_cluster_classes_params P, int32_t* __restrict__ hdr,
                                                   const int32_t* __restrict__ status, int32_t* __restrict__ sizes) {
  __shared__ int kept_groups[kMaxCls];
  const int c = threadIdx.x;
  const int G = P.n_classes;
  if (c < G) {
    const int n_c = P.class_off[c + 1] - P.class_off[c];
    const int rule = (n_c > 0 && hdr[kHdrPtsValid + c] == 0) ? 1 : 0;
    hdr[kHdrRule + c] = rule;
    sizes[c] = rule ? n_c : hdr[kHdrPtsValid + c];
    kept_groups[c] = sizes[G + c] = rule ? hdr[kHdrGroups + c] : hdr[kHdrCrowded + c];
  }
  __syncthreads();
  if (c == 0) {
    int run = 0;
    for (int k = 0; k < G; ++k) {
      hdr[kHdrCentStart + k] = run;
      run += kept_groups[k];
    }
    hdr[kHdrCentStart + G] = run;
    sizes[2 * G] = *status;
  }
}

// flags over the fixed length n (groups >= *d_m: 0), so that both scans run over a host-known length
__global__ __launch_bounds__(256) void ccl_flags_k(const int32_t* __restrict__ inverse, const int32_t* __restrict__ gpart,
                                                   const int32_t* __restrict__ gcrowded, const int32_t* __restrict__ d_m,
                                                   int64_t n, const sst_cluster_classes_params P, const int32_t* __restrict__ hdr,
                                                   int32_t* __restrict__ gkeep, int32_t* __restrict__ pkeep) {
  const int64_t m = *d_m;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int kg = 0;
    if (i < m) {
      const int c = P.per_sample ? gpart[i] / SST_CCL_MAX_SAMPLES : gpart[i];
      kg = (gcrowded[i] || hdr[kHdrRule + c]) ? 1 : 0;
    }
    gkeep[i] = kg;
    const int g = inverse[i];
    const int cp = P.per_sample ? gpart[g] / SST_CCL_MAX_SAMPLES : gpart[g];
    pkeep[i] = (gcrowded[g] || hdr[kHdrRule + cp]) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void ccl_centroids_k(const float* __restrict__ cent, const int32_t* __restrict__ gpart,
                                                       const int32_t* __restrict__ gkeep, const int32_t* __restrict__ grank,
                                                       const int32_t* __restrict__ d_m, float* __restrict__ xs,
                                                       float* __restrict__ ys, int32_t* __restrict__ part,
                                                       int* __restrict__ parent) {
  const int64_t m = *d_m;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < m; g += (int64_t)gridDim.x * blockDim.x) {
    if (!gkeep[g]) continue;
    const int j = grank[g];
    xs[j] = cent[g * 3];
    ys[j] = cent[g * 3 + 1];
    part[j] = gpart[g];
    parent[j] = j;
  }
}

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(int* __restrict__ parent, int x) {
  int p = cc_load(parent + x);
  while (p != x) {
    const int gp = cc_load(parent + p);
    if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // path halving
    x = p;
    p = gp;
  }
  return x;
}

__device__ __forceinline__ void cc_union(int* __restrict__ parent, int a, int b) {
  while (true) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(parent + a, a, b);  // hook the larger root under the smaller one
    if (old == a) return;
    a = old;
  }
}

struct ccl_dists {
  float v[kMaxCls];
};

// a fixed grid strides over the tile pairs (ti >= tj) of the lower triangle of the K = hdr[kHdrNumCent] centroids
__global__ __launch_bounds__(kTile) void ccl_pairs_k(const float* __restrict__ xs, const float* __restrict__ ys,
                                                     const int32_t* __restrict__ part, const int32_t* __restrict__ hdr_ro,
                                                     int per_sample, const ccl_dists D, int* __restrict__ parent,
                                                     int32_t* __restrict__ tile_counts) {
  __shared__ float sx[kTile], sy[kTile];
  __shared__ int sp[kTile];
  const int n = hdr_ro[kHdrNumCent];
  const int n_tiles = (n + kTile - 1) / kTile;
  const int64_t n_pairs = (int64_t)n_tiles * (n_tiles + 1) / 2;
  int run = 0, skipped = 0;
  for (int64_t b = blockIdx.x; b < n_pairs; b += gridDim.x) {   // b depends on the block only: the barriers below are uniform
    // row ti holds ti + 1 pairs: ti = floor((sqrt(8 b + 1) - 1) / 2), fixed up for rounding
    int ti = (int)((sqrtf(8.f * (float)b + 1.f) - 1.f) * 0.5f);
    while ((int64_t)(ti + 1) * (ti + 2) / 2 <= b) ++ti;
    while ((int64_t)ti * (ti + 1) / 2 > b) --ti;
    const int tj = (int)(b - (int64_t)ti * (ti + 1) / 2);
    const int i0 = ti * kTile, j0 = tj * kTile;
    const int jn = (n - j0) < kTile ? (n - j0) : kTile;
    // sorted by partition: every centroid of tile tj has a partition <= part[j0 + jn - 1], every one of ti >= part[i0]
    if (tj < ti && part[j0 + jn - 1] < part[i0]) {
      ++skipped;
      continue;
    }
    ++run;
    __syncthreads();   // the previous pair's readers are done with the tile
    if ((int)threadIdx.x < jn) {
      sx[threadIdx.x] = xs[j0 + threadIdx.x];
      sy[threadIdx.x] = ys[j0 + threadIdx.x];
      sp[threadIdx.x] = part[j0 + threadIdx.x];
    }
    __syncthreads();
    const int i = i0 + threadIdx.x;
    if (i < n) {
      const float xi = xs[i], yi = ys[i];
      const int pi = part[i];
      const float dist = D.v[per_sample ? pi / SST_CCL_MAX_SAMPLES : pi];
      for (int q = 0; q < jn; ++q) {
        const int j = j0 + q;
        if (j >= i) break;  // lower triangle only (the graph is undirected)
        if (sp[q] != pi) continue;
        if (sst_xy_dist(xi, yi, sx[q], sy[q]) < dist) cc_union(parent, i, j);
      }
    }
  }
  if (tile_counts != nullptr && threadIdx.x == 0) {
    if (run) atomicAdd(&tile_counts[0], run);
    if (skipped) atomicAdd(&tile_counts[1], skipped);
  }
}

// roots over the fixed length n (rows >= K: no root), so that the scan runs over a host-known length
__global__ __launch_bounds__(256) void ccl_flatten_k(int* __restrict__ parent, const int32_t* __restrict__ hdr_ro, int64_t n,
                                                     int32_t* __restrict__ is_root) {
  const int k = hdr_ro[kHdrNumCent];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i >= k) {
      is_root[i] = 0;
      continue;
    }
    int x = (int)i;
    while (true) {  // no concurrent unions any more: plain walk (other threads only write roots)
      const int p = cc_load(parent + x);
      if (p == x) break;
      x = p;
    }
    is_root[i] = (x == (int)i) ? 1 : 0;
    __hip_atomic_store(parent + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void ccl_points_k(const int32_t* __restrict__ rows, const int32_t* __restrict__ inverse,
                                                    const int32_t* __restrict__ pkeep, const int32_t* __restrict__ ppos,
                                                    const int32_t* __restrict__ grank, const int* __restrict__ parent,
                                                    const int32_t* __restrict__ rrank, const int32_t* __restrict__ hdr_ro,
                                                    int64_t n, const sst_cluster_classes_params P, int32_t* __restrict__ inds,
                                                    int64_t* __restrict__ keep, uint8_t* __restrict__ mask) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int kp = pkeep[i];
    mask[i] = (uint8_t)kp;
    if (!kp) continue;
    const int c = rows[i * 5];
    const int64_t o = ppos[i];
    const int j = grank[inverse[i]];
    // the class's components are the roots from its first centroid on: numbered from 0 inside the class
    const int label = rrank[parent[j]] - rrank[hdr_ro[kHdrCentStart + c]];
    inds[o * 3] = c;
    inds[o * 3 + 1] = rows[i * 5 + 1];
    inds[o * 3 + 2] = label;
    keep[o] = i - P.class_off[c];
  }
}

struct ccl_ws {
  int32_t *hdr, *gpart, *gcrowded, *gkeep, *grank, *pkeep, *ppos, *part, *is_root, *rrank;
  int* parent;
  float *xs, *ys;
  void* scan;
  int64_t bytes;
};

ccl_ws carve(void* base, int64_t n) {
  sst_carver cv(base);
  ccl_ws w;
  w.hdr = cv.take<int32_t>(kHdrWords);
  w.gpart = cv.take<int32_t>(n);
  w.gcrowded = cv.take<int32_t>(n);
  w.gkeep = cv.take<int32_t>(n);
  w.grank = cv.take<int32_t>(n);
  w.pkeep = cv.take<int32_t>(n);
  w.ppos = cv.take<int32_t>(n);
  w.part = cv.take<int32_t>(n);
  w.is_root = cv.take<int32_t>(n);
  w.rrank = cv.take<int32_t>(n);
  w.parent = cv.take<int>(n);
  w.xs = cv.take<float>(n);
  w.ys = cv.take<float>(n);
  w.scan = cv.take<char>(sst_scan_workspace_bytes(n));
  w.bytes = cv.off;
  return w;
}

int check_params(const sst_cluster_classes_params* p, int64_t n) {
  if (!p || n < 0) return SST_ERR_ARG;
  if (n >= (int64_t)1 << 31) return SST_ERR_UNSUPPORTED;
  if (p->n_classes < 1) return SST_ERR_ARG;
  if (p->n_classes > kMaxCls) return SST_ERR_UNSUPPORTED;
  if (p->class_off[0] != 0 || p->class_off[p->n_classes] != n) return SST_ERR_ARG;
  for (int c = 0; c < p->n_classes; ++c) {
    if (p->class_off[c + 1] < p->class_off[c]) return SST_ERR_ARG;
    for (int d = 0; d < 3; ++d)
      if (!(p->cell[c][d] > 0.f)) return SST_ERR_ARG;
    if (!(p->dist[c] == p->dist[c])) return SST_ERR_ARG;
  }
  return SST_OK;
}

}  // namespace

extern "C" {

int sst_cluster_classes_max(void) { return kMaxCls; }

int sst_cluster_classes_key_layout(int n_classes, int64_t* h_mins, int64_t* h_extents) {
  if (n_classes < 1 || !h_mins || !h_extents) return SST_ERR_ARG;
  if (n_classes > kMaxCls) return SST_ERR_UNSUPPORTED;
  const int64_t mins[5] = {0, 0, -kCellXY, -kCellXY, -kCellZ};
  const int64_t ext[5] = {n_classes, SST_CCL_MAX_SAMPLES, 2 * kCellXY, 2 * kCellXY, 2 * kCellZ};
  for (int j = 0; j < 5; ++j) h_mins[j] = mins[j], h_extents[j] = ext[j];
  return SST_OK;
}

int sst_cluster_classes_keys_f32(const float* d_points, int64_t ld, const int32_t* d_batch, int64_t n,
                                 const sst_cluster_classes_params* params, int32_t* d_rows, int32_t* d_status, void* stream) {
  const int rc = check_params(params, n);
  if (rc != SST_OK) return rc;
  if (ld < 3 || !d_status) return SST_ERR_ARG;
  if (n == 0) return SST_OK;
  if (!d_points || !d_batch || !d_rows) return SST_ERR_ARG;
  hipLaunchKernelGGL(ccl_keys_k, dim3(sst_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, d_points, ld, d_batch, n, *params,
                     d_rows, d_status);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int64_t sst_cluster_classes_workspace_bytes(int64_t n) {
  if (n < 1) n = 1;
  return carve(nullptr, n).bytes + 256;
}

int sst_cluster_classes_f32(const float* d_centroids, const int32_t* d_rows, const uint32_t* d_perm, const int32_t* d_offsets,
                            const int32_t* d_inverse, const int32_t* d_num_groups, int64_t n,
                            const sst_cluster_classes_params* params, const int32_t* d_status, int32_t* d_inds, int64_t* d_keep,
                            uint8_t* d_mask, int32_t* d_sizes, void* d_workspace, void* stream) {
  int rc = check_params(params, n);
  if (rc != SST_OK) return rc;
  if (!d_sizes || !d_status) return SST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const sst_cluster_classes_params& P = *params;
  const int G = P.n_classes;
  if (n == 0) {
    SST_HIP(hipMemsetAsync(d_sizes, 0, sizeof(int32_t) * (2 * G + 4), st));
    return SST_OK;
  }
  if (!d_centroids || !d_rows || !d_perm || !d_offsets || !d_inverse || !d_num_groups || !d_inds || !d_keep || !d_mask ||
      !d_workspace)
    return SST_ERR_ARG;
  const ccl_ws w = carve(d_workspace, n);
  ccl_dists D;
  for (int c = 0; c < kMaxCls; ++c) D.v[c] = c < G ? P.dist[c] : 0.f;
  const int g1 = sst_grid_1d(n, 256);
  SST_HIP(hipMemsetAsync(w.hdr, 0, sizeof(int32_t) * kHdrWords, st));
  hipLaunchKernelGGL(ccl_groups_k, dim3(g1), dim3(256), 0, st, d_rows, d_perm, d_offsets, d_num_groups, P, w.gpart, w.gcrowded,
                     w.hdr);
  hipLaunchKernelGGL(ccl_decide_k, dim3(1), dim3(64), 0, st, P, w.hdr, d_status, d_sizes);
  hipLaunchKernelGGL(ccl_flags_k, dim3(g1), dim3(256), 0, st, d_inverse, w.gpart, w.gcrowded, d_num_groups, n, P, w.hdr, w.gkeep,
                     w.pkeep);
  rc = sst_exclusive_scan_i32(w.gkeep, w.grank, n, w.hdr + kHdrNumCent, w.scan, stream);
  if (rc != SST_OK) return rc;
  rc = sst_exclusive_scan_i32(w.pkeep, w.ppos, n, w.hdr + kHdrNumKept, w.scan, stream);
  if (rc != SST_OK) return rc;
  hipLaunchKernelGGL(ccl_centroids_k, dim3(g1), dim3(256), 0, st, d_centroids, w.gpart, w.gkeep, w.grank, d_num_groups, w.xs,
                     w.ys, w.part, w.parent);
  // tile pairs of the upper bound n; the kernel strides over the pairs of the K centroids there are
  const int64_t t_max = sst_div_up(n, kTile);
  int64_t pair_grid = t_max * (t_max + 1) / 2;
  if (pair_grid > 4096) pair_grid = 4096;
  hipLaunchKernelGGL(ccl_pairs_k, dim3((unsigned)pair_grid), dim3(kTile), 0, st, w.xs, w.ys, w.part, w.hdr, P.per_sample, D,
                     w.parent, P.count_tiles ? w.hdr + kHdrTilesRun : nullptr);
  hipLaunchKernelGGL(ccl_flatten_k, dim3(g1), dim3(256), 0, st, w.parent, w.hdr, n, w.is_root);
  rc = sst_exclusive_scan_i32(w.is_root, w.rrank, n, w.hdr + kHdrNumRoots, w.scan, stream);
  if (rc != SST_OK) return rc;
  hipLaunchKernelGGL(ccl_points_k, dim3(g1), dim3(256), 0, st, d_rows, d_inverse, w.pkeep, w.ppos, w.grank, w.parent, w.rrank,
                     w.hdr, n, P, d_inds, d_keep, d_mask);
  // the tail of the one host read: surviving voxels of all classes and the tile counts
  SST_HIP(hipMemcpyAsync(d_sizes + 2 * G + 1, w.hdr + kHdrNumCent, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  SST_HIP(hipMemcpyAsync(d_sizes + 2 * G + 2, w.hdr + kHdrTilesRun, 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

// Furthest point sampling and the SSG cluster assignment of FSD (single_stage_fsd.py:24-28, 83-142, 1002-1194).
//
// Reference: mmdet3d/ops/furthest_point_sample/src/furthest_point_sample_cuda.cu:25-141 (coordinates) and :213-331
// (distance matrix) - one block of B = max(min(2^floor(log2 N), 1024), 1) threads per batch entry; per sample a pass over
// the points through global memory (coordinates and the running minimum `temp`), then a shared-memory tree of up to ten
// barriers.  ssg_single_sample then builds the [K, K] and [K, N] distance matrices and the [K, N] mask on the device,
// calls nonzero, sorts, and asserts (one read-back each).
//
// Here:
//   fps_k       one workgroup of 1024 threads (16 waves) per SEGMENT of the point array.  Segments of up to 16 384 points
//               live in registers for the whole call (x, y, z and the running minimum of 1 | 2 | 4 | 8 | 16 points per
//               thread, compile-time indexed); longer ones keep their first 12 288 points there and stream the rest -
//               coordinates from the input, the running minimum through `temp` - on every sample.  The
//               arg-max of a sample is ONE 64-bit maximum - distance bits in the high word (distances are >= 0, their bits
//               order as unsigned integers), 0xFFFFFFFF - tie_rank in the low word - reduced inside a wave with DPP and
//               across the 16 waves through a double-buffered LDS slot: one barrier per sample.  The slot carries the
//               winner's coordinates, so nobody goes back to memory for them.
//   tie rank    the reference's winner among equal distances is NOT the lowest index: thread t scans k = t, t + B, ... and
//               keeps the first strict maximum, and its tree lets the left operand win with partners at +512 ... +1, so
//               the winner is the k with the smallest (bitreverse_{log2 B}(k mod B), k div B).  That pair, as one 32-bit
//               number, is the rank.  B comes from the SEGMENT's length.
//   arithmetic  d = (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1), left to right, every product and sum rounded on
//               its own: plain operators under -ffp-contract=off (the __f*_rn names this toolchain gives them ARE the plain
//               operators and pin nothing, exact_math.h): the form a numpy float32 restatement reproduces.
//   ssg_*_k     pruning (parallel K x K: keypoint j falls if ANY earlier keypoint of its segment is closer than thr2),
//               numbering (exclusive scan of the surviving flags over all segments) and assignment (every point counts the
//               surviving keypoints of its segment closer than radius; exactly one -> its id, else -1), keypoints staged
//               through LDS one per lane; no [K, N] matrix.  sqrt(dx*dx + dy*dy) is sst_xy_dist of exact_math.h: separately
//               rounded operations and the correctly rounded root (the fp64 root rounded once more; __fsqrt_rn is the
//               approximate v_sqrt_f32 in this build and decided pairs on the threshold wrongly).
#include "common.h"
#include "exact_math.h"

namespace {

typedef unsigned long long u64;

constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / SST_WAVE;
constexpr int kFpsRegPoints = 16;                       // points per thread of the largest register tier
constexpr int kFpsRegMax = kFpsThreads * kFpsRegPoints;  // 16 384
constexpr int kFpsTailRegPoints = 12;                   // longer segments: 12 288 points in registers, the rest streamed

struct FpsSlots {
  u64 key[2][kFpsWaves];
  float4 pt[2][kFpsWaves];  // x, y, z, index bits
};

template <int CTRL>
__device__ __forceinline__ u64 fps_dpp_max(u64 v) {
  const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  const unsigned plo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const unsigned phi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const u64 p = ((u64)phi << 32) | plo;
  return p > v ? p : v;
}

// maximum over each row of 16 lanes, in every lane of the row
__device__ __forceinline__ u64 fps_row_max(u64 v) {
  v = fps_dpp_max<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = fps_dpp_max<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v = fps_dpp_max<0x141>(v);  // row_half_mirror
  v = fps_dpp_max<0x140>(v);  // row_mirror
  return v;
}

__device__ __forceinline__ u64 fps_wave_max(u64 v) {
  v = fps_row_max(v);
  u64 p = __shfl_xor(v, 16, 64);
  v = p > v ? p : v;
  p = __shfl_xor(v, 32, 64);
  return p > v ? p : v;
}

// the workgroup's arg-max: `best` = this thread's key (0: no point), (bx, by, bz, bk) its best point.  Returns the winner in
// (x1, y1, z1, old).  One barrier; `buf` alternates between consecutive calls.
__device__ __forceinline__ void fps_argmax(FpsSlots& s, int buf, u64 best, float bx, float by, float bz, int bk, float& x1,
                                           float& y1, float& z1, int& old) {
  const int lane = sst_lane(), wave = (int)(threadIdx.x >> 6);
  const u64 w = fps_wave_max(best);
  if (w == 0 ? lane == 0 : best == w) {  // keys of points are distinct and non-zero: exactly one lane writes
    s.key[buf][wave] = w;
    s.pt[buf][wave] = make_float4(bx, by, bz, __int_as_float(bk));
  }
  __syncthreads();
  const u64 k = s.key[buf][lane & (kFpsWaves - 1)];
  const float4 p = s.pt[buf][lane & (kFpsWaves - 1)];
  const u64 g = fps_row_max(k);
  const unsigned hit = (unsigned)__ballot(k == g) & 0xffffu;
  const int src = __builtin_amdgcn_readfirstlane(__ffs((int)hit) - 1);
  x1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.x), src));
  y1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.y), src));
  z1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.z), src));
  old = __builtin_amdgcn_readlane(__float_as_int(p.w), src);
}

__device__ __forceinline__ float fps_sqdist(float x2, float y2, float z2, float x1, float y1, float z1) {
  const float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;  // no contraction: exact_math.h's pragma and the Makefile's flag
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}

// low word of the key of this thread's point 0 (k = t); point i (k = t + 1024 i) has low word - i.  n >= 1.
__device__ __forceinline__ unsigned fps_low_base(int n, int t) {
  const int lb = n >= kFpsThreads ? 10 : 31 - __clz(n);  // B = 2^lb threads in the reference's launch
  const unsigned bsz = 1u << lb;
  const unsigned q = ((unsigned)n + bsz - 1) >> lb;       // k div B < q
  const unsigned kmod = (unsigned)t & (bsz - 1), kdiv = (unsigned)t >> lb;
  const unsigned rev = lb ? (__brev(kmod) >> (32 - lb)) : 0u;
  return 0xFFFFFFFFu - (rev * q + kdiv);
}

// SRC 0: src = the segment's points (row stride ld); SRC 1: src = its [n, n] distance matrix.  The first PPT * 1024 points
// stay in registers for the whole call; with TAIL the points behind them are streamed from memory on every sample,
// coordinates from `src` and the running minimum through `temp`.
template <int SRC, int PPT, bool TAIL>
__device__ __forceinline__ void fps_run(FpsSlots& s, const float* __restrict__ src, int64_t ld, int n, int m,
                                        float* __restrict__ temp, int32_t* __restrict__ out) {
  const int t = (int)threadIdx.x;
  float x[PPT], y[PPT], z[PPT], d[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int k = t + i * kFpsThreads;
    const bool ok = k < n;
    if (SRC == 0) {
      x[i] = ok ? src[(int64_t)k * ld] : 0.f;
      y[i] = ok ? src[(int64_t)k * ld + 1] : 0.f;
      z[i] = ok ? src[(int64_t)k * ld + 2] : 0.f;
    } else {
      x[i] = y[i] = z[i] = 0.f;
    }
    d[i] = ok ? 1e10f : -1.f;  // a slot without a point keeps -1 under the minimum and never wins
  }
  if (TAIL)
    for (int k = PPT * kFpsThreads + t; k < n; k += kFpsThreads) temp[k] = 1e10f;  // a thread only touches its own k
  const unsigned low0 = fps_low_base(n, t);
  float x1 = 0.f, y1 = 0.f, z1 = 0.f;
  int old = 0;
  if (SRC == 0) {
    x1 = src[0];
    y1 = src[1];
    z1 = src[2];
  }
  if (t == 0) out[0] = 0;
  for (int j = 1; j < m; ++j) {
    // the thread's own arg-max is the reference's scan: first strict maximum over k = t, t + 1024, ...
    float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
    int bk = 0;
    const float* __restrict__ row = src + (int64_t)old * n;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int k = t + i * kFpsThreads;
      float dd;
      if (SRC == 0) {
        dd = fps_sqdist(x[i], y[i], z[i], x1, y1, z1);
      } else {
        dd = k < n ? row[k] : 0.f;
      }
      d[i] = fminf(dd, d[i]);
      if (d[i] > best) {
        best = d[i];
        bk = k;
        bx = x[i];
        by = y[i];
        bz = z[i];
      }
    }
    if (TAIL) {
#pragma unroll 4
      for (int k = PPT * kFpsThreads + t; k < n; k += kFpsThreads) {
        float x2 = 0.f, y2 = 0.f, z2 = 0.f, dd;
        if (SRC == 0) {
          x2 = src[(int64_t)k * ld];
          y2 = src[(int64_t)k * ld + 1];
          z2 = src[(int64_t)k * ld + 2];
          dd = fps_sqdist(x2, y2, z2, x1, y1, z1);
        } else {
          dd = row[k];
        }
        const float dn = fminf(dd, temp[k]);
        temp[k] = dn;
        if (dn > best) {
          best = dn;
          bk = k;
          bx = x2;
          by = y2;
          bz = z2;
        }
      }
    }
    const u64 key = best < 0.f ? 0 : ((u64)__float_as_uint(best) << 32) | (low0 - ((unsigned)bk >> 10));
    fps_argmax(s, j & 1, key, bx, by, bz, bk, x1, y1, z1, old);
    if (t == 0) out[j] = old;
  }
}

template <int SRC>
__global__ __launch_bounds__(kFpsThreads) void fps_k(const float* __restrict__ data, int64_t ld,
                                                     const int32_t* __restrict__ seg_offsets, int64_t uniform_len, int m,
                                                     int identity_if_short, float* __restrict__ temp,
                                                     int32_t* __restrict__ idx, int32_t* __restrict__ count) {
  __shared__ FpsSlots slots;
  const int seg = (int)blockIdx.x, t = (int)threadIdx.x;
  int64_t start;
  int n;
  if (seg_offsets) {
    start = seg_offsets[seg];
    n = seg_offsets[seg + 1] - seg_offsets[seg];
  } else {
    start = (int64_t)seg * uniform_len;
    n = (int)uniform_len;
  }
  int32_t* out = idx + (int64_t)seg * m;
  if (n <= 0 || (identity_if_short && n <= m)) {  // nothing to sample: 0 .. n-1 in order, the rest of the row is -1
    if (n < 0) n = 0;
    for (int j = t; j < m; j += kFpsThreads) out[j] = j < n ? j : -1;
    if (t == 0 && count) count[seg] = n;
    return;
  }
  if (t == 0 && count) count[seg] = m;
  const float* src = SRC == 0 ? data + start * ld : data + start * (int64_t)n;  // SRC 1: start = seg * n, matrix seg
  float* tmp = temp + start;
  if (n <= 1 * kFpsThreads) fps_run<SRC, 1, false>(slots, src, ld, n, m, tmp, out);
  else if (n <= 2 * kFpsThreads) fps_run<SRC, 2, false>(slots, src, ld, n, m, tmp, out);
  else if (n <= 4 * kFpsThreads) fps_run<SRC, 4, false>(slots, src, ld, n, m, tmp, out);
  else if (n <= 8 * kFpsThreads) fps_run<SRC, 8, false>(slots, src, ld, n, m, tmp, out);
  else if (n <= kFpsRegMax) fps_run<SRC, kFpsRegPoints, false>(slots, src, ld, n, m, tmp, out);
  else fps_run<SRC, kFpsTailRegPoints, true>(slots, src, ld, n, m, tmp, out);
}

// ---------------------------------------------------------------------------------------------------------------
// SSG: pruning, numbering, assignment
// ---------------------------------------------------------------------------------------------------------------
constexpr int kSsgTile = 256;

__device__ __forceinline__ float ssg_dist(float ax, float ay, float bx, float by) { return sst_xy_dist(ax, ay, bx, by); }

// blockIdx.y = segment, blockIdx.x = tile of 256 keypoints j; the earlier keypoints i < j pass through LDS tile by tile
__global__ __launch_bounds__(kSsgTile) void ssg_prune_k(const float* __restrict__ pts, int64_t ld,
                                                        const int32_t* __restrict__ seg_offsets,
                                                        const int32_t* __restrict__ key_idx,
                                                        const int32_t* __restrict__ key_count, int m, float thr2,
                                                        int32_t* __restrict__ valid, int32_t* __restrict__ status) {
  __shared__ float xs[kSsgTile], ys[kSsgTile];
  const int seg = (int)blockIdx.y, t = (int)threadIdx.x;
  const int start = seg_offsets[seg], n = seg_offsets[seg + 1] - start;
  int cnt = key_count[seg];
  cnt = cnt < 0 ? 0 : (cnt > m ? m : cnt);
  const int j = (int)blockIdx.x * kSsgTile + t;
  const int32_t* kidx = key_idx + (int64_t)seg * m;
  float xj = 0.f, yj = 0.f;
  bool live = j < cnt, bad = false;
  if (live) {
    const int p = kidx[j];
    if (p < 0 || p >= n) {
      bad = true;
      live = false;
    } else {
      xj = pts[(int64_t)(start + p) * ld];
      yj = pts[(int64_t)(start + p) * ld + 1];
    }
  }
  if (bad) atomicOr(status, SST_SSG_BAD_KEYPOINT);
  bool hit = false;
  for (int tile = 0; tile <= (int)blockIdx.x; ++tile) {
    const int i = tile * kSsgTile + t;
    const int p = i < cnt ? kidx[i] : -1;
    const bool ok = p >= 0 && p < n;
    // a keypoint that cannot be read prunes nobody: NaN compares false
    xs[t] = ok ? pts[(int64_t)(start + p) * ld] : __int_as_float(0x7fc00000);
    ys[t] = ok ? pts[(int64_t)(start + p) * ld + 1] : 0.f;
    __syncthreads();
    if (live) {
      const int lim = j - tile * kSsgTile < kSsgTile ? j - tile * kSsgTile : kSsgTile;  // i < j only
      for (int q = 0; q < lim; ++q) hit |= ssg_dist(xs[q], ys[q], xj, yj) < thr2;
    }
    __syncthreads();
  }
  if (j < m) valid[(int64_t)seg * m + j] = (live && !hit) ? 1 : 0;
}

// blockIdx.y = segment; the blocks of a segment stride over its points, the keypoints pass through LDS
__global__ __launch_bounds__(kSsgTile) void ssg_assign_k(const float* __restrict__ pts, int64_t ld,
                                                         const int32_t* __restrict__ seg_offsets,
                                                         const int32_t* __restrict__ key_idx,
                                                         const int32_t* __restrict__ key_count, int m, float radius,
                                                         const int32_t* __restrict__ valid,
                                                         const int32_t* __restrict__ key_id,
                                                         int32_t* __restrict__ cluster_id, int32_t* __restrict__ seg_any,
                                                         int32_t* __restrict__ status) {
  __shared__ float xs[kSsgTile], ys[kSsgTile];
  __shared__ int ids[kSsgTile];
  const int seg = (int)blockIdx.y, t = (int)threadIdx.x;
  const int start = seg_offsets[seg], n = seg_offsets[seg + 1] - start;
  int cnt = key_count[seg];
  cnt = cnt < 0 ? 0 : (cnt > m ? m : cnt);
  const int32_t* kidx = key_idx + (int64_t)seg * m;
  bool any = false, many = false;
  for (int base = (int)blockIdx.x * kSsgTile; base < n; base += (int)gridDim.x * kSsgTile) {
    const int i = base + t;
    const bool live = i < n;
    const float xi = live ? pts[(int64_t)(start + i) * ld] : 0.f;
    const float yi = live ? pts[(int64_t)(start + i) * ld + 1] : 0.f;
    int hits = 0, id = -1;
    for (int k0 = 0; k0 < cnt; k0 += kSsgTile) {
      const int k = k0 + t;
      const bool ok = k < cnt && valid[(int64_t)seg * m + k] != 0;  // valid implies a readable index
      const int p = ok ? kidx[k] : 0;
      xs[t] = ok ? pts[(int64_t)(start + p) * ld] : 0.f;
      ys[t] = ok ? pts[(int64_t)(start + p) * ld + 1] : 0.f;
      ids[t] = ok ? key_id[(int64_t)seg * m + k] : -1;
      __syncthreads();
      if (live) {
        const int lim = cnt - k0 < kSsgTile ? cnt - k0 : kSsgTile;
        for (int q = 0; q < lim; ++q) {
          if (ids[q] >= 0 && ssg_dist(xs[q], ys[q], xi, yi) < radius) {
            ++hits;
            id = ids[q];
          }
        }
      }
      __syncthreads();
    }
    if (live) {
      cluster_id[start + i] = hits == 1 ? id : -1;
      any |= hits == 1;
      many |= hits > 1;
    }
  }
  if (__ballot(any) != 0 && sst_lane() == 0) atomicOr(seg_any + seg, 1);
  if (__ballot(many) != 0 && sst_lane() == 0) atomicOr(status, SST_SSG_MULTI_BALL);
}

__global__ __launch_bounds__(256) void ssg_finish_k(const int32_t* __restrict__ seg_offsets, int64_t n_segments,
                                                    const int32_t* __restrict__ seg_any, int32_t* __restrict__ status) {
  bool lost = false;
  for (int64_t s = threadIdx.x; s < n_segments; s += blockDim.x)
    lost |= seg_offsets[s + 1] > seg_offsets[s] && seg_any[s] == 0;
  if (lost) atomicOr(status, SST_SSG_EMPTY_SEGMENT);
}

}  // namespace

extern "C" {

int sst_fps_segmented_f32(const float* d_points, int64_t ld, int64_t n_points, const int32_t* d_seg_offsets,
                          int64_t uniform_len, int64_t n_segments, int m, int identity_if_short, float* d_temp,
                          int32_t* d_idx, int32_t* d_count, void* stream) {
  if (n_segments < 0 || m < 0 || n_points < 0 || ld < 3 || uniform_len < 0) return SST_ERR_ARG;
  if (n_points > 0x7fffffffLL || n_segments > 0x7fffffffLL) return SST_ERR_UNSUPPORTED;
  if (!d_seg_offsets && uniform_len * n_segments > n_points) return SST_ERR_ARG;
  if (n_segments == 0 || m == 0) return SST_OK;
  if (!d_idx || (n_points > 0 && (!d_points || !d_temp))) return SST_ERR_ARG;
  hipLaunchKernelGGL(fps_k<0>, dim3((unsigned)n_segments), dim3(kFpsThreads), 0, (hipStream_t)stream, d_points, ld,
                     d_seg_offsets, uniform_len, m, identity_if_short, d_temp, d_idx, d_count);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int sst_fps_with_dist_f32(const float* d_dist, int64_t batch, int64_t n, int m, float* d_temp, int32_t* d_idx,
                          void* stream) {
  if (batch < 0 || n < 0 || m < 0) return SST_ERR_ARG;
  if (n * batch > 0x7fffffffLL) return SST_ERR_UNSUPPORTED;
  if (batch == 0 || m == 0) return SST_OK;
  if (!d_idx || (n > 0 && (!d_dist || !d_temp))) return SST_ERR_ARG;
  hipLaunchKernelGGL(fps_k<1>, dim3((unsigned)batch), dim3(kFpsThreads), 0, (hipStream_t)stream, d_dist, (int64_t)1,
                     (const int32_t*)nullptr, n, m, 0, d_temp, d_idx, (int32_t*)nullptr);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int64_t sst_ssg_assign_workspace_bytes(int64_t n_segments, int m) {
  const int64_t k = (n_segments > 0 ? n_segments : 1) * (int64_t)(m > 0 ? m : 1);
  return 2 * sst_align_up(k * (int64_t)sizeof(int32_t), 256) +
         sst_align_up((n_segments > 0 ? n_segments : 1) * (int64_t)sizeof(int32_t), 256) + sst_scan_workspace_bytes(k) + 256;
}

int sst_ssg_assign_f32(const float* d_points, int64_t ld, int64_t n_points, const int32_t* d_seg_offsets,
                       int64_t n_segments, const int32_t* d_key_idx, const int32_t* d_key_count, int m, float thr2,
                       float radius, int32_t* d_cluster_id, int32_t* d_n_clusters, int32_t* d_status, void* d_workspace,
                       void* stream) {
  if (n_segments < 0 || m < 0 || n_points < 0 || ld < 2) return SST_ERR_ARG;
  if (n_points > 0x7fffffffLL || n_segments > 65535 || n_segments * (int64_t)m > 0x7fffffffLL) return SST_ERR_UNSUPPORTED;
  if (!d_n_clusters || !d_status) return SST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  SST_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
  SST_HIP(hipMemsetAsync(d_n_clusters, 0, sizeof(int32_t), st));
  if (n_segments == 0 || n_points == 0) return SST_OK;
  if (!d_points || !d_seg_offsets || !d_cluster_id || !d_workspace || !d_key_count || (m > 0 && !d_key_idx))
    return SST_ERR_ARG;
  if (m == 0) {  // no keypoints: nothing is assigned
    SST_HIP(hipMemsetAsync(d_cluster_id, 0xff, n_points * sizeof(int32_t), st));
    int32_t* seg_any0 = (int32_t*)d_workspace;
    SST_HIP(hipMemsetAsync(seg_any0, 0, n_segments * sizeof(int32_t), st));
    hipLaunchKernelGGL(ssg_finish_k, dim3(1), dim3(256), 0, st, d_seg_offsets, n_segments, seg_any0, d_status);
    SST_LAUNCH_CHECK();
    return SST_OK;
  }
  sst_carver ws(d_workspace);
  const int64_t k = n_segments * (int64_t)m;
  int32_t* valid = ws.take<int32_t>(k);
  int32_t* key_id = ws.take<int32_t>(k);
  int32_t* seg_any = ws.take<int32_t>(n_segments);
  void* scan_ws = ws.take<char>(sst_scan_workspace_bytes(k));
  SST_HIP(hipMemsetAsync(seg_any, 0, n_segments * sizeof(int32_t), st));
  hipLaunchKernelGGL(ssg_prune_k, dim3((unsigned)sst_div_up(m, kSsgTile), (unsigned)n_segments), dim3(kSsgTile), 0, st,
                     d_points, ld, d_seg_offsets, d_key_idx, d_key_count, m, thr2, valid, d_status);
  const int rc = sst_exclusive_scan_i32(valid, key_id, k, d_n_clusters, scan_ws, stream);
  if (rc != SST_OK) return rc;
  int64_t gx = sst_div_up(n_points, kSsgTile);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(ssg_assign_k, dim3((unsigned)gx, (unsigned)n_segments), dim3(kSsgTile), 0, st, d_points, ld,
                     d_seg_offsets, d_key_idx, d_key_count, m, radius, valid, key_id, d_cluster_id, seg_any, d_status);
  hipLaunchKernelGGL(ssg_finish_k, dim3(1), dim3(256), 0, st, d_seg_offsets, n_segments, seg_any, d_status);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

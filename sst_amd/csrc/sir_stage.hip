// One stage of FSD's SIRLayer in one launch forward and one backward (voxel_encoders/voxel_encoder.py:738-750, layers
// voxel_encoders/utils.py:147-189, stack backbones/sir.py:67-88, pooling ops/sst/sst_ops.py:172-177):
//   pre[r]  = x[r, 0:K] W[128, K]^T (+ add_rows[inverse[r]])      Linear without bias; the optional rows are the split-weight
//                                                                 form of cat([point_feats, pooled[unq_inv]]) W^T
//   y[r]    = act(LayerNorm(pre[r]))
//   pooled  = segmented max of y over the grouping's CSR, with the arg-max rows
// instead of a library GEMM, the row kernel of csrc/dense.hip, the tile reduction of csrc/scatter.hip and the gather + concat.
//
// Forward: a workgroup (4 waves) owns a tile of 64 consecutive SORTED positions, the tile of seg_tiles_k at c = 128; wave w
// holds rows 16 w .. 16 w + 15 of it as eight 16 x 16 accumulators of v_mfma_f32_16x16x4_f32 (exact fp32, as
// csrc/dense_f32.hip).  W is STREAMED through LDS in chunks of 32 columns of K rather than kept resident: a resident fp32 image at
// K = 256 is 128 KB of the CU's 160 KB, one workgroup per CU and a 128 KB fill in front of a tile that needs 7 us of MFMAs;
// with 28 KB of chunk buffers three workgroups share a CU, and the next chunk's global loads are in flight (registers) while
// the current one is multiplied.  The 100 KB of W stay in L2.  The gathered x rows go the same way, 4 bytes at a time: K = 133
// or 213 makes rows that are not 16-byte aligned, and K is padded to the chunk with ZERO operands, never with reads.
// The tile of pre-activations then lies in LDS (aliasing the chunk buffers); a 32-lane group per row applies the LayerNorm and
// the activation with the arithmetic of add_ln_fwd_k, writes pre / stats / y at the row's own index and leaves y in LDS,
// where the walk, merge and ticket step of csrc/seg_tiles.h reduce it.
// Backward: add_ln_bwd_k<true> (csrc/ln_rows.h), the LayerNorm + activation backward with the pooling's gradient routed in on
// load, then the column sums of its block partials: the scheme of sst_add_layernorm_act_bwd_f32.
#include <math.h>
#include "common.h"
#include "ln_rows.h"
#include "seg_tiles.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSirC = 128;                   // output width
constexpr int kSirLanes = 8;                 // row lanes of the reduction: 256 threads / 32 channel vectors
constexpr int kSirRows = kSirLanes * kSegSpan;   // 64 sorted rows per tile
constexpr int kSirKC = 32;                   // columns of K per chunk
constexpr int kSirRS = kSirKC + 4;           // LDS row stride of a chunk: 16-byte reads of 16 rows hit distinct banks
constexpr int kSirPS = kSirC + 4;            // LDS row stride of the pre-activation tile
constexpr int kSirXPer = kSirRows * kSirKC / 256;   // 8 x elements per thread and chunk
constexpr int kSirWPer = kSirC * kSirKC / 256;      // 16 W elements per thread and chunk
static_assert(kSirRows * kSirPS >= (kSirRows + kSirC) * kSirRS, "the tile aliases the chunk buffers");

__global__ __launch_bounds__(256) void sir_stage_fwd_k(const float* __restrict__ x, int K, const float* __restrict__ W,
                                                       int64_t ldw, const float* __restrict__ add_rows,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float eps, int act, const uint32_t* __restrict__ perm,
                                                       const int32_t* __restrict__ inverse,
                                                       const int32_t* __restrict__ offsets, int32_t n,
                                                       float* __restrict__ pre, float2* __restrict__ stats,
                                                       float* __restrict__ y, float* __restrict__ pooled,
                                                       int32_t* __restrict__ argmax, seg_rec* __restrict__ recs,
                                                       int32_t* __restrict__ counters) {
  __shared__ __attribute__((aligned(16))) float smem[kSirRows * kSirPS];   // chunks [64 + 128][36], then the tile [64][132]
  __shared__ __attribute__((aligned(16))) seg_rec lrec[kSirLanes * 2 * (kSirC / 4)];
  __shared__ int lgrp[kSirLanes * 2];
  __shared__ uint32_t srow[kSirRows];   // row index of every sorted position of the tile
  __shared__ int sgrp[kSirRows];        // its group (kSegNone behind the last position)
  __shared__ int tile_grp[2], finish[3], edge_grp[2];
  float* xs = smem;
  float* ws = smem + kSirRows * kSirRS;
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kSirRows;
  const int64_t t1 = t0 + kSirRows < n ? t0 + kSirRows : n;
  if (tid < kSirRows) {
    const int64_t p = t0 + tid;
    const uint32_t r = p < n ? perm[p] : 0u;
    srow[tid] = r;
    sgrp[tid] = p < n ? inverse[r] : kSegNone;
  } else if (tid < kSirRows + 2) {
    const int e = tid - kSirRows;
    tile_grp[e] = kSegNone;
    const int64_t pos = e == 0 ? t0 - 1 : t1;
    edge_grp[e] = (pos >= 0 && pos < n) ? inverse[perm[pos]] : kSegNone;
  }
  __syncthreads();

  // ---- pre = x W^T on the matrix pipe, K in chunks of 32 ----
  const int kk = tid & 31, r8 = tid >> 5;     // a thread fetches column kk of the chunk for rows r8, r8 + 8, ...
  const float* xrow[kSirXPer];
#pragma unroll
  for (int i = 0; i < kSirXPer; ++i) {
    const int row = r8 + 8 * i;
    xrow[i] = t0 + row < n ? x + (int64_t)srow[row] * K : nullptr;
  }
  float xr[kSirXPer], wr[kSirWPer];
  auto fetch = [&](int k0) {
    const int k = k0 + kk;
#pragma unroll
    for (int i = 0; i < kSirXPer; ++i) xr[i] = (k < K && xrow[i] != nullptr) ? xrow[i][k] : 0.f;
#pragma unroll
    for (int i = 0; i < kSirWPer; ++i) wr[i] = k < K ? W[(int64_t)(r8 + 8 * i) * ldw + k] : 0.f;
  };
  const int wave = tid >> 6, l = tid & 63;
  const int frag = (l & 15) * kSirRS + 4 * (l >> 4);   // MFMA step s of a 16-column group reads column 4 (l / 16) + s of it
  f32x4 acc[8];
#pragma unroll
  for (int T = 0; T < 8; ++T) acc[T] = (f32x4){0.f, 0.f, 0.f, 0.f};
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += kSirKC) {
    if (k0 > 0) __syncthreads();   // everybody has read the previous chunk
#pragma unroll
    for (int i = 0; i < kSirXPer; ++i) xs[(r8 + 8 * i) * kSirRS + kk] = xr[i];
#pragma unroll
    for (int i = 0; i < kSirWPer; ++i) ws[(r8 + 8 * i) * kSirRS + kk] = wr[i];
    __syncthreads();
    if (k0 + kSirKC < K) fetch(k0 + kSirKC);   // in flight behind this chunk's MFMAs
#pragma unroll
    for (int j = 0; j < kSirKC / 16; ++j) {
      const f32x4 a = *(const f32x4*)(xs + wave * 16 * kSirRS + frag + 16 * j);
      f32x4 b[8];
#pragma unroll
      for (int T = 0; T < 8; ++T) b[T] = *(const f32x4*)(ws + T * 16 * kSirRS + frag + 16 * j);
#pragma unroll
      for (int s = 0; s < 4; ++s)   // eight independent accumulators between two MFMAs on the same one
#pragma unroll
        for (int T = 0; T < 8; ++T) acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[T][s], acc[T], 0, 0, 0);
    }
  }
  __syncthreads();   // the chunk buffers are free: the tile takes their place
  float* tile = smem;
#pragma unroll
  for (int T = 0; T < 8; ++T)
#pragma unroll
    for (int v = 0; v < 4; ++v) tile[(wave * 16 + 4 * (l >> 4) + v) * kSirPS + T * 16 + (l & 15)] = acc[T][v];
  __syncthreads();

  // ---- LayerNorm + activation: a 32-lane group per row, one float4 per lane (the row functions of add_ln_fwd_k, csrc/ln_rows.h) ----
  {
    const int lane = tid & 31, sub = tid >> 5, col = lane * 4;
    const float4 wv = *(const float4*)(gamma + col);
    const float4 bv = *(const float4*)(beta + col);
#pragma unroll 2
    for (int pass = 0; pass < kSirRows / 8; ++pass) {
      const int row = pass * 8 + sub;
      const bool live = t0 + row < n;
      float4 v = *(const float4*)(tile + row * kSirPS + col);
      if (add_rows != nullptr && live) {
        const float4 rv = *(const float4*)(add_rows + (int64_t)sgrp[row] * kSirC + col);
        v.x += rv.x;
        v.y += rv.y;
        v.z += rv.z;
        v.w += rv.w;
      }
      const float s = v.x + v.y + v.z + v.w;
      const float mean = group32_sum(s) / (float)kSirC;
      const float var = group32_sum(ln_sqdev4(v, mean)) / (float)kSirC;
      const float rstd = rsqrtf(var + eps);
      const float4 o = ln_norm_act4(v, mean, rstd, wv, bv, act);
      *(float4*)(tile + row * kSirPS + col) = o;   // only this lane reads and writes these four words
      if (live) {
        const int64_t r = srow[row];
        *(float4*)(pre + r * kSirC + col) = v;
        *(float4*)(y + r * kSirC + col) = o;
        if (lane == 0) stats[r] = make_float2(mean, rstd);
      }
    }
  }
  __syncthreads();

  // ---- segmented max of the tile's y rows: csrc/seg_tiles.h, 8 row lanes x 32 channel vectors ----
  constexpr int cv = kSirC / 4;
  const int q = tid % cv, lane = tid / cv, ch = 4 * q;
  const float4 ident = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  const int4 noarg = make_int4(n, n, n, n);
  {
    const int64_t s0 = t0 + (int64_t)lane * kSegSpan;
    const int cnt = s0 >= n ? 0 : (int)(n - s0 < kSegSpan ? n - s0 : kSegSpan);
    uint32_t rows[kSegSpan];
    int grp[kSegSpan];
    float4 xv[kSegSpan];
#pragma unroll
    for (int i = 0; i < kSegSpan; ++i) {
      const int at = lane * kSegSpan + (cnt > 0 && i >= cnt ? cnt - 1 : i);
      rows[i] = srow[at];
      grp[i] = cnt > 0 ? sgrp[at] : kSegNone;
      xv[i] = *(const float4*)(tile + at * kSirPS + ch);
    }
    seg_span_walk<4>(SST_REDUCE_MAX, cnt, rows, grp, xv, ident, noarg, pooled, argmax, kSirC, ch, lane, q, cv, lrec, lgrp);
  }
  __syncthreads();
  if (lane == 0)
    seg_tile_merge<4>(SST_REDUCE_MAX, kSirLanes, cv, q, ch, kSirC, lrec, lgrp, edge_grp[0], edge_grp[1], ident, noarg, pooled,
                      argmax, recs + (int64_t)blockIdx.x * 2 * cv, tile_grp);
  seg_tile_finish<4>(SST_REDUCE_MAX, kSirLanes, cv, lane, q, ch, kSirC, kSirRows, offsets, counters, recs, lrec, tile_grp, finish,
                     ident, noarg, pooled, argmax);
}

inline bool sir_misaligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) != 0; }

}  // namespace

extern "C" {

int sst_sir_stage_tile_rows(void) { return kSirRows; }

int sst_sir_gather_segmax_fwd_f32(const float* d_x, int64_t n, int k, const float* d_weight, int64_t ldw, int c,
                                  const float* d_add_rows, const float* d_gamma, const float* d_beta, float eps, int act,
                                  const uint32_t* d_perm, const int32_t* d_inverse, const int32_t* d_offsets, int64_t m,
                                  void* d_scratch, float* d_pre, float* d_stats, float* d_y, float* d_pooled, int32_t* d_argmax,
                                  void* stream) {
  if (n < 0 || m < 0 || n > 0x7fffffff || ldw < k) return SST_ERR_ARG;
  if (c != kSirC || k < 1 || k > 256 || act < 0 || act > 2) return SST_ERR_UNSUPPORTED;
  if (n == 0 || m == 0) return SST_OK;
  if (!d_x || !d_weight || !d_gamma || !d_beta || !d_perm || !d_inverse || !d_offsets || !d_scratch || !d_pre || !d_stats ||
      !d_y || !d_pooled || !d_argmax)
    return SST_ERR_ARG;
  if (sir_misaligned(d_pre, 16) || sir_misaligned(d_y, 16) || sir_misaligned(d_pooled, 16) || sir_misaligned(d_argmax, 16) ||
      sir_misaligned(d_add_rows, 16) || sir_misaligned(d_gamma, 16) || sir_misaligned(d_beta, 16) || sir_misaligned(d_stats, 8) ||
      sir_misaligned(d_x, 4) || sir_misaligned(d_weight, 4) || sir_misaligned(d_scratch, 256))
    return SST_ERR_ARG;
  const int64_t tiles = sst_div_up(n, kSirRows);
  int32_t* counters = (int32_t*)d_scratch;   // [m], zeroed once by the caller, left zeroed: the layout of seg_tiles_k at c = 128
  seg_rec* recs = (seg_rec*)((char*)d_scratch + sst_align_up(m * 4, 256));
  hipLaunchKernelGGL(sir_stage_fwd_k, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, d_x, k, d_weight, ldw, d_add_rows,
                     d_gamma, d_beta, eps, act, d_perm, d_inverse, d_offsets, (int32_t)n, d_pre, (float2*)d_stats, d_y, d_pooled,
                     d_argmax, recs, counters);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int64_t sst_sir_gather_segmax_bwd_workspace_bytes(int64_t n) {
  (void)n;
  return (int64_t)1024 * 2 * kSirC * sizeof(float) + 256;
}

int sst_sir_gather_segmax_bwd_f32(const float* d_dy, const float* d_dpooled, const int32_t* d_argmax, const int32_t* d_inverse,
                                  const float* d_pre, const float* d_stats, const float* d_gamma, const float* d_beta, int act,
                                  int64_t n, int c, int64_t m, float* d_dpre, float* d_dgamma, float* d_dbeta, void* d_workspace,
                                  void* stream) {
  if (n < 0 || m < 0 || n > 0x7fffffff) return SST_ERR_ARG;
  if (c != kSirC || act < 0 || act > 2) return SST_ERR_UNSUPPORTED;
  if (!d_dgamma || !d_dbeta) return SST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    SST_HIP(hipMemsetAsync(d_dgamma, 0, sizeof(float) * c, st));
    SST_HIP(hipMemsetAsync(d_dbeta, 0, sizeof(float) * c, st));
    return SST_OK;
  }
  if (!d_pre || !d_stats || !d_gamma || !d_beta || !d_dpre || !d_workspace) return SST_ERR_ARG;
  if (d_dpooled != nullptr && (!d_argmax || !d_inverse || m < 1)) return SST_ERR_ARG;
  if (sir_misaligned(d_dy, 16) || sir_misaligned(d_dpooled, 16) || sir_misaligned(d_argmax, 16) || sir_misaligned(d_pre, 16) ||
      sir_misaligned(d_dpre, 16) || sir_misaligned(d_gamma, 16) || sir_misaligned(d_beta, 16) || sir_misaligned(d_stats, 8) ||
      sir_misaligned(d_workspace, 4))
    return SST_ERR_ARG;
  int grid = (int)sst_div_up(n, kLnRowsPerBlock * 4);   // the partial rows of sst_add_layernorm_act_bwd_f32: same sums, same order
  if (grid > 512) grid = 512;
  float* partials = (float*)d_workspace;
  hipLaunchKernelGGL(add_ln_bwd_k<true>, dim3(grid), dim3(kLnThreads), 2 * c * sizeof(float), st, d_dy, d_pre,
                     (const float2*)d_stats, d_gamma, d_beta, act, n, c, d_dpre, partials, d_dpooled, d_argmax, d_inverse);
  hipLaunchKernelGGL(colsum_partials_k, dim3((2 * c + 31) / 32), dim3(1024), 0, st, partials, grid, 2 * c, d_dgamma, d_dbeta, c);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

// (section 8 f4, 'bf16' operand mode) sparse 3-D convolution with bf16 OPERANDS: the contraction of csrc/spconv_os.hip (indiceConv
// and the data gradient of indiceConvBackward, mmdet3d/ops/spconv/include/spconv/spconv_ops.h:256-446),
//     Y[r, :] = sum_k X[map[k][r], :] W[k],
// and its filter gradient dW[k] = sum_p X[a_p]^T dY[b_p], with every operand rounded to bf16 ONCE (round to nearest even, the
// compiler's v_cvt_pk_bf16_f32: pack2 of csrc/mfma_tile.h), one v_mfma_f32_16x16x32_bf16 product per pair, fp32 accumulation in
// ONE accumulator set per tile, fp32 results.  Everything stays fp32 in memory: what a call returns is the contraction of
// round_bf16(x) and round_bf16(w) up to the fp32 summation order - the quantity the 'f32x6' kernels return on operands rounded
// beforehand (the exact split of a bf16 value is that value), which is how tests/test_gpu_spconv_bf16.py pins the mode.
// Per-module switch: sst_amd.spconv.SparseConvolution.set_precision('bf16').
//
// Contraction = csrc/spconv_os_mma.h, of which this file states one policy (csrc/spconv_os_x6.hip minus the split): W[k] packed
// as ONE bf16 image, 2 bytes per element, partner rows gathered as fp32 and converted in registers, the offsets of a thin level
// dealt out.
// Occupancy: a W slab is 64 channels x 16 NCT columns x 2 bytes = 8 KB (NCT = 4) or 16 KB (NCT = 8), a third of the x6 kernel's;
// with the index image (kvol x 64 words, 6.75 KB at 27 offsets) a workgroup holds 23 / 39 KB of the CU's 160 KB, so LDS admits
// 6 / 4 workgroups where the x6 kernel fits 3 / 1.  The kernel is a gather: what hides the latency of the partner rows is other
// workgroups' products, so the register budget is set for that residency - __launch_bounds__(256, 4) (one wave of every
// workgroup per SIMD: at least 4 waves per SIMD; the 64-column kernel holds 16 accumulator + 16 gathered + 8 packed + 8 weight
// registers) and (256, 3) for the 128-column class (32 accumulator registers, 16 weight registers in flight).  The compiler
// reports 68 and 92 VGPRs, no spills and private_segment_fixed_size 0 for the two: registers would allow 7 / 5 waves per SIMD,
// LDS is what bounds the residency.  Column classes as the x6 kernel's: 64 columns per workgroup, 128 only where that still
// leaves 2048 units (a wider class would halve the gathers per output column but the thin levels need the workgroups).
//
// Filter gradient = sp_wgrad_os_x6_k (csrc/spconv_os.hip) minus the split: same 64 x 64 blocks of dW[k], pair chunks, workspace
// and fixed-order reduction (sp_wgrad_os_reduce_k), per operand ONE bf16 image [64 channels][64 pairs] in the same swizzled
// layout; the two images are 16 KB, so they are double-buffered (32 KB) and a stage costs one barrier instead of two.
// No float atomics anywhere: two runs agree bit for bit.
#include "spconv_os_mma.h"
#include "spconv_os_wgrad.h"

namespace {

struct bf16_mode {
  static constexpr int P = 1, ACCS = 1;   // one image, one accumulator set
  static constexpr bool kSplit = true, kWholePack = true;
  static constexpr int kWsAlign = 256, kPackSlack = 0;
  static constexpr int min_wg(int nct) { return nct == 4 ? 4 : 3; }   // the residency argument above
  static const char* split_env() { return "SST_SPCONV_BF16_SPLIT"; }
  static __device__ __forceinline__ void split(f32x4 a, f32x4 b, u32x4 (&p)[1]) {
    p[0] = (u32x4){pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3])};
  }
  static __device__ __forceinline__ f32x4 leading(const u32x4 (&w)[1], const u32x4 (&x)[1], f32x4 acc) { return mma32(w[0], x[0], acc); }
};

// ---------------------------------------------------------------------------------------------------------------
// The filter gradient.  Decomposition of sp_wgrad_os_k / sp_wgrad_os_x6_k (csrc/spconv_os.hip): grid = (chunk slots, 64 x 64
// blocks of dW[k]), a workgroup walks its chunk of one offset's pairs in stages of 64, wave = 32 x 32 quadrant, rows global ->
// registers -> LDS transposed, indices two stages ahead; partials [chunk slot][cin][cout] summed by sp_wgrad_os_reduce_k.
// LDS image per operand: [64 channels][64 pairs] bf16 in 128-byte rows, written as 8-byte groups of 4 consecutive pairs, read as
// the 16-byte fragments the instruction wants (lane (l15, g): pairs 32 ks + 8 g .. + 7 of channel row l15), swizzled by
// os_wg_unit (csrc/spconv_os_wgrad.h: the x6 kernel's); the chunk slots are numbered by os_find_chunk, as theirs.
__global__ __launch_bounds__(256) void sp_wgrad_os_bf16_k(const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ dy, int64_t lddy,
                                                          const int32_t* __restrict__ pairs, int64_t pair_ld, int x_side,
                                                          const int32_t* __restrict__ num, int kvol, int cin, int cout,
                                                          int n_bj, int csize, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) unsigned char img[2][2][64 * 128];   // [buffer][X | dY]
  int k, first;
  if (!os_find_chunk(num, kvol, blockIdx.x, csize, k, first)) return;  // uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int bi = blockIdx.y / n_bj, bj = blockIdx.y - bi * n_bj;
  const int ci0 = bi * 64, co0 = bj * 64;
  const int np = num[k];
  const int p0 = (blockIdx.x - first) * csize;
  const int p1 = p0 + csize < np ? p0 + csize : np;
  const int32_t* pa = pairs + ((int64_t)k * 2 + x_side) * pair_ld;
  const int32_t* pb = pairs + ((int64_t)k * 2 + (1 - x_side)) * pair_ld;
  // staging role of this thread: pairs 4 pq + u (u < 4) of the stage, channels 4 ch4 .. + 3 of the block
  const int ch4 = tid & 15, pq = tid >> 4;
  int ca = ci0 + 4 * ch4, cb = co0 + 4 * ch4;
  ca = ca < cin - 4 ? ca : cin - 4;      // channel tails: a clamped (finite) piece whose products are never stored
  cb = cb < cout - 4 ? cb : cout - 4;
  int ia[4], ib[4];
  f32x4 ra[4], rb[4];
  bool live[4];
  auto load_idx = [&](int p) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int pp = p + 4 * pq + u;
      pp = pp < p1 ? pp : p1 - 1;
      ia[u] = pa[pp];
      ib[u] = pb[pp];
    }
  };
  auto load_rows = [&](int p) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      live[u] = p + 4 * pq + u < p1;
      ra[u] = *(const f32x4*)(x + (int64_t)ia[u] * ldx + ca);
      rb[u] = *(const f32x4*)(dy + (int64_t)ib[u] * lddy + cb);
    }
  };
  auto store_rows = [&](int buf) {   // pairs beyond the chunk (the chunk's last pair, loaded again): both operands 0
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = 4 * ch4 + e;
      const int off = row * 128 + os_wg_unit(row, pq >> 1) * 16 + (pq & 1) * 8;
      *(u32x2*)(img[buf][0] + off) = (u32x2){pack2(live[0] ? ra[0][e] : 0.f, live[1] ? ra[1][e] : 0.f),
                                             pack2(live[2] ? ra[2][e] : 0.f, live[3] ? ra[3][e] : 0.f)};
      *(u32x2*)(img[buf][1] + off) = (u32x2){pack2(live[0] ? rb[0][e] : 0.f, live[1] ? rb[1][e] : 0.f),
                                             pack2(live[2] ? rb[2][e] : 0.f, live[3] ? rb[3][e] : 0.f)};
    }
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;   // this wave's quadrant of the 64 x 64 block
  load_idx(p0);
  load_rows(p0);
  load_idx(p0 + kWgStage);
  store_rows(0);
  __syncthreads();
  int buf = 0;
  for (int p = p0; p < p1; p += kWgStage) {
    load_rows(p + kWgStage);        // rows of the next stage (their indices were requested a stage ago)
    load_idx(p + 2 * kWgStage);     // indices of the stage after it
    __builtin_amdgcn_sched_barrier(0);   // the loads are issued HERE, in front of the products that hide their latency
#pragma unroll
    for (int ks = 0; ks < kWgStage / 32; ++ks) {
      u32x4 af[2], bf[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ra_ = wi + 16 * h + l15, rb_ = wj + 16 * h + l15;
        af[h] = *(const u32x4*)(img[buf][0] + ra_ * 128 + os_wg_unit(ra_, 4 * ks + g) * 16);
        bf[h] = *(const u32x4*)(img[buf][1] + rb_ * 128 + os_wg_unit(rb_, 4 * ks + g) * 16);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = mma32(af[a], bf[b], acc[a][b]);
    }
    __builtin_amdgcn_sched_barrier(0);
    store_rows(buf ^ 1);              // the other buffer: its last readers passed the barrier of the stage before
    __syncthreads();
    buf ^= 1;
  }
  // D[i][j]: lane = (j = l15, rows i = 4 g + r): dW[k][ci0 + wi + 16 a + 4 g + r][co0 + wj + 16 b + l15]
  float* dst = part + (int64_t)blockIdx.x * cin * cout;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int n = co0 + wj + 16 * b + l15;
      if (n >= cout) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = ci0 + wi + 16 * a + 4 * g + r;
        if (c < cin) dst[(int64_t)c * cout + n] = acc[a][b][r];
      }
    }
}

}  // namespace

extern "C" {

// packed weights (2 bytes per element, worst-case column class) + the partial tiles of a call on m rows when its offsets are
// dealt out over several workgroups (thin levels): what sst_spconv_conv_os_rows_bf16 wants for its own choice of the split
int64_t sst_spconv_conv_os_bf16_workspace_bytes_rows(int kvol, int cin, int cout, int64_t m) {
  if (kvol < 1 || cin < 1 || cout < 1 || m < 0) return SST_ERR_ARG;
  return sp_mma_pack_bytes<bf16_mode>(kvol, cin, cout) + sp_mma_partial_bytes<bf16_mode>(m, kvol, cin, cout);
}

int sst_spconv_conv_os_rows_bf16(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                                 int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                                 const int32_t* d_tile_order, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return sp_mma_conv<bf16_mode>(d_x, ldx, d_map, m, kvol, d_w, cin, cout, trans_w, d_bias, d_y, ldy, tile_cfg, d_tile_order,
                                d_workspace, workspace_bytes, stream);
}

}  // extern "C"

// the launch plan of sst_spconv_conv_os_rows_bf16 on workspace_bytes; asked by sst_spconv_conv_os_plan (csrc/spconv_os.hip)
int sst_internal_spconv_bf16_plan(int64_t m, int kvol, int cin, int cout, int64_t workspace_bytes, int32_t* tile_rows,
                                  int32_t* cols, int32_t* n_split, int64_t* workgroups) {
  return sp_mma_plan_query<bf16_mode>(m, kvol, cin, cout, workspace_bytes, tile_rows, cols, n_split, workgroups);
}

// the filter-gradient launch of sst_spconv_wgrad_os_bf16 (csrc/spconv_os.hip: wgrad_os_any checks the arguments, sizes the
// chunks and reduces the partials)
void sst_internal_spconv_wgrad_bf16_launch(const float* d_x, int64_t ldx, const float* d_dy, int64_t lddy, const int32_t* d_pairs,
                                           int64_t pair_ld, int x_side, const int32_t* d_num, int kvol, int cin, int cout,
                                           int64_t chunks, int n_bi, int n_bj, int csize, float* d_part, void* stream) {
  hipLaunchKernelGGL(sp_wgrad_os_bf16_k, dim3((unsigned)chunks, (unsigned)(n_bi * n_bj)), dim3(256), 0, (hipStream_t)stream, d_x,
                     ldx, d_dy, lddy, d_pairs, pair_ld, x_side, d_num, kvol, cin, cout, n_bj, csize, d_part);
}

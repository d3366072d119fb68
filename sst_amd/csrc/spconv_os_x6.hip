// (section 8 f4, exact-split mode) sparse 3-D convolution on the bf16 matrix pipe with the EXACT three-way operand split of
// csrc/dense_f32x6.hip: the contraction of csrc/spconv_os.hip (indiceConv and the data gradient of indiceConvBackward,
// mmdet3d/ops/spconv/include/spconv/spconv_ops.h:256-446),
//     Y[r, :] = sum_k X[map[k][r], :] W[k],
// x = x0 + x1 + x2 and w = w0 + w1 + w2 (bf16 parts, 8 + 8 + 8 significand bits: exact), the six products x_i w_j with
// i + j <= 2 accumulated in fp32 by v_mfma_f32_16x16x32_bf16: what is dropped is below 2^-24 of a product.  Two accumulator
// sets per column tile - the leading product alone, the five corrections together - summed once at the end (the long chains
// of this contraction, 27 offsets x C_in / 32 steps, are where a single set drifts: csrc/wgrad_x6.hip).  Everything stays fp32
// in memory.  Why: with all workgroups resident the fp32 kernel is bound by the fp32 matrix pipe (64 x v_mfma_f32_16x16x4_f32 =
// 2 048 pipe cycles per wave and 64-channel stage); the same stage is 48 bf16 instructions = 768 cycles here.
// Admissibility (same arithmetic class as the fp32 kernel): tests/test_gpu_spconv.py::test_exact_split_convolution_kernel -
// error against the float64 oracle <= 2 x the fp32 kernel's.  `sst_amd.spconv.set_conv_precision('f32x6')`.
//
// Structure = csrc/spconv_os_mma.h, of which this file states one policy: W[k] packed as THREE bf16 images, 6 bytes per element
// (2 workgroups per CU at 64 columns, 1 at 128), partner rows split in registers, the offsets of a thin level dealt out.
#include "spconv_os_mma.h"

namespace {

struct x6_mode {
  static constexpr int P = 3, ACCS = 2;   // the three parts; leading product | the five corrections
  static constexpr bool kSplit = true, kWholePack = false;
  static constexpr int kWsAlign = 256, kPackSlack = 256;
  static constexpr int min_wg(int nct) { return nct == 4 ? 2 : 1; }
  static const char* split_env() { return "SST_SPCONV_X6_SPLIT"; }
  static __device__ __forceinline__ void split(const f32x4& a, const f32x4& b, u32x4 (&p)[3]) { split8(a, b, p[0], p[1], p[2]); }
  // corrections, smallest first: (0,2) (2,0) (1,1) ~ 2^-16, (0,1) (1,0) ~ 2^-8; then the leading product
  static __device__ __forceinline__ f32x4 corrections(const u32x4 (&w)[3], const u32x4 (&x)[3], f32x4 acl) {
    acl = mma32(w[0], x[2], acl);
    acl = mma32(w[2], x[0], acl);
    acl = mma32(w[1], x[1], acl);
    acl = mma32(w[0], x[1], acl);
    return mma32(w[1], x[0], acl);
  }
  static __device__ __forceinline__ f32x4 leading(const u32x4 (&w)[3], const u32x4 (&x)[3], f32x4 acc) { return mma32(w[0], x[0], acc); }
};

}  // namespace

extern "C" {

// packed weights of one call: kvol x column groups x channel chunks slabs of 2 x nct x 3 x 64 x 4 words (worst case nct = 8)
int64_t sst_spconv_conv_os_f32x6_workspace_bytes(int kvol, int cin, int cout) {
  if (kvol < 1 || cin < 1 || cout < 1) return SST_ERR_ARG;
  return sp_mma_pack_bytes_max<x6_mode>(kvol, cin, cout) + x6_mode::kPackSlack;
}
// ... plus the partial tiles of a call on m rows when its offsets are dealt out over several workgroups (thin levels):
// what sst_spconv_conv_os_rows_f32x6 wants for its own choice of the split
int64_t sst_spconv_conv_os_f32x6_workspace_bytes_rows(int kvol, int cin, int cout, int64_t m) {
  if (kvol < 1 || cin < 1 || cout < 1 || m < 0) return SST_ERR_ARG;
  return sp_mma_pack_bytes<x6_mode>(kvol, cin, cout) + sp_mma_partial_bytes<x6_mode>(m, kvol, cin, cout) + 256;
}

// same arguments as sst_spconv_conv_os_f32 + the size of the workspace: sst_spconv_conv_os_f32x6_workspace_bytes_rows bytes let
// the call deal the offsets of a thin level out over several workgroups; with less (sst_spconv_conv_os_f32x6_workspace_bytes:
// the packed weights alone) it runs unsplit.  tile_cfg must be 0.
int sst_spconv_conv_os_rows_f32x6(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                                  int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                                  const int32_t* d_tile_order, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return sp_mma_conv<x6_mode>(d_x, ldx, d_map, m, kvol, d_w, cin, cout, trans_w, d_bias, d_y, ldy, tile_cfg, d_tile_order,
                              d_workspace, workspace_bytes, stream);
}

// the unsplit call (workspace: sst_spconv_conv_os_f32x6_workspace_bytes)
int sst_spconv_conv_os_f32x6(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                             int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                             const int32_t* d_tile_order, void* d_workspace, void* stream) {
  return sp_mma_conv<x6_mode>(d_x, ldx, d_map, m, kvol, d_w, cin, cout, trans_w, d_bias, d_y, ldy, tile_cfg, d_tile_order,
                              d_workspace, kvol > 0 && cin > 0 && cout > 0 ? sp_mma_pack_bytes<x6_mode>(kvol, cin, cout) : 0, stream);
}

}  // extern "C"

// the launch plan of sst_spconv_conv_os_rows_f32x6 on workspace_bytes (rows = 1), or of sst_spconv_conv_os_f32x6 and the
// packed weights it offers itself; asked by sst_spconv_conv_os_plan (csrc/spconv_os.hip)
int sst_internal_spconv_x6_plan(int rows, int64_t m, int kvol, int cin, int cout, int64_t workspace_bytes, int32_t* tile_rows,
                                int32_t* cols, int32_t* n_split, int64_t* workgroups) {
  if (!rows) workspace_bytes = sp_mma_pack_bytes<x6_mode>(kvol, cin, cout);
  return sp_mma_plan_query<x6_mode>(m, kvol, cin, cout, workspace_bytes, tile_rows, cols, n_split, workgroups);
}

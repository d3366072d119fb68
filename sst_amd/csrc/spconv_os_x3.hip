// (§8 f4, precision mode) sparse 3-D convolution in SPLIT precision: the contraction of csrc/spconv_os.hip
// (indiceConv and the data gradient of indiceConvBackward, mmdet3d/ops/spconv/include/spconv/spconv_ops.h:256-446),
//     Y[r, :] = sum_k X[map[k][r], :] W[k],
// with every fp32 product formed as three bf16 products of split operands,
//     x w ~= x_hi w_hi + x_lo w_hi + x_hi w_lo      (x = x_hi + x_lo, x_hi = bf16(x), x_lo = bf16(x - x_hi); fp32 accumulation)
// on v_mfma_f32_16x16x32_bf16 - the scheme of csrc/dense_f32x3.hip for the dense layers.  Everything stays fp32 in memory.
// Why: with all workgroups resident the fp32 kernel is bound by the fp32 matrix pipe (64 x v_mfma_f32_16x16x4_f32 = 2 048
// pipe cycles per wave and 64-channel stage); the same stage is 24 bf16 instructions = 384 cycles here.  What remains is
// the skeleton of the stage (gathers, LDS staging, barrier).  Error ~1e-5 of the output scale per layer (tighter than the
// TF32 products the reference's torch 1.8 used on Ampere, `allow_tf32` default); the exact-fp32 kernel stays the default and
// the parity mode, this one is `sst_amd.spconv.set_conv_precision('f32x3')`.
//
// Structure = csrc/spconv_os_mma.h, of which this file states one policy: W[k] packed as bf16 hi / lo fragment images (the same
// 4 bytes per element as the fp32 kernel's), partner rows gathered straight into MFMA operands (a lane's two 16-byte loads = the
// 8 consecutive channels the 16x16x32 B operand wants) and split in registers.  No offset split for thin levels: the entry is
// not told its workspace size (it shares sst_spconv_conv_os_workspace_bytes and its 16-byte alignment with the fp32 entry).
#include "spconv_os_mma.h"

namespace {

struct x3_mode {
  static constexpr int P = 2, ACCS = 1;   // hi | lo images; one accumulator set
  static constexpr bool kSplit = false, kWholePack = false;
  static constexpr int kWsAlign = 16, kPackSlack = 0;
  static constexpr int min_wg(int nct) { return nct == 4 ? 4 : 2; }
  static const char* split_env() { return nullptr; }
  static __device__ __forceinline__ void split(const f32x4& a, const f32x4& b, u32x4 (&p)[2]) { split8(a, b, p[0], p[1]); }
  // x w ~= x_hi w_hi + x_lo w_hi + x_hi w_lo
  static __device__ __forceinline__ f32x4 leading(const u32x4 (&w)[2], const u32x4 (&x)[2], f32x4 acc) {
    acc = mma32(w[0], x[0], acc);
    acc = mma32(w[0], x[1], acc);
    return mma32(w[1], x[0], acc);
  }
};

}  // namespace

extern "C" {

// same arguments and workspace size (sst_spconv_conv_os_workspace_bytes) as sst_spconv_conv_os_f32; tile_cfg must be 0
int sst_spconv_conv_os_f32x3(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                             int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                             const int32_t* d_tile_order, void* d_workspace, void* stream) {
  return sp_mma_conv<x3_mode>(d_x, ldx, d_map, m, kvol, d_w, cin, cout, trans_w, d_bias, d_y, ldy, tile_cfg, d_tile_order,
                              d_workspace, INT64_MAX, stream);
}

}  // extern "C"

// the launch plan of sst_spconv_conv_os_f32x3; asked by sst_spconv_conv_os_plan (csrc/spconv_os.hip)
int sst_internal_spconv_x3_plan(int64_t m, int kvol, int cin, int cout, int32_t* tile_rows, int32_t* cols, int32_t* n_split,
                                int64_t* workgroups) {
  return sp_mma_plan_query<x3_mode>(m, kvol, cin, cout, INT64_MAX, tile_rows, cols, n_split, workgroups);
}

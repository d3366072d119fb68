// What the kernels built on v_mfma_f32_16x16x32_bf16 share: the vector types, the bf16 pack / unpack pair, the EXACT split of an
// fp32 value into bf16 parts, the product itself, and the LDS image of a weight matrix that those kernels read their A operands
// from (row permutation, fragment order, the LDS-DMA that fills it, the barrier behind it).  The exactness of the split is the
// premise of the library's default arithmetic ("f32x6": csrc/dense_f32x6.hip) - it is stated HERE and nowhere else, and the
// exact-operand suites of every including file pin it.  No kernels, no host code.
#pragma once
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short bf16_t;

// round-to-nearest-even pair -> (hi << 16) | lo: the conversion of the whole vector compiles to ONE v_cvt_pk_bf16_f32 (RNE)
// (two scalar casts `{(__bf16)lo, (__bf16)hi}` give the same bits from one conversion per element and a merge).  It must be
// the compiler's own instruction, not inline asm: an MFMA that reads a register written by the VALU two instructions earlier
// needs wait states on gfx950, and the hazard pass cannot see inside an asm statement (measured: stale operands, NaN).
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float lo_f(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float hi_f(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
__device__ __forceinline__ f32x4 mma32(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// two floats -> their three bf16 parts, packed pairwise: p0 = bf16(x), p1 = bf16(x - p0), p2 = x - p0 - p1.  EXACT: an fp32
// significand is 24 bits = 8 + 8 + 8, every subtraction is exact and the last pack rounds nothing away.
__device__ __forceinline__ void split2(float a, float b, unsigned& p0, unsigned& p1, unsigned& p2) {
  p0 = pack2(a, b);
  const float ra = a - lo_f(p0), rb = b - hi_f(p0);
  p1 = pack2(ra, rb);
  p2 = pack2(ra - lo_f(p1), rb - hi_f(p1));
}
// 8 consecutive k (one lane's share of a k-step) -> the three parts as MFMA operands
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, u32x4& p0, u32x4& p1, u32x4& p2) {
  unsigned q0[4], q1[4], q2[4];
  split2(a[0], a[1], q0[0], q1[0], q2[0]);
  split2(a[2], a[3], q0[1], q1[1], q2[1]);
  split2(b[0], b[1], q0[2], q1[2], q2[2]);
  split2(b[2], b[3], q0[3], q1[3], q2[3]);
  p0 = (u32x4){q0[0], q0[1], q0[2], q0[3]};
  p1 = (u32x4){q1[0], q1[1], q1[2], q1[3]};
  p2 = (u32x4){q2[0], q2[1], q2[2], q2[3]};
}
// the two-way split of the "f32x3" arithmetic: hi = bf16(x), lo = bf16(x - hi) (what lo rounds away, 2^-16 |x|, is dropped)
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, u32x4& hi, u32x4& lo) {
  hi[0] = pack2(a[0], a[1]);
  hi[1] = pack2(a[2], a[3]);
  hi[2] = pack2(b[0], b[1]);
  hi[3] = pack2(b[2], b[3]);
  lo[0] = pack2(a[0] - lo_f(hi[0]), a[1] - hi_f(hi[0]));
  lo[1] = pack2(a[2] - lo_f(hi[1]), a[3] - hi_f(hi[1]));
  lo[2] = pack2(b[0] - lo_f(hi[2]), b[1] - hi_f(hi[2]));
  lo[3] = pack2(b[2] - lo_f(hi[3]), b[3] - hi_f(hi[3]));
}

// LDS image of a weight matrix W[N][K]: row rho = 16 T + i holds W[n(T, i)][0..K), n(T, i) = 32 (T >> 1) + 8 (i >> 2) +
// 4 (T & 1) + (i & 3); w_lds_row is the inverse, n -> rho.  The TRANSPOSED product Y^T = W X^T over the tile pair (2 tp, 2 tp + 1)
// then leaves lane (g, c) with columns 32 tp + 8 g .. + 7 of row c: 8 consecutive columns of one row, which is one 16-byte
// store - and, packed to bf16, the B operand (token c, k = 8 g .. 8 g + 7) of the next product's k-step.
__device__ __forceinline__ int w_lds_row(int n) {
  const int tp = n >> 5, within = n & 31;
  return 16 * (2 * tp + ((within >> 2) & 1)) + ((within >> 3) << 2) + (within & 3);
}

// The image is FRAGMENT-contiguous: the 16 rows x 32 k (bf16) an MFMA A operand covers are one 1 KiB block in lane order (lane
// (c, g) = row c, k 8 g .. 8 g + 7 at byte 16 * (16 g + c)), a fragment read is base + 16 * lane.  ds_read_b128 is served in four
// groups of 16 NON-contiguous lanes: lane order has every group cover all 64 banks exactly once, and needs no padding.
constexpr int kFrag = 1024;
// byte offset inside an image of the 16 bytes (row lr of the image, k8 .. k8 + 7), the image having `ks` k-steps per row tile
__device__ __forceinline__ int frag_off(int lr, int k8, int ks) {
  return ((lr >> 4) * ks + (k8 >> 5)) * kFrag + (16 * ((k8 >> 3) & 3) + (lr & 15)) * 16;
}

// sum over the 16 lanes of a DPP row (the 16 tokens of a tile held by the lanes of one k group), every lane gets the total:
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror - four v_add_f32 with a DPP operand, no LDS crossbar
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_sum16(float v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  return dpp_add<0x140>(v);
}

// THE barrier of a choreography that fills LDS by DMA: every vector-memory operation of this wave - its LDS-DMA pieces among
// them - and every LDS operation has completed, then the workgroup meets ("landed for all waves" and "nobody reads any more" in
// one).  Written out: __syncthreads() leaves the vmcnt wait to the compiler's view of which LDS-DMA may alias which ds_read, and
// a missing one shows as rare wrong tiles in workgroups that start late (found by running a kernel twice on the same input:
// 2 % of the rows differed).
__device__ __forceinline__ void barrier_drain() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS-DMA (global_load_lds_dwordx4: no registers, no VALU) of `pieces` KiB from src to the LDS address dst, both in 1 KiB
// pieces, the WAVES waves of the workgroup taking pieces in turn.  Completion: the issuing wave's vmcnt, then a barrier -
// barrier_drain() is both.
template <int WAVES>
__device__ __forceinline__ void dma_pieces(const unsigned char* __restrict__ src, unsigned char* dst, int pieces, int wave, int lane) {
  for (int i = wave; i < pieces; i += WAVES)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i * 1024 + lane * 16),
                                     (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
}

}  // namespace

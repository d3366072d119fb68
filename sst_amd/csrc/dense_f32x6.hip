// Tall fp32 linear layers on the bf16 matrix pipe with an EXACT three-way operand split ("f32x6"):
//   Y[M, N] = epilogue(X[M, K] W^T + b),   x = x0 + x1 + x2,  w = w0 + w1 + w2   (bf16 each, the split is EXACT:
//   an fp32 significand is 24 bits = 8 + 8 + 8; x0 = bf16(x), x1 = bf16(x - x0), x2 = x - x0 - x1, every subtraction exact)
//   x w  =  sum over the nine products x_i w_j;  kept: the six with i + j <= 2
//        =  x0 w0 + (x0 w1 + x1 w0) + (x0 w2 + x1 w1 + x2 w0)      [+ x1 w2 + x2 w1 + x2 w2, dropped: <= 2^-24 |x w| together]
// Each kept product of two 8-bit significands is exact in the fp32 accumulator of v_mfma_f32_16x16x32_bf16, so what is left
// against the exact product is the dropped tail (~2^-25 |x w| per term, sign-random: below the rounding an fp32 FMA chain of
// the same length makes per addend) and the accumulator's own roundings.  Measured against float64 beside the native fp32
// kernel on the same inputs: tests/test_gpu_dense_f32x6.py (the admissibility bar of VERDICT round 3, item 3: <= 2 x the
// error of the v_mfma_f32_16x16x4_f32 kernel for every shape and through the 12-layer stack).
//
// for the projections and the FFN of an SRA encoder layer, forward and data gradient (sst_basic_block_v2.py:41-75, 104-126),
// (K, N) in {(128,128), (128,256), (128,384), (256,128), (384,128)}, fp32 operands in HBM, the epilogues of csrc/dense_f32.hip.
//
// Why: six bf16 instructions per 16 x 16 x 32 block are 6 x 16 = 96 matrix-pipe cycles against 8 x 32 = 256 for the same block
// on the fp32 pipe (MI355X_MICROARCH.md: 16x16x32 bf16 ~16 cycles, 16x16x4 f32 32 cycles per SIMD): the exact-fp32 kernels of
// dense_f32.hip are bound by that pipe (54-60 % of 157 TFLOP/s, 7.1 of the 13.7 ms step), this one by HBM on its fp32
// operands ((K + N) x 4 B / token) - same numbers in, same numbers out.
//
// Structure = tall_linear_f32x3_k with THREE bf16 images of W in LDS.  3 x N x K x 2 B is 196 KB for the 256-wide shapes,
// so the output columns are cut into groups of NW (128 for K = 128, 64 for K = 256: 104 / 101 KB) and a workgroup owns
// (row block, column group): W of ITS columns resident for the whole kernel, 8 waves, 16-row steps, X read in ROW shape (a
// lane takes 16 bytes of a row, 8 lanes a 128-byte line) and turned into MFMA fragments through a wave-private 2 KiB LDS block
// (csrc/tile_io.h), split into the three packs in registers once per k-step, the blocks of the next tile requested as those of
// this one are used, the finished accumulators of a tile written out during the next one.  X is read once per column group;
// the groups of one row block are launched `row_blocks` ids apart with row_blocks % 8 == 0, i.e. on the SAME XCD at the
// same time: the second reader is served by that XCD's L2.
// A column group may read a different input matrix (`X2` from group `x2_from` on): q | k = (x + pos) W_qk and v = x W_v of
// an encoder layer are ONE launch over N = 384 (sst_basic_block_v2.py:56-62: q = k = feat + pos, v = feat).
#include <math.h>
#include <stdlib.h>
#include "common.h"
#include "gelu.h"
#include "mfma_tile.h"   // the three-way split8
#include "tile_io.h"

namespace {

struct ln_epi {   // see csrc/dense_f32.hip
  const float* w;
  const float* b;
  float eps;
  float2* stats;
  const float* pos_table;
  const int32_t* pos_idx;
  float* yp;
};

// The bias image leaves LDS where the eight 2 KiB transposition blocks (csrc/tile_io.h) do not fit beside it: <384, 64> has
// 3 x 64 x 384 x 2 = 147 456 B of images, 163 840 - 147 456 = 16 384 B free = exactly 8 x 2 048; its 256 B of bias are then held in
// registers in the row layout (4 floats per 32-column block and lane: 8 VGPRs).
template <int K, int NW, int EPI>
constexpr bool x6_bias_in_regs() {
  return 3 * NW * K * 2 + NW * (EPI == kEpiAddLN ? 3 : 1) * 4 + 8 * 2048 > 160 * 1024;
}
template <int K, int NW, int EPI>
constexpr int x6_lds_bytes() {
  return 3 * NW * K * 2 + (x6_bias_in_regs<K, NW, EPI>() ? 0 : NW * (EPI == kEpiAddLN ? 3 : 1) * 4) + 8 * 2048;
}

// K: contraction width; NW: output columns per workgroup (the whole row when EPI == kEpiAddLN); blockIdx.x = group * row_blocks
// + row block; `X2` replaces X for the column groups >= x2_from (x2_from >= number of groups: never).
// XADD: the column groups < x2_from multiply X + xadd_rows[xadd_idx[row]] (rows of width K) instead of X - q | k = (x + positional
// rows) W_qk and v = x W_v from ONE input tensor: "x + pos" never exists in memory (the table is a few KB and stays in L2)
//
// Global access is ROW-shaped (csrc/tile_io.h): every activation-sized stream - X (+ the positional rows, added on the row side),
// aux_in, the gathered rows, Y, aux_out, ln.yp - is moved with lane l on row l / 8, 16-byte piece l % 8 of a 32-column block, and
// a block changes between that and the MFMA fragment layout in the wave's 2 KiB of LDS.  The element-wise epilogues run on the
// row side (same operations per element, so the same bits; aux_in needs no transposition at all); LayerNorm sums a row in the
// fragment layout as before and only its loads and stores pass through the block.
// Loads are a ROLLING prefetch through a ring of D blocks (8 VGPRs each): as block s goes to LDS its registers take block s + D -
// of this tile, or of the NEXT row tile once s + D passes the end - so a request has D k-steps of products to land in.  D = K / 32,
// a whole tile ahead, for K <= 256; D = 6, half a tile (48 VGPRs, where the fragment-shaped kernel held all 96 without any
// prefetch), for K = 384; D = 2 under the LayerNorm epilogue, which holds a 128-wide residual as well.  The epilogue operands roll
// the same way: emit(tp) consumes block tp of the tile being written out and requests block tp of the tile being multiplied.
// Two places where a request has less cover than that (both on the positional table of the LayerNorm epilogue's second output,
// a few KB that stay in L2): qr is ONE block, requested a quarter tile before its use, and in a wave's last tile, where nothing
// is multiplied any more, block tp + 1 is requested in emit(tp) and waited for in emit(tp + 1).
// After its last tile a wave requests its own first blocks once more, and a wave without rows D blocks of row M - 1 (clamped, in
// range, never used): every load of the loop is issued on every path, because the compiler's vmcnt for a register only counts
// requests that are certain to follow - at most D x 512 B per wave of lines that are in L2 already.
template <int K, int NW, int EPI, bool XADD = false>
__global__ __launch_bounds__(512, 2) void tall_linear_f32x6_k(
    const float* __restrict__ X, const float* __restrict__ X2, int x2_from, int64_t ldx, const float* __restrict__ W,
    int64_t ldw, int trans_w, const float* __restrict__ bias, int64_t M, int row_blocks, int rows_per_wave,
    float* __restrict__ Y, int64_t ldy, const float* __restrict__ aux_in, float* __restrict__ aux_out, int64_t ldaux,
    const ln_epi ln, const float* __restrict__ xadd_rows = nullptr, const int32_t* __restrict__ xadd_idx = nullptr) {
  static_assert(EPI != kEpiAddLN || NW == 128, "the LayerNorm epilogue needs a whole 128-wide row in one accumulator set");
  static_assert(NW == 64 || NW == 128, "column group");
  // LDS images are FRAGMENT-contiguous (round 6): the 16 rows x 32 k of an MFMA A operand are one 1 KiB block in lane order
  // (lane (c, g) at byte 16 (16 g + c)), a fragment read is base + 16 * lane.  ds_read_b128 is served in four groups of 16
  // NON-contiguous lanes ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH.md, LDS): the row-major image with a padded row stride
  // (K * 2 + 16 bytes) of rounds 3-5 put two lanes of every group on the same banks - SQ_LDS_BANK_CONFLICT was 47-51 % of
  // SQ_LDS_IDX_ACTIVE in every instantiation (profiles/r06); lane order covers all 64 banks once per group and needs no padding.
  constexpr int KS = K / 32, NTH = 512, TILES = NW / 16, EMITS = TILES / 2;
  constexpr int IMG = NW * K * 2;   // bytes of one bf16 image
  constexpr bool BIAS_REG = x6_bias_in_regs<K, NW, EPI>();
  constexpr bool HAS_AUX = EPI == kEpiMulGeluGrad || EPI == kEpiMulReluGrad || EPI == kEpiAdd || EPI == kEpiAddLN || EPI == kEpiAddRows;
  static_assert(!(BIAS_REG && EPI == kEpiAddLN), "the LayerNorm epilogue reads its row parameters from LDS");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem6[];
  unsigned char* w0 = smem6;
  unsigned char* w1 = smem6 + IMG;
  unsigned char* w2 = smem6 + 2 * IMG;
  float* bimg = (float*)(smem6 + 3 * IMG);   // absent when BIAS_REG
  auto frag_off = [](int lr, int k8) { return ((lr >> 4) * KS + (k8 >> 5)) * 1024 + (16 * ((k8 >> 3) & 3) + (lr & 15)) * 16; };
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: the row range and every branch on it are uniform
  const int rr = lane >> 3, rcol = (lane & 7) * 4;   // row side: rows rr and rr + 8 of a tile, columns rcol .. rcol + 3 of a block
  const tile_xpose io =
      make_tile_xpose(smem6 + 3 * IMG + (BIAS_REG ? 0 : NW * (EPI == kEpiAddLN ? 3 : 1) * 4) + wv * 2048, lane);
  const int grp = blockIdx.x / row_blocks, rb = blockIdx.x - grp * row_blocks;
  const int nb = grp * NW;   // first output column of this workgroup
  const float* __restrict__ Xg = grp >= x2_from ? X2 : X;
  const int64_t wave = (int64_t)rb * 8 + wv;
  int64_t r0 = wave * rows_per_wave;
  const int64_t r1 = r0 + rows_per_wave < M ? r0 + rows_per_wave : M;
  // row i (0, 1) of this lane in the tile that starts at r, clamped for loads (a tile past the end reads row M - 1)
  auto row_of = [&](int64_t r, int i) {
    const int64_t row = r + 8 * i + rr;
    return row < M ? row : M - 1;
  };
  // row side: a ring of D blocks, block s in slot s % D; D < KS where a whole tile in flight does not fit the registers
  // (K = 384: half a tile = 6 k-steps x 24 MFMAs, the time a whole K = 128 tile takes; LayerNorm: its epilogue holds a 128-wide
  // residual as well)
  constexpr int D = EPI == kEpiAddLN ? 2 : (KS > 8 ? KS / 2 : KS);
  static_assert(!XADD || D == KS, "the positional rows of a tile are requested with one set of indices");
  static_assert(KS % D == 0, "a block keeps its slot from tile to tile");
  f32x4 xr[D][2];
  auto issue_x = [&](int64_t r, int s) {
#pragma unroll
    for (int i = 0; i < 2; ++i) xr[s % D][i] = *(const f32x4*)(Xg + row_of(r, i) * ldx + 32 * s + rcol);
  };
  // XADD: the positional rows of the same blocks in pr; the row indices of a tile are loaded one tile before its rows are
  // requested, so that a table address never waits for its index
  const bool xadd = XADD && grp < x2_from;
  f32x4 pr[XADD ? D : 1][2];
  int32_t pi[2] = {0, 0};   // indices of the tile whose table rows are requested next
  auto load_pidx = [&](int64_t r, int32_t (&dst)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) dst[i] = xadd_idx[row_of(r, i)];
  };
  auto issue_p = [&](int s) {
#pragma unroll
    for (int i = 0; i < 2; ++i) pr[XADD ? s % D : 0][i] = *(const f32x4*)(xadd_rows + (int64_t)pi[i] * K + 32 * s + rcol);
  };
#pragma unroll
  for (int s = 0; s < D; ++s) issue_x(r0, s);
  if (xadd) load_pidx(r0, pi);
  // weight fill: W[nb + n][k] (trans_w = 0: row of W; trans_w = 1: W is [K][N], the data gradient of a layer whose parameter is
  // W) -> three bf16 images, row w_lds_row(n).  8 consecutive k per thread and step.
  if (!trans_w) {
    constexpr int CHUNKS = NW * K / 8;
    for (int idx = threadIdx.x; idx < CHUNKS; idx += NTH) {
      const int n = idx / (K / 8), k8 = (idx - n * (K / 8)) * 8;
      const f32x4 a = *(const f32x4*)(W + (size_t)(nb + n) * ldw + k8);
      const f32x4 b = *(const f32x4*)(W + (size_t)(nb + n) * ldw + k8 + 4);
      u32x4 p0, p1, p2;
      split8(a, b, p0, p1, p2);
      const int off = frag_off(w_lds_row(n), k8);
      *(u32x4*)(w0 + off) = p0;
      *(u32x4*)(w1 + off) = p1;
      *(u32x4*)(w2 + off) = p2;
    }
  } else {
    // W is [K][N] rows: a thread takes an 8 (k) x 4 (n) block - eight 16-byte loads, consecutive threads along n (coalesced
    // rows; the element-wise gather this replaces cost ~6 us of the launch) - and writes four 8-k chunks, one per column
    constexpr int BLOCKS = (NW / 4) * (K / 8);
    for (int idx = threadIdx.x; idx < BLOCKS; idx += NTH) {
      const int k8 = (idx / (NW / 4)) * 8, n4 = (idx % (NW / 4)) * 4;
      f32x4 r[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = *(const f32x4*)(W + (size_t)(k8 + e) * ldw + nb + n4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 a = {r[0][j], r[1][j], r[2][j], r[3][j]}, b = {r[4][j], r[5][j], r[6][j], r[7][j]};
        u32x4 p0, p1, p2;
        split8(a, b, p0, p1, p2);
        const int off = frag_off(w_lds_row(n4 + j), k8);
        *(u32x4*)(w0 + off) = p0;
        *(u32x4*)(w1 + off) = p1;
        *(u32x4*)(w2 + off) = p2;
      }
    }
  }
  f32x4 breg[BIAS_REG ? EMITS : 1];   // BIAS_REG: the bias of this lane's row-side columns
  if (BIAS_REG) {
#pragma unroll
    for (int tp = 0; tp < (BIAS_REG ? EMITS : 1); ++tp)
#pragma unroll
      for (int e = 0; e < 4; ++e) breg[tp][e] = bias != nullptr ? bias[nb + 32 * tp + rcol + e] : 0.f;
  } else {
    for (int n = threadIdx.x; n < NW; n += NTH) {
      bimg[n] = bias != nullptr ? bias[nb + n] : 0.f;
      if (EPI == kEpiAddLN) {
        bimg[NW + n] = ln.w[n];
        bimg[2 * NW + n] = ln.b[n];
      }
    }
  }
  __syncthreads();
  if (r0 >= r1) return;
  if (xadd) {
#pragma unroll
    for (int s = 0; s < D; ++s) issue_p(s);
    load_pidx(r0 + 16, pi);
  }
  const int lane_off = lane * 16;

  // epilogue operands, row side: ar[tp] = block tp of aux_in (kEpiAddRows: of the gathered rows) for the tile that is written
  // out next; qr = the positional rows (ln.yp) of the block that is written out next.  ec / ep: the gather indices
  // (ln.pos_idx) of the tile being multiplied / being written out, each loaded one tile before it is used.
  constexpr bool GATHER = EPI == kEpiAddRows || EPI == kEpiAddLN;
  const bool gather = EPI == kEpiAddRows || (EPI == kEpiAddLN && ln.yp != nullptr);
  f32x4 ar[HAS_AUX ? EMITS : 1][2], qr[2];
  int32_t ec[2] = {0, 0}, ep[2] = {0, 0}, en[2] = {0, 0};
  auto load_eidx = [&](int64_t r, int32_t (&dst)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) dst[i] = ln.pos_idx[row_of(r, i)];
  };
  auto issue_aux = [&](int64_t r, int tp) {   // rows of the tile at r (kEpiAddRows: the rows ec points at)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t src = EPI == kEpiAddRows ? (int64_t)(ec[i] < 0 ? 0 : ec[i]) : row_of(r, i);
      ar[HAS_AUX ? tp : 0][i] = *(const f32x4*)(aux_in + src * ldaux + (EPI == kEpiAddLN ? 0 : nb) + 32 * tp + rcol);
    }
  };
  auto issue_q = [&](const int32_t (&idx)[2], int tp) {
#pragma unroll
    for (int i = 0; i < 2; ++i) qr[i] = *(const f32x4*)(ln.pos_table + (size_t)idx[i] * 128 + 32 * tp + rcol);
  };
  if (GATHER && gather) load_eidx(r0, ec);

  f32x4 pend[TILES];
  int64_t pend_r0 = 0;
  bool pend_valid = false;
  float ln_rstd = 0.f;
  // 32 finished columns (tiles 2 tp, 2 tp + 1) of the previous row tile; see csrc/dense_f32.hip.  in_loop: a tile (at r0) is
  // being multiplied, its operands are requested as those of the finished one are consumed - also while the first tile is
  // multiplied and nothing is written out yet, which is where the first requests come from.  Every load of the main loop is
  // issued on every path: the compiler's vmcnt for a register only counts the requests that are certain to follow its own
  auto request = [&](int tp) {
    if (EPI == kEpiAddLN) {
      if (tp == 0) {
#pragma unroll
        for (int u = 0; u < EMITS; ++u) issue_aux(r0, u);
      }
      if (gather) {
        if (tp + 1 < EMITS)
          issue_q(ep, tp + 1);   // (while the first tile is multiplied: rows nobody reads)
        else
          issue_q(ec, 0);
      }
    } else if (HAS_AUX) {
      issue_aux(r0, tp);
    }
  };
  auto consume = [&](int tp) {
    int64_t prow[2];
    bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      prow[i] = pend_r0 + 8 * i + rr;
      pv[i] = prow[i] < M;
    }
    if (EPI == kEpiAddLN) {
      if (tp == 0) {
        float sum = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int n0 = 32 * u + 8 * g;
          f32x4 s0, s1;
          tile_to_frag(io, ar[HAS_AUX ? u : 0][0], ar[HAS_AUX ? u : 0][1], s0, s1);
          pend[2 * u] += *(const f32x4*)(bimg + n0) + s0;
          pend[2 * u + 1] += *(const f32x4*)(bimg + n0 + 4) + s1;
          if (aux_out != nullptr) {
            f32x4 t[2];
            tile_to_rows(io, pend[2 * u], pend[2 * u + 1], t[0], t[1]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
              if (pv[i]) *(f32x4*)(aux_out + prow[i] * ldaux + 32 * u + rcol) = t[i];
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) sum += pend[2 * u][r] + pend[2 * u + 1][r];
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float mean = sum * (1.f / 128.f);
        float sq = 0.f;
#pragma unroll
        for (int T = 0; T < TILES; ++T)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pend[T][r] -= mean;
            sq = fmaf(pend[T][r], pend[T][r], sq);
          }
        sq += __shfl_xor(sq, 16, 64);
        sq += __shfl_xor(sq, 32, 64);
        ln_rstd = rsqrtf(sq * (1.f / 128.f) + ln.eps);
        if (g == 0 && pend_r0 + c < M) ln.stats[pend_r0 + c] = make_float2(mean, ln_rstd);
      }
      const int n0 = 32 * tp + 8 * g;
      const f32x4 y0 = pend[2 * tp] * ln_rstd * *(const f32x4*)(bimg + NW + n0) + *(const f32x4*)(bimg + 2 * NW + n0);
      const f32x4 y1 =
          pend[2 * tp + 1] * ln_rstd * *(const f32x4*)(bimg + NW + n0 + 4) + *(const f32x4*)(bimg + 2 * NW + n0 + 4);
      f32x4 t[2];
      tile_to_rows(io, y0, y1, t[0], t[1]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (pv[i]) *(f32x4*)(Y + prow[i] * ldy + 32 * tp + rcol) = t[i];
      if (gather) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
          if (pv[i]) *(f32x4*)(ln.yp + prow[i] * 128 + 32 * tp + rcol) = t[i] + qr[i];
      }
      return;
    }
    const int n0 = nb + 32 * tp + rcol;
    const f32x4 bv = BIAS_REG ? breg[BIAS_REG ? tp : 0] : *(const f32x4*)(bimg + 32 * tp + rcol);
    f32x4 t[2];
    tile_to_rows(io, pend[2 * tp], pend[2 * tp + 1], t[0], t[1]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4 v = t[i] + bv;
      if (EPI == kEpiGelu || EPI == kEpiRelu) {
        if (aux_out != nullptr && pv[i]) *(f32x4*)(aux_out + prow[i] * ldaux + n0) = v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = EPI == kEpiGelu ? gelu_f(v[r]) : fmaxf(v[r], 0.f);
      }
      if (EPI == kEpiMulGeluGrad || EPI == kEpiMulReluGrad) {
        const f32x4 p = ar[HAS_AUX ? tp : 0][i];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= EPI == kEpiMulGeluGrad ? gelu_grad_f(p[r]) : (p[r] > 0.f ? 1.f : 0.f);
      }
      if (EPI == kEpiAdd || EPI == kEpiAddRows) v += ar[HAS_AUX ? tp : 0][i];
      if (pv[i]) *(f32x4*)(Y + prow[i] * ldy + n0) = v;
    }
  };
  auto emit = [&](int tp, bool in_loop) {
    if (pend_valid) consume(tp);
    if (in_loop)
      request(tp);
    else if (EPI == kEpiAddLN && gather && tp + 1 < EMITS)
      issue_q(ep, tp + 1);   // the last tile of the wave: nothing is multiplied meanwhile
  };

  for (; r0 < r1; r0 += 16) {
    asm volatile("" ::: "memory");  // W fragments are re-read from LDS per row tile (never hoisted into registers)
    // the tile requested during this one; after the last tile the wave asks for its own rows again (lines it has just read)
    // instead of branching around the requests
    const int64_t rn = r0 + 16 < r1 ? r0 + 16 : r0;
    // the indices of the tiles after this one (rows past the end read row M - 1's); pi: those of the tile at r0 + 16
    int32_t pj[2] = {0, 0};
    if (xadd) load_pidx(r0 + 32, pj);
    if (GATHER && gather) load_eidx(r0 + 16, en);
    f32x4 acc[TILES];
#pragma unroll
    for (int T = 0; T < TILES; ++T) acc[T] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // (k-step s, group of 4 column tiles): six products per tile, smallest first (x2 w0, x0 w2, x1 w1 ~ 2^-16; x1 w0, x0 w1 ~
    // 2^-8; x0 w0), issued product by product over the four tiles so that a dependent MFMA is four instructions behind its
    // predecessor; one emit (32 columns of the previous row tile) after every 1 / EMITS of the groups
    constexpr int QPS = TILES / 4;   // groups per k-step
    constexpr int G = KS * QPS;
    u32x4 x0, x1, x2;
#pragma clang loop unroll(full)
    for (int q = 0; q < G; ++q) {
      const int s = q / QPS, t0 = (q % QPS) * 4;
      if (q % QPS == 0) {
        // block s of this tile: row side (+ its positional rows: the same single fp32 addition) -> fragments -> three packs;
        // its registers then take block s of the next tile
        f32x4 a = xr[s % D][0], b = xr[s % D][1];
        if (XADD && xadd) {
          a += pr[XADD ? s % D : 0][0];
          b += pr[XADD ? s % D : 0][1];
        }
        f32x4 v0, v1;
        tile_to_frag(io, a, b, v0, v1);
        split8(v0, v1, x0, x1, x2);
        if (s + D < KS) {
          issue_x(r0, s + D);
        } else {
          issue_x(rn, s + D - KS);
          if (XADD && xadd) issue_p(s + D - KS);
        }
        // the requests stay here, ahead of this k-step's products (nothing but VALU / SALU / LDS work may cross): sunk towards
        // their use they would have no products to land in
        __builtin_amdgcn_sched_barrier(0x786);
      }
      u32x4 a0[4], a1[4], a2[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int off = lane_off + ((t0 + u) * KS + s) * 1024;
        a0[u] = *(const u32x4*)(w0 + off);
        a1[u] = *(const u32x4*)(w1 + off);
        a2[u] = *(const u32x4*)(w2 + off);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t0 + u] = mma32(a0[u], x2, acc[t0 + u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t0 + u] = mma32(a2[u], x0, acc[t0 + u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t0 + u] = mma32(a1[u], x1, acc[t0 + u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t0 + u] = mma32(a0[u], x1, acc[t0 + u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t0 + u] = mma32(a1[u], x0, acc[t0 + u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t0 + u] = mma32(a0[u], x0, acc[t0 + u]);
      if ((q + 1) % (G / EMITS) == 0) emit((q + 1) / (G / EMITS) - 1, true);
    }
#pragma unroll
    for (int T = 0; T < TILES; ++T) pend[T] = acc[T];
    pend_r0 = r0;
    pend_valid = true;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      pi[i] = pj[i];
      ep[i] = ec[i];
      ec[i] = en[i];
    }
  }
#pragma unroll
  for (int tp = 0; tp < EMITS; ++tp) emit(tp, false);
}

// one 8-wave workgroup per CU: row blocks x column groups <= 256 workgroups, row blocks a multiple of 8 so that the groups of
// one row block (ids row_blocks apart) share an XCD and its L2; a wave walks rpw rows (a multiple of 16) in 16-row tiles
void x6_partition(int64_t m, int groups, int64_t& row_blocks, int64_t& rpw) {
  row_blocks = (256 / groups) & ~7;
  rpw = sst_align_up(sst_div_up(m, row_blocks * 8), 16);
  row_blocks = sst_align_up(sst_div_up(m, rpw * 8), 8);
}

template <int K, int NW, int EPI, bool XADD = false>
int launch_x6(const float* x, const float* x2, int x2_from, int64_t ldx, const float* w, int64_t ldw, int trans_w,
              const float* bias, int64_t m, int n, float* y, int64_t ldy, const float* aux_in, float* aux_out, int64_t ldaux,
              hipStream_t st, const ln_epi ln = ln_epi(), const float* xadd_rows = nullptr, const int32_t* xadd_idx = nullptr) {
  // three weight images of a column group, the bias image (where it fits: x6_bias_in_regs) and one 2 KiB block per wave
  constexpr int lds = x6_lds_bytes<K, NW, EPI>();
  static_assert(lds <= 160 * 1024, "three weight images of a column group and the waves' blocks must fit the CU's LDS");
  static unsigned long long configured = 0;
  if (sst_first_use_on_device(&configured)) {
    SST_HIP(hipFuncSetAttribute((const void*)tall_linear_f32x6_k<K, NW, EPI, XADD>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    sst_mark_device(&configured);
  }
  const int groups = n / NW;
  int64_t row_blocks, rpw;
  x6_partition(m, groups, row_blocks, rpw);
  if (x2 == nullptr) x2_from = groups;
  hipLaunchKernelGGL((tall_linear_f32x6_k<K, NW, EPI, XADD>), dim3((unsigned)(row_blocks * groups)), dim3(512), lds, st, x, x2,
                     x2_from, ldx, w, ldw, trans_w, bias, m, (int)row_blocks, (int)rpw, y, ldy, aux_in, aux_out, ldaux, ln, xadd_rows,
                     xadd_idx);
  return SST_OK;
}

template <int K, int NW>
int dispatch_x6(int epi, const float* x, const float* x2, int x2_from, int64_t ldx, const float* w, int64_t ldw, int trans_w,
                const float* bias, int64_t m, int n, float* y, int64_t ldy, const float* aux_in, float* aux_out, int64_t ldaux,
                hipStream_t st) {
#define SST_CASE(E) \
  case E: return launch_x6<K, NW, E>(x, x2, x2_from, ldx, w, ldw, trans_w, bias, m, n, y, ldy, aux_in, aux_out, ldaux, st)
  switch (epi) {
    SST_CASE(kEpiBias);
    SST_CASE(kEpiGelu);
    SST_CASE(kEpiRelu);
    SST_CASE(kEpiMulGeluGrad);
    SST_CASE(kEpiMulReluGrad);
    SST_CASE(kEpiAdd);
  }
#undef SST_CASE
  return SST_ERR_ARG;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int sst_tall_linear_epi2_f32x6(const float* d_x, const float* d_x2, int x2_from_col, int64_t ldx, const float* d_w, int64_t ldw,
                               int trans_w, const float* d_bias, int64_t m, int k, int n, int epilogue, const float* d_aux_in,
                               float* d_aux_out, int64_t ldaux, float* d_y, int64_t ldy, void* stream) {
  if (m < 0 || !d_w || epilogue < 0 || epilogue > kEpiAdd) return SST_ERR_ARG;
  if (m == 0) return SST_OK;
  if (!d_x || !d_y || (ldx & 3) || (ldy & 3) || (ldw & 3) || !aligned16(d_x) || !aligned16(d_y) || !aligned16(d_w))
    return SST_ERR_ARG;
  if (d_x2 && (!aligned16(d_x2) || x2_from_col < 0 || x2_from_col > n)) return SST_ERR_ARG;
  if (epilogue >= kEpiMulGeluGrad && (!d_aux_in || (ldaux & 3) || !aligned16(d_aux_in))) return SST_ERR_ARG;
  if (d_aux_out && ((ldaux & 3) || !aligned16(d_aux_out))) return SST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (k == 128 && (n == 128 || n == 256 || n == 384)) {
    if (d_x2 && (x2_from_col % 128)) return SST_ERR_ARG;
    rc = dispatch_x6<128, 128>(epilogue, d_x, d_x2, x2_from_col / 128, ldx, d_w, ldw, trans_w, d_bias, m, n, d_y, ldy, d_aux_in,
                               d_aux_out, ldaux, st);
  } else if (k == 64 && n == 128 && !d_x2) {      // the voxel encoder's second layer in its split-weight form
    rc = dispatch_x6<64, 128>(epilogue, d_x, nullptr, 0, ldx, d_w, ldw, trans_w, d_bias, m, n, d_y, ldy, d_aux_in, d_aux_out, ldaux,
                              st);
  } else if (k == 64 && n == 64 && !d_x2) {       // ... with 64 output channels (FSD's DynamicScatterVFE, feat_channels [64, 64])
    rc = dispatch_x6<64, 64>(epilogue, d_x, nullptr, 0, ldx, d_w, ldw, trans_w, d_bias, m, n, d_y, ldy, d_aux_in, d_aux_out, ldaux,
                             st);
  } else if (k == 128 && n == 64 && !d_x2) {      // ... and its data gradient
    rc = dispatch_x6<128, 64>(epilogue, d_x, nullptr, 0, ldx, d_w, ldw, trans_w, d_bias, m, n, d_y, ldy, d_aux_in, d_aux_out, ldaux,
                              st);
  } else if (k == 256 && n == 128) {
    if (d_x2 && (x2_from_col % 64)) return SST_ERR_ARG;
    rc = dispatch_x6<256, 64>(epilogue, d_x, d_x2, x2_from_col / 64, ldx, d_w, ldw, trans_w, d_bias, m, n, d_y, ldy, d_aux_in,
                              d_aux_out, ldaux, st);
  } else if (k == 384 && n == 128) {
    // d(x) of the whole in-projection as ONE product: [dq | dk | dv] (M x 384) times in_proj_weight (384 x 128), the residual
    // branch's gradient in the epilogue (three images of a 64-column group, 144 KB, + the waves' blocks: all 160 KB of LDS)
    if (d_x2 && (x2_from_col % 64)) return SST_ERR_ARG;
    rc = dispatch_x6<384, 64>(epilogue, d_x, d_x2, x2_from_col / 64, ldx, d_w, ldw, trans_w, d_bias, m, n, d_y, ldy, d_aux_in,
                              d_aux_out, ldaux, st);
  } else {
    return SST_ERR_UNSUPPORTED;
  }
  if (rc) return rc;
  SST_LAUNCH_CHECK();
  return SST_OK;
}

/* The in-projection of an SRA encoder layer from x alone (sst_basic_block_v2.py:56-62: q = k = feat + pos, v = feat):
 * y[m, 384] = [(x + rows[index]) W[:256]^T | x W[256:]^T] + bias, rows = the positional table [P][128] (fp32), index int32 [m].
 * One launch, x read once per column group, "x + pos" never materialised. */
int sst_inproj_pos_f32x6(const float* d_x, int64_t ldx, const float* d_rows, const int32_t* d_index, const float* d_w, int64_t ldw,
                         const float* d_bias, int64_t m, float* d_y, int64_t ldy, void* stream) {
  if (m < 0 || !d_w) return SST_ERR_ARG;
  if (m == 0) return SST_OK;
  if (!d_x || !d_y || !d_rows || !d_index || (ldx & 3) || (ldy & 3) || (ldw & 3) || !aligned16(d_x) || !aligned16(d_y) ||
      !aligned16(d_w) || !aligned16(d_rows))
    return SST_ERR_ARG;
  const int rc = launch_x6<128, 128, kEpiBias, true>(d_x, d_x, 2, ldx, d_w, ldw, 0, d_bias, m, 384, d_y, ldy, nullptr, nullptr, 0,
                                                     (hipStream_t)stream, ln_epi(), d_rows, d_index);
  if (rc) return rc;
  SST_LAUNCH_CHECK();
  return SST_OK;
}

/* How a launch of the kernels above cuts m rows over `groups` column groups (1, 2 or 3): the row blocks per group and the rows
 * a wave walks.  Host arithmetic only (no launch): the tests take their boundary token counts from it. */
int sst_tall_linear_f32x6_partition(int64_t m, int groups, int64_t* row_blocks, int64_t* rows_per_wave) {
  if (m <= 0 || groups < 1 || groups > 3 || !row_blocks || !rows_per_wave) return SST_ERR_ARG;
  x6_partition(m, groups, *row_blocks, *rows_per_wave);
  return SST_OK;
}

int sst_tall_linear_epi_f32x6(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, int trans_w, const float* d_bias,
                              int64_t m, int k, int n, int epilogue, const float* d_aux_in, float* d_aux_out, int64_t ldaux,
                              float* d_y, int64_t ldy, void* stream) {
  return sst_tall_linear_epi2_f32x6(d_x, nullptr, 0, ldx, d_w, ldw, trans_w, d_bias, m, k, n, epilogue, d_aux_in, d_aux_out, ldaux,
                                    d_y, ldy, stream);
}

/* y = x W^T + rows[row_index[r]] (negative index: row 0), (K, N) = (64, 128): DynamicVFE's second layer on
 * [point feature | pooled feature of the point's voxel] (voxel_encoder.py:286-294: cat + Linear(128 -> 128 or 64)) as
 * point_feats W[:, :64]^T + (pooled W[:, 64:]^T)[voxel of the point] - the concatenated matrix is never formed and the pooled half
 * is multiplied once per voxel instead of once per point. */
int sst_tall_linear_add_rows_f32x6(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, int64_t m, int k, int n,
                                   const float* d_rows, int64_t ldrows, const int32_t* d_row_index, float* d_y, int64_t ldy,
                                   void* stream) {
  if (m < 0 || !d_w) return SST_ERR_ARG;
  if (k != 64 || (n != 128 && n != 64)) return SST_ERR_UNSUPPORTED;
  if (m == 0) return SST_OK;
  if (!d_x || !d_y || !d_rows || !d_row_index || (ldx & 3) || (ldy & 3) || (ldw & 3) || (ldrows & 3) || !aligned16(d_x) ||
      !aligned16(d_y) || !aligned16(d_w) || !aligned16(d_rows))
    return SST_ERR_ARG;
  ln_epi ln = ln_epi();
  ln.pos_idx = d_row_index;
  const int rc = n == 128 ? launch_x6<64, 128, kEpiAddRows>(d_x, nullptr, 0, ldx, d_w, ldw, 0, nullptr, m, 128, d_y, ldy, d_rows,
                                                            nullptr, ldrows, (hipStream_t)stream, ln)
                          : launch_x6<64, 64, kEpiAddRows>(d_x, nullptr, 0, ldx, d_w, ldw, 0, nullptr, m, 64, d_y, ldy, d_rows,
                                                           nullptr, ldrows, (hipStream_t)stream, ln);
  if (rc) return rc;
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int sst_tall_linear_ln_f32x6(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, const float* d_bias, int64_t m, int k,
                             const float* d_res, int64_t ldres, const float* d_ln_weight, const float* d_ln_bias, float eps,
                             float* d_y, float* d_sum, float* d_stats, const float* d_pos_table, const int32_t* d_pos_idx,
                             float* d_y_plus_pos, void* stream) {
  if (m < 0 || !d_w || !d_ln_weight || !d_ln_bias || !d_stats) return SST_ERR_ARG;
  if (k != 128) return SST_ERR_UNSUPPORTED;   // K = 256: three images of a 128-column group do not fit (203 KB); see the file head
  if (m == 0) return SST_OK;
  if (!d_x || !d_y || !d_res || (ldx & 3) || (ldw & 3) || (ldres & 3) || !aligned16(d_x) || !aligned16(d_y) ||
      !aligned16(d_w) || !aligned16(d_res) || (d_sum && !aligned16(d_sum)))
    return SST_ERR_ARG;
  if ((d_pos_table != nullptr) != (d_pos_idx != nullptr) || (d_pos_table != nullptr) != (d_y_plus_pos != nullptr))
    return SST_ERR_ARG;
  ln_epi ln;
  ln.w = d_ln_weight;
  ln.b = d_ln_bias;
  ln.eps = eps;
  ln.stats = (float2*)d_stats;
  ln.pos_table = d_pos_table;
  ln.pos_idx = d_pos_idx;
  ln.yp = d_y_plus_pos;
  const int rc = launch_x6<128, 128, kEpiAddLN>(d_x, nullptr, 0, ldx, d_w, ldw, 0, d_bias, m, 128, d_y, 128, d_res, d_sum, ldres,
                                                (hipStream_t)stream, ln);
  if (rc) return rc;
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

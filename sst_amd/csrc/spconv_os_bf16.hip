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
// Contraction = csrc/spconv_os_x6.hip minus the split: 64-row workgroups, a wave owns 16 rows x all columns of the group, W[k]
// packed once per call into fragment order - ONE bf16 image, 2 bytes per element - and staged through LDS double-buffered,
// partner rows gathered as fp32 straight into registers and converted there, heaviest-first launch order, XCD round-robin, the
// offsets of a thin level dealt out over workgroups with a fixed-order reduce kernel.
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
#include <stdlib.h>

#include "common.h"
#include "mfma_tile.h"   // pack2, mma32

namespace {

constexpr int kBfMaxK = 32;    // kernel offsets the index image holds
constexpr int kBfChunk = 64;   // input channels per stage
constexpr int kBfXcdChunk = 4;

// Packed weights: slab (k, column group cg, channel chunk cc) = [2 ks][NCT ct][64 lanes][4 words of 2 bf16], with
//   the 8 values of lane (l15, g) = bf16(W[k][c = 64 cc + 32 ks + 8 g + 0..7][n = 16 NCT cg + 16 ct + l15])   (0 outside cin x cout):
// the A operand (16 columns x 32 channels) of v_mfma_f32_16x16x32_bf16, one ds_read_b128 per lane.
// trans_w: W[k] is stored [n][c] (the data gradient reads the forward weights with the roles swapped).
__global__ __launch_bounds__(256) void sp_bf16_pack_w_k(const float* __restrict__ w, int kvol, int cin, int cout, int trans_w,
                                                        int nct, int n_cg, int n_cc, unsigned* __restrict__ wp) {
  const int64_t total = (int64_t)kvol * n_cg * n_cc * 2 * nct * 64;   // one thread = one lane's 8 values
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(e & 63);
    int64_t rest = e >> 6;
    const int ct = (int)(rest % nct);
    rest /= nct;
    const int ks = (int)(rest & 1);
    int64_t slab = rest >> 1;
    const int cc = (int)(slab % n_cc);
    slab /= n_cc;
    const int cg = (int)(slab % n_cg);
    const int k = (int)(slab / n_cg);
    const int n = cg * 16 * nct + 16 * ct + (lane & 15);
    const int c0 = cc * kBfChunk + 32 * ks + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int c = c0 + t;
      v[t] = 0.f;
      if (c < cin && n < cout) v[t] = trans_w ? w[((int64_t)k * cout + n) * cin + c] : w[((int64_t)k * cin + c) * cout + n];
    }
    // slab base in words: ((k, cg, cc) * 2 * nct * 64 * 4); inside: [ks][ct][lane][4] - e itself, in 16-byte pieces
    *(u32x4*)(wp + e * 4) = (u32x4){pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
  }
}

template <int NCT>
__global__ __launch_bounds__(256, NCT == 4 ? 4 : 3) void sp_conv_os_bf16_k(
    const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ map, int64_t m, int kvol,
    const unsigned* __restrict__ wp, int cin, int cout, const float* __restrict__ bias, float* __restrict__ y, int64_t ldy,
    int n_units, int n_cg, int n_cc, int xcd_chunk, int vec_store, const int32_t* __restrict__ tile_order, int n_split,
    float* __restrict__ partial) {
  constexpr int ROWS = 64;
  constexpr int SLAB = 64 * 4 * 2 * NCT;   // 32-bit words of one packed W slab
  constexpr int WREG = SLAB / 4 / 256;     // 16-byte pieces of a slab per thread
  extern __shared__ __attribute__((aligned(16))) unsigned bf_smem[];
  unsigned (*wbuf)[SLAB] = (unsigned (*)[SLAB])bf_smem;                    // [2][SLAB]
  int (*idx)[ROWS] = (int (*)[ROWS])(bf_smem + 2 * SLAB);                  // [kvol][ROWS]
  unsigned* live_w = (unsigned*)(bf_smem + 2 * SLAB + kvol * ROWS);        // [4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int unit_s = ((slot / xcd_chunk) * 8 + xcd) * xcd_chunk + slot % xcd_chunk;
  if (unit_s >= n_units * n_split) return;  // uniform
  // THIN levels: the offsets are dealt out over n_split workgroups per unit (offset k belongs to workgroup k % n_split), which
  // write partial tiles that sp_bf16_split_reduce_k adds in a fixed order.  n_split = 1: the plain kernel.
  const int unit = unit_s / n_split, split = unit_s - unit * n_split;
  const int pos = unit / n_cg, cg = unit - pos * n_cg;
  const int tile = tile_order ? tile_order[pos] : pos;
  const int64_t r0 = (int64_t)tile * ROWS;
  // ---- partner rows of the tile for every offset -> LDS; which offsets are populated, per wave ----
  if (tid < 4) live_w[tid] = 0u;
  __syncthreads();
  {
    constexpr int NIT = (kBfMaxK * ROWS + 255) / 256;
    int vals[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = it * 256 + tid;
      const int k = e / ROWS, row = e - k * ROWS;
      vals[it] = (k < kvol && r0 + row < m) ? map[(int64_t)k * m + r0 + row] : -1;
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = it * 256 + tid;
      const int k = e / ROWS, row = e - k * ROWS;   // a wave holds the 64 rows of ONE offset
      const int v = vals[it];
      if (k < kvol) idx[k][row] = v;
      const unsigned long long b = __ballot(v >= 0);
      if (lane < 4 && k < kvol && ((b >> (16 * (lane & 3))) & 0xffffull)) atomicOr(&live_w[lane & 3], 1u << k);
    }
  }
  __syncthreads();
  unsigned mine = 0xffffffffu;
  if (n_split > 1) {
    mine = 0u;
    for (int k = split; k < 32; k += n_split) mine |= 1u << k;
  }
  const unsigned wave_live = live_w[wave] & mine;
  const unsigned live = (live_w[0] | live_w[1] | live_w[2] | live_w[3]) & mine;
  const int wave_row = wave * 16;

  f32x4 acc[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (live != 0u) {
    const int c_last = cin - 4;  // cin % 4 == 0 (host check)
    f32x4 xn[4];                 // requested stage: channels 32 ks + 8 kq + 4 h + 0..3 at xn[2 ks + h]
    u32x4 xb[2], wr[WREG];       // the current stage's rows as bf16 operands | the requested W slab
    int sn;
    auto fetch_w = [&](int k, int cc) {
      const u32x4* src = (const u32x4*)(wp + ((int64_t)(k * n_cg + cg) * n_cc + cc) * SLAB);
#pragma unroll
      for (int u = 0; u < WREG; ++u) wr[u] = src[tid + 256 * u];
    };
    auto gather_x = [&](int k, int cc) {
      sn = idx[k][wave_row + l15];
      const float* p = x + (int64_t)(sn >= 0 ? sn : 0) * ldx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int c = cc * kBfChunk + 32 * (j >> 1) + 8 * kq + 4 * (j & 1);
        c = c < c_last ? c : c_last;  // beyond cin the packed weights are zero: any finite value will do
        xn[j] = *(const f32x4*)(p + c);
      }
    };
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto commit = [&](int buf) {   // requested W -> LDS buffer, requested X -> bf16 operands of the current stage
#pragma unroll
      for (int u = 0; u < WREG; ++u) *(u32x4*)(&wbuf[buf][4 * (tid + 256 * u)]) = wr[u];
      const bool has = sn >= 0;     // rows without a partner contribute 0
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const f32x4 a = has ? xn[2 * ks] : zero4, b = has ? xn[2 * ks + 1] : zero4;
        xb[ks] = (u32x4){pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3])};
      }
    };
    auto next_live = [&](int k) {
      const unsigned rest = k < 32 ? (live >> k) : 0u;
      return rest ? k + __builtin_ctz(rest) : 32;
    };
    int k = next_live(0), cc = 0, buf = 0;
    fetch_w(k, 0);
    gather_x(k, 0);
    commit(0);
    __syncthreads();
    while (true) {
      int nk = k, ncc = cc + 1;
      if (ncc == n_cc) {
        ncc = 0;
        nk = next_live(k + 1);
      }
      const bool has_next = nk < 32;
      if (!has_next) {  // keep the loads unconditional: the last stage requests itself once more
        nk = k;
        ncc = cc;
      }
      fetch_w(nk, ncc);
      gather_x(nk, ncc);
      if ((wave_live >> k) & 1u) {  // uniform per wave
        const unsigned* wb = &wbuf[buf][4 * lane];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct)
            acc[ct] = mma32(*(const u32x4*)(wb + (ks * NCT + ct) * 256), xb[ks], acc[ct]);
        }
      }
      commit(buf ^ 1);
      __syncthreads();
      if (!has_next) break;
      k = nk;
      cc = ncc;
      buf ^= 1;
    }
  }
  // ---- epilogue: lane = (row l15 of the wave's block, 4 consecutive columns at 4 kq of every column tile) ----
  const int64_t row = r0 + wave_row + l15;
  if (row >= m) return;
  if (n_split > 1) {   // partial tile of this workgroup's offsets: [split][row][cout padded to 4], no bias
    const int64_t cpad = (int64_t)((cout + 3) & ~3);
    float* dst = partial + ((int64_t)split * m + row) * cpad;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int n = cg * 16 * NCT + 16 * ct + 4 * kq;
      if (n < cout) *(f32x4*)(dst + n) = acc[ct];
    }
    return;
  }
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int n = cg * 16 * NCT + 16 * ct + 4 * kq;
    if (n >= cout) continue;
    f32x4 v = acc[ct];
    if (vec_store && n + 3 < cout) {
      if (bias) v += *(const f32x4*)(bias + n);
      *(f32x4*)(y + row * ldy + n) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < cout) y[row * ldy + n + e] = v[e] + (bias ? bias[n + e] : 0.f);
    }
  }
}

// y[row][n] = bias[n] + sum over the splits, in split order (deterministic)
__global__ __launch_bounds__(256) void sp_bf16_split_reduce_k(const float* __restrict__ partial, int64_t m, int cout, int n_split,
                                                              const float* __restrict__ bias, float* __restrict__ y, int64_t ldy) {
  const int64_t cpad = (int64_t)((cout + 3) & ~3), c4 = cpad >> 2;
  const int64_t total = m * c4;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = e / c4;
    const int n = (int)(e - row * c4) * 4;
    f32x4 v = *(const f32x4*)(partial + row * cpad + n);
    for (int sp = 1; sp < n_split; ++sp) v += *(const f32x4*)(partial + ((int64_t)sp * m + row) * cpad + n);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (n + t < cout) y[row * ldy + n + t] = v[t] + (bias ? bias[n + t] : 0.f);
  }
}

// tile shape and offset split of a call
struct bf_cfg {
  int nct, n_cg, n_cc, n_split;
  int64_t n_tiles, pack_words;
};
bf_cfg bf_pick(int64_t m, int kvol, int cin, int cout) {
  bf_cfg c;
  c.n_tiles = sst_div_up(m, 64);
  c.nct = cout <= 64 ? 4 : 8;
  if (c.nct == 8 && c.n_tiles * sst_div_up(cout, 128) < 2048) c.nct = 4;   // as sp_conv_os_k's os_pick
  c.n_cg = (int)sst_div_up(cout, 16 * c.nct);
  c.n_cc = (int)sst_div_up(cin, kBfChunk);
  c.pack_words = (int64_t)kvol * c.n_cg * c.n_cc * (64 * 4 * 2 * c.nct);
  // offsets dealt out over workgroups while the launch has fewer than ~3 workgroups per CU and an offset's worth of work is
  // left to each (SST_SPCONV_BF16_SPLIT overrides: 1 = never)
  static int env = -1;
  if (env < 0) {
    const char* e = getenv("SST_SPCONV_BF16_SPLIT");
    env = e ? atoi(e) : 0;
  }
  const int64_t units = c.n_tiles * c.n_cg;
  int s = 1;
  while (s < 8 && units * s * 2 <= 1024 && kvol >= 2 * s * 2) s *= 2;
  if (env >= 1 && env <= 16) s = env < kvol ? env : kvol;
  c.n_split = s;
  return c;
}

// the packed weights of a call, whichever column class it takes (worst case), in bytes, rounded up to 256
int64_t bf_pack_bytes(int kvol, int cin, int cout) {
  const int64_t slabs4 = (int64_t)kvol * sst_div_up(cout, 64) * sst_div_up(cin, kBfChunk) * (64 * 4 * 2 * 4);
  const int64_t slabs8 = (int64_t)kvol * sst_div_up(cout, 128) * sst_div_up(cin, kBfChunk) * (64 * 4 * 2 * 8);
  return sst_align_up((slabs4 > slabs8 ? slabs4 : slabs8) * 4, 256);
}

// what a call on a workspace of workspace_bytes launches: the split halved until its partial tiles fit behind the packed
// weights, the workgroups numbered in XCD runs of kBfXcdChunk from 64 runs on, the grid padded to whole rounds of runs
struct bf_launch {
  bf_cfg c;
  int64_t pack_bytes, wgs, grid;
  int chunk;
};
bf_launch bf_plan(int64_t m, int kvol, int cin, int cout, int64_t workspace_bytes) {
  bf_launch p;
  p.c = bf_pick(m, kvol, cin, cout);
  p.pack_bytes = bf_pack_bytes(kvol, cin, cout);
  const int64_t cpad = (cout + 3) & ~3;
  while (p.c.n_split > 1 && p.pack_bytes + (int64_t)p.c.n_split * m * cpad * 4 > workspace_bytes) p.c.n_split >>= 1;
  p.wgs = p.c.n_tiles * p.c.n_cg * p.c.n_split;
  p.chunk = p.wgs >= 64 * (int64_t)kBfXcdChunk ? kBfXcdChunk : 1;
  p.grid = sst_div_up(p.wgs, 8 * p.chunk) * 8 * p.chunk;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------
// The filter gradient.  Decomposition of sp_wgrad_os_k / sp_wgrad_os_x6_k (csrc/spconv_os.hip): grid = (chunk slots, 64 x 64
// blocks of dW[k]), a workgroup walks its chunk of one offset's pairs in stages of 64, wave = 32 x 32 quadrant, rows global ->
// registers -> LDS transposed, indices two stages ahead; partials [chunk slot][cin][cout] summed by sp_wgrad_os_reduce_k.
// LDS image per operand: [64 channels][64 pairs] bf16 in 128-byte rows, written as 8-byte groups of 4 consecutive pairs, read as
// the 16-byte fragments the instruction wants (lane (l15, g): pairs 32 ks + 8 g .. + 7 of channel row l15); 16-byte unit G of
// row r sits at G ^ f(r), f(r) = ((r >> 1) & 7) ^ ((r >> 3) & 7) (the swizzle of the x6 kernel: conflict-free fragment reads).
constexpr int kBfWgStage = 64;   // pairs per stage (kWgStage of csrc/spconv_os.hip)

__device__ __forceinline__ int wbf_unit(int row, int G) { return (G ^ ((row >> 1) & 7) ^ ((row >> 3) & 7)) & 7; }

// chunk slot -> (offset, first slot of that offset): os_find_chunk of csrc/spconv_os.hip (the slot numbering both share)
__device__ __forceinline__ bool bf_find_chunk(const int32_t* __restrict__ num, int kvol, int chunk, int csize, int& k, int& first) {
  int c0 = 0;
  for (int i = 0; i < kvol; ++i) {
    const int nc = (num[i] + csize - 1) / csize;
    if (chunk < c0 + nc) {
      k = i;
      first = c0;
      return true;
    }
    c0 += nc;
  }
  return false;
}

__global__ __launch_bounds__(256) void sp_wgrad_os_bf16_k(const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ dy, int64_t lddy,
                                                          const int32_t* __restrict__ pairs, int64_t pair_ld, int x_side,
                                                          const int32_t* __restrict__ num, int kvol, int cin, int cout,
                                                          int n_bj, int csize, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) unsigned char img[2][2][64 * 128];   // [buffer][X | dY]
  int k, first;
  if (!bf_find_chunk(num, kvol, blockIdx.x, csize, k, first)) return;  // uniform
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
      const int off = row * 128 + wbf_unit(row, pq >> 1) * 16 + (pq & 1) * 8;
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
  load_idx(p0 + kBfWgStage);
  store_rows(0);
  __syncthreads();
  int buf = 0;
  for (int p = p0; p < p1; p += kBfWgStage) {
    load_rows(p + kBfWgStage);        // rows of the next stage (their indices were requested a stage ago)
    load_idx(p + 2 * kBfWgStage);     // indices of the stage after it
    __builtin_amdgcn_sched_barrier(0);   // the loads are issued HERE, in front of the products that hide their latency
#pragma unroll
    for (int ks = 0; ks < kBfWgStage / 32; ++ks) {
      u32x4 af[2], bf[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ra_ = wi + 16 * h + l15, rb_ = wj + 16 * h + l15;
        af[h] = *(const u32x4*)(img[buf][0] + ra_ * 128 + wbf_unit(ra_, 4 * ks + g) * 16);
        bf[h] = *(const u32x4*)(img[buf][1] + rb_ * 128 + wbf_unit(rb_, 4 * ks + g) * 16);
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
  const bf_cfg c = bf_pick(m > 0 ? m : 1, kvol, cin, cout);
  const int64_t part = c.n_split > 1 ? (int64_t)c.n_split * m * ((cout + 3) & ~3) * 4 : 0;
  return bf_pack_bytes(kvol, cin, cout) + part;
}

int sst_spconv_conv_os_rows_bf16(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                                 int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                                 const int32_t* d_tile_order, void* d_workspace, int64_t workspace_bytes, void* stream) {
  if (m < 0 || kvol < 1 || cin < 1 || cout < 1 || ldx < cin || ldy < cout || tile_cfg != 0) return SST_ERR_ARG;
  if (m == 0) return SST_OK;
  if (!d_x || !d_map || !d_w || !d_y || !d_workspace) return SST_ERR_ARG;
  if (kvol > kBfMaxK || (cin & 3) || (ldx & 3) || (((uintptr_t)d_x) & 15) || (((uintptr_t)d_workspace) & 255) ||
      m > 0x3fffffff)
    return SST_ERR_UNSUPPORTED;
  const bf_launch p = bf_plan(m, kvol, cin, cout, workspace_bytes);
  const bf_cfg& c = p.c;
  if (workspace_bytes < p.pack_bytes) return SST_ERR_ARG;   // the packed weights at least (p.pack_bytes >= 4 c.pack_words)
  const int64_t cpad = (cout + 3) & ~3;
  const int nct = c.nct, n_cg = c.n_cg, n_cc = c.n_cc;
  const int64_t n_units = c.n_tiles * n_cg;
  if (n_units * c.n_split > 0x3fffffff) return SST_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  unsigned* wp = (unsigned*)d_workspace;
  float* partial = c.n_split > 1 ? (float*)((char*)d_workspace + p.pack_bytes) : nullptr;
  const int64_t lanes = (int64_t)kvol * n_cg * n_cc * 2 * nct * 64;
  hipLaunchKernelGGL(sp_bf16_pack_w_k, dim3(sst_grid_1d(lanes, 256)), dim3(256), 0, st, d_w, kvol, cin, cout, trans_w, nct, n_cg,
                     n_cc, wp);
  const dim3 grid((unsigned)p.grid);
  const int vec_store = ((ldy & 3) == 0 && (((uintptr_t)d_y) & 15) == 0 && (!d_bias || (((uintptr_t)d_bias) & 15) == 0)) ? 1 : 0;
  const int lds = (2 * 64 * 4 * 2 * nct + kvol * 64 + 4) * (int)sizeof(unsigned);   // <= 40 976 bytes: no attribute needed
  if (nct == 4)
    hipLaunchKernelGGL(sp_conv_os_bf16_k<4>, grid, dim3(256), lds, st, d_x, ldx, d_map, m, kvol, wp, cin, cout, d_bias, d_y, ldy,
                       (int)n_units, n_cg, n_cc, p.chunk, vec_store, d_tile_order, c.n_split, partial);
  else
    hipLaunchKernelGGL(sp_conv_os_bf16_k<8>, grid, dim3(256), lds, st, d_x, ldx, d_map, m, kvol, wp, cin, cout, d_bias, d_y, ldy,
                       (int)n_units, n_cg, n_cc, p.chunk, vec_store, d_tile_order, c.n_split, partial);
  if (c.n_split > 1)
    hipLaunchKernelGGL(sp_bf16_split_reduce_k, dim3(sst_grid_1d(m * (cpad >> 2), 256)), dim3(256), 0, st, partial, m, cout,
                       c.n_split, d_bias, d_y, ldy);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

// the launch plan of sst_spconv_conv_os_rows_bf16 on workspace_bytes; asked by sst_spconv_conv_os_plan (csrc/spconv_os.hip)
int sst_internal_spconv_bf16_plan(int64_t m, int kvol, int cin, int cout, int64_t workspace_bytes, int32_t* tile_rows,
                                  int32_t* cols, int32_t* n_split, int64_t* workgroups) {
  if (kvol > kBfMaxK || (cin & 3) || m > 0x3fffffff) return SST_ERR_UNSUPPORTED;
  const bf_launch p = bf_plan(m, kvol, cin, cout, workspace_bytes);
  if (workspace_bytes < p.pack_bytes) return SST_ERR_ARG;
  if (p.wgs > 0x3fffffff) return SST_ERR_UNSUPPORTED;
  *tile_rows = 64;
  *cols = 16 * p.c.nct;
  *n_split = p.c.n_split;
  *workgroups = p.grid;
  return SST_OK;
}

// the filter-gradient launch of sst_spconv_wgrad_os_bf16 (csrc/spconv_os.hip: wgrad_os_any checks the arguments, sizes the
// chunks and reduces the partials)
void sst_internal_spconv_wgrad_bf16_launch(const float* d_x, int64_t ldx, const float* d_dy, int64_t lddy, const int32_t* d_pairs,
                                           int64_t pair_ld, int x_side, const int32_t* d_num, int kvol, int cin, int cout,
                                           int64_t chunks, int n_bi, int n_bj, int csize, float* d_part, void* stream) {
  hipLaunchKernelGGL(sp_wgrad_os_bf16_k, dim3((unsigned)chunks, (unsigned)(n_bi * n_bj)), dim3(256), 0, (hipStream_t)stream, d_x,
                     ldx, d_dy, lddy, d_pairs, pair_ld, x_side, d_num, kvol, cin, cout, n_bj, csize, d_part);
}

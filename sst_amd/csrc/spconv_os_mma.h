// The output-stationary sparse convolution on v_mfma_f32_16x16x32_bf16, once, for its three operand MODES: the contraction of
// csrc/spconv_os.hip (indiceConv and the data gradient of indiceConvBackward, spconv_ops.h:256-446),
//     Y[r, :] = sum_k X[map[k][r], :] W[k],
// on 64-row workgroups (a wave owns 16 rows x all columns of the group), W[k] packed once per call into fragment order and
// staged through LDS double-buffered, partner rows gathered as fp32 straight into registers and turned into MFMA operands
// there, heaviest-first launch order, XCD round-robin, the offsets of a thin level dealt out over workgroups with a fixed-order
// reduce kernel.  A mode is a policy struct, stated in the file that exports its entries (why it exists, its error class and its
// occupancy reasoning are that file's header): csrc/spconv_os_x3.hip, csrc/spconv_os_x6.hip, csrc/spconv_os_bf16.hip.
//   P            bf16 images an fp32 value becomes (operand parts): 2, 3, 1
//   ACCS         accumulator sets per column tile: 2 = the leading product apart from the corrections
//   min_wg(nct)  workgroups per CU the register budget is set for (__launch_bounds__)
//   kSplit       whether the offsets of a thin level are dealt out; split_env() names the variable that overrides the choice
//   kWsAlign, kPackSlack, kWholePack    the workspace rules of the mode's entries (sp_mma_conv)
//   split(a, b, p)                 8 floats -> the P operand images
//   corrections(w, x, c), leading(w, x, c)    the products of one k-step and column tile added to an accumulator of the
//                  correction set (ACCS == 2 only; it runs first) and of the leading set, in the mode's order
// Kernels and host templates live in the anonymous namespace: every including file instantiates its own.
#pragma once
#include <stdlib.h>

#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int kMmaMaxK = 32;     // kernel offsets the index image holds
constexpr int kMmaChunk = 64;    // input channels per stage
constexpr int kMmaXcdChunk = 4;  // consecutive units that stay on one XCD
constexpr int kMmaDefaultLds = 64 * 1024;   // dynamic LDS a kernel may ask for without hipFuncSetAttribute

// 32-bit words of one packed W slab, and the LDS of a workgroup: two slabs, the index image, the four live masks
template <class Mode>
constexpr int sp_mma_slab(int nct) { return 64 * 4 * 2 * nct * Mode::P; }
template <class Mode>
constexpr int sp_mma_lds_bytes(int nct, int kvol) { return (2 * sp_mma_slab<Mode>(nct) + kvol * 64 + 4) * (int)sizeof(unsigned); }

// Packed weights: slab (k, column group cg, channel chunk cc) = [2 ks][NCT ct][P parts][64 lanes][4 words of 2 bf16], with
//   the 8 values of lane (l15, g) = W[k][c = 64 cc + 32 ks + 8 g + 0..7][n = 16 NCT cg + 16 ct + l15]   (0 outside cin x cout):
// the A operand (16 columns x 32 channels) of v_mfma_f32_16x16x32_bf16, one ds_read_b128 per lane and image.
// trans_w: W[k] is stored [n][c] (the data gradient reads the forward weights with the roles swapped).
template <class Mode>
__global__ __launch_bounds__(256) void sp_mma_pack_w_k(const float* __restrict__ w, int kvol, int cin, int cout, int trans_w,
                                                       int nct, int n_cg, int n_cc, unsigned* __restrict__ wp) {
  const int64_t total = (int64_t)kvol * n_cg * n_cc * 2 * nct * 64;   // one thread = one lane's 8 values (all parts)
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
    const int c0 = cc * kMmaChunk + 32 * ks + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int c = c0 + t;
      v[t] = 0.f;
      if (c < cin && n < cout) v[t] = trans_w ? w[((int64_t)k * cout + n) * cin + c] : w[((int64_t)k * cin + c) * cout + n];
    }
    u32x4 p[Mode::P];
    Mode::split((f32x4){v[0], v[1], v[2], v[3]}, (f32x4){v[4], v[5], v[6], v[7]}, p);
    // slab base in words: ((k, cg, cc) * 2 * nct * P * 64 * 4); inside: [ks][ct][part][lane][4]
    if constexpr (Mode::P == 1) {   // one image: that place is e itself, in 16-byte pieces
      *(u32x4*)(wp + e * 4) = p[0];
    } else {
      unsigned* dst = wp + ((((int64_t)(k * n_cg + cg) * n_cc + cc) * 2 + ks) * nct + ct) * Mode::P * 256;
#pragma unroll
      for (int part = 0; part < Mode::P; ++part) *(u32x4*)(dst + part * 256 + lane * 4) = p[part];
    }
  }
}

// the accumulator sets of a column tile meet once, in the epilogue (by value: a capture would keep the sets in memory form)
template <int ACCS>
__device__ __forceinline__ f32x4 sp_mma_sum(f32x4 lead, f32x4 corr) { return ACCS == 2 ? lead + corr : lead; }

// The kernel is a gather: what hides the latency of the partner rows is other workgroups' products, so the register budget is
// set for the residency LDS admits - Mode::min_wg (the argument in full: csrc/spconv_os_bf16.hip, whose slabs are the smallest).
template <class Mode, int NCT>
__global__ __launch_bounds__(256, Mode::min_wg(NCT)) void sp_conv_os_mma_k(
    const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ map, int64_t m, int kvol,
    const unsigned* __restrict__ wp, int cin, int cout, const float* __restrict__ bias, float* __restrict__ y, int64_t ldy,
    int n_units, int n_cg, int n_cc, int xcd_chunk, int vec_store, const int32_t* __restrict__ tile_order, int n_split_arg,
    float* __restrict__ partial) {
  constexpr int ROWS = 64;
  constexpr int P = Mode::P;
  constexpr int SLAB = sp_mma_slab<Mode>(NCT);
  constexpr int WREG = SLAB / 4 / 256;   // 16-byte pieces of a slab per thread
  constexpr int NCL = Mode::ACCS == 2 ? NCT : 1;   // a mode with one accumulator set never touches the second
  extern __shared__ __attribute__((aligned(16))) unsigned sp_mma_smem[];
  unsigned (*wbuf)[SLAB] = (unsigned (*)[SLAB])sp_mma_smem;                    // [2][SLAB]
  int (*idx)[ROWS] = (int (*)[ROWS])(sp_mma_smem + 2 * SLAB);                  // [kvol][ROWS]
  unsigned* live_w = (unsigned*)(sp_mma_smem + 2 * SLAB + kvol * ROWS);        // [4]
  const int n_split = Mode::kSplit ? n_split_arg : 1;   // a mode without the split carries none of its branches
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int unit_s = ((slot / xcd_chunk) * 8 + xcd) * xcd_chunk + slot % xcd_chunk;
  if (unit_s >= n_units * n_split) return;  // uniform
  // THIN levels (a few thousand rows: 30-200 (tile, column group) units for 256 CUs, each walking 27 offsets x the channel
  // chunks alone): the offsets are dealt out over n_split workgroups per unit (offset k belongs to workgroup k % n_split), which
  // write partial tiles that sp_mma_split_reduce_k adds in a fixed order.  n_split = 1: the plain kernel.
  const int unit = unit_s / n_split, split = unit_s - unit * n_split;
  const int pos = unit / n_cg, cg = unit - pos * n_cg;
  const int tile = tile_order ? tile_order[pos] : pos;
  const int64_t r0 = (int64_t)tile * ROWS;
  // ---- partner rows of the tile for every offset -> LDS; which offsets are populated, per wave ----
  if (tid < 4) live_w[tid] = 0u;
  __syncthreads();
  {
    constexpr int NIT = (kMmaMaxK * ROWS + 255) / 256;
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

  // Two SEPARATE arrays handed to the mode by value, never one two-dimensional array, a reference or a capture: those keep the
  // sets apart from the <16 x float> the compiler otherwise makes of each, and cost moves and branches in the stage loop.  The
  // order of these declarations, and of the loop counters below, is the one that reproduces the register assignment of the
  // three kernels this template replaced (profiles/spconv_os_mma/isa_compare.txt).
  f32x4 acl[NCL], acc[NCT];      // the corrections | leading product (a single set: every product)
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < NCL; ++ct) acl[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (live != 0u) {
    const int c_last = cin - 4;  // cin % 4 == 0 (host check)
    f32x4 xn[4];                 // requested stage: channels 32 ks + 8 kq + 4 h + 0..3 at xn[2 ks + h]
    u32x4 xs[2][P], wr[WREG];    // the current stage's rows as operand images [ks][part] | the requested W slab
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
        int c = cc * kMmaChunk + 32 * (j >> 1) + 8 * kq + 4 * (j & 1);
        c = c < c_last ? c : c_last;  // beyond cin the packed weights are zero: any finite value will do
        xn[j] = *(const f32x4*)(p + c);
      }
    };
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto commit = [&](int buf) {   // requested W -> LDS buffer, requested X -> operand images of the current stage
#pragma unroll
      for (int u = 0; u < WREG; ++u) *(u32x4*)(&wbuf[buf][4 * (tid + 256 * u)]) = wr[u];
      const bool has = sn >= 0;     // rows without a partner contribute 0
      Mode::split(has ? xn[0] : zero4, has ? xn[1] : zero4, xs[0]);
      Mode::split(has ? xn[2] : zero4, has ? xn[3] : zero4, xs[1]);
    };
    auto next_live = [&](int k) {
      const unsigned rest = k < 32 ? (live >> k) : 0u;
      return rest ? k + __builtin_ctz(rest) : 32;
    };
    int buf = 0, cc = 0, k = next_live(0);
    fetch_w(k, 0);
    gather_x(k, 0);
    commit(0);
    __syncthreads();
    while (true) {
      int ncc = cc + 1, nk = k;
      if (ncc == n_cc) {
        ncc = 0;
        nk = next_live(k + 1);
      }
      const bool has_next = nk < 32;
      if (!has_next) {  // keep the loads unconditional (no branch around a request in the stage loop): the last stage
                        // requests itself once more
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
          for (int ct = 0; ct < NCT; ++ct) {
            u32x4 wv[P];
#pragma unroll
            for (int part = 0; part < P; ++part) wv[part] = *(const u32x4*)(wb + ((ks * NCT + ct) * P + part) * 256);
            if constexpr (Mode::ACCS == 2) acl[ct] = Mode::corrections(wv, xs[ks], acl[ct]);
            acc[ct] = Mode::leading(wv, xs[ks], acc[ct]);
          }
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
      if (n < cout) *(f32x4*)(dst + n) = sp_mma_sum<Mode::ACCS>(acc[ct], acl[ct % NCL]);
    }
    return;
  }
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int n = cg * 16 * NCT + 16 * ct + 4 * kq;
    if (n >= cout) continue;
    f32x4 v = sp_mma_sum<Mode::ACCS>(acc[ct], acl[ct % NCL]);
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

// y[row][n] = bias[n] + sum over the splits, in split order (deterministic).  Not mode-dependent: a template only so that a
// file whose mode has no split does not carry the kernel.
template <class Mode>
__global__ __launch_bounds__(256) void sp_mma_split_reduce_k(const float* __restrict__ partial, int64_t m, int cout, int n_split,
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
struct sp_mma_cfg {
  int nct, n_cg, n_cc, n_split;
  int64_t n_tiles, pack_words;
};
template <class Mode>
sp_mma_cfg sp_mma_pick(int64_t m, int kvol, int cin, int cout) {
  sp_mma_cfg c;
  c.n_tiles = sst_div_up(m, 64);
  c.nct = cout <= 64 ? 4 : 8;   // 128 columns per workgroup only while that leaves a few workgroups per CU
  if (c.nct == 8 && c.n_tiles * sst_div_up(cout, 128) < 2048) c.nct = 4;   // as sp_conv_os_k's os_pick
  c.n_cg = (int)sst_div_up(cout, 16 * c.nct);
  c.n_cc = (int)sst_div_up(cin, kMmaChunk);
  c.pack_words = (int64_t)kvol * c.n_cg * c.n_cc * sp_mma_slab<Mode>(c.nct);
  c.n_split = 1;
  if constexpr (Mode::kSplit) {
    // offsets dealt out over workgroups while the launch has fewer than ~3 workgroups per CU and an offset's worth of work is
    // left to each (the mode's variable overrides: 1 = never)
    static int env = -1;
    if (env < 0) {
      const char* e = getenv(Mode::split_env());
      env = e ? atoi(e) : 0;
    }
    const int64_t units = c.n_tiles * c.n_cg;
    int s = 1;
    while (s < 8 && units * s * 2 <= 1024 && kvol >= 2 * s * 2) s *= 2;
    if (env >= 1 && env <= 16) s = env < kvol ? env : kvol;
    c.n_split = s;
  }
  return c;
}

// the packed weights of a call, whichever column class it takes (worst case), in bytes
template <class Mode>
int64_t sp_mma_pack_bytes_max(int kvol, int cin, int cout) {
  const int64_t slabs4 = (int64_t)kvol * sst_div_up(cout, 64) * sst_div_up(cin, kMmaChunk) * sp_mma_slab<Mode>(4);
  const int64_t slabs8 = (int64_t)kvol * sst_div_up(cout, 128) * sst_div_up(cin, kMmaChunk) * sp_mma_slab<Mode>(8);
  return (slabs4 > slabs8 ? slabs4 : slabs8) * 4;
}
// ... the part of a workspace in front of the partial tiles (Mode::kPackSlack: bytes the mode's size query adds to the weights)
template <class Mode>
int64_t sp_mma_pack_bytes(int kvol, int cin, int cout) {
  return sst_align_up(sp_mma_pack_bytes_max<Mode>(kvol, cin, cout) + Mode::kPackSlack, 256);
}
// ... and the partial tiles of a call on m rows for its own choice of the split
template <class Mode>
int64_t sp_mma_partial_bytes(int64_t m, int kvol, int cin, int cout) {
  const sp_mma_cfg c = sp_mma_pick<Mode>(m > 0 ? m : 1, kvol, cin, cout);
  return c.n_split > 1 ? (int64_t)c.n_split * m * ((cout + 3) & ~3) * 4 : 0;
}

// what a call on a workspace of workspace_bytes launches: the split halved until its partial tiles fit behind the packed
// weights, the workgroups numbered in XCD runs of kMmaXcdChunk from 64 runs on, the grid padded to whole rounds of runs
struct sp_mma_launch {
  sp_mma_cfg c;
  int64_t pack_bytes, wgs, grid;
  int chunk;
};
template <class Mode>
sp_mma_launch sp_mma_plan(int64_t m, int kvol, int cin, int cout, int64_t workspace_bytes) {
  sp_mma_launch p;
  p.c = sp_mma_pick<Mode>(m, kvol, cin, cout);
  p.pack_bytes = sp_mma_pack_bytes<Mode>(kvol, cin, cout);
  const int64_t cpad = (cout + 3) & ~3;
  while (p.c.n_split > 1 && p.pack_bytes + (int64_t)p.c.n_split * m * cpad * 4 > workspace_bytes) p.c.n_split >>= 1;
  p.wgs = p.c.n_tiles * p.c.n_cg * p.c.n_split;
  p.chunk = p.wgs >= 64 * (int64_t)kMmaXcdChunk ? kMmaXcdChunk : 1;
  p.grid = sst_div_up(p.wgs, 8 * p.chunk) * 8 * p.chunk;
  return p;
}
// the workspace a planned call needs at least: the packed weights - of every column class (kWholePack) or of the one it takes
template <class Mode>
int64_t sp_mma_need_bytes(const sp_mma_launch& p) { return Mode::kWholePack ? p.pack_bytes : p.c.pack_words * 4; }

// the plan hooks' answer (sst_spconv_conv_os_plan, csrc/spconv_os.hip): the refusals of sp_mma_conv that depend on the shape
template <class Mode>
int sp_mma_plan_query(int64_t m, int kvol, int cin, int cout, int64_t workspace_bytes, int32_t* tile_rows, int32_t* cols,
                      int32_t* n_split, int64_t* workgroups) {
  if (kvol > kMmaMaxK || (cin & 3) || m > 0x3fffffff) return SST_ERR_UNSUPPORTED;
  const sp_mma_launch p = sp_mma_plan<Mode>(m, kvol, cin, cout, workspace_bytes);
  if (workspace_bytes < sp_mma_need_bytes<Mode>(p)) return SST_ERR_ARG;
  if (p.wgs > 0x3fffffff) return SST_ERR_UNSUPPORTED;
  *tile_rows = 64;
  *cols = 16 * p.c.nct;
  *n_split = p.c.n_split;
  *workgroups = p.grid;
  return SST_OK;
}

template <class Mode, int NCT, class... Args>
int sp_mma_launch_k(dim3 grid, int lds, hipStream_t st, Args... args) {
  if (sp_mma_lds_bytes<Mode>(8, kMmaMaxK) > kMmaDefaultLds) {   // the mode's wider class does not fit the default: once per device
    static unsigned long long attr = 0;
    if (sst_first_use_on_device(&attr)) {
      SST_HIP(hipFuncSetAttribute((const void*)sp_conv_os_mma_k<Mode, NCT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  sp_mma_lds_bytes<Mode>(NCT, kMmaMaxK)));
      sst_mark_device(&attr);
    }
  }
  hipLaunchKernelGGL((sp_conv_os_mma_k<Mode, NCT>), grid, dim3(256), lds, st, args...);
  return SST_OK;
}

// The call: same arguments as sst_spconv_conv_os_f32 + the size of the workspace (an entry that is not told it passes
// INT64_MAX); tile_cfg must be 0.  With room behind the packed weights the offsets of a thin level are dealt out.
template <class Mode>
int sp_mma_conv(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w, int cin, int cout,
                int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg, const int32_t* d_tile_order,
                void* d_workspace, int64_t workspace_bytes, void* stream) {
  if (m < 0 || kvol < 1 || cin < 1 || cout < 1 || ldx < cin || ldy < cout || tile_cfg != 0) return SST_ERR_ARG;
  if (m == 0) return SST_OK;
  if (!d_x || !d_map || !d_w || !d_y || !d_workspace) return SST_ERR_ARG;
  if (kvol > kMmaMaxK || (cin & 3) || (ldx & 3) || (((uintptr_t)d_x) & 15) || (((uintptr_t)d_workspace) & (Mode::kWsAlign - 1)) ||
      m > 0x3fffffff)
    return SST_ERR_UNSUPPORTED;
  const sp_mma_launch p = sp_mma_plan<Mode>(m, kvol, cin, cout, workspace_bytes);
  const sp_mma_cfg& c = p.c;
  if (workspace_bytes < sp_mma_need_bytes<Mode>(p)) return SST_ERR_ARG;
  const int64_t cpad = (cout + 3) & ~3;
  const int64_t n_units = c.n_tiles * c.n_cg;
  if (p.wgs > 0x3fffffff) return SST_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  unsigned* wp = (unsigned*)d_workspace;
  float* partial = c.n_split > 1 ? (float*)((char*)d_workspace + p.pack_bytes) : nullptr;
  const int64_t lanes = (int64_t)kvol * c.n_cg * c.n_cc * 2 * c.nct * 64;
  hipLaunchKernelGGL(sp_mma_pack_w_k<Mode>, dim3(sst_grid_1d(lanes, 256)), dim3(256), 0, st, d_w, kvol, cin, cout, trans_w, c.nct,
                     c.n_cg, c.n_cc, wp);
  const dim3 grid((unsigned)p.grid);
  const int vec_store = ((ldy & 3) == 0 && (((uintptr_t)d_y) & 15) == 0 && (!d_bias || (((uintptr_t)d_bias) & 15) == 0)) ? 1 : 0;
  const int lds = sp_mma_lds_bytes<Mode>(c.nct, kvol);
  const int rc = c.nct == 4 ? sp_mma_launch_k<Mode, 4>(grid, lds, st, d_x, ldx, d_map, m, kvol, (const unsigned*)wp, cin, cout, d_bias,
                                                       d_y, ldy, (int)n_units, c.n_cg, c.n_cc, p.chunk, vec_store, d_tile_order,
                                                       c.n_split, partial)
                            : sp_mma_launch_k<Mode, 8>(grid, lds, st, d_x, ldx, d_map, m, kvol, (const unsigned*)wp, cin, cout, d_bias,
                                                       d_y, ldy, (int)n_units, c.n_cg, c.n_cc, p.chunk, vec_store, d_tile_order,
                                                       c.n_split, partial);
  if (rc != SST_OK) return rc;
  if constexpr (Mode::kSplit)
    if (c.n_split > 1)
      hipLaunchKernelGGL(sp_mma_split_reduce_k<Mode>, dim3(sst_grid_1d(m * (cpad >> 2), 256)), dim3(256), 0, st, partial, m, cout,
                         c.n_split, d_bias, d_y, ldy);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // namespace

// Deformable convolution v1 (fp32, NCHW): one fused forward launch without a column buffer, and a deterministic backward.
//
// Definition (mmcv's deform_conv2d, restated from its published kernel; tests/deform_conv_ref.py is the float64 restatement):
//   out[b, o, ho, wo] = sum over the input channels c of o's convolution group and the taps (i, j) of
//                       W[o, c_local, i, j] * sample(x[b, c], h, w)
//   h = ho * stride_h - pad_h + i * dil_h + off_h,   w = wo * stride_w - pad_w + j * dil_w + off_w
//   off_h = offset[b, d * 2 * kh * kw + 2 * (i * kw + j), ho, wo], off_w = the channel after it, d = c / (Cin / deform_groups)
//   sample = 0 unless h > -1 && w > -1 && h < H && w < W; otherwise the bilinear value over the cell (floor(h), floor(w)), the
//   corners outside the image contributing 0.  No bias, no modulation mask.  The derivative in an offset is that of the cell
//   floor() selects, and 0 where the sample is 0.
// The position is kept as an integer cell and a fraction (floor(off) is added to the integer part of the position in integer
// arithmetic, off - floor(off) is the fraction): the bilinear weights carry the rounding of the offset alone, not that of a sum
// of an offset and a large coordinate.  |off| >= 1e9 (and NaN) is outside every image this file accepts.
//
// Forward: a workgroup owns kTile consecutive output pixels of one sample, pixels along lanes.  Per segment of at most kChunk
// input channels (inside one convolution group and one deformable group) it forms the sampled columns [channels * taps][kTile]
// in LDS, holds the matching weights in LDS and accumulates 4 output channels per thread in registers (plain fp32 FMAs, fixed
// order).  The cell, fraction and validity of every (pixel, tap) are computed once per deformable group and kept in LDS.
//
// Backward, no float atomics:
//   sst_dcn_bound_kernel   max|gout| and max over (c, tap) of sum_o |W| by integer maxima of the float bits
//   sst_dcn_bwd_kernel     the column gradient of a tile in LDS; the (pixel, tap) owner sums the offset gradient over the
//                          channels in a fixed order; the input gradient is added as 64-bit fixed point (power-of-two scale
//                          from the bound, chosen on the device) with integer atomics into a zeroed int64 image - first
//                          into an LDS window around the tile's footprint, which then goes to memory in whole rows
//   sst_dcn_fix_kernel     that image -> fp32
//   sst_dcn_wgrad_kernel   the column tile recomputed as in the forward, gout * col^T per segment; block x of the grid takes
//                          the tiles x, x + G, ... and writes one partial;  sst_dcn_wsum_kernel adds the partials in order
#include "common.h"

namespace {

constexpr int kTile = 64;       // output pixels per workgroup = one wave of lanes
constexpr int kThreads = 256;   // 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 8;       // input channels per segment
constexpr int kMaxTaps = 9;     // kh, kw <= 3
constexpr int kOut = 16;        // output channels per pass (4 per thread)
constexpr int kLd = kTile + 1;  // row stride of the column tile: rows read along pixels and across rows without bank conflicts
constexpr int kRowsMax = kChunk * kMaxTaps;
constexpr int kInvalid = INT32_MIN;
constexpr int kWinRows = 12;   // LDS window of the input gradient's scatter: rows x columns of input cells per tile
constexpr int kWinCols = 80;
constexpr int kWinMargin = 6;  // columns in front of the tile's first undeformed tap
constexpr int kFixBits = 60;    // |sum of the fixed-point contributions to one input element| < 2^kFixBits

struct Shape {
  int B, Cin, H, W, Cout, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg;
  int Cg, Og, cpd, KK, tps;     // channels per group, outputs per group, channels per deformable group, taps, tiles per sample
  int64_t HW, HoWo, tiles;
};

struct Segment {
  int g, c0, cn, d;             // convolution group, first channel (global), channels, deformable group
};

// the s-th segment in (group, channel) order; returns the number of segments when s is past the end
__host__ __device__ inline int dcn_segment(const Shape& sp, int s, Segment* out) {
  int n = 0;
  for (int g = 0; g < sp.groups; ++g) {
    int c = g * sp.Cg;
    const int end = c + sp.Cg;
    while (c < end) {
      int c1 = c + kChunk;
      if (c1 > end) c1 = end;
      const int dn = (c / sp.cpd + 1) * sp.cpd;
      if (c1 > dn) c1 = dn;
      if (n == s) {
        out->g = g; out->c0 = c; out->cn = c1 - c; out->d = c / sp.cpd;
        return n;
      }
      ++n;
      c = c1;
    }
  }
  return n;
}

struct Params {                 // per (tap, pixel of the tile): integer cell and fractions; hl == kInvalid: the sample is 0
  int hl[kMaxTaps * kTile];
  int wl[kMaxTaps * kTile];
  float lh[kMaxTaps * kTile];
  float lw[kMaxTaps * kTile];
};

__device__ __forceinline__ void dcn_params(const Shape& sp, const float* __restrict__ off_bd, int p0, Params& pr) {
  for (int e = threadIdx.x; e < sp.KK * kTile; e += kThreads) {
    const int k = e >> 6, p = e & 63;
    const int64_t pix = (int64_t)p0 + p;
    int hl = kInvalid, wl = 0;
    float lh = 0.f, lw = 0.f;
    if (pix < sp.HoWo) {
      const int ho = (int)(pix / sp.Wo), wo = (int)(pix - (int64_t)ho * sp.Wo);
      const int i = k / sp.kw, j = k - i * sp.kw;
      const float oh = off_bd[(int64_t)(2 * k) * sp.HoWo + pix], ow = off_bd[(int64_t)(2 * k + 1) * sp.HoWo + pix];
      if (fabsf(oh) < 1e9f && fabsf(ow) < 1e9f) {
        const float fh = floorf(oh), fw = floorf(ow);
        const int bh = ho * sp.sh - sp.ph + i * sp.dh + (int)fh, bw = wo * sp.sw - sp.pw + j * sp.dw + (int)fw;
        lh = oh - fh;
        lw = ow - fw;
        // h = bh + lh > -1 and < H, likewise w
        const bool ok = (bh > -1 || (bh == -1 && lh > 0.f)) && bh < sp.H && (bw > -1 || (bw == -1 && lw > 0.f)) && bw < sp.W;
        if (ok) { hl = bh; wl = bw; }
      }
    }
    pr.hl[e] = hl; pr.wl[e] = wl; pr.lh[e] = lh; pr.lw[e] = lw;
  }
}

// the four corners of the cell (0 outside the image)
__device__ __forceinline__ void dcn_corners(const float* __restrict__ xc, int H, int W, int hl, int wl, float& v1, float& v2,
                                            float& v3, float& v4) {
  const bool h0 = hl >= 0, h1 = hl + 1 <= H - 1, w0 = wl >= 0, w1 = wl + 1 <= W - 1;
  const int64_t at = (int64_t)hl * W + wl;
  v1 = (h0 && w0) ? xc[at] : 0.f;
  v2 = (h0 && w1) ? xc[at + 1] : 0.f;
  v3 = (h1 && w0) ? xc[at + W] : 0.f;
  v4 = (h1 && w1) ? xc[at + W + 1] : 0.f;
}

// sampled columns of the segment's channels: col[(cl * KK + k) * kLd + p]
__device__ __forceinline__ void dcn_gather(const Shape& sp, const float* __restrict__ x_b, const Segment& sg, const Params& pr,
                                           float* col) {
  const int rows = sg.cn * sp.KK;
  for (int e = threadIdx.x; e < rows * kTile; e += kThreads) {
    const int r = e >> 6, p = e & 63;
    const int cl = r / sp.KK, k = r - cl * sp.KK;
    const int q = k * kTile + p;
    const int hl = pr.hl[q];
    float v = 0.f;
    if (hl != kInvalid) {
      const int wl = pr.wl[q];
      const float lh = pr.lh[q], lw = pr.lw[q], hh = 1.f - lh, hw = 1.f - lw;
      float v1, v2, v3, v4;
      dcn_corners(x_b + (int64_t)(sg.c0 + cl) * sp.HW, sp.H, sp.W, hl, wl, v1, v2, v3, v4);
      v = hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4;
    }
    col[r * kLd + p] = v;
  }
}

// weights of kOut outputs from o0 of group g over the segment: wt[r * kOut + oo], zero for outputs past the group
__device__ __forceinline__ void dcn_stage_weights(const Shape& sp, const float* __restrict__ w, const Segment& sg, int o0,
                                                  float* wt) {
  const int rows = sg.cn * sp.KK;
  const int cl0 = sg.c0 - sg.g * sp.Cg;
  for (int e = threadIdx.x; e < kOut * rows; e += kThreads) {
    const int oo = e / rows, r = e - oo * rows;
    const int o = o0 + oo;
    wt[r * kOut + oo] = o < sp.Og ? w[((int64_t)(sg.g * sp.Og + o) * sp.Cg + cl0) * sp.KK + r] : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void sst_dcn_fwd_kernel(Shape sp, const float* __restrict__ x,
                                                               const float* __restrict__ off, const float* __restrict__ w,
                                                               float* __restrict__ out) {
  __shared__ Params pr;
  __shared__ float col[kRowsMax * kLd];
  __shared__ __attribute__((aligned(16))) float wt[kRowsMax * kOut];
  const int64_t tile = blockIdx.x;
  const int b = (int)(tile / sp.tps);
  const int p0 = (int)(tile - (int64_t)b * sp.tps) * kTile;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* x_b = x + (int64_t)b * sp.Cin * sp.HW;
  const float* off_b = off + (int64_t)b * sp.dg * 2 * sp.KK * sp.HoWo;
  const int64_t pix = (int64_t)p0 + lane;
  int cur_d = -1;
  Segment sg;
  const int n_seg = dcn_segment(sp, INT32_MAX, &sg);
  const int n_oc = (sp.Og + kOut - 1) / kOut;
  int s_first = 0;
  for (int g = 0; g < sp.groups; ++g) {
    int s_end = s_first;
    for (int oc = 0; oc < n_oc; ++oc) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int s = s_first;
      for (; s < n_seg; ++s) {
        dcn_segment(sp, s, &sg);
        if (sg.g != g) break;
        __syncthreads();                       // the products of the previous segment are done with col / wt / pr
        if (sg.d != cur_d) {
          dcn_params(sp, off_b + (int64_t)sg.d * 2 * sp.KK * sp.HoWo, p0, pr);
          cur_d = sg.d;
          __syncthreads();
        }
        dcn_stage_weights(sp, w, sg, oc * kOut, wt);
        dcn_gather(sp, x_b, sg, pr, col);
        __syncthreads();
        const int rows = sg.cn * sp.KK;
        for (int r = 0; r < rows; ++r) {
          const float cv = col[r * kLd + lane];
          const float4 wq = *reinterpret_cast<const float4*>(&wt[r * kOut + 4 * wv]);
          a0 += cv * wq.x; a1 += cv * wq.y; a2 += cv * wq.z; a3 += cv * wq.w;
        }
      }
      s_end = s;
      if (pix < sp.HoWo) {
        const int o = oc * kOut + 4 * wv;
        float* dst = out + ((int64_t)b * sp.Cout + (int64_t)g * sp.Og + o) * sp.HoWo + pix;
        if (o < sp.Og) dst[0] = a0;
        if (o + 1 < sp.Og) dst[sp.HoWo] = a1;
        if (o + 2 < sp.Og) dst[2 * sp.HoWo] = a2;
        if (o + 3 < sp.Og) dst[3 * sp.HoWo] = a3;
      }
    }
    s_first = s_end;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------

struct BoundState {
  unsigned int gmax_bits;       // bits of max|gout| (non-negative floats order as their bits do)
  unsigned int wmax_bits;       // bits of max over (c, tap) of sum_o |W[o, c, tap]|
};

__global__ __launch_bounds__(kThreads) void sst_dcn_bound_kernel(Shape sp, const float* __restrict__ gout, int64_t n_gout,
                                                                 const float* __restrict__ w, BoundState* st) {
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_gout; i += (int64_t)gridDim.x * kThreads)
    m = fmaxf(m, fabsf(gout[i]));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_down(m, d, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(&st->gmax_bits, __float_as_uint(m));
  if (blockIdx.x == 0) {
    const int per = sp.Cg * sp.KK;             // (c_local, tap) columns of a group
    float wm = 0.f;
    for (int e = threadIdx.x; e < sp.groups * per; e += kThreads) {
      const int g = e / per, r = e - g * per;
      float s = 0.f;
      for (int o = 0; o < sp.Og; ++o) s += fabsf(w[((int64_t)(g * sp.Og + o)) * per + r]);
      wm = fmaxf(wm, s);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wm = fmaxf(wm, __shfl_down(wm, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&st->wmax_bits, __float_as_uint(wm));
  }
}

// the exponent s of the fixed-point scale 2^s: every contribution is below M = gmax * wmax < 2^e in magnitude and at most
// 2^log_n of them meet in one element, so with s = kFixBits - log_n - e the sums stay below 2^kFixBits
__device__ __forceinline__ int dcn_fix_exponent(const BoundState* st, int log_n) {
  const double m = (double)__uint_as_float(st->gmax_bits) * (double)__uint_as_float(st->wmax_bits);
  if (!(m > 0.0) || !(m < 1e300)) return 0;    // nothing to add, or no finite bound
  int e;
  frexp(m, &e);                                // m = f * 2^e, f in [0.5, 1)
  return kFixBits - log_n - e;
}

__global__ __launch_bounds__(kThreads) void sst_dcn_bwd_kernel(Shape sp, const float* __restrict__ x,
                                                               const float* __restrict__ off, const float* __restrict__ w,
                                                               const float* __restrict__ gout, const BoundState* st, int log_n,
                                                               long long* __restrict__ gin_fix, float* __restrict__ goff) {
  __shared__ Params pr;
  __shared__ float gcol[kRowsMax * kLd];
  __shared__ __attribute__((aligned(16))) float wt[kRowsMax * kOut];
  __shared__ float goff_s[2 * kMaxTaps * kTile];
  __shared__ unsigned long long win[kWinRows * kWinCols];
  const int64_t tile = blockIdx.x;
  const int b = (int)(tile / sp.tps);
  const int p0 = (int)(tile - (int64_t)b * sp.tps) * kTile;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // the window of input cells around the tile's first pixel: the rows and columns its undeformed taps reach, with a margin for
  // the offsets; pixels of the tile behind a row break and far offsets fall outside and go to memory directly
  const int win_r0 = (p0 / sp.Wo) * sp.sh - sp.ph + (sp.dh * (sp.kh - 1)) / 2 - (kWinRows / 2 - 1);
  const int win_c0 = (p0 % sp.Wo) * sp.sw - sp.pw - kWinMargin;
  for (int i = threadIdx.x; i < kWinRows * kWinCols; i += kThreads) win[i] = 0;
  const float* x_b = x + (int64_t)b * sp.Cin * sp.HW;
  long long* gin_b = gin_fix + (int64_t)b * sp.Cin * sp.HW;
  const float* off_b = off + (int64_t)b * sp.dg * 2 * sp.KK * sp.HoWo;
  float* goff_b = goff + (int64_t)b * sp.dg * 2 * sp.KK * sp.HoWo;
  const int64_t pix = (int64_t)p0 + lane;
  const double scale = ldexp(1.0, dcn_fix_exponent(st, log_n));
  const int n_oc = (sp.Og + kOut - 1) / kOut;
  Segment sg;
  const int n_seg = dcn_segment(sp, INT32_MAX, &sg);
  int cur_d = -1;
  for (int s = 0; s <= n_seg; ++s) {
    if (s < n_seg) dcn_segment(sp, s, &sg);
    if (s == n_seg || sg.d != cur_d) {
      __syncthreads();                         // the previous segment's owners are done with pr and goff_s
      if (cur_d >= 0) {
        for (int e = threadIdx.x; e < 2 * sp.KK * kTile; e += kThreads) {
          const int ch = e >> 6, p = e & 63;
          if ((int64_t)p0 + p < sp.HoWo) goff_b[((int64_t)cur_d * 2 * sp.KK + ch) * sp.HoWo + p0 + p] = goff_s[e];
        }
      }
      if (s == n_seg) break;
      __syncthreads();
      dcn_params(sp, off_b + (int64_t)sg.d * 2 * sp.KK * sp.HoWo, p0, pr);
      for (int e = threadIdx.x; e < 2 * sp.KK * kTile; e += kThreads) goff_s[e] = 0.f;
      cur_d = sg.d;
    }
    const int rows = sg.cn * sp.KK;
    // column gradient of the segment: gcol[r][p] = sum_o W[o][r] * gout[o][p], outputs in index order
    for (int oc = 0; oc < n_oc; ++oc) {
      __syncthreads();
      dcn_stage_weights(sp, w, sg, oc * kOut, wt);
      float gv[kOut];
#pragma unroll
      for (int oo = 0; oo < kOut; ++oo) {
        const int o = oc * kOut + oo;
        gv[oo] = (o < sp.Og && pix < sp.HoWo) ? gout[((int64_t)b * sp.Cout + (int64_t)sg.g * sp.Og + o) * sp.HoWo + pix] : 0.f;
      }
      __syncthreads();
      for (int r = wv; r < rows; r += kWaves) {
        float acc = oc == 0 ? 0.f : gcol[r * kLd + lane];
#pragma unroll
        for (int q = 0; q < kOut / 4; ++q) {
          const float4 wq = *reinterpret_cast<const float4*>(&wt[r * kOut + 4 * q]);
          acc += wq.x * gv[4 * q]; acc += wq.y * gv[4 * q + 1]; acc += wq.z * gv[4 * q + 2]; acc += wq.w * gv[4 * q + 3];
        }
        gcol[r * kLd + lane] = acc;
      }
    }
    __syncthreads();
    // channel by channel: the owner of (tap, pixel) adds its offset-gradient terms (channels in order) and its four corner
    // contributions as fixed point - into the LDS window where they fall inside it, to memory otherwise; then the window is
    // added to memory, consecutive lanes on consecutive addresses, and cleared
    for (int cl = 0; cl < sg.cn; ++cl) {
      const float* xc = x_b + (int64_t)(sg.c0 + cl) * sp.HW;
      unsigned long long* gi_c = reinterpret_cast<unsigned long long*>(gin_b + (int64_t)(sg.c0 + cl) * sp.HW);
      for (int e = threadIdx.x; e < sp.KK * kTile; e += kThreads) {
        const int k = e >> 6, p = e & 63;
        const int hl = pr.hl[e];
        if (hl == kInvalid) continue;
        const int wl = pr.wl[e];
        const float lh = pr.lh[e], lw = pr.lw[e], hh = 1.f - lh, hw = 1.f - lw;
        const bool h0 = hl >= 0, h1 = hl + 1 <= sp.H - 1, w0 = wl >= 0, w1 = wl + 1 <= sp.W - 1;
        const int64_t at = (int64_t)hl * sp.W + wl;
        const float gc = gcol[(cl * sp.KK + k) * kLd + p];
        const float v1 = (h0 && w0) ? xc[at] : 0.f, v2 = (h0 && w1) ? xc[at + 1] : 0.f;
        const float v3 = (h1 && w0) ? xc[at + sp.W] : 0.f, v4 = (h1 && w1) ? xc[at + sp.W + 1] : 0.f;
        goff_s[(2 * k) * kTile + p] += gc * (hw * (v3 - v1) + lw * (v4 - v2));
        goff_s[(2 * k + 1) * kTile + p] += gc * (hh * (v2 - v1) + lh * (v4 - v3));
        const float t[4] = {hh * hw * gc, hh * lw * gc, lh * hw * gc, lh * lw * gc};
        const bool in[4] = {h0 && w0, h0 && w1, h1 && w0, h1 && w1};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!in[q] || t[q] == 0.f) continue;
          const int row = hl + (q >> 1), col = wl + (q & 1);
          const unsigned long long add = (unsigned long long)__double2ll_rn((double)t[q] * scale);
          const int wr = row - win_r0, wc = col - win_c0;
          if ((unsigned)wr < (unsigned)kWinRows && (unsigned)wc < (unsigned)kWinCols)
            atomicAdd(&win[wr * kWinCols + wc], add);
          else
            atomicAdd(gi_c + (int64_t)row * sp.W + col, add);
        }
      }
      __syncthreads();
      for (int i = threadIdx.x; i < kWinRows * kWinCols; i += kThreads) {
        const unsigned long long v = win[i];
        if (v != 0) {                          // only cells inside the image were ever added to
          const int wr = i / kWinCols, wc = i - wr * kWinCols;
          atomicAdd(gi_c + (int64_t)(win_r0 + wr) * sp.W + (win_c0 + wc), v);
          win[i] = 0;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kThreads) void sst_dcn_fix_kernel(const long long* __restrict__ fix, const BoundState* st, int log_n,
                                                               int64_t n, float* __restrict__ gin) {
  const double inv = ldexp(1.0, -dcn_fix_exponent(st, log_n));
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    gin[i] = (float)((double)fix[i] * inv);
}

// grid (G, segments * output passes): block x adds the tiles x, x + G, ... of its (segment, pass) in that order
__global__ __launch_bounds__(kThreads) void sst_dcn_wgrad_kernel(Shape sp, const float* __restrict__ x,
                                                                 const float* __restrict__ off, const float* __restrict__ gout,
                                                                 float* __restrict__ partials) {
  __shared__ Params pr;
  __shared__ float col[kRowsMax * kLd];
  __shared__ __attribute__((aligned(16))) float gt[kTile * kOut];   // gt[p * kOut + oo]
  const int n_oc = (sp.Og + kOut - 1) / kOut;
  Segment sg;
  dcn_segment(sp, (int)blockIdx.y / n_oc, &sg);
  const int oc = (int)blockIdx.y % n_oc;
  const int rows = sg.cn * sp.KK;
  float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int64_t tile = blockIdx.x; tile < sp.tiles; tile += gridDim.x) {
    const int b = (int)(tile / sp.tps);
    const int p0 = (int)(tile - (int64_t)b * sp.tps) * kTile;
    __syncthreads();                           // the products of the previous tile are done
    dcn_params(sp, off + ((int64_t)b * sp.dg + sg.d) * 2 * sp.KK * sp.HoWo, p0, pr);
    for (int e = threadIdx.x; e < kOut * kTile; e += kThreads) {
      const int oo = e >> 6, p = e & 63;
      const int o = oc * kOut + oo;
      const int64_t pix = (int64_t)p0 + p;
      gt[p * kOut + oo] = (o < sp.Og && pix < sp.HoWo)
                              ? gout[((int64_t)b * sp.Cout + (int64_t)sg.g * sp.Og + o) * sp.HoWo + pix] : 0.f;
    }
    __syncthreads();
    dcn_gather(sp, x + (int64_t)b * sp.Cin * sp.HW, sg, pr, col);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = threadIdx.x + j * kThreads;
      if (e < rows * 4) {
        const int oq = e & 3, r = e >> 2;
        for (int p = 0; p < kTile; ++p) {
          const float cv = col[r * kLd + p];
          const float4 gq = *reinterpret_cast<const float4*>(&gt[p * kOut + 4 * oq]);
          acc[j][0] += cv * gq.x; acc[j][1] += cv * gq.y; acc[j][2] += cv * gq.z; acc[j][3] += cv * gq.w;
        }
      }
    }
  }
  const int64_t wn = (int64_t)sp.Cout * sp.Cg * sp.KK;
  const int cl0 = sg.c0 - sg.g * sp.Cg;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = threadIdx.x + j * kThreads;
    if (e < rows * 4) {
      const int oq = e & 3, r = e >> 2;
      for (int i = 0; i < 4; ++i) {
        const int o = oc * kOut + 4 * oq + i;
        if (o < sp.Og)
          partials[(int64_t)blockIdx.x * wn + ((int64_t)(sg.g * sp.Og + o) * sp.Cg + cl0) * sp.KK + r] = acc[j][i];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void sst_dcn_wsum_kernel(const float* __restrict__ partials, int n_part, int64_t wn,
                                                                float* __restrict__ gw) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= wn) return;
  float s = partials[i];
  for (int j = 1; j < n_part; ++j) s += partials[(int64_t)j * wn + i];
  gw[i] = s;
}

int dcn_shape(const sst_deform_conv_shape* a, Shape* sp) {
  if (!a) return SST_ERR_ARG;
  if (a->batch < 0 || a->in_channels <= 0 || a->out_channels <= 0 || a->height <= 0 || a->width <= 0 || a->kernel_h <= 0 ||
      a->kernel_w <= 0 || a->stride_h <= 0 || a->stride_w <= 0 || a->pad_h < 0 || a->pad_w < 0 || a->dil_h <= 0 || a->dil_w <= 0 ||
      a->groups <= 0 || a->deform_groups <= 0)
    return SST_ERR_ARG;
  if (a->in_channels % a->groups || a->out_channels % a->groups || a->in_channels % a->deform_groups) return SST_ERR_ARG;
  if (a->kernel_h > 3 || a->kernel_w > 3) return SST_ERR_UNSUPPORTED;
  const int64_t eh = (int64_t)a->height + 2 * (int64_t)a->pad_h - ((int64_t)a->dil_h * (a->kernel_h - 1) + 1);
  const int64_t ew = (int64_t)a->width + 2 * (int64_t)a->pad_w - ((int64_t)a->dil_w * (a->kernel_w - 1) + 1);
  if (eh < 0 || ew < 0) return SST_ERR_ARG;
  const int64_t ho = eh / a->stride_h + 1, wo = ew / a->stride_w + 1;
  // positions and plane indices are 32-bit integers with room for an offset below 1e9
  const int64_t lim = 1 << 28;
  if ((int64_t)a->height * a->width >= ((int64_t)1 << 31) || ho * wo >= ((int64_t)1 << 31) || ho * a->stride_h >= lim ||
      wo * a->stride_w >= lim || a->pad_h >= lim || a->pad_w >= lim || (int64_t)a->dil_h * 3 >= lim || (int64_t)a->dil_w * 3 >= lim)
    return SST_ERR_UNSUPPORTED;
  sp->B = a->batch; sp->Cin = a->in_channels; sp->H = a->height; sp->W = a->width; sp->Cout = a->out_channels;
  sp->Ho = (int)ho; sp->Wo = (int)wo; sp->kh = a->kernel_h; sp->kw = a->kernel_w; sp->sh = a->stride_h; sp->sw = a->stride_w;
  sp->ph = a->pad_h; sp->pw = a->pad_w; sp->dh = a->dil_h; sp->dw = a->dil_w; sp->groups = a->groups; sp->dg = a->deform_groups;
  sp->Cg = a->in_channels / a->groups; sp->Og = a->out_channels / a->groups; sp->cpd = a->in_channels / a->deform_groups;
  sp->KK = a->kernel_h * a->kernel_w;
  sp->HW = (int64_t)a->height * a->width; sp->HoWo = ho * wo;
  sp->tps = (int)sst_div_up(sp->HoWo, kTile);
  sp->tiles = (int64_t)sp->B * sp->tps;
  if (sp->tiles >= ((int64_t)1 << 31)) return SST_ERR_UNSUPPORTED;
  return SST_OK;
}

int dcn_log_n(const Shape& sp) {               // ceil(log2(addends that can meet in one input element))
  const int64_t n = sp.HoWo * sp.KK;
  int l = 0;
  while (((int64_t)1 << l) < n) ++l;
  return l;
}

int dcn_wgrad_blocks(int64_t tiles) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus <= 0)
    cus = 256;
  return (int)(tiles < cus ? (tiles > 0 ? tiles : 1) : cus);
}

int64_t dcn_fix_bytes(const Shape& sp) { return sst_align_up(256 + 8 * (int64_t)sp.B * sp.Cin * sp.HW, 256); }

}  // namespace

extern "C" {

int sst_deform_conv_tile_pixels(void) { return kTile; }

int sst_deform_conv_wgrad_blocks(int64_t total_tiles) { return dcn_wgrad_blocks(total_tiles); }

int sst_deform_conv_out_size(const sst_deform_conv_shape* shape, int32_t* out_h, int32_t* out_w) {
  Shape sp;
  const int rc = dcn_shape(shape, &sp);
  if (rc != SST_OK) return rc;
  if (out_h) *out_h = sp.Ho;
  if (out_w) *out_w = sp.Wo;
  return SST_OK;
}

int64_t sst_deform_conv_bwd_workspace_bytes(const sst_deform_conv_shape* shape) {
  Shape sp;
  const int rc = dcn_shape(shape, &sp);
  if (rc != SST_OK) return rc;
  const int64_t wn = (int64_t)sp.Cout * sp.Cg * sp.KK;
  return dcn_fix_bytes(sp) + sst_align_up(4 * wn * dcn_wgrad_blocks(sp.tiles), 256);
}

int sst_deform_conv_fwd_f32(const sst_deform_conv_shape* shape, const float* d_input, const float* d_offset,
                            const float* d_weight, float* d_out, void* stream) {
  Shape sp;
  const int rc = dcn_shape(shape, &sp);
  if (rc != SST_OK) return rc;
  if (sp.tiles == 0) return SST_OK;
  if (!d_input || !d_offset || !d_weight || !d_out) return SST_ERR_ARG;
  sst_dcn_fwd_kernel<<<dim3((unsigned)sp.tiles), dim3(kThreads), 0, (hipStream_t)stream>>>(sp, d_input, d_offset, d_weight, d_out);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

int sst_deform_conv_bwd_f32(const sst_deform_conv_shape* shape, const float* d_input, const float* d_offset,
                            const float* d_weight, const float* d_out_grad, float* d_input_grad, float* d_offset_grad,
                            float* d_weight_grad, void* d_workspace, void* stream) {
  Shape sp;
  const int rc = dcn_shape(shape, &sp);
  if (rc != SST_OK) return rc;
  if (!d_weight_grad || !d_workspace) return SST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t wn = (int64_t)sp.Cout * sp.Cg * sp.KK;
  if (sp.tiles == 0) return (int)hipMemsetAsync(d_weight_grad, 0, 4 * wn, st);
  if (!d_input || !d_offset || !d_weight || !d_out_grad || !d_input_grad || !d_offset_grad) return SST_ERR_ARG;
  const int log_n = dcn_log_n(sp);
  if (log_n > 22) return SST_ERR_UNSUPPORTED;  // the quantum stays below 2^-36 of the bound (at most 2^-(kFixBits - 1 - log_n))
  const int64_t n_in = (int64_t)sp.B * sp.Cin * sp.HW, n_gout = (int64_t)sp.B * sp.Cout * sp.HoWo;
  BoundState* state = (BoundState*)d_workspace;
  long long* fix = (long long*)((char*)d_workspace + 256);
  float* partials = (float*)((char*)d_workspace + dcn_fix_bytes(sp));
  SST_HIP(hipMemsetAsync(d_workspace, 0, 256 + 8 * n_in, st));
  sst_dcn_bound_kernel<<<dim3(sst_grid_1d(n_gout, kThreads)), dim3(kThreads), 0, st>>>(sp, d_out_grad, n_gout, d_weight, state);
  SST_LAUNCH_CHECK();
  sst_dcn_bwd_kernel<<<dim3((unsigned)sp.tiles), dim3(kThreads), 0, st>>>(sp, d_input, d_offset, d_weight, d_out_grad, state, log_n,
                                                                           fix, d_offset_grad);
  SST_LAUNCH_CHECK();
  sst_dcn_fix_kernel<<<dim3(sst_grid_1d(n_in, kThreads)), dim3(kThreads), 0, st>>>(fix, state, log_n, n_in, d_input_grad);
  SST_LAUNCH_CHECK();
  Segment sg;
  const int n_seg = dcn_segment(sp, INT32_MAX, &sg);
  const int n_oc = (sp.Og + kOut - 1) / kOut;
  const int g_blocks = dcn_wgrad_blocks(sp.tiles);
  if ((int64_t)n_seg * n_oc > 65535) return SST_ERR_UNSUPPORTED;
  sst_dcn_wgrad_kernel<<<dim3(g_blocks, n_seg * n_oc), dim3(kThreads), 0, st>>>(sp, d_input, d_offset, d_out_grad, partials);
  SST_LAUNCH_CHECK();
  sst_dcn_wsum_kernel<<<dim3((unsigned)sst_div_up(wn, kThreads)), dim3(kThreads), 0, st>>>(partials, g_blocks, wn, d_weight_grad);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

// Row-wise LayerNorm pieces shared by csrc/dense.hip and the fused SIR stage (csrc/sir_stage.hip): the activation folded into
// the LayerNorm passes, the 32-lane row sum, the LayerNorm + activation backward and the reduction of its block partials.
#pragma once
#include <math.h>
#include "common.h"

namespace {

constexpr int kLnThreads = 256;
constexpr int kLnRowsPerBlock = kLnThreads / 32;  // one row per 32-lane half-wave
constexpr int kLnMaxVec = 4;                      // up to 4 float4 per lane -> C <= 512

// activation folded into the LayerNorm passes ("Linear -> LN -> GELU" of FSD's SIR layers, voxel_encoder.py:628-650):
// 0 none, 1 GELU (erf form; Abramowitz-Stegun 7.1.26, |error| < 1.5e-7, as in csrc/dense_f32.hip), 2 ReLU
__device__ __forceinline__ float ln_erf(float z, float& e) {
  const float az = fabsf(z);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.f));
  e = __expf(-az * az);
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  return copysignf(fmaf(-poly, e, 1.f), z);
}
__device__ __forceinline__ float ln_act(float x, int act) {
  if (act == 1) {
    float e;
    return 0.5f * x * (1.f + ln_erf(x * 0.70710678118654752f, e));
  }
  return act == 2 ? fmaxf(x, 0.f) : x;
}
__device__ __forceinline__ float ln_act_grad(float x, int act) {
  if (act == 1) {
    float e;
    const float phi = 0.5f * (1.f + ln_erf(x * 0.70710678118654752f, e));
    return fmaf(x * 0.3989422804014327f, e, phi);
  }
  return act == 2 ? (x > 0.f ? 1.f : 0.f) : 1.f;
}

// the forward row arithmetic of a float4 of columns (add_ln_fwd_k, sir_stage_fwd_k): its share of the sum of squared
// deviations, and y = act((v - mean) * rstd * w + b)
__device__ __forceinline__ float ln_sqdev4(const float4 v, float mean) {
  const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
  return dx * dx + dy * dy + dz * dz + dw * dw;
}
__device__ __forceinline__ float4 ln_norm_act4(const float4 v, float mean, float rstd, const float4 wv, const float4 bv, int act) {
  float4 o;
  o.x = (v.x - mean) * rstd * wv.x + bv.x;
  o.y = (v.y - mean) * rstd * wv.y + bv.y;
  o.z = (v.z - mean) * rstd * wv.z + bv.z;
  o.w = (v.w - mean) * rstd * wv.w + bv.w;
  if (act) o.x = ln_act(o.x, act), o.y = ln_act(o.y, act), o.z = ln_act(o.z, act), o.w = ln_act(o.w, act);
  return o;
}

__device__ __forceinline__ float group32_sum(float v) {
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// Given s = x + r (saved), stats, dy:  dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * w
// dw += sum_rows dy * xhat ; db += sum_rows dy   (block partials in LDS, then one atomic per column per block)
// ROUTE (the fused SIR stage, csrc/sir_stage.hip; c == 128): the gradient of a segmented max over the rows is routed in on
// load, dy_total[row, col] = dy[row, col] + (argmax[g, col] == row ? dpooled[g, col] : 0), g = inverse[row]; dy or dpooled may
// then be null.  The row arithmetic behind the load is the same code for both forms.
template <bool ROUTE>
__global__ __launch_bounds__(kLnThreads) void add_ln_bwd_k(const float* __restrict__ dy, const float* __restrict__ s,
                                                           const float2* __restrict__ stats,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ b, int act, int64_t m, int c,
                                                           float* __restrict__ dx,
                                                           float* __restrict__ partials,
                                                           const float* __restrict__ dpooled = nullptr,
                                                           const int32_t* __restrict__ argmax = nullptr,
                                                           const int32_t* __restrict__ inverse = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float part[];  // [2][c]
  for (int i = threadIdx.x; i < 2 * c; i += kLnThreads) part[i] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 31;
  const int sub = threadIdx.x >> 5;
  const int nvec = (c + 127) / 128;
  float4 aw[kLnMaxVec], ab[kLnMaxVec];
#pragma unroll
  for (int k = 0; k < kLnMaxVec; ++k) aw[k] = ab[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t row = (int64_t)blockIdx.x * kLnRowsPerBlock + sub; row < m; row += (int64_t)gridDim.x * kLnRowsPerBlock) {
    const float2 st = stats[row];
    const int64_t grow = (ROUTE && dpooled != nullptr) ? (int64_t)inverse[row] : 0;
    float4 g[kLnMaxVec], xh[kLnMaxVec];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int k = 0; k < kLnMaxVec; ++k) {
      const int col = k * 128 + lane * 4;
      g[k] = xh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < nvec && col < c) {
        float4 d;
        if (!ROUTE) {
          d = *(const float4*)(dy + row * c + col);
        } else {
          d = dy != nullptr ? *(const float4*)(dy + row * c + col) : make_float4(0.f, 0.f, 0.f, 0.f);
          if (dpooled != nullptr) {
            const int4 am = *(const int4*)(argmax + grow * c + col);
            const float4 dp = *(const float4*)(dpooled + grow * c + col);
            if (am.x == (int)row) d.x += dp.x;
            if (am.y == (int)row) d.y += dp.y;
            if (am.z == (int)row) d.z += dp.z;
            if (am.w == (int)row) d.w += dp.w;
          }
        }
        const float4 sv = *(const float4*)(s + row * c + col);
        const float4 wv = *(const float4*)(w + col);
        xh[k] = make_float4((sv.x - st.x) * st.y, (sv.y - st.x) * st.y, (sv.z - st.x) * st.y, (sv.w - st.x) * st.y);
        if (act) {   // the gradient arrives behind the activation: through it first, at the recomputed LayerNorm output
          const float4 bv = *(const float4*)(b + col);
          d.x *= ln_act_grad(fmaf(xh[k].x, wv.x, bv.x), act);
          d.y *= ln_act_grad(fmaf(xh[k].y, wv.y, bv.y), act);
          d.z *= ln_act_grad(fmaf(xh[k].z, wv.z, bv.z), act);
          d.w *= ln_act_grad(fmaf(xh[k].w, wv.w, bv.w), act);
        }
        g[k] = make_float4(d.x * wv.x, d.y * wv.y, d.z * wv.z, d.w * wv.w);
        sg += g[k].x + g[k].y + g[k].z + g[k].w;
        sgx += g[k].x * xh[k].x + g[k].y * xh[k].y + g[k].z * xh[k].z + g[k].w * xh[k].w;
        aw[k].x += d.x * xh[k].x;
        aw[k].y += d.y * xh[k].y;
        aw[k].z += d.z * xh[k].z;
        aw[k].w += d.w * xh[k].w;
        ab[k].x += d.x;
        ab[k].y += d.y;
        ab[k].z += d.z;
        ab[k].w += d.w;
      }
    }
    const float mg = group32_sum(sg) / (float)c;
    const float mgx = group32_sum(sgx) / (float)c;
#pragma unroll
    for (int k = 0; k < kLnMaxVec; ++k) {
      const int col = k * 128 + lane * 4;
      if (k < nvec && col < c) {
        float4 o;
        o.x = st.y * (g[k].x - mg - xh[k].x * mgx);
        o.y = st.y * (g[k].y - mg - xh[k].y * mgx);
        o.z = st.y * (g[k].z - mg - xh[k].z * mgx);
        o.w = st.y * (g[k].w - mg - xh[k].w * mgx);
        *(float4*)(dx + row * c + col) = o;
      }
    }
  }
  // the row groups of the block add their column sums one after the other (a float atomicAdd into LDS made the order - and
  // the last bits of d(gamma), d(beta) - depend on the schedule)
  for (int turn = 0; turn < kLnRowsPerBlock; ++turn) {
    if (sub == turn) {
#pragma unroll
      for (int k = 0; k < kLnMaxVec; ++k) {
        const int col = k * 128 + lane * 4;
        if (k < nvec && col < c) {
          part[col + 0] += aw[k].x, part[col + 1] += aw[k].y, part[col + 2] += aw[k].z, part[col + 3] += aw[k].w;
          part[c + col + 0] += ab[k].x, part[c + col + 1] += ab[k].y, part[c + col + 2] += ab[k].z, part[c + col + 3] += ab[k].w;
        }
      }
    }
    __syncthreads();
  }
  // block partials [gridDim.x][2c]; reduced by colsum_partials_k (no global atomics, deterministic)
  float* dst = partials + (int64_t)blockIdx.x * 2 * c;
  for (int i = threadIdx.x; i < 2 * c; i += kLnThreads) dst[i] = part[i];
}

// out[i] = sum_b partials[b][i], i < width.  Block = 32 columns x 32 slices of the nb partial rows.
__global__ __launch_bounds__(1024) void colsum_partials_k(const float* __restrict__ partials, int nb, int width,
                                                          float* __restrict__ out0, float* __restrict__ out1,
                                                          int split) {
  __shared__ float red[32][33];
  const int cx = threadIdx.x & 31, gy = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + cx;
  float acc = 0.f;
  if (i < width)
    for (int b = gy; b < nb; b += 32) acc += partials[(int64_t)b * width + i];
  red[gy][cx] = acc;
  __syncthreads();
  if (gy == 0 && i < width) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) t += red[k][cx];
    if (i < split)
      out0[i] = t;
    else
      out1[i - split] = t;
  }
}

}  // namespace

// Loss arithmetic and fixed-order reductions shared by the five head files (seg_loss.hip, center_head.hip, cluster_head.hip,
// roi_head.hip, anchor_head.hip).  Every function here carries a numerical contract that the heads' tests pin:
// sums in one fixed order, so that two runs agree bit for bit; q = |t - p| with its relative accuracy kept at |z| = 60;
// correctly rounded square roots.  A change here reaches every head.
#pragma once
#include <math.h>
#include "common.h"
#include "exact_math.h"  // sst_sqrt_rn, the correctly rounded root (shared with the clustering kernels)

// the functions below round operation by operation whatever file includes them
#pragma clang fp contract(off)

namespace {

// Python's scalars rounded to fp32 once, as torch does with a Python scalar operand
constexpr float kPi = 3.14159265358979323846f;         // (float)np.pi
constexpr float kTwoPi = 6.28318530717958647692f;      // (float)(2 * np.pi)
constexpr float kHalfPi = 1.57079632679489661923f;     // (float)(np.pi / 2)
constexpr float kQuarterPi = 0.78539816339744830962f;  // (float)(np.pi / 4)

// ------------------------------------------------------------------------------------------------------------------
// fixed-order sums
// ------------------------------------------------------------------------------------------------------------------

// sum over the 64 lanes of a wave by a fixed shuffle tree; the result in lane 0
__device__ __forceinline__ double sst_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;  // lane 0: lanes added in a fixed tree
}

// sum over the workgroup in a fixed order (lanes by the shuffle tree, then the waves in index order); the result in thread 0.
// wsum: one double per wave in LDS; every thread of the workgroup must call (two barriers)
__device__ __forceinline__ double sst_block_sum(double v, double* wsum) {
  v = sst_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = wsum[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += wsum[w];
  return r;
}

// The double slots of a workgroup's partial record: thread d < kDoubles adds the lane-0 wave sums wsum[d][0 .. kWaves) in wave
// order and writes the bits to rec[d].  Call after the barrier that follows the writes of wsum; the integer slots behind the
// doubles are the calling kernel's own.
template <int kWaves, int kDoubles>
__device__ __forceinline__ void sst_write_record(double (*wsum)[kWaves], unsigned long long* rec) {
  const int d = threadIdx.x;
  if (d >= kDoubles) return;
  double v = wsum[d][0];
  for (int w = 1; w < kWaves; ++w) v += wsum[d][w];
  rec[d] = (unsigned long long)__double_as_longlong(v);
}

// ------------------------------------------------------------------------------------------------------------------
// elements of the losses
// ------------------------------------------------------------------------------------------------------------------

// p = sigmoid(z) and q = 1 - p, both formed from e = exp(-|z|) without a subtraction: sigmoid(|z|) = 1 / (1 + e) and its
// complement e * (1 / (1 + e)), handed out by the sign of z, so each keeps its relative accuracy at either end.  Returns e (the
// softplus of z is max(z, 0) + log1p(e)).
__device__ __forceinline__ float sst_sigmoid_pair(float z, float& p, float& q) {
  const float e = expf(-fabsf(z));
  const float hi = 1.f / (1.f + e), lo = e * hi;
  p = z >= 0.f ? hi : lo;
  q = z >= 0.f ? lo : hi;
  return e;
}

// q^gamma: products for gamma 0, 1, 2 and 3 (each product rounded once), powf for every other gamma
__device__ __forceinline__ float sst_pow_gamma(float q, float gamma) {
  if (gamma == 2.f) return q * q;
  if (gamma == 3.f) return q * q * q;
  if (gamma == 1.f) return q;
  if (gamma == 0.f) return 1.f;
  return powf(q, gamma);
}

// One element of the sigmoid focal loss at z with target t: the probability p, the loss term and its derivative in z.
//   e = (max(z, 0) - t z + log1p(exp(-|z|))) * (t ? alpha : 1 - alpha) * q^gamma,   q = |t - p|
// sigmoid(|z|) = 1 / (1 + exp(-|z|)) and its complement exp(-|z|) / (1 + exp(-|z|)) are formed without a subtraction, so
// q keeps its relative accuracy at |z| = 60.  With s = 1 - 2t: p - t = s q and dq/dz = s q (1 - q), hence
//   de/dz = (t ? alpha : 1 - alpha) * s * q^gamma * (q + gamma * bce * (1 - q)).
__device__ __forceinline__ void sst_focal_elem(float z, bool t, float alpha, float gamma, float& p, float& loss, float& dz) {
  float pc;
  const float e = sst_sigmoid_pair(z, p, pc);
  const float q = t ? pc : p, qc = t ? p : pc;
  const float bce = fmaxf(z, 0.f) - (t ? z : 0.f) + log1pf(e);
  const float aw = t ? alpha : 1.f - alpha;
  const float mod = sst_pow_gamma(q, gamma);
  loss = bce * aw * mod;
  dz = (t ? -aw : aw) * mod * (q + gamma * bce * qc);
}

// one regression element: |d| (L1Loss, beta == 0) or mmdet's smooth_l1_loss, 0.5 d^2 / beta below beta and |d| - 0.5 beta above
__device__ __forceinline__ float sst_reg_elem(float d, float beta) {
  const float ad = fabsf(d);
  return ad < beta ? 0.5f * ad * ad / beta : ad - 0.5f * beta;
}
// its derivative in d: d / beta below beta, sign(d) above (sign(0) = 0)
__device__ __forceinline__ float sst_reg_grad(float d, float beta) {
  return fabsf(d) < beta ? d / beta : d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// the [class][row] LDS image of the row kernels
// ------------------------------------------------------------------------------------------------------------------

// rows [r0, r0 + rows) of a [n, c] matrix -> the [class][row] LDS image of row stride kLd, by consecutive lanes of a workgroup of
// kThreads reading consecutive floats
template <int kThreads, int kLd>
__device__ __forceinline__ void sst_stage_rows(const float* __restrict__ src, int64_t r0, int rows, int c, float* img) {
  const float* base = src + r0 * c;
  const int total = rows * c;
  for (int i = threadIdx.x; i < total; i += kThreads) {
    const int r = i / c, k = i - r * c;
    img[k * kLd + r] = base[i];
  }
}

// floats of that image for c classes, rounded up to 16 bytes
template <int kLd>
__host__ __device__ __forceinline__ int sst_image_floats(int c) { return (c * kLd + 3) / 4 * 4; }

}  // namespace

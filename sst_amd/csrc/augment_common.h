// What the augmentation kernels of points share (augment.hip; tracklet_augment.hip): the
// per-sample transform, the shuffle key and the ownership of workgroups by samples.  ONE definition serves both files, so a
// row that goes through either leaves with the same bits.  Both are built without floating-point contraction (Makefile).
#pragma once
#include "common.h"

namespace sst_aug {

constexpr int kBlock = 256;

inline int sample_bits(int batch) {
  int bits = 1;
  while (bits < 31 && (1ll << bits) < batch) ++bits;
  return bits;
}

// the last sample whose first workgroup is <= b (samples without rows own no workgroup)
__device__ __forceinline__ int sample_of_block(const int32_t* __restrict__ block_offsets, int batch, int b) {
  int lo = 0, hi = batch;                              // first s with block_offsets[s] > b
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (block_offsets[mid] <= b) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

__device__ __forceinline__ uint32_t shuffle_key(uint64_t seed, uint32_t sample, uint32_t row) {
  uint64_t x = seed + 0x9E3779B97F4A7C15ull * ((((uint64_t)sample << 32) | row) + 1ull);
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (uint32_t)(x >> 32);
}

// flips, rotation, scale, translation of one point; -> inside the range (strict on all six bounds; a NaN fails)
__device__ __forceinline__ bool transform_point(const sst_augment_params& p, float& x, float& y, float& z) {
  if (p.flip_h) y = -y;
  if (p.flip_v) x = -x;
  if (p.rotate) {
    const float xr = __fadd_rn(__fmul_rn(x, p.cos), __fmul_rn(y, p.sin));
    const float yr = __fadd_rn(__fmul_rn(x, -p.sin), __fmul_rn(y, p.cos));
    x = xr;
    y = yr;
  }
  x = __fmul_rn(x, p.scale);
  y = __fmul_rn(y, p.scale);
  z = __fmul_rn(z, p.scale);
  x = __fadd_rn(x, p.trans[0]);
  y = __fadd_rn(y, p.trans[1]);
  z = __fadd_rn(z, p.trans[2]);
  return x > p.range[0] && y > p.range[1] && z > p.range[2] && x < p.range[3] && y < p.range[4] && z < p.range[5];
}

}  // namespace sst_aug

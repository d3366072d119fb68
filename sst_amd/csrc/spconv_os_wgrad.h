// What the output-stationary filter-gradient kernels share (sp_wgrad_os_k and sp_wgrad_os_x6_k of csrc/spconv_os.hip,
// sp_wgrad_os_bf16_k of csrc/spconv_os_bf16.hip): the stage length, the numbering of the chunk slots, and the swizzle of the bf16
// LDS images of the two kernels on v_mfma_f32_16x16x32_bf16.  The kernel bodies stay apart: they buffer differently on purpose.
#pragma once
#include "common.h"

namespace {

constexpr int kWgStage = 64;    // pairs per stage

// chunk slot (blockIdx.x) -> (offset k, first slot of that offset): offset i owns ceil(num[i] / csize) consecutive slots
__device__ __forceinline__ bool os_find_chunk(const int32_t* __restrict__ num, int kvol, int chunk, int csize, int& k,
                                              int& first) {
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

// bf16 image [64 channels][64 pairs] in 128-byte rows: 16-byte unit G of row r sits at G ^ f(r), f(r) = ((r >> 1) & 7) ^
// ((r >> 3) & 7) - the sixteen rows of a fragment read cover all 64 banks once, the sixteen channel blocks of a transposing
// write land two per 8-byte slot
__device__ __forceinline__ int os_wg_unit(int row, int G) { return (G ^ ((row >> 1) & 7) ^ ((row >> 3) & 7)) & 7; }

}  // namespace

// The ranking half of the foreground sampling kernels, shared by fg_sample.hip and fg_group_sample.hip (3.19):
// the workspace, the block counts of launch A, and launch B (the at-least-one-point rule and the scans).
#pragma once
#include "head_math.h"

namespace {

constexpr int kBlock = 256;             // lanes (points) per workgroup of the point kernels
constexpr int kWaves = kBlock / 64;
constexpr int kMaxClasses = SST_FG_MAX_CLASSES;
constexpr int kLdsTable = 8192;         // (C + 1) * B words of the LDS histogram; larger tables go to global atomics directly

// layout of the record the host reads (int32): totals[C] | rule[C] | class_off[C + 1] | status
__host__ __device__ inline int info_rule(int C) { return C; }
__host__ __device__ inline int info_off(int C) { return 2 * C; }
__host__ __device__ inline int info_status(int C) { return 3 * C + 1; }

struct Work {
  uint32_t* words;   // [n] the mask bits before the at-least-one rule
  int32_t* blk;      // [C][nb] selected points per block and class (launch B adds the rule's points)
  int32_t* blkoff;   // [C][nb] exclusive scan of blk
  int32_t* table;    // [C + 1][B] selected points per (class, sample); row C: points per sample.  + 1 status word.  Zeroed.
  int32_t* first;    // [B] index of the first point of every sample (batch_idx is non-decreasing)
  int32_t* rowpre;   // [B] sample-major layout: output rows of the samples in front
  int32_t* base;     // [C][B] sample-major layout: output row of (class, sample) minus the class rows in front of the sample
};

Work carve(void* ws, int64_t n, int C, int B) {
  const int64_t nb = sst_div_up(n, kBlock);
  sst_carver cv(ws);
  Work w;
  w.words = cv.take<uint32_t>(n);
  w.blk = cv.take<int32_t>(C * nb);
  w.blkoff = cv.take<int32_t>(C * nb);
  w.table = cv.take<int32_t>((int64_t)(C + 1) * B + 1);
  w.first = cv.take<int32_t>(B);
  w.rowpre = cv.take<int32_t>(B);
  w.base = cv.take<int32_t>((int64_t)C * B);
  return w;
}

__device__ __forceinline__ int64_t load_batch(const void* p, int is64, int64_t i) {
  return is64 ? ((const int64_t*)p)[i] : (int64_t)((const int32_t*)p)[i];
}

__device__ __forceinline__ int lanes_below(unsigned long long ballot) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// what launch B reads of an entry point's arguments (classes here are the groups of fg_group_sample.hip)
struct FgRule {
  int32_t* info;
  int32_t num_classes, batch, apply_rule, sample_major;
};

inline int64_t fg_workspace_bytes(int64_t n, int num_classes, int batch) {
  const int64_t nb = sst_div_up(n, kBlock);
  return sst_align_up(4 * (n > 0 ? n : 1), 256) + 2 * sst_align_up(4 * (num_classes * nb > 0 ? num_classes * nb : 1), 256) +
         sst_align_up(4 * ((int64_t)(num_classes + 1) * batch + 1), 256) + 2 * sst_align_up(4 * (int64_t)batch, 256) +
         sst_align_up(4 * (int64_t)num_classes * batch, 256);
}

// The counting half of launch A: word holds the mask bits of this lane's point, s its sample (-1: none).  Block counts by wave
// ballots into w.blk, the (class, sample) table and the points per sample (row C) into tab.
__device__ __forceinline__ void fg_block_counts(uint32_t word, int64_t s, bool active, int C, int B, int32_t* tab, const Work& w,
                                                int64_t nb, int32_t (*wcnt)[kWaves]) {
  const int wave = threadIdx.x >> 6, lane = sst_lane();
  // batch_idx is non-decreasing, so nearly every wave holds one sample: its counts are ballots and one add per class
  const long long s0 = __shfl((long long)s, 0, 64);     // the active lanes of a wave are a prefix: lane 0 is one, or none is
  const bool uniform = __ballot(active && s != s0) == 0ull;
  for (int c = 0; c < C; ++c) {
    const int cnt = __popcll(__ballot((word >> c) & 1u));
    if (lane == 0) wcnt[c][wave] = cnt;
    if (uniform) {
      if (lane == 0 && s0 >= 0 && cnt > 0) atomicAdd(&tab[c * B + (int)s0], cnt);
    } else if (s >= 0 && ((word >> c) & 1u)) {
      atomicAdd(&tab[c * B + (int)s], 1);
    }
  }
  if (uniform) {
    const int cnt = __popcll(__ballot(active));
    if (lane == 0 && s0 >= 0 && cnt > 0) atomicAdd(&tab[C * B + (int)s0], cnt);
  } else if (s >= 0) {
    atomicAdd(&tab[C * B + (int)s], 1);
  }
  __syncthreads();
  if ((int)threadIdx.x < C) {
    int t = 0;
    for (int v = 0; v < kWaves; ++v) t += wcnt[threadIdx.x][v];
    w.blk[(int64_t)threadIdx.x * nb + blockIdx.x] = t;
  }
}

// Launch B.  One workgroup: the rule per class, the counts of the blocks that hold a sample's first point, the scans.
__global__ __launch_bounds__(kBlock) void fg_rule_scan_kernel(FgRule a, Work w, int64_t nb) {
  __shared__ int32_t s_total[kMaxClasses];
  const int C = a.num_classes, B = a.batch;
  const int32_t* npts = w.table + (int64_t)C * B;
  if (threadIdx.x == 0) {                              // first point of every sample
    int run = 0;
    for (int s = 0; s < B; ++s) {
      w.first[s] = run;
      run += npts[s];
    }
  }
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    int last = -1;                                     // largest sample index present
    for (int s = 0; s < B; ++s)
      if (npts[s] > 0) last = s;
    bool rule = false;
    if (a.apply_rule)
      for (int s = 0; s <= last; ++s) rule = rule || w.table[c * B + s] == 0;
    a.info[info_rule(C) + c] = rule;
    if (rule) {
      int run = 0;
      for (int s = 0; s < B; ++s) {
        const int f = run;
        run += npts[s];
        if (npts[s] == 0) continue;
        if (!((w.words[f] >> c) & 1u)) {               // a first point already selected is not counted twice
          w.blk[(int64_t)c * nb + f / kBlock] += 1;
          w.table[c * B + s] += 1;
        }
      }
    }
  }
  __syncthreads();
  if (a.sample_major) {
    // rows sorted by sample, inside a sample class after class: (class c, sample s) starts at
    // rows of the samples in front + rows of the classes in front within s; base = that start - class rows in front of s
    for (int s = threadIdx.x; s < B; s += kBlock) {
      int t = 0;
      for (int c = 0; c < C; ++c) t += w.table[c * B + s];
      w.rowpre[s] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int run = 0;
      for (int s = 0; s < B; ++s) {
        const int t = w.rowpre[s];
        w.rowpre[s] = run;
        run += t;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
      const int c = threadIdx.x;
      int run = 0;
      for (int s = 0; s < B; ++s) {
        int front = w.rowpre[s];
        for (int k = 0; k < c; ++k) front += w.table[k * B + s];
        w.base[c * B + s] = front - run;
        run += w.table[c * B + s];
      }
    }
    __syncthreads();
  }
  // exclusive scan of the block counts: a wave per class, 64 blocks per step
  const int wave = threadIdx.x >> 6, lane = sst_lane();
  for (int c = wave; c < C; c += kWaves) {
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 64) {
      const int64_t b = b0 + lane;
      const int v = b < nb ? w.blk[(int64_t)c * nb + b] : 0;
      const int inc = sst_wave_incl_scan(v);
      if (b < nb) w.blkoff[(int64_t)c * nb + b] = carry + inc - v;
      carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) s_total[c] = carry;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int c = 0; c < C; ++c) {
      a.info[c] = s_total[c];
      a.info[info_off(C) + c] = run;
      run += s_total[c];
    }
    a.info[info_off(C) + C] = run;
    a.info[info_status(C)] = w.table[(int64_t)(C + 1) * B];
  }
}

}  // namespace

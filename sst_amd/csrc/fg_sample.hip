// FSD foreground sampling: the stage between the segmentor and the clustering, SingleStageFSD.sample /
// get_fg_mask / get_sample_beg_position / update_sample_results_by_mask / combine_classes of
// mmdet3d/models/detectors/single_stage_fsd.py:571-593, 698-797, as compaction kernels.  The reference runs a chain of boolean
// indexings (one nonzero, one device synchronisation each) per class and per tensor; here the masks of all classes are one
// 32-bit word per point, the rows of a class are ranked by wave ballots and a scan of per-block counts, and the host reads
// one small record.  No workgroup waits on another inside a launch; every count is an integer, so no sum depends on order.
#include "fg_rank.h"

namespace {

// Launch A.  One lane per point: the C mask bits, the block counts by wave ballots, the (class, sample) table.
__global__ __launch_bounds__(kBlock) void fg_mask_count_kernel(sst_fg_sample_args a, Work w, int64_t nb, int lds_table) {
  extern __shared__ int32_t hist[];                    // [(C + 1) * B] when lds_table
  __shared__ int32_t wcnt[kMaxClasses][kWaves];
  const int C = a.num_classes, B = a.batch;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool active = i < a.n;
  if (lds_table) {
    for (int k = threadIdx.x; k < (C + 1) * B; k += kBlock) hist[k] = 0;
    __syncthreads();
  }
  int32_t* tab = lds_table ? hist : w.table;

  uint32_t word = 0;
  int64_t s = -1;
  if (active) {
    s = load_batch(a.batch_idx, a.batch_is_i64, i);
    if (s < 0 || s >= B) {                             // outside the table: counted nowhere, reported in the status word
      s = -1;
      atomicOr(&w.table[(int64_t)(C + 1) * B], 1);
    }
    for (int c = 0; c < C; ++c) {
      bool bit = false;
      if (a.logits != nullptr) {
        float p, q;
        sst_sigmoid_pair(a.logits[i * a.ld_logits + c], p, q);
        bit = p > a.thresholds[c];
      }
      if (a.extra_mask != nullptr) bit = bit || a.extra_mask[(int64_t)c * a.n + i] != 0;
      word |= (uint32_t)bit << c;
    }
    w.words[i] = word;
  }
  fg_block_counts(word, s, active, C, B, tab, w, nb, wcnt);
  if (lds_table)
    for (int k = threadIdx.x; k < (C + 1) * B; k += kBlock)
      if (hist[k] != 0) atomicAdd(&w.table[k], hist[k]);
}

// Launch C.  One lane per point: the final bits, the row of every selected point, the narrow per-class rows.
__global__ __launch_bounds__(kBlock) void fg_compact_kernel(sst_fg_sample_args a, Work w, int64_t nb) {
  __shared__ int32_t wcnt[kMaxClasses][kWaves];
  const int C = a.num_classes, B = a.batch;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool active = i < a.n;
  const int wave = threadIdx.x >> 6, lane = sst_lane();
  uint32_t word = 0;
  int64_t s = -1;
  if (active) {
    word = w.words[i];
    s = load_batch(a.batch_idx, a.batch_is_i64, i);
    if (s >= 0 && s < B && (int64_t)w.first[s] == i) {
      uint32_t rules = 0;
      for (int c = 0; c < C; ++c) rules |= (uint32_t)(a.info[info_rule(C) + c] != 0) << c;
      word |= rules;
    }
  }
  for (int c = 0; c < C; ++c) {
    const int cnt = __popcll(__ballot((word >> c) & 1u));
    if (lane == 0) wcnt[c][wave] = cnt;
  }
  __syncthreads();
  for (int c = 0; c < C; ++c) {
    const bool bit = (word >> c) & 1u;
    const int rank = lanes_below(__ballot(bit));
    if (!active) continue;
    int row = -1;
    if (bit) {
      row = w.blkoff[(int64_t)c * nb + blockIdx.x] + rank;
      for (int v = 0; v < wave; ++v) row += wcnt[c][v];
    }
    // the output row: class after class, or (sample_major) sample after sample and class after class inside a sample
    int64_t g = -1;
    if (bit) {
      if (!a.sample_major) g = (int64_t)a.info[info_off(C) + c] + row;
      else if (s >= 0 && s < B) g = (int64_t)w.base[c * B + (int)s] + row;
      if (g >= a.max_rows) g = -1;                      // a caller's row count that the masks exceed: nothing is written there
    }
    a.slot[(int64_t)c * a.n + i] = a.sample_major ? (int32_t)g : row;
    a.mask[(int64_t)c * a.n + i] = bit;
    if (g < 0) continue;
    a.src[g] = (int32_t)i;
    if (a.aux != nullptr) {
      const int32_t x = a.aux[(int64_t)c * a.n + i];
      a.aux_out[g] = x;
      if (x >= 0 && x < a.aux_rows) a.aux_inv[x] = (int32_t)g;
    }
    if (a.centers != nullptr)
      for (int k = 0; k < 3; ++k) a.centers[g * 3 + k] = a.points[i * a.ld_points + k] + a.votes[i * a.ld_votes + 3 * c + k];
    if (a.batch_out != nullptr) {
      if (a.batch_is_i64) ((int64_t*)a.batch_out)[g] = s;
      else ((int32_t*)a.batch_out)[g] = (int32_t)s;
    }
    if (a.points_out != nullptr)
      for (int k = 0; k < a.point_cols; ++k) a.points_out[g * a.point_cols + k] = a.points[i * a.ld_points + k];
  }
}

struct KeepOffsets {
  int64_t off[kMaxClasses + 1];
};

// slot2[c][i]: the row of point i, class c in the output of the cluster filter (keep: ascending rows of each class that
// stay, class after class), or -1; the final masks.  A binary search per (class, point): every element is written.
__global__ __launch_bounds__(kBlock) void fg_slot2_kernel(const int32_t* __restrict__ slot, int64_t n, int C,
                                                           const int64_t* __restrict__ keep, KeepOffsets ko,
                                                           int32_t* __restrict__ slot2, uint8_t* __restrict__ fmask) {
  const int64_t total = n * C;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int c = (int)(e / n);
    const int64_t r = slot[e];
    int64_t out = -1;
    if (r >= 0) {
      int64_t lo = ko.off[c], hi = ko.off[c + 1];       // first position with keep >= r
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keep[mid] < r) lo = mid + 1;
        else hi = mid;
      }
      if (lo < ko.off[c + 1] && keep[lo] == r) out = lo;
    }
    slot2[e] = (int32_t)out;
    fmask[e] = out >= 0;
  }
}

// out[j] = (logits[idx[j]] | votes[idx[j]] | feats[idx[j]]), points_out[j] = points[idx[j]]: consecutive lanes write consecutive
// floats of the output; a row is never read past its width
__global__ __launch_bounds__(kBlock) void fg_gather_cat_fwd_kernel(sst_fg_gather_args g) {
  const int64_t w = (int64_t)g.c_logits + g.c_votes + g.c_feats;
  const int64_t wide = g.m * w, total = wide + g.m * g.c_points;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    if (e < wide) {
      const int64_t j = e / w;
      int k = (int)(e - j * w);
      const int64_t i = g.idx[j];
      float v;
      if (i < 0 || i >= g.n) v = 0.f;                   // an index outside the source rows reads nothing
      else if (k < g.c_logits) v = g.logits[i * g.ld_logits + k];
      else if ((k -= g.c_logits) < g.c_votes) v = g.votes[i * g.ld_votes + k];
      else v = g.feats[i * g.ld_feats + (k - g.c_votes)];
      g.out[e] = v;
    } else {
      const int64_t e2 = e - wide, j = e2 / g.c_points;
      const int k = (int)(e2 - j * g.c_points);
      const int64_t i = g.idx[j];
      g.points_out[e2] = i < 0 || i >= g.n ? 0.f : g.points[i * g.ld_points + k];
    }
  }
}

// RoI input rows: out[g] = (cluster_feats[row[g]] or zeros where row[g] < 0 | seg_feats[src[g]]); src == NULL: src[g] = g
__global__ __launch_bounds__(kBlock) void fg_roi_cat_fwd_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ row,
                                                                 int64_t rows, int64_t n, int64_t m,
                                                                 const float* __restrict__ cluster, int64_t ld_cluster, int fc, const float* __restrict__ feats, int64_t ld_feats, int f,
                                                                 float* __restrict__ out) {
  const int64_t w = (int64_t)fc + f, total = rows * w;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t g = e / w;
    const int k = (int)(e - g * w);
    float v;
    if (k < fc) {
      const int r = row[g];
      v = r >= 0 && r < m ? cluster[(int64_t)r * ld_cluster + k] : 0.f;
    } else {
      const int64_t i = src != nullptr ? (int64_t)src[g] : g;
      v = i >= 0 && i < n ? feats[i * ld_feats + (k - fc)] : 0.f;   // a row the masks did not fill names no point
    }
    out[e] = v;
  }
}

// d_feats[i][f] = sum over the classes, ascending, of d_out[slot2[c][i]][col0 + f]; rows of no class get zeros.  Every element
// is written once: no memset, no float atomic, one order of the additions.
__global__ __launch_bounds__(kBlock) void fg_gather_cat_bwd_kernel(const float* __restrict__ d_out, int64_t rows, int64_t ld_out, int col0,
                                                                    const int32_t* __restrict__ slot2, int64_t n, int C, int F,
                                                                    float* __restrict__ d_feats) {
  const int64_t total = n * F;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t i = e / F;
    const int f = (int)(e - i * F);
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
      const int r = slot2[(int64_t)c * n + i];
      if (r >= 0 && r < rows) acc += d_out[(int64_t)r * ld_out + col0 + f];
    }
    d_feats[e] = acc;
  }
}

}  // namespace

extern "C" {

int64_t sst_fg_sample_workspace_bytes(int64_t n, int num_classes, int batch) {
  if (n < 0 || num_classes < 1 || num_classes > kMaxClasses || batch < 1) return 0;
  return fg_workspace_bytes(n, num_classes, batch);
}

int sst_fg_sample_info_words(int num_classes) { return 3 * num_classes + 2; }

int sst_fg_sample_f32(const sst_fg_sample_args* args, void* d_workspace, void* stream) {
  if (args == nullptr || d_workspace == nullptr) return SST_ERR_ARG;
  const sst_fg_sample_args& a = *args;
  if (a.num_classes < 1 || a.num_classes > kMaxClasses) return SST_ERR_UNSUPPORTED;
  if (a.n < 1 || a.n > (int64_t)INT32_MAX - kBlock || a.batch < 1 || a.batch_idx == nullptr || a.slot == nullptr ||
      a.mask == nullptr || a.src == nullptr || a.info == nullptr)
    return SST_ERR_ARG;
  if (a.logits == nullptr && a.extra_mask == nullptr) return SST_ERR_ARG;
  if (a.logits != nullptr && a.ld_logits < a.num_classes) return SST_ERR_ARG;
  if (a.centers != nullptr && (a.points == nullptr || a.votes == nullptr || a.ld_points < 3 || a.ld_votes < 3 * a.num_classes))
    return SST_ERR_ARG;
  if (a.points_out != nullptr && (a.points == nullptr || a.point_cols < 1 || a.ld_points < a.point_cols)) return SST_ERR_ARG;
  if (a.max_rows < 0 || (a.aux != nullptr && (a.aux_out == nullptr || a.aux_rows < 0 || (a.aux_rows > 0 && a.aux_inv == nullptr)))) return SST_ERR_ARG;
  const int C = a.num_classes, B = a.batch;
  const int64_t nb = sst_div_up(a.n, kBlock);
  const Work w = carve(d_workspace, a.n, C, B);
  hipStream_t st = (hipStream_t)stream;
  const int64_t table_words = (int64_t)(C + 1) * B;
  SST_HIP(hipMemsetAsync(w.table, 0, 4 * (table_words + 1), st));
  const int lds_table = table_words <= kLdsTable;
  hipLaunchKernelGGL(fg_mask_count_kernel, dim3((unsigned)nb), dim3(kBlock), lds_table ? 4 * table_words : 0, st, a, w, nb,
                     lds_table);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(fg_rule_scan_kernel, dim3(1), dim3(kBlock), 0, st, FgRule{a.info, C, B, a.apply_rule, a.sample_major}, w,
                     nb);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(fg_compact_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, a, w, nb);
  SST_LAUNCH_CHECK();
  return 0;
}

int sst_fg_slot2_i32(const int32_t* d_slot, int64_t n, int num_classes, const int64_t* d_keep, const int64_t* keep_offsets,
                     int32_t* d_slot2, uint8_t* d_final_mask, void* stream) {
  if (num_classes < 1 || num_classes > kMaxClasses) return SST_ERR_UNSUPPORTED;
  if (n < 0 || keep_offsets == nullptr) return SST_ERR_ARG;
  if (n == 0) return 0;
  if (d_slot == nullptr || d_slot2 == nullptr || d_final_mask == nullptr) return SST_ERR_ARG;
  KeepOffsets ko;
  for (int c = 0; c <= num_classes; ++c) {
    ko.off[c] = keep_offsets[c];
    if (ko.off[c] < 0 || (c > 0 && ko.off[c] < ko.off[c - 1])) return SST_ERR_ARG;
  }
  if (ko.off[0] != 0 || ko.off[num_classes] > INT32_MAX || (ko.off[num_classes] > 0 && d_keep == nullptr)) return SST_ERR_ARG;
  hipLaunchKernelGGL(fg_slot2_kernel, dim3(sst_grid_1d(n * num_classes, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, d_slot,
                     n, num_classes, d_keep, ko, d_slot2, d_final_mask);
  SST_LAUNCH_CHECK();
  return 0;
}

int sst_fg_gather_cat_fwd_f32(const sst_fg_gather_args* args, void* stream) {
  if (args == nullptr) return SST_ERR_ARG;
  const sst_fg_gather_args& g = *args;
  if (g.m < 0 || g.n < 0 || g.c_logits < 0 || g.c_votes < 0 || g.c_feats < 0 || g.c_points < 0) return SST_ERR_ARG;
  if (g.m == 0) return 0;
  const int64_t w = (int64_t)g.c_logits + g.c_votes + g.c_feats;
  if (g.idx == nullptr || (w > 0 && g.out == nullptr) || (g.c_points > 0 && (g.points == nullptr || g.points_out == nullptr)))
    return SST_ERR_ARG;
  if ((g.c_logits > 0 && (g.logits == nullptr || g.ld_logits < g.c_logits)) ||
      (g.c_votes > 0 && (g.votes == nullptr || g.ld_votes < g.c_votes)) ||
      (g.c_feats > 0 && (g.feats == nullptr || g.ld_feats < g.c_feats)) || (g.c_points > 0 && g.ld_points < g.c_points))
    return SST_ERR_ARG;
  const int64_t total = g.m * (w + g.c_points);
  if (total == 0) return 0;
  hipLaunchKernelGGL(fg_gather_cat_fwd_kernel, dim3(sst_grid_1d(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, g);
  SST_LAUNCH_CHECK();
  return 0;
}

int sst_fg_roi_cat_fwd_f32(const int32_t* d_src, const int32_t* d_row, int64_t rows, int64_t n_points, int64_t n_cluster,
                           const float* d_cluster_feats, int64_t ld_cluster, int cluster_cols, const float* d_seg_feats,
                           int64_t ld_feats, int feat_cols, float* d_out, void* stream) {
  if (rows < 0 || n_points < 0 || n_cluster < 0 || (d_src == nullptr && rows > n_points) || cluster_cols < 0 || feat_cols < 0 || ld_cluster < cluster_cols || ld_feats < feat_cols) return SST_ERR_ARG;
  const int64_t total = rows * ((int64_t)cluster_cols + feat_cols);
  if (total == 0) return 0;
  if (d_out == nullptr || (cluster_cols > 0 && d_row == nullptr) || (feat_cols > 0 && d_seg_feats == nullptr)) return SST_ERR_ARG;
  hipLaunchKernelGGL(fg_roi_cat_fwd_kernel, dim3(sst_grid_1d(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, d_src, d_row,
                     rows, n_points, n_cluster, d_cluster_feats, ld_cluster, cluster_cols, d_seg_feats, ld_feats, feat_cols, d_out);
  SST_LAUNCH_CHECK();
  return 0;
}

int sst_fg_gather_cat_bwd_f32(const float* d_out_grad, int64_t rows, int64_t ld_out, int col0, const int32_t* d_slot2, int64_t n,
                              int num_classes, int feat_cols, float* d_feats_grad, void* stream) {
  if (num_classes < 1 || num_classes > kMaxClasses) return SST_ERR_UNSUPPORTED;
  if (n < 0 || rows < 0 || feat_cols < 0 || col0 < 0 || ld_out < (int64_t)col0 + feat_cols) return SST_ERR_ARG;
  if (n == 0 || feat_cols == 0) return 0;
  if (d_slot2 == nullptr || d_feats_grad == nullptr) return SST_ERR_ARG;   // d_out_grad may be NULL only if no slot is >= 0
  hipLaunchKernelGGL(fg_gather_cat_bwd_kernel, dim3(sst_grid_1d(n * feat_cols, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     d_out_grad, rows, ld_out, col0, d_slot2, n, num_classes, feat_cols, d_feats_grad);
  SST_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

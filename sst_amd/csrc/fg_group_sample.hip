// FSDv2 grouped foreground sampling: the stage between the segmentor and the virtual voxels,
// SingleStageFSDV2.batched_group_sample / group_sample / get_fg_mask / gather_group_by_names / get_offset_weight of
// mmdet3d/models/detectors/single_stage_fsd_v2.py:662-891, in the three launches of fg_sample.hip (fg_rank.h): the softmax
// scores of a point are summed per class group and compared in launch A, launch B is the shared rule and scan, launch C votes
// the centre of every selected (group, point) with the 'max' offset weights and writes the narrow rows.  Then the input rows of
// the virtual-point projector (SingleStageFSDV2.extract_feat :164-176) as one gather, and its gradient in a fixed order.
#include "fg_rank.h"

// every product, sum and division of this file is an IEEE operation of its own, as the reference's tensor operations are
#pragma clang fp contract(off)

namespace {

// Launch A.  One lane per point: softmax over the K logits, the G group scores, the mask bits, the counts.
__global__ __launch_bounds__(kBlock) void fg_group_mask_count_kernel(sst_fg_group_sample_args a, Work w, int64_t nb, int lds_table) {
  extern __shared__ int32_t hist[];                    // [(G + 1) * B] when lds_table
  __shared__ int32_t wcnt[kMaxClasses][kWaves];
  const int G = a.num_groups, B = a.batch, K = a.num_logits;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool active = i < a.n;
  if (lds_table) {
    for (int k = threadIdx.x; k < (G + 1) * B; k += kBlock) hist[k] = 0;
    __syncthreads();
  }
  int32_t* tab = lds_table ? hist : w.table;

  uint32_t word = 0;
  int64_t s = -1;
  if (active) {
    s = load_batch(a.batch_idx, a.batch_is_i64, i);
    if (s < 0 || s >= B) {                             // outside the table: counted nowhere, reported in the status word
      s = -1;
      atomicOr(&w.table[(int64_t)(G + 1) * B], 1);
    }
    if (a.logits != nullptr) {
      // the row is read three times (44 bytes at K = 11, held by the cache): no register array indexed by the class
      const float* row = a.logits + i * a.ld_logits;
      float top = row[0];
      for (int k = 1; k < K; ++k) top = fmaxf(top, row[k]);
      float denom = 0.f;
      for (int k = 0; k < K; ++k) denom += expf(row[k] - top);
      for (int g = 0; g < G; ++g) {
        float score = 0.f;
        for (int j = a.group_begin[g]; j < a.group_begin[g + 1]; ++j) score += expf(row[a.group_class[j]] - top) / denom;
        word |= (uint32_t)(score > a.thresholds[g]) << g;      // +inf: never
      }
    }
    if (a.extra_mask != nullptr)
      for (int g = 0; g < G; ++g) word |= (uint32_t)(a.extra_mask[(int64_t)g * a.n + i] != 0) << g;
    w.words[i] = word;
  }
  fg_block_counts(word, s, active, G, B, tab, w, nb, wcnt);
  if (lds_table)
    for (int k = threadIdx.x; k < (G + 1) * B; k += kBlock)
      if (hist[k] != 0) atomicAdd(&w.table[k], hist[k]);
}

// Launch C.  One lane per point: the final bits, the row of every selected (group, point), the voted centre, the narrow rows.
__global__ __launch_bounds__(kBlock) void fg_group_compact_kernel(sst_fg_group_sample_args a, Work w, int64_t nb) {
  __shared__ int32_t wcnt[kMaxClasses][kWaves];
  const int G = a.num_groups, B = a.batch;
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
      for (int g = 0; g < G; ++g) rules |= (uint32_t)(a.info[info_rule(G) + g] != 0) << g;
      word |= rules;
    }
  }
  for (int g = 0; g < G; ++g) {
    const int cnt = __popcll(__ballot((word >> g) & 1u));
    if (lane == 0) wcnt[g][wave] = cnt;
  }
  __syncthreads();
  for (int g = 0; g < G; ++g) {
    const bool bit = (word >> g) & 1u;
    const int rank = lanes_below(__ballot(bit));
    if (!active) continue;
    int row = -1;
    if (bit) {
      row = w.blkoff[(int64_t)g * nb + blockIdx.x] + rank;
      for (int v = 0; v < wave; ++v) row += wcnt[g][v];
    }
    int64_t r = -1;
    if (bit) {
      r = (int64_t)a.info[info_off(G) + g] + row;
      if (r >= a.max_rows) r = -1;                      // a caller's row count that the masks exceed: nothing is written there
    }
    a.slot[(int64_t)g * a.n + i] = row;
    a.mask[(int64_t)g * a.n + i] = bit;
    if (r < 0) continue;
    a.src[r] = (int32_t)i;
    if (a.centers != nullptr) {
      // get_offset_weight 'max' (:855-861): weight 1 / count on every class of the group whose logit is within 1e-6 of the
      // group's maximum; the offset is the weighted sum in listed order (:837), the centre p + scale * offset (:839)
      const float* row_l = a.logits + i * a.ld_logits;
      const float* row_v = a.votes + i * a.ld_votes;
      const int j0 = a.group_begin[g], j1 = a.group_begin[g + 1];
      float top = row_l[a.group_class[j0]];
      for (int j = j0 + 1; j < j1; ++j) top = fmaxf(top, row_l[a.group_class[j]]);
      int count = 0;
      for (int j = j0; j < j1; ++j) count += fabsf(row_l[a.group_class[j]] - top) < 1e-6f;
      const float wt = 1.0f / (float)count;
      float off[3] = {0.f, 0.f, 0.f};
      for (int j = j0; j < j1; ++j) {
        const int k = a.group_class[j];
        const float wk = fabsf(row_l[k] - top) < 1e-6f ? wt : 0.f;
        for (int d = 0; d < 3; ++d) off[d] += row_v[3 * k + d] * wk;
      }
      for (int d = 0; d < 3; ++d) a.centers[r * 3 + d] = a.points[i * a.ld_points + d] + a.offset_scale * off[d];
    }
    if (a.batch_out != nullptr) {
      if (a.batch_is_i64) ((int64_t*)a.batch_out)[r] = s;
      else ((int32_t*)a.batch_out)[r] = (int32_t)s;
    }
    if (a.points_out != nullptr)
      for (int k = 0; k < a.point_cols; ++k) a.points_out[r * a.point_cols + k] = a.points[i * a.ld_points + k];
  }
}

// out[j] = (feats[i] | (clip(centre[j]) - xyz[i]) / 10 | logits[i] | points[i][3:]) with i = src[j]; clipped[j] = clip(centre[j]).
// The division is what `tensor / 10` is on the device: torch's GPU kernel for a scalar divisor multiplies by the float32
// reciprocal (one rounding of 1 / 10, one of the product), and the rows must equal extract_feat's own concatenation bit for bit.
// Consecutive lanes write consecutive floats of the output; a row is never read past its width.
__global__ __launch_bounds__(kBlock) void fg_virtual_rows_fwd_kernel(sst_fg_virtual_rows_args v) {
  const int extra = v.c_points - 3;
  const int64_t w = (int64_t)v.c_feats + 3 + v.c_logits + extra, total = v.m * w;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t j = e / w;
    int k = (int)(e - j * w);
    const int64_t i = v.src[j];
    const bool inside = i >= 0 && i < v.n;             // an index outside the source rows reads nothing
    float val;
    if (k < v.c_feats) {
      val = inside ? v.feats[i * v.ld_feats + k] : 0.f;
    } else if ((k -= v.c_feats) < 3) {
      const float c = fminf(fmaxf(v.centers[j * 3 + k], v.lo[k]), v.hi[k]);
      v.clipped[j * 3 + k] = c;
      val = inside ? (c - v.points[i * v.ld_points + k]) * (1.0f / 10.0f) : 0.f;
    } else if ((k -= 3) < v.c_logits) {
      val = inside ? v.logits[i * v.ld_logits + k] : 0.f;
    } else {
      val = inside ? v.points[i * v.ld_points + 3 + (k - v.c_logits)] : 0.f;
    }
    v.out[e] = val;
  }
}

// d_feats[i][f] = sum over the groups, ascending, of d_out[off[g] + slot[g][i]][f]; rows of no group get zeros.  Every element is
// written once: no memset, no float atomic, one order of the additions.
__global__ __launch_bounds__(kBlock) void fg_virtual_rows_bwd_kernel(const float* __restrict__ d_out, int64_t rows, int64_t ld_out,
                                                                      const int32_t* __restrict__ slot, sst_fg_group_offsets off,
                                                                      int64_t n, int G, int F, float* __restrict__ d_feats) {
  const int64_t total = n * F;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t i = e / F;
    const int f = (int)(e - i * F);
    float acc = 0.f;
    for (int g = 0; g < G; ++g) {
      const int r = slot[(int64_t)g * n + i];
      const int64_t q = off.off[g] + r;
      if (r >= 0 && q < off.off[g + 1] && q < rows) acc += d_out[q * ld_out + f];
    }
    d_feats[e] = acc;
  }
}

}  // namespace

extern "C" {

int64_t sst_fg_group_sample_workspace_bytes(int64_t n, int num_groups, int batch) {
  if (n < 0 || num_groups < 1 || num_groups > kMaxClasses || batch < 1) return 0;
  return fg_workspace_bytes(n, num_groups, batch);
}

int sst_fg_group_sample_f32(const sst_fg_group_sample_args* args, void* d_workspace, void* stream) {
  if (args == nullptr || d_workspace == nullptr) return SST_ERR_ARG;
  const sst_fg_group_sample_args& a = *args;
  if (a.num_groups < 1 || a.num_groups > kMaxClasses || a.num_logits < 1 || a.num_logits > SST_FG_MAX_LOGITS) return SST_ERR_UNSUPPORTED;
  if (a.n < 1 || a.n > (int64_t)INT32_MAX - kBlock || a.batch < 1 || a.batch_idx == nullptr || a.slot == nullptr ||
      a.mask == nullptr || a.src == nullptr || a.info == nullptr)
    return SST_ERR_ARG;
  if (a.logits == nullptr && (a.extra_mask == nullptr || a.centers != nullptr)) return SST_ERR_ARG;
  if (a.logits != nullptr && a.ld_logits < a.num_logits) return SST_ERR_ARG;
  // the group lists: non-empty, inside the logit columns, no class twice (a class of two groups is refused by name in Python)
  if (a.group_begin[0] != 0) return SST_ERR_ARG;
  uint64_t seen = 0;
  for (int g = 0; g < a.num_groups; ++g) {
    if (a.group_begin[g + 1] <= a.group_begin[g] || a.group_begin[g + 1] > SST_FG_MAX_LOGITS) return SST_ERR_ARG;
    for (int j = a.group_begin[g]; j < a.group_begin[g + 1]; ++j) {
      const int k = a.group_class[j];
      if (k >= a.num_logits || ((seen >> k) & 1ull)) return SST_ERR_ARG;
      seen |= 1ull << k;
    }
  }
  if (a.centers != nullptr && (a.points == nullptr || a.votes == nullptr || a.ld_points < 3 || a.ld_votes < 3 * (int64_t)a.num_logits))
    return SST_ERR_ARG;
  if (a.points_out != nullptr && (a.points == nullptr || a.point_cols < 1 || a.ld_points < a.point_cols)) return SST_ERR_ARG;
  if (a.max_rows < 0) return SST_ERR_ARG;
  const int G = a.num_groups, B = a.batch;
  const int64_t nb = sst_div_up(a.n, kBlock);
  const Work w = carve(d_workspace, a.n, G, B);
  hipStream_t st = (hipStream_t)stream;
  const int64_t table_words = (int64_t)(G + 1) * B;
  SST_HIP(hipMemsetAsync(w.table, 0, 4 * (table_words + 1), st));
  const int lds_table = table_words <= kLdsTable;
  hipLaunchKernelGGL(fg_group_mask_count_kernel, dim3((unsigned)nb), dim3(kBlock), lds_table ? 4 * table_words : 0, st, a, w, nb,
                     lds_table);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(fg_rule_scan_kernel, dim3(1), dim3(kBlock), 0, st, FgRule{a.info, G, B, a.apply_rule, 0}, w, nb);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(fg_group_compact_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, a, w, nb);
  SST_LAUNCH_CHECK();
  return 0;
}

int sst_fg_virtual_rows_fwd_f32(const sst_fg_virtual_rows_args* args, void* stream) {
  if (args == nullptr) return SST_ERR_ARG;
  const sst_fg_virtual_rows_args& v = *args;
  if (v.m < 0 || v.n < 0 || v.c_feats < 0 || v.c_logits < 0 || v.c_points < 3) return SST_ERR_ARG;
  if (v.m == 0) return 0;
  if (v.src == nullptr || v.centers == nullptr || v.points == nullptr || v.out == nullptr || v.clipped == nullptr ||
      v.ld_points < v.c_points || (v.c_feats > 0 && (v.feats == nullptr || v.ld_feats < v.c_feats)) ||
      (v.c_logits > 0 && (v.logits == nullptr || v.ld_logits < v.c_logits)))
    return SST_ERR_ARG;
  const int64_t total = v.m * ((int64_t)v.c_feats + v.c_logits + v.c_points);
  hipLaunchKernelGGL(fg_virtual_rows_fwd_kernel, dim3(sst_grid_1d(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, v);
  SST_LAUNCH_CHECK();
  return 0;
}

int sst_fg_virtual_rows_bwd_f32(const float* d_out_grad, int64_t rows, int64_t ld_out, const int32_t* d_slot,
                                const sst_fg_group_offsets* offsets, int64_t n, int num_groups, int feat_cols, float* d_feats_grad,
                                void* stream) {
  if (num_groups < 1 || num_groups > kMaxClasses) return SST_ERR_UNSUPPORTED;
  if (offsets == nullptr || n < 0 || rows < 0 || feat_cols < 0 || ld_out < feat_cols) return SST_ERR_ARG;
  for (int g = 0; g <= num_groups; ++g)
    if (offsets->off[g] < 0 || (g > 0 && offsets->off[g] < offsets->off[g - 1])) return SST_ERR_ARG;
  if (n == 0 || feat_cols == 0) return 0;
  if (d_slot == nullptr || d_feats_grad == nullptr || (rows > 0 && d_out_grad == nullptr)) return SST_ERR_ARG;
  hipLaunchKernelGGL(fg_virtual_rows_bwd_kernel, dim3(sst_grid_1d(n * feat_cols, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     d_out_grad, rows, ld_out, d_slot, *offsets, n, num_groups, feat_cols, d_feats_grad);
  SST_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

// Training side of VoteSegHead: the point targets of a whole batch in one launch, and the decode loss, the vote loss and the
// logged statistics in two launches forward and one backward.  fp32 data, no float atomics, no host read-back, bit-reproducible.
//
// Reference (mmdet3d/models/decode_heads/segmentation_head.py):
//   sst_seg_targets_f32    get_targets :212-249 (the per-sample loop, the label >= 0 filter, enlarged_box_hw of
//                          core/bbox/structures/lidar_box3d.py:331-346, points_in_boxes), get_point_labels :252-258,
//                          get_vote_target :260-272 (gravity_center or a given centre), encode_vote_targets :274-275
//   sst_seg_loss_fwd_f32   losses :106-173: loss_decode, the class gather of the vote predictions :122-140, loss_vote, the
//                          recall / num_fg statistics :146-171 (gather_group_by_names :198-210); the asserts :124-126 and
//                          :134-135 become the status word
//   sst_seg_loss_bwd_f32   what autograd derives from the above
//
// PARITY.  Targets: the membership test is dpp_box / dpp_classify of pib_test.h (pinned to the reference's compiled
// points_in_boxes_cpu); every later operation is rounded once, the root correctly (through fp64), so the targets equal a float32 restatement
// bit for bit (tests/seg_loss_ref.py) and the reference's own methods to 1 ulp (torch's CPU sqrt / pow(0.5) is itself off by one
// ulp on some inputs).  Losses: mmdet / mmcv / mmseg, whose FocalLoss, L1Loss and CrossEntropyLoss the reference builds, are
// not part of the reference tree.  The focal formula is the tree's own py_sigmoid_focal_loss
// (mmdet3d/models/losses/focal_loss.py:13-67) with reduction 'mean'; cross entropy and L1 are torch's functions; the division
// by N (not by the sum of the class weights) in cross-entropy mode is mmseg's documented behaviour and is unpinned beyond that.
// Checked against the reference's methods run from their source text (tests/golden/seg_head_train.npz).
#include "common.h"
#include "head_math.h"
#include "pib_test.h"

namespace {

constexpr int kSegThreads = 256;
constexpr int kSegBoxTile = 256;    // boxes per LDS tile of the targets kernel (256 x 48 B)
constexpr int kLossSub = 256;       // rows per pass of a workgroup: one row per thread
constexpr int kLossTileRows = 1024; // rows per workgroup of the forward's first launch
constexpr int kLossLd = kLossSub + 1;  // row stride of the [class][row] LDS image: class c of row r on bank (c + r) % 32
constexpr int kMaxClasses = 32;
constexpr int kFinalRows = 64;      // partial records per LDS chunk of the finishing launch

// ------------------------------------------------------------------------------------------------------------------
// targets
// ------------------------------------------------------------------------------------------------------------------

// sample of point p: the s with off[s] <= p < off[s + 1] (empty samples are skipped over), or -1
__device__ __forceinline__ int sample_of(const int32_t* __restrict__ off, int batch, int64_t p) {
  if (p < off[0] || p >= off[batch]) return -1;
  int lo = 0, hi = batch;  // off[lo] <= p < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kSegThreads) void seg_targets_k(
    const float* __restrict__ pts, int64_t ld, int64_t n, const int32_t* __restrict__ pt_off, int batch,
    const float* __restrict__ boxes, const int64_t* __restrict__ box_labels, const int32_t* __restrict__ box_off,
    int64_t n_boxes, float ew, int64_t bg_label, const float* __restrict__ centers, int32_t* __restrict__ inbox,
    int64_t* __restrict__ labels, float* __restrict__ vote_targets, uint8_t* __restrict__ vote_mask) {
  __shared__ DppBox sb[kSegBoxTile];
  __shared__ int sb_ok[kSegBoxTile];
  const int64_t p0 = (int64_t)blockIdx.x * kSegThreads;
  const int64_t p = p0 + threadIdx.x;
  const bool live = p < n;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const float* q = pts + p * ld;
    x = q[0];
    y = q[1];
    z = q[2];
  }
  const int mine = live ? sample_of(pt_off, batch, p) : -1;
  // the samples this workgroup's points belong to: a range every thread computes alike, so the barriers below are uniform
  const int64_t p_last = min(p0 + kSegThreads, n) - 1;
  int s_lo = sample_of(pt_off, batch, p0), s_hi = sample_of(pt_off, batch, p_last);
  if (s_lo < 0) s_lo = 0;
  if (s_hi < 0) s_hi = batch - 1;
  int found = -1;
  float cx = 0.f, cy = 0.f, cz = 0.f;
  for (int s = s_lo; s <= s_hi; ++s) {
    const int64_t b0 = max((int64_t)box_off[s], (int64_t)0), b1 = min((int64_t)box_off[s + 1], n_boxes);
    for (int64_t t0 = b0; t0 < b1; t0 += kSegBoxTile) {
      const int nt = (int)min((int64_t)kSegBoxTile, b1 - t0);
      __syncthreads();
      if ((int)threadIdx.x < nt) {
        const float* roi = boxes + (t0 + threadIdx.x) * 7;
        float e = ew;
        // enlarged_box_hw with a negative width: a box that would lose its width or length keeps its own extents
        if (ew < 0.f && (__fadd_rn(roi[3], ew) <= 0.f || __fadd_rn(roi[4], ew) <= 0.f)) e = 0.f;
        sb[threadIdx.x] = dpp_box(roi, e, e, 0.f);
        sb_ok[threadIdx.x] = box_labels[t0 + threadIdx.x] >= 0 ? 1 : 0;
      }
      __syncthreads();
      if (mine == s && found < 0) {
        for (int k = 0; k < nt; ++k) {
          float lx, ly, lz;
          if (sb_ok[k] && dpp_classify(sb[k], x, y, z, lx, ly, lz) != 0) {
            found = (int)(t0 + k);
            cx = sb[k].cx;
            cy = sb[k].cy;
            cz = sb[k].cz;  // z_bottom + h * 0.5, each rounded: gravity_center
            break;
          }
        }
      }
    }
  }
  if (!live) return;
  inbox[p] = found;
  vote_mask[p] = found >= 0 ? 1 : 0;
  labels[p] = found >= 0 ? box_labels[found] : bg_label;
  float t[3] = {0.f, 0.f, 0.f};
  if (found >= 0) {
    if (centers) {
      cx = centers[(int64_t)found * 3];
      cy = centers[(int64_t)found * 3 + 1];
      cz = centers[(int64_t)found * 3 + 2];
    }
    const float d[3] = {__fsub_rn(cx, x), __fsub_rn(cy, y), __fsub_rn(cz, z)};
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = d[k] == 0.f ? 0.f : copysignf(sst_sqrt_rn(fabsf(d[k])), d[k]);  // the correctly rounded root
  }
  vote_targets[p * 3] = t[0];
  vote_targets[p * 3 + 1] = t[1];
  vote_targets[p * 3 + 2] = t[2];
}

// ------------------------------------------------------------------------------------------------------------------
// losses
// ------------------------------------------------------------------------------------------------------------------

struct LossArgs {
  const float* logits;
  const float* vote_preds;
  const int64_t* labels;
  const float* vote_targets;
  const uint8_t* vote_mask;
  const float* class_weight;
  const float* score_thresh;
  const int32_t* class_group;
  int64_t n;
  int c, mode, n_groups;
  float scale, gamma, alpha;
};

// partial record of a workgroup, 8-byte slots: [0] sum of the decode terms (double), [1] sum of the vote terms (double),
// [2] num_valid, [3] status, [4] num_fg, [5, 5 + C) tp, [5 + C, 5 + 2C) real (int64)
__host__ __device__ __forceinline__ int record_slots(int c) { return 5 + 2 * c; }

// dynamic LDS of the two row kernels, every offset a multiple of 16 bytes: the wave sums (forward only), then the image
constexpr int kWaveCounters = 3 + 2 * kMaxClasses;
constexpr int kWaveCountersAt = 2 * (kSegThreads / 64) * 8;
constexpr int kImageAt = kWaveCountersAt + (kSegThreads / 64) * kWaveCounters * 8;
static_assert(kWaveCountersAt % 16 == 0 && kImageAt % 16 == 0, "LDS carve offsets");

__global__ __launch_bounds__(kSegThreads) void seg_loss_partial_k(LossArgs a, unsigned long long* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = a.c;
  double(*wsum)[kSegThreads / 64] = (double(*)[kSegThreads / 64])smem;
  long long(*wcnt)[kWaveCounters] = (long long(*)[kWaveCounters])(smem + kWaveCountersAt);
  float* img = (float*)(smem + kImageAt);           // [c][kLossLd]
  float* gsc = img + sst_image_floats<kLossLd>(c);  // [n_groups][kSegThreads]: the group scores of this thread's row
  const bool sigmoid = a.mode == SST_SEG_SIGMOID_FOCAL;
  const bool stats = a.score_thresh != nullptr;
  const int64_t tile0 = (int64_t)blockIdx.x * kLossTileRows;
  double sem = 0.0, vote = 0.0;
  long long n_valid = 0, status = 0, n_fg = 0;  // the same value in every lane of a wave
  long long tp = 0, real = 0;                   // lane k of a wave: class k
  for (int sub = 0; sub < kLossTileRows / kLossSub; ++sub) {
    const int64_t r0 = tile0 + (int64_t)sub * kLossSub;
    if (r0 >= a.n) break;
    const int rows = (int)min((int64_t)kLossSub, a.n - r0);
    __syncthreads();
    sst_stage_rows<kSegThreads, kLossLd>(a.logits, r0, rows, c, img);
    __syncthreads();
    const bool live = tid < rows;
    const int64_t r = r0 + tid;
    const int64_t lab = live ? a.labels[r] : -1;
    const bool masked = live && a.vote_mask[r] != 0;
    const bool is_class = lab >= 0 && lab < c;
    const bool ok = live && (is_class || (sigmoid && lab == c));
    if (__any(live && !ok)) status |= 1;
    if (__any(masked && !is_class)) status |= 2;
    const bool voter = masked && is_class;
    n_valid += __popcll(__ballot(voter));
    if (voter) {
      const float* vp = a.vote_preds + r * 3 * c + 3 * lab;
      const float* vt = a.vote_targets + r * 3;
      float s = fabsf(vp[0] - vt[0]);
      s += fabsf(vp[1] - vt[1]);
      s += fabsf(vp[2] - vt[2]);
      vote += (double)s;
    }
    float* col = img + tid;
    if (sigmoid) {
      for (int k = 0; k < c; ++k) {
        const bool t = lab == k;
        bool hit = false;
        if (ok) {
          float p, e, dz;
          sst_focal_elem(a.scale * col[k * kLossLd], t, a.alpha, a.gamma, p, e, dz);
          sem += (double)e;
          hit = stats && t && p > a.score_thresh[k];
        }
        const long long n_real = __popcll(__ballot(ok && t)), n_tp = __popcll(__ballot(hit));
        if (lane == k) {
          real += n_real;
          tp += n_tp;
        }
      }
    } else {
      float m = -__builtin_inff(), s = 0.f;
      if (ok) {
        for (int k = 0; k < c; ++k) {
          const float z = a.scale * col[k * kLossLd];
          col[k * kLossLd] = z;
          m = fmaxf(m, z);
        }
        for (int k = 0; k < c; ++k) s += expf(col[k * kLossLd] - m);
        const float w = a.class_weight ? a.class_weight[lab] : 1.f;
        // (m - z_label) first: it is small where the loss is, and m + log(s) would round at the size of the logits
        sem += (double)(w * (logf(s) + (m - col[lab * kLossLd])));
      }
      bool own_pred = false;  // the prediction of the group of this row's own class
      if (stats) {
        float* g = gsc + tid;
        for (int j = 0; j < a.n_groups; ++j) g[j * kSegThreads] = 0.f;
        for (int k = 0; k < c - 1; ++k) {
          const int j = a.class_group[k];
          if (ok && j >= 0 && j < a.n_groups) g[j * kSegThreads] += expf(col[k * kLossLd] - m) / s;
        }
        for (int j = 0; j < a.n_groups; ++j) n_fg += __popcll(__ballot(ok && g[j * kSegThreads] > a.score_thresh[j]));
        if (ok && lab < c - 1) {
          const int j = a.class_group[lab];
          own_pred = j >= 0 && j < a.n_groups && g[j * kSegThreads] > a.score_thresh[j];
        }
      }
      for (int k = 0; k < c; ++k) {
        const long long n_real = __popcll(__ballot(ok && lab == k)), n_tp = __popcll(__ballot(own_pred && lab == k));
        if (lane == k) {
          real += n_real;
          tp += n_tp;
        }
      }
    }
  }
  // the workgroup's record: lanes by a fixed shuffle tree, then the four waves in order
  sem = sst_wave_sum(sem);
  vote = sst_wave_sum(vote);
  if (lane == 0) {
    wsum[0][wave] = sem;
    wsum[1][wave] = vote;
    wcnt[wave][0] = n_valid;
    wcnt[wave][1] = status;
    wcnt[wave][2] = n_fg;
  }
  if (lane < c) {
    wcnt[wave][3 + lane] = tp;
    wcnt[wave][3 + c + lane] = real;
  }
  __syncthreads();
  unsigned long long* rec = partials + (int64_t)blockIdx.x * record_slots(c);
  sst_write_record<kSegThreads / 64, 2>(wsum, rec);
  if (tid >= 2 && tid < record_slots(c)) {
    const int j = tid - 2;
    long long v = 0;
    for (int w = 0; w < kSegThreads / 64; ++w) v = j == 1 ? (v | wcnt[w][j]) : (v + wcnt[w][j]);
    rec[tid] = (unsigned long long)v;
  }
}

// one workgroup: thread q adds slot q of the records in index order (staged through LDS in chunks), then the results
__global__ __launch_bounds__(kSegThreads) void seg_loss_final_k(const unsigned long long* __restrict__ partials, int nb,
                                                                int64_t n, int c, int mode, int has_stats,
                                                                float* __restrict__ out, int64_t* __restrict__ counts) {
  __shared__ unsigned long long chunk[kFinalRows * (5 + 2 * kMaxClasses)];
  __shared__ long long tot[5 + 2 * kMaxClasses];
  __shared__ double dsum[2];
  const int tid = threadIdx.x, q = record_slots(c);
  double dv = 0.0;
  long long iv = 0;
  for (int b0 = 0; b0 < nb; b0 += kFinalRows) {
    const int rows = min(kFinalRows, nb - b0);
    __syncthreads();
    for (int i = tid; i < rows * q; i += kSegThreads) chunk[i] = partials[(int64_t)b0 * q + i];
    __syncthreads();
    if (tid < 2) {
      for (int r = 0; r < rows; ++r) dv += __longlong_as_double((long long)chunk[r * q + tid]);
    } else if (tid < q) {
      for (int r = 0; r < rows; ++r) {
        const long long v = (long long)chunk[r * q + tid];
        iv = tid == 3 ? (iv | v) : (iv + v);
      }
    }
  }
  if (tid < 2) dsum[tid] = dv; else if (tid < q) tot[tid] = iv;
  __syncthreads();
  const long long n_valid = tot[2];
  if (tid == 0) {
    const double denom = mode == SST_SEG_SIGMOID_FOCAL ? (double)n * (double)c : (double)n;
    out[0] = (float)(dsum[0] / denom);
    out[1] = n_valid > 0 ? (float)(dsum[1] / (3.0 * (double)n_valid)) : 0.f;
    out[2 + c] = (float)tot[4];
    counts[0] = n_valid;
    counts[1] = tot[3];
  }
  if (tid < c) {
    const long long tp = tot[5 + tid], real = tot[5 + c + tid];
    // tp.float() / (real_true.sum().float() + 1e-5)
    out[2 + tid] = has_stats ? (float)tp / ((float)real + 1e-5f) : 0.f;
    counts[2 + tid] = tp;
    counts[2 + c + tid] = real;
  }
}

__global__ __launch_bounds__(kSegThreads) void seg_loss_bwd_k(LossArgs a, const float* __restrict__ g,
                                                              const int64_t* __restrict__ counts,
                                                              float* __restrict__ d_logits,
                                                              float* __restrict__ d_vote_preds) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int c = a.c;
  float* img = (float*)smem;                                     // [c][kLossLd]
  int* vote_class = (int*)(img + sst_image_floats<kLossLd>(c));  // the class whose three vote columns carry a gradient, or -1
  const bool sigmoid = a.mode == SST_SEG_SIGMOID_FOCAL;
  const int64_t r0 = (int64_t)blockIdx.x * kLossSub;
  const int rows = (int)min((int64_t)kLossSub, a.n - r0);
  const int64_t n_valid = counts[0];
  const double denom = sigmoid ? (double)a.n * (double)c : (double)a.n;
  const float k_sem = (float)((double)g[0] * (double)a.scale / denom);
  const float k_vote = n_valid > 0 ? (float)((double)g[1] / (3.0 * (double)n_valid)) : 0.f;
  sst_stage_rows<kSegThreads, kLossLd>(a.logits, r0, rows, c, img);
  const bool live = tid < rows;
  const int64_t r = r0 + tid;
  const int64_t lab = live ? a.labels[r] : -1;
  const bool is_class = lab >= 0 && lab < c;
  const bool ok = live && (is_class || (sigmoid && lab == c));
  if (live) vote_class[tid] = (a.vote_mask[r] != 0 && is_class && n_valid > 0) ? (int)lab : -1;
  __syncthreads();
  if (live) {
    float* col = img + tid;
    if (!ok) {
      for (int k = 0; k < c; ++k) col[k * kLossLd] = 0.f;
    } else if (sigmoid) {
      for (int k = 0; k < c; ++k) {
        float p, e, dz;
        sst_focal_elem(a.scale * col[k * kLossLd], lab == k, a.alpha, a.gamma, p, e, dz);
        col[k * kLossLd] = k_sem * dz;
      }
    } else {
      float m = -__builtin_inff(), s = 0.f;
      for (int k = 0; k < c; ++k) {
        const float z = a.scale * col[k * kLossLd];
        col[k * kLossLd] = z;
        m = fmaxf(m, z);
      }
      for (int k = 0; k < c; ++k) {
        const float e = expf(col[k * kLossLd] - m);
        col[k * kLossLd] = e;
        s += e;
      }
      const float w = k_sem * (a.class_weight ? a.class_weight[lab] : 1.f);
      for (int k = 0; k < c; ++k) col[k * kLossLd] = w * (col[k * kLossLd] / s - (lab == k ? 1.f : 0.f));
    }
  }
  __syncthreads();
  {  // d_logits: consecutive lanes write consecutive floats
    float* base = d_logits + r0 * c;
    const int total = rows * c;
    for (int i = tid; i < total; i += kSegThreads) {
      const int rr = i / c, k = i - rr * c;
      base[i] = img[k * kLossLd + rr];
    }
  }
  {  // d_vote_preds: sign(pred - target) / (3 num_valid) in the three columns of the row's class, zero elsewhere
    const int w3 = 3 * c;
    const int64_t base = r0 * w3;
    const int total = rows * w3;
    for (int i = tid; i < total; i += kSegThreads) {
      const int rr = i / w3, k = i - rr * w3;
      const int kc = k / 3, d = k - kc * 3;
      float v = 0.f;
      if (vote_class[rr] == kc) {
        const float diff = a.vote_preds[base + i] - a.vote_targets[(r0 + rr) * 3 + d];
        v = diff > 0.f ? k_vote : diff < 0.f ? -k_vote : 0.f;
      }
      d_vote_preds[base + i] = v;
    }
  }
}

}  // namespace

extern "C" int sst_seg_targets_box_tile(void) { return kSegBoxTile; }

extern "C" int sst_seg_targets_f32(const float* d_points, int64_t ld, int64_t n, const int32_t* d_pt_offsets, int batch,
                                   const float* d_boxes, const int64_t* d_box_labels, const int32_t* d_box_offsets,
                                   int64_t n_boxes, int has_extra_width, double extra_width, int64_t bg_label,
                                   const float* d_centers, int32_t* d_inbox, int64_t* d_labels, float* d_vote_targets,
                                   uint8_t* d_vote_mask, void* stream) {
  if (n < 0 || batch < 1 || n_boxes < 0 || ld < 3) return SST_ERR_ARG;
  if (n == 0) return SST_OK;
  if (!d_points || !d_pt_offsets || !d_box_offsets || !d_inbox || !d_labels || !d_vote_targets || !d_vote_mask)
    return SST_ERR_ARG;
  if (n_boxes > 0 && (!d_boxes || !d_box_labels)) return SST_ERR_ARG;
  if (sst_div_up(n, kSegThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  const float ew = has_extra_width ? (float)(2.0 * extra_width) : 0.f;
  hipLaunchKernelGGL(seg_targets_k, dim3((unsigned)sst_div_up(n, kSegThreads)), dim3(kSegThreads), 0, (hipStream_t)stream,
                     d_points, ld, n, d_pt_offsets, batch, d_boxes, d_box_labels, d_box_offsets, n_boxes, ew, bg_label,
                     d_centers, d_inbox, d_labels, d_vote_targets, d_vote_mask);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_seg_loss_tile_rows(void) { return kLossTileRows; }

extern "C" int64_t sst_seg_loss_workspace_bytes(int64_t n, int c) {
  if (n < 1 || c < 1 || c > kMaxClasses) return 256;
  return sst_align_up(sst_div_up(n, kLossTileRows) * record_slots(c) * 8, 256);
}

static int loss_args(LossArgs& a, const float* d_logits, const float* d_vote_preds, const int64_t* d_labels,
                     const float* d_vote_targets, const uint8_t* d_vote_mask, int64_t n, int c, int mode, float logit_scale,
                     float gamma, float alpha, const float* d_class_weight, const float* d_score_thresh,
                     const int32_t* d_class_group, int n_groups) {
  if (n < 1 || !d_logits || !d_vote_preds || !d_labels || !d_vote_targets || !d_vote_mask) return SST_ERR_ARG;
  if (c < 1 || c > kMaxClasses || (mode != SST_SEG_SIGMOID_FOCAL && mode != SST_SEG_SOFTMAX_CE)) return SST_ERR_UNSUPPORTED;
  if (mode == SST_SEG_SIGMOID_FOCAL && !(gamma >= 0.f)) return SST_ERR_ARG;
  if (sst_div_up(n, kLossSub) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  const bool ce_stats = mode == SST_SEG_SOFTMAX_CE && d_score_thresh;
  if (ce_stats && (!d_class_group || n_groups < 1)) return SST_ERR_ARG;
  if (ce_stats && n_groups > kMaxClasses - 1) return SST_ERR_UNSUPPORTED;
  a.logits = d_logits;
  a.vote_preds = d_vote_preds;
  a.labels = d_labels;
  a.vote_targets = d_vote_targets;
  a.vote_mask = d_vote_mask;
  a.class_weight = mode == SST_SEG_SOFTMAX_CE ? d_class_weight : nullptr;
  a.score_thresh = d_score_thresh;
  a.class_group = d_class_group;
  a.n = n;
  a.c = c;
  a.mode = mode;
  a.n_groups = ce_stats ? n_groups : 0;
  a.scale = logit_scale;
  a.gamma = gamma;
  a.alpha = alpha;
  return SST_OK;
}

extern "C" int sst_seg_loss_fwd_f32(const float* d_logits, const float* d_vote_preds, const int64_t* d_labels,
                                    const float* d_vote_targets, const uint8_t* d_vote_mask, int64_t n, int c, int mode,
                                    float logit_scale, float gamma, float alpha, const float* d_class_weight,
                                    const float* d_score_thresh, const int32_t* d_class_group, int n_groups, float* d_out,
                                    int64_t* d_counts, void* d_workspace, void* stream) {
  LossArgs a;
  const int rc = loss_args(a, d_logits, d_vote_preds, d_labels, d_vote_targets, d_vote_mask, n, c, mode, logit_scale, gamma,
                           alpha, d_class_weight, d_score_thresh, d_class_group, n_groups);
  if (rc != SST_OK) return rc;
  if (!d_out || !d_counts || !d_workspace) return SST_ERR_ARG;
  const int nb = (int)sst_div_up(n, kLossTileRows);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = kImageAt + (size_t)(sst_image_floats<kLossLd>(c) + a.n_groups * kSegThreads) * sizeof(float);
  if (lds > 65536) return SST_ERR_UNSUPPORTED;  // 32 classes in more than 28 groups
  hipLaunchKernelGGL(seg_loss_partial_k, dim3(nb), dim3(kSegThreads), lds, s, a, (unsigned long long*)d_workspace);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_loss_final_k, dim3(1), dim3(kSegThreads), 0, s, (const unsigned long long*)d_workspace, nb, n, c,
                     mode, d_score_thresh ? 1 : 0, d_out, d_counts);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_seg_loss_bwd_f32(const float* d_logits, const float* d_vote_preds, const int64_t* d_labels,
                                    const float* d_vote_targets, const uint8_t* d_vote_mask, int64_t n, int c, int mode,
                                    float logit_scale, float gamma, float alpha, const float* d_class_weight,
                                    const float* d_g, const int64_t* d_counts, float* d_dlogits, float* d_dvote_preds,
                                    void* stream) {
  LossArgs a;
  const int rc = loss_args(a, d_logits, d_vote_preds, d_labels, d_vote_targets, d_vote_mask, n, c, mode, logit_scale, gamma,
                           alpha, d_class_weight, nullptr, nullptr, 0);
  if (rc != SST_OK) return rc;
  if (!d_g || !d_counts || !d_dlogits || !d_dvote_preds) return SST_ERR_ARG;
  const size_t lds = (size_t)(sst_image_floats<kLossLd>(c) + kLossSub) * sizeof(float);
  hipLaunchKernelGGL(seg_loss_bwd_k, dim3((unsigned)sst_div_up(n, kLossSub)), dim3(kSegThreads), lds, (hipStream_t)stream,
                     a, d_g, d_counts, d_dlogits, d_dvote_preds);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

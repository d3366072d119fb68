// Training and decoding side of the FSD cluster heads (SparseClusterHeadV2, FSDV2Head): the targets of every task and every
// sample in one launch, the focal / L1 losses of every task in two launches forward and one backward, box encoding and decoding.
// fp32 data, no float atomics, no host read-back, bit-reproducible.
//
// Reference (mmdet3d/models/dense_heads):
//   sst_cluster_targets_f32    sparse_cluster_head_v2.py:299-405 (modify_gt_for_single_task(_single_sample), get_targets,
//                              get_targets_single), fsd_v2_head.py:306-395 (the same with centroid_assign),
//                              sparse_cluster_head.py:269-289 (split_by_batch, combine_by_batch) and :364-397 (assign_single),
//                              enlarged_box of core/bbox/structures/lidar_box3d.py:269-285, points_in_boxes,
//                              BasePointBBoxCoder.encode of core/bbox/coders/base_point_bbox_coder.py:36-58
//   sst_cluster_loss_fwd_f32   loss_single_task of sparse_cluster_head_v2.py:192-297 / fsd_v2_head.py:168-275 for every task:
//                              FocalLoss (sigmoid) with avg_factor, the nonzero() of pos_inds, the gathered L1 losses; the
//                              asserts :220, :395-396 become the status word
//   sst_cluster_loss_bwd_f32   what autograd derives from the above
//   sst_cluster_encode_f32 /   BasePointBBoxCoder.encode / decode (base_point_bbox_coder.py:36-82), the sigmoid and the padding
//   sst_cluster_decode_f32     column of _get_bboxes_single (sparse_cluster_head_v2.py:534-554), xywhr2xyxyr of the BEV boxes
//
// PARITY.  Targets: membership is dpp_box / dpp_classify of pib_test.h on the enlarged box (pinned to the reference's compiled
// points_in_boxes_cpu); the centre deltas are one rounded subtraction; log / sin / cos are the device library's (see DESIGN.md
// 3.13 for the 2-ulp rule).  Losses: mmdet's FocalLoss and L1Loss are not part of the reference tree; the focal formula is the
// tree's own py_sigmoid_focal_loss, sum / avg_factor, L1 is sum(|pred - target| weight) / avg_factor.
// Checked against the reference's methods run from their source text (tests/golden/cluster_head_train.npz).
#include "common.h"
#include "head_math.h"
#include "pib_test.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBoxTile = 256;     // boxes per LDS tile of the targets kernel
constexpr int kMaxTasks = SST_CLUSTER_MAX_TASKS;
constexpr int kMaxClasses = 64;   // classes of the class -> task table
constexpr int kMaxTaskClasses = 32;
constexpr int kMaxCode = 10;
constexpr int kSub = 256;         // rows per pass of a workgroup: one row per thread
constexpr int kTileRows = 1024;   // rows per workgroup of the forward's first launch
constexpr int kLd = kSub + 1;     // row stride of the [class][row] LDS image: class c of row r on bank (c + r) % 32
constexpr int kRecord = 7;        // 8-byte slots of a partial record: 5 sums (double), num_pos, status (int64)

// ------------------------------------------------------------------------------------------------------------------
// targets
// ------------------------------------------------------------------------------------------------------------------

struct TargetsArgs {
  const float* xyz_assign;
  const float* xyz_base;
  const int64_t* bidx;
  int64_t bstride, n;
  const float* boxes;
  const int64_t* box_labels;
  const int32_t* box_off;
  int64_t n_boxes;
  int batch, cols, code, n_tasks, n_classes, has_ew;
  float ew2, ew1;  // (float)(2 * width), (float)width
  int8_t cls_task[kMaxClasses], cls_idx[kMaxClasses];
  int32_t task_classes[kMaxTasks];
  char* out;
  int64_t off[kMaxTasks][4];
};

// BasePointBBoxCoder.encode of one box at one base point; columns >= code are left alone
__device__ __forceinline__ void encode_row(const float* __restrict__ bx, int cols, const float* __restrict__ base, int code,
                                           float* t) {
  t[0] = __fsub_rn(bx[0], base[0]);
  t[1] = __fsub_rn(bx[1], base[1]);
  t[2] = __fsub_rn(bx[2], base[2]);
  t[3] = logf(__fadd_rn(bx[3], 1e-6f));
  t[4] = logf(__fadd_rn(bx[4], 1e-6f));
  t[5] = logf(__fadd_rn(bx[5], 1e-6f));
  t[6] = sinf(bx[6]);
  t[7] = cosf(bx[6]);
  if (code == kMaxCode && cols >= 9) {
    t[8] = bx[7];
    t[9] = bx[8];
  }
}

__global__ __launch_bounds__(kThreads) void cluster_targets_k(TargetsArgs a) {
  __shared__ DppBox sb[kBoxTile];
  __shared__ int sb_key[kBoxTile];  // (task << 8) | class index within the task, or -1: in no task's list
  const int tid = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kThreads + tid;
  const bool live = p < a.n;
  float x = 0.f, y = 0.f, z = 0.f;
  int mine = -1;
  if (live) {
    x = a.xyz_assign[p * 3];
    y = a.xyz_assign[p * 3 + 1];
    z = a.xyz_assign[p * 3 + 2];
    const int64_t s = a.bidx[p * a.bstride];
    if (s >= 0 && s < a.batch) mine = (int)s;
  }
  // per task the smallest (class index within the task, box index) among the hits: the first hit of the class-regrouped list
  unsigned long long best[kMaxTasks];
#pragma unroll
  for (int t = 0; t < kMaxTasks; ++t) best[t] = ~0ull;
  for (int s = 0; s < a.batch; ++s) {
    // rows of several samples may sit in one workgroup in any order: every sample present gets its pass (uniform decision)
    if (!__syncthreads_or(mine == s ? 1 : 0)) continue;
    const int64_t b0 = max((int64_t)a.box_off[s], (int64_t)0), b1 = min((int64_t)a.box_off[s + 1], a.n_boxes);
    for (int64_t t0 = b0; t0 < b1; t0 += kBoxTile) {
      const int nt = (int)min((int64_t)kBoxTile, b1 - t0);
      __syncthreads();
      if (tid < nt) {
        const float* roi = a.boxes + (t0 + tid) * a.cols;
        float r[7] = {roi[0], roi[1], roi[2], roi[3], roi[4], roi[5], roi[6]};
        if (a.has_ew) {
          // enlarged_box: w, l, h += 2 * width, z -= width; for a negative width a box that would lose an extent keeps its own
          const float w = __fadd_rn(r[3], a.ew2), l = __fadd_rn(r[4], a.ew2), h = __fadd_rn(r[5], a.ew2);
          if (!(a.ew1 < 0.f && (w <= 0.f || l <= 0.f || h <= 0.f))) {
            r[2] = __fsub_rn(r[2], a.ew1);
            r[3] = w;
            r[4] = l;
            r[5] = h;
          }
        }
        sb[tid] = dpp_box(r, 0.f, 0.f, 0.f);
        const int64_t lab = a.box_labels[t0 + tid];
        int key = -1;
        if (lab >= 0 && lab < a.n_classes && a.cls_task[lab] >= 0) key = ((int)a.cls_task[lab] << 8) | (int)a.cls_idx[lab];
        sb_key[tid] = key;
      }
      __syncthreads();
      if (mine == s) {
        for (int k = 0; k < nt; ++k) {
          const int key = sb_key[k];
          float lx, ly, lz;
          if (key >= 0 && dpp_classify(sb[k], x, y, z, lx, ly, lz) != 0) {
            const int tk = key >> 8;
            const unsigned long long cand = ((unsigned long long)(key & 255) << 32) | (unsigned)(t0 + k);
#pragma unroll
            for (int t = 0; t < kMaxTasks; ++t)
              if (tk == t && cand < best[t]) best[t] = cand;
          }
        }
      }
    }
  }
  if (!live) return;
  float base[3] = {a.xyz_base[p * 3], a.xyz_base[p * 3 + 1], a.xyz_base[p * 3 + 2]};
#pragma unroll
  for (int t = 0; t < kMaxTasks; ++t) {
    if (t >= a.n_tasks) break;
    int64_t* labels = (int64_t*)(a.out + a.off[t][0]);
    float* tg = (float*)(a.out + a.off[t][1]) + p * a.code;
    float* wt = (float*)(a.out + a.off[t][2]) + p * a.code;
    int32_t* assigned = (int32_t*)(a.out + a.off[t][3]);
    const bool hit = best[t] != ~0ull;
    const int g = (int)(unsigned)(best[t] & 0xffffffffull);
    labels[p] = hit ? (int64_t)(best[t] >> 32) : (int64_t)a.task_classes[t];
    assigned[p] = hit ? g : -1;
    float tv[kMaxCode] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float w = 0.f, wlast = 0.f;
    if (hit) {
      const float* bx = a.boxes + (int64_t)g * a.cols;
      encode_row(bx, a.cols, base, a.code, tv);
      w = 1.f;
      wlast = a.cols == 10 ? bx[9] : 1.f;  // the copy-paste flag: no velocity loss for pasted objects
    }
#pragma unroll
    for (int c = 0; c < kMaxCode; ++c) {
      if (c < a.code) {
        tg[c] = tv[c];
        wt[c] = c >= a.code - 2 ? wlast : w;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void cluster_encode_k(const float* __restrict__ boxes, int cols,
                                                             const float* __restrict__ base, int64_t n, int code,
                                                             float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  float t[kMaxCode] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float b[3] = {base[p * 3], base[p * 3 + 1], base[p * 3 + 2]};
  encode_row(boxes + p * cols, cols, b, code, t);
#pragma unroll
  for (int c = 0; c < kMaxCode; ++c)
    if (c < code) out[p * code + c] = t[c];
}

// ------------------------------------------------------------------------------------------------------------------
// losses
// ------------------------------------------------------------------------------------------------------------------

struct LossArgs {
  sst_cluster_loss_task task[kMaxTasks];
  int64_t n;
  int n_tasks, code;
  float gamma, alpha;
  float cw[kMaxCode];  // code_weight (1 when none is given)
  float w[5];          // loss weights: cls, center, size, rot, vel
  float beta[5];       // SmoothL1Loss beta of the regression losses (same order; 0: L1Loss)
};

// the loss a regression column belongs to: 1 center, 2 size, 3 rot, 4 vel
__device__ __forceinline__ constexpr int group_of(int col) { return col < 3 ? 1 : col < 6 ? 2 : col < 8 ? 3 : 4; }

constexpr int kWaves = kThreads / 64;
constexpr int kWaveCntAt = 5 * kWaves * 8;
constexpr int kImageAt = kWaveCntAt + 2 * kWaves * 8;
static_assert(kImageAt % 16 == 0, "LDS carve offsets");

__global__ __launch_bounds__(kThreads) void cluster_loss_partial_k(LossArgs a, int nb, unsigned long long* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const sst_cluster_loss_task& tk = a.task[blockIdx.y];
  const int c = tk.classes, code = a.code;
  double(*wsum)[kWaves] = (double(*)[kWaves])smem;
  long long(*wcnt)[kWaves] = (long long(*)[kWaves])(smem + kWaveCntAt);
  float* img = (float*)(smem + kImageAt);  // [c][kLd]
  const int64_t tile0 = (int64_t)blockIdx.x * kTileRows;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
  long long n_pos = 0, status = 0;  // the same value in every lane of a wave
  for (int sub = 0; sub < kTileRows / kSub; ++sub) {
    const int64_t r0 = tile0 + (int64_t)sub * kSub;
    if (r0 >= a.n) break;
    const int rows = (int)min((int64_t)kSub, a.n - r0);
    __syncthreads();
    sst_stage_rows<kThreads, kLd>(tk.logits, r0, rows, c, img);
    __syncthreads();
    const bool live = tid < rows;
    const int64_t r = r0 + tid;
    const int64_t lab = live ? tk.labels[r] : -1;
    const bool pos = live && lab >= 0 && lab < c;
    const bool ok = pos || (live && lab == c);
    if (__any(live && !ok)) status |= 1;
    n_pos += __popcll(__ballot(pos));
    if (ok) {
      const float* col = img + tid;
      for (int k = 0; k < c; ++k) {
        float p, e, dz;
        sst_focal_elem(col[k * kLd], lab == k, a.alpha, a.gamma, p, e, dz);
        s0 += (double)e;
      }
    }
    bool bad_flag = false;
    if (pos) {
      const float* pr = tk.reg_preds + r * code;
      const float* tg = tk.bbox_targets + r * code;
      const float* wt = tk.bbox_weights + r * code;
#pragma unroll
      for (int k = 0; k < kMaxCode; ++k) {
        if (k < code) {
          const float w = wt[k];
          const double v = (double)(sst_reg_elem(pr[k] - tg[k], a.beta[group_of(k)]) * (w * a.cw[k]));
          if (group_of(k) == 1) s1 += v;
          else if (group_of(k) == 2) s2 += v;
          else if (group_of(k) == 3) s3 += v;
          else s4 += v;
          if (k >= 8 && w != 0.f && w != 1.f) bad_flag = true;
        }
      }
    }
    if (__any(bad_flag)) status |= 2;
  }
  // the workgroup's record: lanes by a fixed shuffle tree, then the four waves in order
  s0 = sst_wave_sum(s0);
  s1 = sst_wave_sum(s1);
  s2 = sst_wave_sum(s2);
  s3 = sst_wave_sum(s3);
  s4 = sst_wave_sum(s4);
  if (lane == 0) {
    wsum[0][wave] = s0;
    wsum[1][wave] = s1;
    wsum[2][wave] = s2;
    wsum[3][wave] = s3;
    wsum[4][wave] = s4;
    wcnt[0][wave] = n_pos;
    wcnt[1][wave] = status;
  }
  __syncthreads();
  unsigned long long* rec = partials + ((int64_t)blockIdx.y * nb + blockIdx.x) * kRecord;
  sst_write_record<kWaves, 5>(wsum, rec);
  if (tid >= 5 && tid < kRecord) {
    const int j = tid - 5;
    long long v = 0;
    for (int w = 0; w < kWaves; ++w) v = j == 1 ? (v | wcnt[j][w]) : (v + wcnt[j][w]);
    rec[tid] = (unsigned long long)v;
  }
}

struct FinalArgs {
  int64_t n;
  int n_tasks, nb, phase;
  float w[5];
};

// one workgroup: thread q adds slot q % 7 of task q / 7's records in index order, then one thread per task writes the results.
// phase SST_CLUSTER_LOSS_COUNTS writes counts only (averaging factors at their defaults), SST_CLUSTER_LOSS_FINISH reads the
// averaging factors from counts, both together do the whole thing.
__global__ __launch_bounds__(kThreads) void cluster_loss_final_k(FinalArgs a, const unsigned long long* __restrict__ partials,
                                                                 float* __restrict__ out, double* __restrict__ counts) {
  __shared__ double tot[kMaxTasks * kRecord];
  const int tid = threadIdx.x;
  if (tid < a.n_tasks * kRecord) {
    const int t = tid / kRecord, slot = tid - t * kRecord;
    const unsigned long long* src = partials + (int64_t)t * a.nb * kRecord + slot;
    if (slot < 5) {
      double v = 0.0;
      for (int b = 0; b < a.nb; ++b) v += __longlong_as_double((long long)src[(int64_t)b * kRecord]);
      tot[tid] = v;
    } else {
      long long v = 0;
      for (int b = 0; b < a.nb; ++b) {
        const long long u = (long long)src[(int64_t)b * kRecord];
        v = slot == 6 ? (v | u) : (v + u);
      }
      tot[tid] = (double)v;
    }
  }
  __syncthreads();
  if (tid >= a.n_tasks) return;
  const double* s = tot + tid * kRecord;
  double* cnt = counts + tid * 4;
  const double n_pos = s[5];
  double cls_avg = (double)a.n, reg_avg = n_pos;
  if (a.phase & SST_CLUSTER_LOSS_COUNTS) {
    cnt[0] = n_pos;
    cnt[1] = s[6];
    cnt[2] = cls_avg;
    cnt[3] = reg_avg;
  } else {
    cls_avg = cnt[2];
    reg_avg = cnt[3];
  }
  if (!(a.phase & SST_CLUSTER_LOSS_FINISH)) return;
  float* o = out + tid * 5;
  o[0] = (float)((double)a.w[0] * s[0] / cls_avg);
  const bool any = n_pos > 0.0 && reg_avg > 0.0;
  o[1] = any ? (float)((double)a.w[1] * s[1] / reg_avg) : 0.f;
  o[2] = any ? (float)((double)a.w[2] * s[2] / reg_avg) : 0.f;
  o[3] = any ? (float)((double)a.w[3] * s[3] / reg_avg) : 0.f;
  o[4] = any ? (float)((double)a.w[4] * s[4] / (2.0 * n_pos)) : 0.f;  // loss_vel has no avg_factor: the mean over elements
}

__global__ __launch_bounds__(kThreads) void cluster_loss_bwd_k(LossArgs a, const float* __restrict__ g,
                                                               const double* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const sst_cluster_loss_task& tk = a.task[blockIdx.y];
  const int c = tk.classes, code = a.code;
  float* img = (float*)smem;             // [c][kLd]
  float* regbuf = img + sst_image_floats<kLd>(c);  // [kSub][code]
  const int64_t r0 = (int64_t)blockIdx.x * kSub;
  const int rows = (int)min((int64_t)kSub, a.n - r0);
  const double* cnt = counts + blockIdx.y * 4;
  const float* gt = g + blockIdx.y * 5;
  const double n_pos = cnt[0], cls_avg = cnt[2], reg_avg = cnt[3];
  const bool any = n_pos > 0.0 && reg_avg > 0.0;
  float kk[5];
  kk[0] = (float)((double)gt[0] * (double)a.w[0] / cls_avg);
#pragma unroll
  for (int j = 1; j < 4; ++j) kk[j] = any ? (float)((double)gt[j] * (double)a.w[j] / reg_avg) : 0.f;
  kk[4] = any ? (float)((double)gt[4] * (double)a.w[4] / (2.0 * n_pos)) : 0.f;
  sst_stage_rows<kThreads, kLd>(tk.logits, r0, rows, c, img);
  __syncthreads();
  if (tid < rows) {
    const int64_t r = r0 + tid;
    const int64_t lab = tk.labels[r];
    const bool pos = lab >= 0 && lab < c;
    const bool ok = pos || lab == c;
    float* col = img + tid;
    for (int k = 0; k < c; ++k) {
      float p, e, dz = 0.f;
      if (ok) sst_focal_elem(col[k * kLd], lab == k, a.alpha, a.gamma, p, e, dz);
      col[k * kLd] = ok ? kk[0] * dz : 0.f;
    }
    const float* pr = tk.reg_preds + r * code;
    const float* tg = tk.bbox_targets + r * code;
    const float* wt = tk.bbox_weights + r * code;
#pragma unroll
    for (int k = 0; k < kMaxCode; ++k) {
      if (k < code) {
        float v = 0.f;
        if (pos) {
          v = sst_reg_grad(pr[k] - tg[k], a.beta[group_of(k)]) * ((wt[k] * a.cw[k]) * kk[group_of(k)]);
        }
        regbuf[tid * code + k] = v;
      }
    }
  }
  __syncthreads();
  {  // consecutive lanes write consecutive floats
    float* base = tk.d_logits + r0 * c;
    const int total = rows * c;
    for (int i = tid; i < total; i += kThreads) {
      const int rr = i / c, k = i - rr * c;
      base[i] = img[k * kLd + rr];
    }
  }
  {
    float* base = tk.d_reg_preds + r0 * code;
    const int total = rows * code;
    for (int i = tid; i < total; i += kThreads) base[i] = regbuf[i];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// decoding
// ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void cluster_decode_k(const float* __restrict__ reg, const float* __restrict__ base,
                                                             const float* __restrict__ logits, int64_t n, int code, int c,
                                                             float* __restrict__ boxes, float* __restrict__ scores,
                                                             float* __restrict__ bev) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  const float* r = reg + p * code;
  const int cols = code - 1;
  float* o = boxes + p * cols;
  const float x = __fadd_rn(r[0], base[p * 3]), y = __fadd_rn(r[1], base[p * 3 + 1]), z = __fadd_rn(r[2], base[p * 3 + 2]);
  const float w = __fsub_rn(expf(r[3]), 1e-6f), l = __fsub_rn(expf(r[4]), 1e-6f), h = __fsub_rn(expf(r[5]), 1e-6f);
  const float yaw = atan2f(r[6], r[7]);
  o[0] = x;
  o[1] = y;
  o[2] = z;
  o[3] = w;
  o[4] = l;
  o[5] = h;
  o[6] = yaw;
  if (code == kMaxCode) {
    o[7] = r[8];
    o[8] = r[9];
  }
  if (bev) {  // xywhr2xyxyr(LiDARInstance3DBoxes.bev): (x - w / 2, y - l / 2, x + w / 2, y + l / 2, yaw)
    const float hw = __fmul_rn(w, 0.5f), hl = __fmul_rn(l, 0.5f);
    float* b = bev + p * 5;
    b[0] = __fsub_rn(x, hw);
    b[1] = __fsub_rn(y, hl);
    b[2] = __fadd_rn(x, hw);
    b[3] = __fadd_rn(y, hl);
    b[4] = yaw;
  }
  if (scores) {
    const float* lg = logits + p * c;
    float* s = scores + p * (c + 1);
    // the sigmoid through fp64: within half an ulp of the value whatever the sign of the logit
    for (int k = 0; k < c; ++k) s[k] = (float)(1.0 / (1.0 + exp(-(double)lg[k])));
    s[c] = 0.f;  // the padding (background) column box3d_multiclass_nms expects
  }
}

int fill_loss_args(LossArgs& a, const sst_cluster_loss_task* tasks, int n_tasks, int64_t n, int code, float gamma, float alpha,
                   const float* code_weight, const float* loss_weights, const float* smooth_l1_beta, bool backward) {
  if (!tasks || !loss_weights || n < 1) return SST_ERR_ARG;
  if (n_tasks < 1 || n_tasks > kMaxTasks || (code != 8 && code != kMaxCode)) return SST_ERR_UNSUPPORTED;
  if (!(gamma >= 0.f)) return SST_ERR_ARG;
  if (sst_div_up(n, kSub) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  for (int t = 0; t < n_tasks; ++t) {
    const sst_cluster_loss_task& k = tasks[t];
    if (!k.logits || !k.reg_preds || !k.labels || !k.bbox_targets || !k.bbox_weights) return SST_ERR_ARG;
    if (backward && (!k.d_logits || !k.d_reg_preds)) return SST_ERR_ARG;
    if (k.classes < 1 || k.classes > kMaxTaskClasses) return SST_ERR_UNSUPPORTED;
    a.task[t] = k;
  }
  for (int t = n_tasks; t < kMaxTasks; ++t) a.task[t] = sst_cluster_loss_task{};
  a.n = n;
  a.n_tasks = n_tasks;
  a.code = code;
  a.gamma = gamma;
  a.alpha = alpha;
  for (int k = 0; k < kMaxCode; ++k) a.cw[k] = (code_weight && k < code) ? code_weight[k] : 1.f;
  for (int k = 0; k < 5; ++k) a.w[k] = loss_weights[k];
  a.beta[0] = 0.f;
  for (int k = 1; k < 5; ++k) {
    a.beta[k] = smooth_l1_beta ? smooth_l1_beta[k] : 0.f;
    if (!(a.beta[k] >= 0.f)) return SST_ERR_ARG;
  }
  return SST_OK;
}

int max_classes(const LossArgs& a) {
  int c = 1;
  for (int t = 0; t < a.n_tasks; ++t) c = a.task[t].classes > c ? a.task[t].classes : c;
  return c;
}

}  // namespace

extern "C" int sst_cluster_max_tasks(void) { return kMaxTasks; }
extern "C" int sst_cluster_targets_box_tile(void) { return kBoxTile; }
extern "C" int sst_cluster_loss_tile_rows(void) { return kTileRows; }

extern "C" int64_t sst_cluster_targets_layout(int64_t n, int n_tasks, int code_size, int64_t* offsets) {
  if (n < 0 || n_tasks < 1 || n_tasks > kMaxTasks || (code_size != 8 && code_size != kMaxCode)) return SST_ERR_ARG;
  int64_t at = 0;
  for (int t = 0; t < n_tasks; ++t) {
    const int64_t sizes[4] = {n * 8, n * code_size * 4, n * code_size * 4, n * 4};
    for (int k = 0; k < 4; ++k) {
      if (offsets) offsets[4 * t + k] = at;
      at += sst_align_up(sizes[k] > 0 ? sizes[k] : 1, 256);
    }
  }
  return at;
}

extern "C" int sst_cluster_targets_f32(const float* d_xyz_assign, const float* d_xyz_base, int64_t n,
                                       const int64_t* d_batch_idx, int64_t batch_idx_stride, int batch, const float* d_boxes,
                                       int box_cols, const int64_t* d_box_labels, const int32_t* d_box_offsets,
                                       int64_t n_boxes, const int32_t* class_table, int n_classes, const int32_t* task_classes,
                                       int n_tasks, int code_size, int has_enlarge_width, double enlarge_width, void* d_out,
                                       void* stream) {
  if (n < 0 || batch < 1 || n_boxes < 0 || batch_idx_stride < 1 || !class_table || !task_classes) return SST_ERR_ARG;
  if (n_tasks < 1 || n_tasks > kMaxTasks || n_classes < 1 || n_classes > kMaxClasses) return SST_ERR_UNSUPPORTED;
  if (code_size != 8 && code_size != kMaxCode) return SST_ERR_UNSUPPORTED;
  if (box_cols != 7 && box_cols != 9 && box_cols != 10) return SST_ERR_UNSUPPORTED;
  // encode asserts code_size == 10 for boxes with velocities; 7-column boxes give 8 target columns
  if (n_boxes > 0 && (box_cols == 7) != (code_size == 8)) return SST_ERR_ARG;
  if (n == 0) return SST_OK;
  if (!d_xyz_assign || !d_xyz_base || !d_batch_idx || !d_box_offsets || !d_out) return SST_ERR_ARG;
  if (n_boxes > 0 && (!d_boxes || !d_box_labels)) return SST_ERR_ARG;
  if (sst_div_up(n, kThreads) > 0x7fffffff || n_boxes > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  TargetsArgs a;
  a.xyz_assign = d_xyz_assign;
  a.xyz_base = d_xyz_base;
  a.bidx = d_batch_idx;
  a.bstride = batch_idx_stride;
  a.n = n;
  a.boxes = d_boxes;
  a.box_labels = d_box_labels;
  a.box_off = d_box_offsets;
  a.n_boxes = n_boxes;
  a.batch = batch;
  a.cols = box_cols;
  a.code = code_size;
  a.n_tasks = n_tasks;
  a.n_classes = n_classes;
  a.has_ew = has_enlarge_width ? 1 : 0;
  a.ew2 = has_enlarge_width ? (float)(enlarge_width * 2.0) : 0.f;
  a.ew1 = has_enlarge_width ? (float)enlarge_width : 0.f;
  for (int k = 0; k < kMaxClasses; ++k) {
    int task = -1, idx = 0;
    if (k < n_classes) {
      task = class_table[2 * k];
      idx = class_table[2 * k + 1];
      if (task >= n_tasks || (task >= 0 && (idx < 0 || idx >= task_classes[task]))) return SST_ERR_ARG;
      if (task < 0) task = -1;
    }
    a.cls_task[k] = (int8_t)task;
    a.cls_idx[k] = (int8_t)idx;
  }
  for (int t = 0; t < kMaxTasks; ++t) {
    a.task_classes[t] = t < n_tasks ? task_classes[t] : 0;
    if (t < n_tasks && (task_classes[t] < 1 || task_classes[t] > kMaxTaskClasses)) return SST_ERR_UNSUPPORTED;
  }
  a.out = (char*)d_out;
  int64_t offsets[4 * kMaxTasks] = {0};
  sst_cluster_targets_layout(n, n_tasks, code_size, offsets);
  for (int t = 0; t < kMaxTasks; ++t)
    for (int k = 0; k < 4; ++k) a.off[t][k] = offsets[4 * t + k];
  hipLaunchKernelGGL(cluster_targets_k, dim3((unsigned)sst_div_up(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_cluster_encode_f32(const float* d_boxes, int box_cols, const float* d_base, int64_t n, int code_size,
                                      float* d_out, void* stream) {
  if (n < 0) return SST_ERR_ARG;
  if ((code_size != 8 && code_size != kMaxCode) || (box_cols != 7 && box_cols != 9 && box_cols != 10)) return SST_ERR_UNSUPPORTED;
  if ((box_cols == 7) != (code_size == 8)) return SST_ERR_ARG;
  if (n == 0) return SST_OK;
  if (!d_boxes || !d_base || !d_out) return SST_ERR_ARG;
  if (sst_div_up(n, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(cluster_encode_k, dim3((unsigned)sst_div_up(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, d_boxes,
                     box_cols, d_base, n, code_size, d_out);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int64_t sst_cluster_loss_workspace_bytes(int64_t n, int n_tasks) {
  if (n < 1 || n_tasks < 1 || n_tasks > kMaxTasks) return 256;
  return sst_align_up(sst_div_up(n, kTileRows) * n_tasks * kRecord * 8, 256);
}

extern "C" int sst_cluster_loss_fwd_f32(const sst_cluster_loss_task* tasks, int n_tasks, int64_t n, int code_size, float gamma,
                                        float alpha, const float* code_weight, const float* loss_weights,
                                        const float* smooth_l1_beta, int phases,
                                        float* d_out, double* d_counts, void* d_workspace, void* stream) {
  LossArgs a;
  const int rc = fill_loss_args(a, tasks, n_tasks, n, code_size, gamma, alpha, code_weight, loss_weights, smooth_l1_beta, false);
  if (rc != SST_OK) return rc;
  if (!d_counts || !d_workspace || !(phases & (SST_CLUSTER_LOSS_COUNTS | SST_CLUSTER_LOSS_FINISH))) return SST_ERR_ARG;
  if ((phases & SST_CLUSTER_LOSS_FINISH) && !d_out) return SST_ERR_ARG;
  const int nb = (int)sst_div_up(n, kTileRows);
  hipStream_t s = (hipStream_t)stream;
  if (phases & SST_CLUSTER_LOSS_COUNTS) {
    const size_t lds = kImageAt + (size_t)sst_image_floats<kLd>(max_classes(a)) * sizeof(float);
    hipLaunchKernelGGL(cluster_loss_partial_k, dim3(nb, n_tasks), dim3(kThreads), lds, s, a, nb,
                       (unsigned long long*)d_workspace);
    SST_LAUNCH_CHECK();
  }
  FinalArgs f;
  f.n = n;
  f.n_tasks = n_tasks;
  f.nb = nb;
  f.phase = phases;
  for (int k = 0; k < 5; ++k) f.w[k] = a.w[k];
  hipLaunchKernelGGL(cluster_loss_final_k, dim3(1), dim3(kThreads), 0, s, f, (const unsigned long long*)d_workspace, d_out,
                     d_counts);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_cluster_loss_bwd_f32(const sst_cluster_loss_task* tasks, int n_tasks, int64_t n, int code_size, float gamma,
                                        float alpha, const float* code_weight, const float* loss_weights,
                                        const float* smooth_l1_beta, const float* d_g,
                                        const double* d_counts, void* stream) {
  LossArgs a;
  const int rc = fill_loss_args(a, tasks, n_tasks, n, code_size, gamma, alpha, code_weight, loss_weights, smooth_l1_beta, true);
  if (rc != SST_OK) return rc;
  if (!d_g || !d_counts) return SST_ERR_ARG;
  const size_t lds = (size_t)(sst_image_floats<kLd>(max_classes(a)) + kSub * code_size) * sizeof(float);
  hipLaunchKernelGGL(cluster_loss_bwd_k, dim3((unsigned)sst_div_up(n, kSub), n_tasks), dim3(kThreads), lds, (hipStream_t)stream,
                     a, d_g, d_counts);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_cluster_decode_f32(const float* d_reg_preds, const float* d_base, const float* d_logits, int64_t n,
                                      int code_size, int classes, float* d_boxes, float* d_scores, float* d_bev,
                                      void* stream) {
  if (n < 0) return SST_ERR_ARG;
  if (code_size != 8 && code_size != kMaxCode) return SST_ERR_UNSUPPORTED;
  if (n == 0) return SST_OK;
  if (!d_reg_preds || !d_base || !d_boxes) return SST_ERR_ARG;
  if (d_scores && (!d_logits || classes < 1)) return SST_ERR_ARG;
  if (sst_div_up(n, kThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(cluster_decode_k, dim3((unsigned)sst_div_up(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     d_reg_preds, d_base, d_logits, n, code_size, classes, d_boxes, d_scores, d_bev);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

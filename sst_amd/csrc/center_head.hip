// Training and decoding side of CenterHead: the targets of a whole batch and of every task in one launch, the Gaussian focal
// heatmap loss and the L1 box loss in two launches forward and two backward, and the box decoding in one launch.  fp32 data,
// no float atomics, no host read-back, bit-reproducible.
//
// Reference:
//   sst_center_targets_f32   CenterHead.get_targets / get_targets_single, mmdet3d/models/dense_heads/centerpoint_head.py:385-560
//                            (the Python loop over every box of every sample), gaussian_radius / draw_heatmap_gaussian /
//                            gaussian_2d of mmdet3d/core/utils/gaussian.py:5-85, LiDARInstance3DBoxes.gravity_center
//   sst_center_loss_fwd_f32  CenterHead.loss :563-610: clip_sigmoid, GaussianFocalLoss (mmdet 2.x gaussian_focal_loss, alpha 2,
//                            gamma 4, mean with avg_factor), the channel concatenation, permute and _gather_feat :360-383 of
//                            the regression maps, L1Loss with weights and avg_factor
//   sst_center_loss_bwd_f32  what autograd derives from the above
//   sst_center_decode_f32    CenterPointBBoxCoder.decode, mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py:115-227, after its
//                            _topk: the five _transpose_and_gather_feat :96-110, the centre arithmetic, atan2, the masks
//
// PARITY.  Targets: every fp32 operation of the reference's scalar-tensor arithmetic is rounded once and in its order (this file
// is compiled with -ffp-contract=off); Python scalars such as 1 - min_overlap are formed in double on the host and rounded to
// fp32 once, as torch does with a Python scalar operand; square roots go through fp64 (correct rounding whatever the build
// flags); the Gaussian is evaluated in fp64 and rounded to fp32, as numpy's is before torch.from_numpy(...).to(float32).
// log / sin / cos are the device library's.  Losses: mmdet is not part of the reference tree; the formulas are those of
// include/sst_amd.h.
#include "common.h"
#include "head_math.h"

namespace {

constexpr int kCtrThreads = 256;
constexpr int kCtrWaves = kCtrThreads / 64;
constexpr int kTgtBoxTile = 64;      // boxes per workgroup of the targets kernel: one thread each, then one wave per box drawing
constexpr int kTgtLabelTile = 1024;  // labels of the sample per LDS pass of the rank count
constexpr int kHmTile = 4096;        // heatmap cells per workgroup of the loss forward's first launch (16 per thread)
constexpr int kMaxObjs = 4096;       // slots per sample the box backward holds in LDS
constexpr int kLink = 1 << 29, kNoSlot = 1 << 30;  // flags of the box backward's chain words (slots are below 2^29)
constexpr int kBoxThreads = 1024;    // threads of the one-workgroup(-per-sample) box launches: a slot per thread at 500 slots
constexpr int kMaxTasks = SST_CENTER_MAX_TASKS;
constexpr int kHeads = 5;            // reg, height, dim, rot, vel
constexpr int kCode = 10;            // columns of anno_box

// ------------------------------------------------------------------------------------------------------------------
// targets
// ------------------------------------------------------------------------------------------------------------------

struct TargetsArgs {
  const float* boxes;
  const int64_t* labels;
  const int32_t* box_off;
  int64_t n_boxes;
  int cols, batch, n_tasks, W, H, max_objs, min_radius, norm_bbox;
  float osf, pcx, pcy, vsx, vsy;
  float k_1m, k_1p, k_m2, k_16, k_m1;  // 1 - o, 1 + o, -2 o, 4 (4 o), o - 1 of min_overlap o: double on the host, fp32 once
  int first[kMaxTasks], count[kMaxTasks];
  int64_t off[kMaxTasks][4];           // byte offsets of heatmap, anno_box, ind, mask in `out`
  char* out;
};

// gaussian_radius((height, width), min_overlap), gaussian.py:56-85, in the reference's fp32 operation order
__device__ __forceinline__ float gaussian_radius(float height, float width, const TargetsArgs& a) {
  const float hw = height + width;
  const float b1 = hw;
  const float c1 = width * height * a.k_1m / a.k_1p;
  const float sq1 = sst_sqrt_rn(b1 * b1 - 4.f * c1);
  const float r1 = (b1 + sq1) / 2.f;
  const float b2 = 2.f * hw;
  const float c2 = a.k_1m * width * height;
  const float sq2 = sst_sqrt_rn(b2 * b2 - 16.f * c2);
  const float r2 = (b2 + sq2) / 2.f;
  const float b3 = a.k_m2 * hw;
  const float c3 = a.k_m1 * width * height;
  const float sq3 = sst_sqrt_rn(b3 * b3 - a.k_16 * c3);
  const float r3 = (b3 + sq3) / 2.f;
  float r = r1;  // Python's min(r1, r2, r3)
  if (r2 < r) r = r2;
  if (r3 < r) r = r3;
  return r;
}

// One workgroup: kTgtBoxTile boxes of one sample for one task.  Phase 1, one thread per box: the slot (the rank of the box in
// the task's class-grouped list: all boxes of the first class in input order, then the second ...), the slot's ind / mask /
// anno_box, and a drawing record in LDS.  Phase 2, one wave per record: heatmap = max(heatmap, gaussian) over the clipped
// patch, as an integer atomicMax on the bit pattern (the values are positive floats, which order as unsigned integers), so the
// result does not depend on the order the boxes arrive in.
// The reference's `h[h < eps * h.max()] = 0` of gaussian_2d never fires: the exponent is (dx^2 + dy^2) / (2 sigma^2) <=
// 2 r^2 * 18 / (2 r + 1)^2 < 9 for every radius, and exp(-9) is far above the fp64 epsilon.  It is not built.
__global__ __launch_bounds__(kCtrThreads) void center_targets_k(TargetsArgs a) {
  __shared__ int s_cls[kTgtLabelTile];
  __shared__ int d_x[kTgtBoxTile], d_y[kTgtBoxTile], d_r[kTgtBoxTile], d_c[kTgtBoxTile];
  const int tid = threadIdx.x, task = blockIdx.y, s = blockIdx.z;
  const int64_t b0 = max((int64_t)a.box_off[s], (int64_t)0), b1 = min((int64_t)a.box_off[s + 1], a.n_boxes);
  const int64_t j0 = b0 + (int64_t)blockIdx.x * kTgtBoxTile;
  if (j0 >= b1) return;  // uniform over the workgroup
  const int first = a.first[task], count = a.count[task];
  const bool boxer = tid < kTgtBoxTile && j0 + tid < b1;
  const int64_t j = j0 + tid;
  int mine = -1;
  if (boxer) {
    const int64_t lab = a.labels[j] - first;
    mine = lab >= 0 && lab < count ? (int)lab : -1;
  }
  // rank: boxes of the sample in the task with a lower class, or the same class and a lower index
  int rank = 0;
  for (int64_t t0 = b0; t0 < b1; t0 += kTgtLabelTile) {
    const int nt = (int)min((int64_t)kTgtLabelTile, b1 - t0);
    __syncthreads();
    for (int i = tid; i < nt; i += kCtrThreads) {
      const int64_t lab = a.labels[t0 + i] - first;
      s_cls[i] = lab >= 0 && lab < count ? (int)lab : -1;
    }
    __syncthreads();
    if (mine >= 0) {
      const int before = (int)min((int64_t)nt, max(j - t0, (int64_t)0));  // entries of this pass with a lower index
      for (int i = 0; i < nt; ++i) {
        const int c = s_cls[i];
        rank += (c >= 0 && (c < mine || (c == mine && i < before))) ? 1 : 0;
      }
    }
  }
  if (tid < kTgtBoxTile) d_c[tid] = -1;
  if (mine >= 0 && rank < a.max_objs) {
    const float* bx = a.boxes + j * a.cols;
    const float width = bx[3] / a.vsx / a.osf, length = bx[4] / a.vsy / a.osf;
    if (width > 0.f && length > 0.f) {
      float rf = gaussian_radius(length, width, a);
      rf = fminf(rf, 1.0e6f);  // the patch is clipped to the map anyway; keeps the conversion defined
      const int radius = max(a.min_radius, (int)rf);
      const float coor_x = (bx[0] - a.pcx) / a.vsx / a.osf, coor_y = (bx[1] - a.pcy) / a.vsy / a.osf;
      // center.to(int32) truncates toward zero: a centre in (-1, 0) lands in cell 0 and is kept, as in the reference
      if (coor_x > -1.f && coor_x < (float)a.W && coor_y > -1.f && coor_y < (float)a.H) {
        const int x = (int)coor_x, y = (int)coor_y;
        d_x[tid] = x;
        d_y[tid] = y;
        d_r[tid] = radius;
        d_c[tid] = mine;
        const int64_t slot = (int64_t)s * a.max_objs + rank;
        ((int64_t*)(a.out + a.off[task][2]))[slot] = (int64_t)y * a.W + x;
        ((uint8_t*)(a.out + a.off[task][3]))[slot] = 1;
        float* an = (float*)(a.out + a.off[task][1]) + slot * kCode;
        an[0] = coor_x - (float)x;
        an[1] = coor_y - (float)y;
        an[2] = bx[2] + bx[5] * 0.5f;  // gravity_center
        an[3] = a.norm_bbox ? logf(bx[3]) : bx[3];
        an[4] = a.norm_bbox ? logf(bx[4]) : bx[4];
        an[5] = a.norm_bbox ? logf(bx[5]) : bx[5];
        an[6] = sinf(bx[6]);
        an[7] = cosf(bx[6]);
        an[8] = a.cols >= 9 ? bx[7] : 0.f;
        an[9] = a.cols >= 9 ? bx[8] : 0.f;
      }
    }
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  unsigned* hm = (unsigned*)(a.out + a.off[task][0]) + (int64_t)s * count * a.H * a.W;
  for (int k = wave; k < kTgtBoxTile; k += kCtrWaves) {
    const int c = d_c[k];
    if (c < 0) continue;  // uniform over the wave
    const int x = d_x[k], y = d_y[k], r = d_r[k];
    const int left = min(x, r), right = min(a.W - x, r + 1), top = min(y, r), bottom = min(a.H - y, r + 1);
    const int pw = left + right, ph = top + bottom;
    const double sigma = (double)(2 * r + 1) / 6.0;
    const double den = 2.0 * sigma * sigma;
    unsigned* plane = hm + (int64_t)c * a.H * a.W;
    for (int64_t i = lane; i < (int64_t)pw * ph; i += 64) {
      const int py = (int)(i / pw), px = (int)(i - (int64_t)py * pw);
      const int dx = px - left, dy = py - top;
      const float g = (float)exp(-(double)((int64_t)dx * dx + (int64_t)dy * dy) / den);
      atomicMax(plane + (int64_t)(y + dy) * a.W + (x + dx), __float_as_uint(g));
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// losses
// ------------------------------------------------------------------------------------------------------------------

// the code channels (the concatenation of the present heads' channels) as planes: channel c of sample b at cp[c] + b * cbs[c],
// its gradient at the same offset behind gofs[c] in the one allocation of the head gradients
struct BoxArgs {
  const float* cp[kCode];
  int64_t cbs[kCode];    // batch stride of the head that holds the channel, in floats
  int64_t gofs[kCode];
  const float* anno;     // [B, max_objs, 10]
  const int64_t* ind;    // [B, max_objs]
  const uint8_t* mask;   // [B, max_objs]
  int batch, max_objs, n_code;
  int64_t hw;
  float cw[kCode];
};

// One heatmap cell at logit z with target t: the loss term and its derivative in z.
//   p = clamp(sigmoid(z), 1e-4, 1 - 1e-4), q = 1 - p
//   e = -log(p + 1e-12) q^2 [t == 1] - log(q + 1e-12) p^2 (1 - t)^4
// p and q are both formed from exp(-|z|) without a subtraction, so each keeps its relative accuracy at either end.  With
// dp/dz = p q where the clamp is inactive (0 where it is active, as torch's clamp gives):
//   de/dz = [t == 1] q^2 (2 p log(p) - q) + (1 - t)^4 p^2 (p - 2 q log(q))
__device__ __forceinline__ void focal_cell(float z, float t, float& loss, float& dz) {
  float p, q;
  sst_sigmoid_pair(z, p, q);
  const float kLo = 1e-4f;
  bool clamped = false;
  if (p < kLo) {
    p = kLo;
    q = 1.f - kLo;
    clamped = true;
  } else if (q < kLo) {
    q = kLo;
    p = 1.f - kLo;
    clamped = true;
  }
  const float lp = logf(p + 1e-12f), lq = logf(q + 1e-12f);
  const float nt = 1.f - t, nw = (nt * nt) * (nt * nt);
  const bool pos = t == 1.f;
  loss = (pos ? -lp * (q * q) : 0.f) - lq * (p * p) * nw;
  dz = clamped ? 0.f : (pos ? (q * q) * (2.f * p * lp - q) : 0.f) + nw * (p * p) * (p - 2.f * q * lq);
}

// partial record of a workgroup: [0] the sum of its cells' terms (double bits), [1] its count of cells with t == 1
__global__ __launch_bounds__(kCtrThreads) void center_loss_partial_k(const float* __restrict__ logits,
                                                                     const float* __restrict__ target, int64_t n,
                                                                     unsigned long long* __restrict__ partials) {
  __shared__ double wsum[kCtrWaves];
  const int64_t base = (int64_t)blockIdx.x * kHmTile;
  double sum = 0.0, npos = 0.0;
  for (int k = 0; k < kHmTile / kCtrThreads; ++k) {
    const int64_t i = base + k * kCtrThreads + threadIdx.x;
    if (i < n) {
      const float t = target[i];
      float e, dz;
      focal_cell(logits[i], t, e, dz);
      sum += (double)e;
      npos += t == 1.f ? 1.0 : 0.0;
    }
  }
  sum = sst_block_sum(sum, wsum);
  npos = sst_block_sum(npos, wsum);  // integers below 2^53: exact
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = (unsigned long long)__double_as_longlong(sum);
    partials[2 * (int64_t)blockIdx.x + 1] = (unsigned long long)(long long)npos;
  }
}

// one workgroup of kBoxThreads: the records in index order, then the box loss over the B x max_objs slots, a slot per thread:
// its ten predictions are independent loads straight from the NCHW maps
__global__ __launch_bounds__(kBoxThreads) void center_loss_final_k(const unsigned long long* __restrict__ partials, int nb,
                                                                   BoxArgs a, float w_cls, float w_bbox,
                                                                   float* __restrict__ out, int64_t* __restrict__ counts) {
  __shared__ double wsum[kBoxThreads / 64];
  const int tid = threadIdx.x;
  double sum = 0.0, npos = 0.0;
  for (int r = tid; r < nb; r += kBoxThreads) {
    sum += __longlong_as_double((long long)partials[2 * (int64_t)r]);
    npos += (double)(long long)partials[2 * (int64_t)r + 1];
  }
  sum = sst_block_sum(sum, wsum);
  npos = sst_block_sum(npos, wsum);
  double box = 0.0, nmask = 0.0;
  const int64_t slots = (int64_t)a.batch * a.max_objs;
  for (int64_t s = tid; s < slots; s += kBoxThreads) {
    if (a.mask[s] == 0) continue;
    nmask += 1.0;
    const int64_t cell = a.ind[s];
    if (cell < 0 || cell >= a.hw) continue;  // the reference's gather raises; here the slot adds nothing
    const int64_t b = s / a.max_objs;
    float pred[kCode], tgt[kCode];
#pragma unroll
    for (int c = 0; c < kCode; ++c) {
      pred[c] = c < a.n_code ? a.cp[c][b * a.cbs[c] + cell] : 0.f;
      tgt[c] = c < a.n_code ? a.anno[s * kCode + c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < kCode; ++c)
      if (c < a.n_code) box += (double)(fabsf(pred[c] - tgt[c]) * a.cw[c]);
  }
  box = sst_block_sum(box, wsum);
  nmask = sst_block_sum(nmask, wsum);
  if (tid == 0) {
    out[0] = (float)(sum / fmax(npos, 1.0) * (double)w_cls);
    out[1] = (float)(box / (double)((float)nmask + 1e-4f) * (double)w_bbox);  // avg_factor = mask.float().sum() + 1e-4 is fp32
    counts[0] = (int64_t)npos;
    counts[1] = (int64_t)nmask;
  }
}

__global__ __launch_bounds__(kCtrThreads) void center_loss_bwd_hm_k(const float* __restrict__ logits,
                                                                    const float* __restrict__ target, int64_t n,
                                                                    const float* __restrict__ g,
                                                                    const int64_t* __restrict__ counts, float w_cls,
                                                                    float* __restrict__ d_logits) {
  const float k = g ? (float)((double)g[0] * (double)w_cls / fmax((double)counts[0], 1.0)) : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * kCtrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCtrThreads) {
    float e, dz;
    focal_cell(logits[i], target[i], e, dz);
    d_logits[i] = k * dz;
  }
}

// One workgroup of kBoxThreads per sample.  Two slots of a sample can name the same cell: the lowest such slot adds the
// contributions of all of them in slot order and writes the cell, so no two threads write one address and the sum has one order.
// Pass 1, a slot per thread: is a lower slot on my cell, and which is the next higher one (two scans of the sample's inds in
// LDS).  Pass 2, a (slot, channel) pair per thread: the lowest slot of a cell walks the chain of its cell.
__global__ __launch_bounds__(kBoxThreads) void center_loss_bwd_box_k(BoxArgs a, const float* __restrict__ g,
                                                                     const int64_t* __restrict__ counts, float w_bbox,
                                                                     float* __restrict__ d_heads) {
  __shared__ int s_ind[kMaxObjs];
  __shared__ int s_next[kMaxObjs];  // 1 + the next higher slot on the same cell (0: none) | kLink: a lower slot is on the cell | kNoSlot
  __shared__ const float* s_cp[kCode];
  __shared__ int64_t s_cbs[kCode], s_gofs[kCode];
  __shared__ float s_kc[kCode];
  const int b = blockIdx.x;
  const int64_t s0 = (int64_t)b * a.max_objs;
  if (threadIdx.x == 0) {
    const double k_all = (double)g[0] * (double)w_bbox / (double)((float)counts[1] + 1e-4f);
#pragma unroll
    for (int c = 0; c < kCode; ++c) {
      s_cp[c] = a.cp[c];
      s_cbs[c] = a.cbs[c];
      s_gofs[c] = a.gofs[c];
      s_kc[c] = (float)(k_all * (double)a.cw[c]);
    }
  }
  for (int k = threadIdx.x; k < a.max_objs; k += kBoxThreads) {
    const int64_t cell = a.ind[s0 + k];
    s_ind[k] = (a.mask[s0 + k] != 0 && cell >= 0 && cell < a.hw) ? (int)cell : -1;
  }
  __syncthreads();
  int chain[kMaxObjs / kBoxThreads];
#pragma unroll
  for (int i = 0; i < kMaxObjs / kBoxThreads; ++i) {
    const int k = threadIdx.x + i * kBoxThreads;
    chain[i] = kNoSlot;
    if (k >= a.max_objs) continue;
    const int cell = s_ind[k];
    if (cell < 0) continue;
    bool lowest = true;
    for (int j = 0; j < k; ++j) lowest = lowest && s_ind[j] != cell;
    int next = 0;
    for (int j = a.max_objs - 1; j > k; --j) next = s_ind[j] == cell ? j + 1 : next;
    chain[i] = lowest ? next : (next | kLink);
  }
#pragma unroll
  for (int i = 0; i < kMaxObjs / kBoxThreads; ++i) {
    const int k = threadIdx.x + i * kBoxThreads;
    if (k < a.max_objs) s_next[k] = chain[i];
  }
  __syncthreads();
  const int items = a.max_objs * a.n_code;
  for (int item = threadIdx.x; item < items; item += kBoxThreads) {
    const int k = item / a.n_code, c = item - k * a.n_code;
    if (s_next[k] & (kLink | kNoSlot)) continue;  // no slot, or not the lowest of its cell
    const int64_t at = (int64_t)b * s_cbs[c] + s_ind[k];
    const float pred = s_cp[c][at], kc = s_kc[c];
    float acc = 0.f;
    for (int j = k; j >= 0; j = (s_next[j] & (kLink - 1)) - 1) {
      const float diff = pred - a.anno[(s0 + j) * kCode + c];
      acc += diff > 0.f ? kc : diff < 0.f ? -kc : 0.f;
    }
    d_heads[s_gofs[c] + at] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------------------------

struct DecodeArgs {
  const int64_t* inds;   // [B, K]
  const float* scores;   // [B, K]
  const float* reg;      // optional
  const float* hei;
  const float* dim;
  const float* rot_sin;
  const float* rot_cos;
  const float* vel;      // optional
  int64_t bs[6];         // batch strides in floats of reg, hei, dim, rot_sin, rot_cos, vel; channels are hw apart
  int batch, k, W, norm_bbox, has_thr, has_range;
  int64_t hw;
  float osf, vsx, vsy, pcx, pcy, thr;
  float range[6];
};

__global__ __launch_bounds__(kCtrThreads) void center_decode_k(DecodeArgs a, float* __restrict__ boxes,
                                                               uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * kCtrThreads + threadIdx.x;
  if (i >= (int64_t)a.batch * a.k) return;
  const int b = (int)(i / a.k);
  const int cols = a.vel ? 9 : 7;
  float* o = boxes + i * cols;
  const int64_t cell = a.inds[i];
  if (cell < 0 || cell >= a.hw) {  // not an index of the map: no box
    for (int c = 0; c < cols; ++c) o[c] = 0.f;
    keep[i] = 0;
    return;
  }
  // _topk: ys = (inds.float() / width).int().float(), xs = (inds % width).int().float()
  const float ys0 = (float)(int)((float)cell / (float)a.W), xs0 = (float)(int)(cell % a.W);
  const float rx = a.reg ? a.reg[b * a.bs[0] + cell] : 0.5f, ry = a.reg ? a.reg[b * a.bs[0] + a.hw + cell] : 0.5f;
  const float x = (xs0 + rx) * a.osf * a.vsx + a.pcx, y = (ys0 + ry) * a.osf * a.vsy + a.pcy;
  const float z = a.hei[b * a.bs[1] + cell];
  o[0] = x;
  o[1] = y;
  o[2] = z;
  for (int c = 0; c < 3; ++c) {
    const float d = a.dim[b * a.bs[2] + c * a.hw + cell];
    o[3 + c] = a.norm_bbox ? expf(d) : d;
  }
  o[6] = atan2f(a.rot_sin[b * a.bs[3] + cell], a.rot_cos[b * a.bs[4] + cell]);
  if (a.vel) {
    o[7] = a.vel[b * a.bs[5] + cell];
    o[8] = a.vel[b * a.bs[5] + a.hw + cell];
  }
  bool ok = !a.has_thr || a.scores[i] > a.thr;
  if (a.has_range)
    ok = ok && x >= a.range[0] && y >= a.range[1] && z >= a.range[2] && x <= a.range[3] && y <= a.range[4] && z <= a.range[5];
  keep[i] = ok ? 1 : 0;
}

bool task_table_ok(int batch, int n_tasks, const int32_t* task_table, int grid_x, int grid_y, int osf, int max_objs) {
  if (batch < 1 || n_tasks < 1 || n_tasks > kMaxTasks || !task_table || osf < 1 || max_objs < 1) return false;
  if (grid_x / osf < 1 || grid_y / osf < 1) return false;
  for (int t = 0; t < n_tasks; ++t)
    if (task_table[2 * t] < 0 || task_table[2 * t + 1] < 1) return false;
  return true;
}

int64_t targets_layout(int batch, int n_tasks, const int32_t* task_table, int64_t h, int64_t w, int max_objs, int64_t* offsets) {
  int64_t at = 0;
  for (int t = 0; t < n_tasks; ++t) {
    const int64_t slots = (int64_t)batch * max_objs;
    const int64_t bytes[4] = {(int64_t)batch * task_table[2 * t + 1] * h * w * 4, slots * kCode * 4, slots * 8, slots};
    for (int k = 0; k < 4; ++k) {
      if (offsets) offsets[4 * t + k] = at;
      at += sst_align_up(bytes[k], 256);
    }
  }
  return at;
}

}  // namespace

extern "C" int sst_center_targets_box_tile(void) { return kTgtBoxTile; }

extern "C" int64_t sst_center_targets_layout(int batch, int n_tasks, const int32_t* task_table, int grid_x, int grid_y,
                                             int out_size_factor, int max_objs, int64_t* offsets) {
  if (!task_table_ok(batch, n_tasks, task_table, grid_x, grid_y, out_size_factor, max_objs)) return SST_ERR_ARG;
  return targets_layout(batch, n_tasks, task_table, grid_y / out_size_factor, grid_x / out_size_factor, max_objs, offsets);
}

extern "C" int sst_center_targets_f32(const float* d_boxes, int box_cols, const int64_t* d_labels, const int32_t* d_box_offsets,
                                      int64_t n_boxes, int batch, const int32_t* task_table, int n_tasks, int grid_x, int grid_y,
                                      const float* point_cloud_range, const float* voxel_size, int out_size_factor,
                                      double gaussian_overlap, int min_radius, int max_objs, int norm_bbox, void* d_out,
                                      void* stream) {
  if (!task_table_ok(batch, n_tasks, task_table, grid_x, grid_y, out_size_factor, max_objs)) return SST_ERR_ARG;
  if (n_boxes < 0 || !d_box_offsets || !d_out || !point_cloud_range || !voxel_size) return SST_ERR_ARG;
  if (n_boxes > 0 && (!d_boxes || !d_labels)) return SST_ERR_ARG;
  if (box_cols != 7 && box_cols != 9) return SST_ERR_UNSUPPORTED;
  if (!(voxel_size[0] > 0.f) || !(voxel_size[1] > 0.f)) return SST_ERR_ARG;
  if (batch > 65535 || sst_div_up(n_boxes, kTgtBoxTile) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  TargetsArgs a;
  a.boxes = d_boxes;
  a.labels = d_labels;
  a.box_off = d_box_offsets;
  a.n_boxes = n_boxes;
  a.cols = box_cols;
  a.batch = batch;
  a.n_tasks = n_tasks;
  a.W = grid_x / out_size_factor;
  a.H = grid_y / out_size_factor;
  if ((int64_t)a.W * a.H > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  a.max_objs = max_objs;
  a.min_radius = min_radius;
  a.norm_bbox = norm_bbox;
  a.osf = (float)out_size_factor;
  a.pcx = point_cloud_range[0];
  a.pcy = point_cloud_range[1];
  a.vsx = voxel_size[0];
  a.vsy = voxel_size[1];
  const double o = gaussian_overlap;
  a.k_1m = (float)(1 - o);
  a.k_1p = (float)(1 + o);
  a.k_m2 = (float)(-2 * o);
  a.k_16 = (float)(4 * (4 * o));
  a.k_m1 = (float)(o - 1);
  for (int t = 0; t < n_tasks; ++t) {
    a.first[t] = task_table[2 * t];
    a.count[t] = task_table[2 * t + 1];
  }
  int64_t offsets[4 * kMaxTasks];
  const int64_t total = targets_layout(batch, n_tasks, task_table, a.H, a.W, max_objs, offsets);
  for (int t = 0; t < n_tasks; ++t)
    for (int k = 0; k < 4; ++k) a.off[t][k] = offsets[4 * t + k];
  a.out = (char*)d_out;
  hipStream_t s = (hipStream_t)stream;
  SST_HIP(hipMemsetAsync(d_out, 0, (size_t)total, s));
  if (n_boxes == 0) return SST_OK;
  hipLaunchKernelGGL(center_targets_k, dim3((unsigned)sst_div_up(n_boxes, kTgtBoxTile), n_tasks, batch), dim3(kCtrThreads), 0,
                     s, a);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_center_loss_tile_cells(void) { return kHmTile; }

extern "C" int sst_center_loss_max_objs(void) { return kMaxObjs; }

extern "C" int64_t sst_center_loss_workspace_bytes(int64_t n_cells) {
  if (n_cells < 1) return 256;
  return sst_align_up(sst_div_up(n_cells, kHmTile) * 16, 256);
}

static int box_args(BoxArgs& a, const float* const* d_heads, const int32_t* head_channels, const float* d_anno,
                    const int64_t* d_ind, const uint8_t* d_mask, int batch, int max_objs, int64_t hw,
                    const float* code_weights) {
  if (!d_heads || !head_channels || !d_anno || !d_ind || !d_mask || !code_weights) return SST_ERR_ARG;
  if (batch < 1 || max_objs < 1 || hw < 1) return SST_ERR_ARG;
  if (hw > 0x7fffffff || batch > 65535) return SST_ERR_UNSUPPORTED;
  int n_code = 0;
  for (int k = 0; k < kHeads; ++k) {
    if (head_channels[k] < 0 || (head_channels[k] > 0 && !d_heads[k])) return SST_ERR_ARG;
    n_code += head_channels[k];
  }
  if (n_code < 1 || n_code > kCode) return SST_ERR_UNSUPPORTED;
  for (int c = 0; c < kCode; ++c) {
    a.cp[c] = nullptr;
    a.cbs[c] = a.gofs[c] = 0;
    a.cw[c] = code_weights[c];
  }
  int c = 0;
  int64_t head_base = 0;  // floats before the head in the allocation of the gradients
  for (int k = 0; k < kHeads; ++k) {
    for (int i = 0; i < head_channels[k]; ++i, ++c) {
      a.cp[c] = d_heads[k] + (int64_t)i * hw;
      a.cbs[c] = (int64_t)head_channels[k] * hw;
      a.gofs[c] = head_base + (int64_t)i * hw;
    }
    head_base += (int64_t)batch * head_channels[k] * hw;
  }
  a.n_code = n_code;
  a.anno = d_anno;
  a.ind = d_ind;
  a.mask = d_mask;
  a.batch = batch;
  a.max_objs = max_objs;
  a.hw = hw;
  return SST_OK;
}

extern "C" int sst_center_loss_fwd_f32(const float* d_logits, const float* d_heatmap, int batch, int classes, int64_t hw,
                                       const float* const* d_heads, const int32_t* head_channels, const float* d_anno,
                                       const int64_t* d_ind, const uint8_t* d_mask, int max_objs, const float* code_weights,
                                       float weight_cls, float weight_bbox, float* d_out, int64_t* d_counts, void* d_workspace,
                                       void* stream) {
  BoxArgs a;
  const int rc = box_args(a, d_heads, head_channels, d_anno, d_ind, d_mask, batch, max_objs, hw, code_weights);
  if (rc != SST_OK) return rc;
  if (!d_logits || !d_heatmap || classes < 1 || !d_out || !d_counts || !d_workspace) return SST_ERR_ARG;
  const int64_t n = (int64_t)batch * classes * hw;
  if (sst_div_up(n, kHmTile) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  const int nb = (int)sst_div_up(n, kHmTile);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(center_loss_partial_k, dim3(nb), dim3(kCtrThreads), 0, s, d_logits, d_heatmap, n,
                     (unsigned long long*)d_workspace);
  SST_LAUNCH_CHECK();
  hipLaunchKernelGGL(center_loss_final_k, dim3(1), dim3(kBoxThreads), 0, s, (const unsigned long long*)d_workspace, nb, a,
                     weight_cls, weight_bbox, d_out, d_counts);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

extern "C" int sst_center_loss_bwd_f32(const float* d_logits, const float* d_heatmap, int batch, int classes, int64_t hw,
                                       const float* const* d_heads, const int32_t* head_channels, const float* d_anno,
                                       const int64_t* d_ind, const uint8_t* d_mask, int max_objs, const float* code_weights,
                                       float weight_cls, float weight_bbox, const float* d_g_heatmap, const float* d_g_bbox,
                                       const int64_t* d_counts, float* d_dlogits, float* d_dheads, void* stream) {
  BoxArgs a;
  const int rc = box_args(a, d_heads, head_channels, d_anno, d_ind, d_mask, batch, max_objs, hw, code_weights);
  if (rc != SST_OK) return rc;
  if (!d_logits || !d_heatmap || classes < 1 || !d_counts || !d_dlogits || !d_dheads) return SST_ERR_ARG;
  if (max_objs > kMaxObjs) return SST_ERR_UNSUPPORTED;
  const int64_t n = (int64_t)batch * classes * hw;
  hipStream_t s = (hipStream_t)stream;
  SST_HIP(hipMemsetAsync(d_dheads, 0, (size_t)((int64_t)batch * a.n_code * hw) * sizeof(float), s));
  hipLaunchKernelGGL(center_loss_bwd_hm_k, dim3(sst_grid_1d(n, kCtrThreads)), dim3(kCtrThreads), 0, s, d_logits, d_heatmap, n,
                     d_g_heatmap, d_counts, weight_cls, d_dlogits);
  SST_LAUNCH_CHECK();
  if (d_g_bbox) {  // without an upstream gradient of the box loss the zero fill is the whole answer
    hipLaunchKernelGGL(center_loss_bwd_box_k, dim3(batch), dim3(kBoxThreads), 0, s, a, d_g_bbox, d_counts, weight_bbox,
                       d_dheads);
    SST_LAUNCH_CHECK();
  }
  return SST_OK;
}

extern "C" int sst_center_decode_f32(const int64_t* d_inds, const float* d_scores, int batch, int k, int grid_w, int64_t hw,
                                     const float* const* d_maps, const int64_t* batch_strides, int out_size_factor,
                                     const float* voxel_size, const float* pc_range, int norm_bbox, int has_score_threshold,
                                     float score_threshold, const float* post_center_range, float* d_boxes, uint8_t* d_keep,
                                     void* stream) {
  if (batch < 1 || k < 0 || grid_w < 1 || hw < 1 || hw % grid_w != 0 || !d_maps || !batch_strides || !voxel_size || !pc_range)
    return SST_ERR_ARG;
  if (k == 0) return SST_OK;
  if (!d_inds || !d_scores || !d_boxes || !d_keep) return SST_ERR_ARG;
  if (!d_maps[1] || !d_maps[2] || !d_maps[3] || !d_maps[4]) return SST_ERR_ARG;  // height, dim, sine, cosine
  const int64_t min_stride[6] = {2 * hw, hw, 3 * hw, hw, hw, 2 * hw};
  for (int m = 0; m < 6; ++m)
    if (d_maps[m] && batch > 1 && batch_strides[m] < min_stride[m]) return SST_ERR_ARG;
  if (sst_div_up((int64_t)batch * k, kCtrThreads) > 0x7fffffff) return SST_ERR_UNSUPPORTED;
  DecodeArgs a;
  a.inds = d_inds;
  a.scores = d_scores;
  a.reg = d_maps[0];
  a.hei = d_maps[1];
  a.dim = d_maps[2];
  a.rot_sin = d_maps[3];
  a.rot_cos = d_maps[4];
  a.vel = d_maps[5];
  for (int m = 0; m < 6; ++m) a.bs[m] = batch_strides[m];
  a.batch = batch;
  a.k = k;
  a.W = grid_w;
  a.hw = hw;
  a.norm_bbox = norm_bbox;
  a.has_thr = has_score_threshold;
  a.thr = score_threshold;
  a.has_range = post_center_range ? 1 : 0;
  for (int c = 0; c < 6; ++c) a.range[c] = post_center_range ? post_center_range[c] : 0.f;
  a.osf = (float)out_size_factor;
  a.vsx = voxel_size[0];
  a.vsy = voxel_size[1];
  a.pcx = pc_range[0];
  a.pcy = pc_range[1];
  hipLaunchKernelGGL(center_decode_k, dim3((unsigned)sst_div_up((int64_t)batch * k, kCtrThreads)), dim3(kCtrThreads), 0,
                     (hipStream_t)stream, a, d_boxes, d_keep);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

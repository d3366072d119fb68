// (§8 f3) dynamic point pool: for every RoI the points that fall inside the box enlarged by `extra_wlh`, with 13
// box-relative features per (point, RoI) pair -- the extractor in front of FSD's second-stage SIR layers.
//
// Replaces `dynamic_point_pool_ext.forward` / `.dynamic_point_pool_mixed_gpu` as called from
// mmdet3d/ops/dynamic_point_pool_op.py:12-51 and :64-104.  That extension is TorchEx's and is NOT part of the
// reference tree, so the per-pair arithmetic is restated from (a) the box convention of the reference's own
// points-in-boxes kernel (ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-50: bottom-centre z, (w, l, h), local
// frame rotated by rz + pi/2, local x measured against l and local y against w) and (b) the invariants the reference
// asserts on the outputs (roi_extractors/dynamic_point_roi_extractor.py:96-105).  PARITY UNPINNED beyond those.
//
// Where the reference claims output slots with atomics (order and, above the caps, the surviving subset depend on
// the race), this implementation is deterministic: pairs are written sorted by (RoI, point index); a RoI keeps its
// first `max_inbox_point` points and the output its first `max_all_pts` pairs -- one of the outcomes the reference
// can produce.  Three passes: count per (RoI, 1024-point chunk) -> exclusive scans -> recompute and write.
#include "common.h"
#include "pib_test.h"

namespace {

constexpr int kDppChunk = 1024;  // points per workgroup, 4 per thread

// ranks of the set flags of a workgroup in (j, thread) order.  flags: bit j of `bits`.
__device__ __forceinline__ void dpp_block_ranks(int bits, int* __restrict__ lds16, int (&rank)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned long long m = __ballot((bits >> j) & 1);
    rank[j] = __popcll(m & ((1ull << lane) - 1ull));
    cnt[j] = __popcll(m);
  }
  __syncthreads();  // the previous RoI's readers are done with lds16
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) lds16[j * 4 + wave] = cnt[j];
  }
  __syncthreads();
  int run = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if ((k & 3) == wave) rank[k >> 2] += run;
    run += lds16[k];
  }
}

// One workgroup = one chunk of 1024 points (4 per thread, held in registers) x one group of kDppRois RoIs: the
// points are read once per RoI group instead of once per RoI.  A bounding-circle test (5 flops) rejects most pairs
// before the rotation; its radius is inflated so that it can never reject a pair the exact test accepts.
constexpr int kDppRois = 16;

template <bool WRITE>
__global__ __launch_bounds__(256) void dpp_pass_k(const float* __restrict__ rois, const int32_t* __restrict__ rois_batch,
                                                  int n_rois, const float* __restrict__ pts, int64_t ld_pts,
                                                  const int32_t* __restrict__ pts_batch, int n_pts, int n_chunks,
                                                  float ew, float el, float eh, int32_t* __restrict__ cnt,
                                                  const int32_t* __restrict__ off, const int32_t* __restrict__ base,
                                                  int max_inbox, int64_t max_all, int64_t* __restrict__ out_pts_idx,
                                                  int64_t* __restrict__ out_roi_idx, float* __restrict__ out_feats) {
  __shared__ DppBox boxes[kDppRois];
  __shared__ float rad2[kDppRois];
  __shared__ int rbatch[kDppRois];
  __shared__ int wave_cnt[kDppRois][4];
  __shared__ int lds16[16];
  const int c = blockIdx.x % n_chunks, g = blockIdx.x / n_chunks;
  const int r0 = g * kDppRois;
  const int nr = n_rois - r0 < kDppRois ? n_rois - r0 : kDppRois;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)threadIdx.x < nr) {
    const int r = r0 + threadIdx.x;
    const DppBox b = dpp_box(rois + (int64_t)r * 7, ew, el, eh);
    boxes[threadIdx.x] = b;
    const float hl = __fmul_rn(b.ll, 0.5f), hw = __fmul_rn(b.lw, 0.5f);
    rad2[threadIdx.x] = (hl * hl + hw * hw) * 1.001f + 1e-6f;
    rbatch[threadIdx.x] = rois_batch ? rois_batch[r] : 0;
  }
  float px[4], py[4], pz[4];
  int pbatch[4], valid = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = c * kDppChunk + j * 256 + threadIdx.x;
    px[j] = py[j] = pz[j] = 0.f;
    pbatch[j] = 0;
    if (p < n_pts) {
      const float* q = pts + (int64_t)p * ld_pts;
      px[j] = q[0];
      py[j] = q[1];
      pz[j] = q[2];
      if (pts_batch) pbatch[j] = pts_batch[p];
      valid |= 1 << j;
    }
  }
  __syncthreads();
  for (int k = 0; k < nr; ++k) {
    const int r = r0 + k;
    if (WRITE && cnt[(int64_t)r * n_chunks + c] == 0) continue;  // uniform
    const DppBox box = boxes[k];
    const float r2 = rad2[k];
    const int rb = rbatch[k];
    float lx[4], ly[4], lz[4];
    int bits = 0, margin = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dx = px[j] - box.cx, dy = py[j] - box.cy;
      int cls = 0;
      if (((valid >> j) & 1) && pbatch[j] == rb && dx * dx + dy * dy <= r2)
        cls = dpp_classify(box, px[j], py[j], pz[j], lx[j], ly[j], lz[j]);
      bits |= (cls != 0) << j;
      margin |= (cls == 2) << j;
    }
    if (!WRITE) {
      int t = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) t += __popcll(__ballot((bits >> j) & 1));
      if (lane == 0) wave_cnt[k][wave] = t;
      continue;
    }
    int rank[4];
    dpp_block_ranks(bits, lds16, rank);
    const int in_roi0 = off[(int64_t)r * n_chunks + c] - off[(int64_t)r * n_chunks];  // pairs of r in earlier chunks
    const int64_t base_r = base[r];
    const float sl = __fmul_rn(box.l, 0.5f), sw = __fmul_rn(box.w, 0.5f), sh = __fmul_rn(box.h, 0.5f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((bits >> j) & 1)) continue;
      const int in_roi = in_roi0 + rank[j];
      if (in_roi >= max_inbox) continue;
      const int64_t pos = base_r + in_roi;
      if (pos >= max_all) continue;
      out_pts_idx[pos] = (int64_t)c * kDppChunk + j * 256 + threadIdx.x;
      out_roi_idx[pos] = r;
      float* f = out_feats + pos * 13;
      f[0] = px[j];
      f[1] = py[j];
      f[2] = pz[j];
      f[3] = lx[j];
      f[4] = ly[j];
      f[5] = lz[j];
      f[6] = __fadd_rn(lx[j], sl);
      f[7] = __fadd_rn(ly[j], sw);
      f[8] = __fadd_rn(lz[j], sh);
      f[9] = __fsub_rn(sl, lx[j]);
      f[10] = __fsub_rn(sw, ly[j]);
      f[11] = __fsub_rn(sh, lz[j]);
      f[12] = ((margin >> j) & 1) ? 1.f : 0.f;
    }
  }
  if (!WRITE) {
    __syncthreads();
    if ((int)threadIdx.x < nr)
      cnt[(int64_t)(r0 + threadIdx.x) * n_chunks + c] =
          wave_cnt[threadIdx.x][0] + wave_cnt[threadIdx.x][1] + wave_cnt[threadIdx.x][2] + wave_cnt[threadIdx.x][3];
  }
}

// kept[r] = min(pairs of RoI r, max_inbox)
__global__ __launch_bounds__(256) void dpp_kept_k(const int32_t* __restrict__ off, const int32_t* __restrict__ total,
                                                  int n_rois, int n_chunks, int max_inbox, int32_t* __restrict__ kept) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rois) return;
  const int hi = (r + 1 < n_rois) ? off[(int64_t)(r + 1) * n_chunks] : total[0];
  const int t = hi - off[(int64_t)r * n_chunks];
  kept[r] = t < max_inbox ? t : max_inbox;
}

__global__ void dpp_num_out_k(const int32_t* __restrict__ total_kept, int64_t max_all, int64_t* __restrict__ num_out) {
  const int64_t t = total_kept[0];
  num_out[0] = t < max_all ? t : max_all;
}

struct DppLayout {
  int64_t n_blocks, seg_blocks, seg_rois, scan_bytes;
};

DppLayout dpp_layout(int64_t n_rois, int64_t n_pts) {
  DppLayout L;
  const int64_t n_chunks = sst_div_up(n_pts > 0 ? n_pts : 1, kDppChunk);
  L.n_blocks = (n_rois > 0 ? n_rois : 1) * n_chunks;
  L.seg_blocks = sst_align_up(L.n_blocks * (int64_t)sizeof(int32_t), 256);
  L.seg_rois = sst_align_up((n_rois > 0 ? n_rois : 1) * (int64_t)sizeof(int32_t), 256);
  L.scan_bytes = sst_align_up(sst_scan_workspace_bytes(L.n_blocks), 256);
  return L;
}

}  // namespace

extern "C" {

int64_t sst_dynamic_point_pool_workspace_bytes(int64_t n_rois, int64_t n_pts) {
  const DppLayout L = dpp_layout(n_rois, n_pts);
  return 2 * L.seg_blocks + 2 * L.seg_rois + L.scan_bytes + 512;
}

int sst_dynamic_point_pool_f32(const float* d_rois, const int32_t* d_rois_batch, int64_t n_rois, const float* d_pts,
                               int64_t ld_pts, const int32_t* d_pts_batch, int64_t n_pts, const float* extra_wlh,
                               int max_inbox_point, int64_t max_all_pts, int64_t* d_out_pts_idx,
                               int64_t* d_out_roi_idx, float* d_out_feats, int64_t* d_num_out, void* d_workspace,
                               void* stream) {
  if (n_rois < 0 || n_pts < 0 || ld_pts < 3 || max_inbox_point < 0 || max_all_pts < 0 || !extra_wlh || !d_num_out)
    return SST_ERR_ARG;
  if ((d_rois_batch == nullptr) != (d_pts_batch == nullptr)) return SST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (n_rois == 0 || n_pts == 0) {
    SST_HIP(hipMemsetAsync(d_num_out, 0, sizeof(int64_t), st));
    return SST_OK;
  }
  const DppLayout L = dpp_layout(n_rois, n_pts);
  if (n_pts > 0x7fffffff - kDppChunk || L.n_blocks > (1ll << 30)) return SST_ERR_UNSUPPORTED;
  if (!d_rois || !d_pts || !d_workspace || (max_all_pts > 0 && (!d_out_pts_idx || !d_out_roi_idx || !d_out_feats)))
    return SST_ERR_ARG;
  char* ws = (char*)d_workspace;
  int32_t* cnt = (int32_t*)ws;
  int32_t* off = (int32_t*)(ws + L.seg_blocks);
  int32_t* kept = (int32_t*)(ws + 2 * L.seg_blocks);
  int32_t* base = (int32_t*)(ws + 2 * L.seg_blocks + L.seg_rois);
  void* scan_ws = ws + 2 * L.seg_blocks + 2 * L.seg_rois;
  int32_t* totals = (int32_t*)(ws + 2 * L.seg_blocks + 2 * L.seg_rois + L.scan_bytes);  // [0] pairs, [64] kept pairs
  const int n_chunks = (int)sst_div_up(n_pts, kDppChunk);
  const float ew = extra_wlh[0], el = extra_wlh[1], eh = extra_wlh[2];
  const unsigned grid = (unsigned)(sst_div_up(n_rois, kDppRois) * n_chunks);
  hipLaunchKernelGGL(dpp_pass_k<false>, dim3(grid), dim3(256), 0, st, d_rois, d_rois_batch, (int)n_rois, d_pts,
                     ld_pts, d_pts_batch, (int)n_pts, n_chunks, ew, el, eh, cnt, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, max_inbox_point, max_all_pts, (int64_t*)nullptr, (int64_t*)nullptr,
                     (float*)nullptr);
  int rc = sst_exclusive_scan_i32(cnt, off, L.n_blocks, totals, scan_ws, stream);
  if (rc != SST_OK) return rc;
  hipLaunchKernelGGL(dpp_kept_k, dim3((unsigned)sst_div_up(n_rois, 256)), dim3(256), 0, st, off, totals, (int)n_rois,
                     n_chunks, max_inbox_point, kept);
  rc = sst_exclusive_scan_i32(kept, base, n_rois, totals + 64, scan_ws, stream);
  if (rc != SST_OK) return rc;
  hipLaunchKernelGGL(dpp_num_out_k, dim3(1), dim3(1), 0, st, totals + 64, max_all_pts, d_num_out);
  if (max_all_pts > 0 && max_inbox_point > 0)
    hipLaunchKernelGGL(dpp_pass_k<true>, dim3(grid), dim3(256), 0, st, d_rois, d_rois_batch, (int)n_rois, d_pts,
                       ld_pts, d_pts_batch, (int)n_pts, n_chunks, ew, el, eh, cnt, off, base, max_inbox_point,
                       max_all_pts, d_out_pts_idx, d_out_roi_idx, d_out_feats);
  SST_LAUNCH_CHECK();
  return SST_OK;
}

}  // extern "C"

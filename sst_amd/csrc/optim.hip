// The training update: unscale, gradient norm, clip, AdamW and the loss-scale bookkeeping of ALL parameter
// tensors in three launches on one stream - no host read, no device allocation, no float atomics; two runs agree bit for bit.
//
//   1. optim_grad_stats_kernel   sum of squares of g * inv_scale in fp64 and a not-finite flag, one partial record per workgroup
//   2. optim_finalize_kernel     one workgroup: partials in index order -> total_norm, clip_coef, found_inf, the loss scale
//                                (torch.amp.GradScaler.update), the per-tensor step counters and their bias corrections
//   3. optim_adamw_kernel        the update itself; writes nothing when the step is skipped
//
// The work is two tables in device memory: one sst_optim_tensor per tensor that has a gradient, and one sst_optim_chunk per
// slice of at most kChunk elements of one tensor.  A chunk is the unit both element kernels walk: thread t of the workgroup
// owns elements 4 (t + 256 i) ... + 3 of its chunk, whether they are moved with one 16-byte access or four 4-byte ones, so the
// order of every sum and every rounding is the same for any alignment of the tensors.
#include "head_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / SST_WAVE;
constexpr int kChunk = 4096;          // elements per chunk: 4 passes of 256 threads x 4 floats
constexpr int kMaxPartials = 1024;    // grid cap of the element kernels = partial records the finalize kernel stages in LDS
constexpr int kFinalizeThreads = 512;

// the device record (sst_optim_record_bytes() bytes, 8-byte aligned); what every slot means is in include/sst_amd.h
struct OptimRecord {
  double total_norm;
  float clip_coef;
  float inv_scale;
  float scale;
  int32_t found_inf;
  int32_t growth_tracker;
  int32_t skipped_steps;
  double clip_coef64;   // the coefficient before its rounding to fp32: the one the update multiplies by
  double inv_scale64;   // 1 / the scale this step's gradients carry, in fp64
  double reserved[2];
};
static_assert(sizeof(OptimRecord) == 64, "record layout");
static_assert(sizeof(sst_optim_tensor) == 48 && sizeof(sst_optim_chunk) == 16, "table layouts");

// per-tensor scalars of one step, written by the finalize kernel
struct TensorScalars {
  double step_size;   // lr / (1 - b1^t)
  double bc2_sqrt;    // sqrt(1 - b2^t)
};

__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// 1 / scale, as GradScaler forms its inverse scale (in fp64); 1 without a loss scale
__device__ __forceinline__ double inverse_scale(float scale, int scale_mode) {
  return scale_mode == SST_OPTIM_SCALE_NONE ? 1.0 : 1.0 / (double)scale;   // without a loss scale the record's scale is not read
}

// b^t by squaring: exact whenever the powers are representable (b = 0.5, t = 1), relative error below t 2^-53 otherwise
__device__ __forceinline__ double pow_int(double b, unsigned t) {
  double r = 1.0;
  while (t) {
    if (t & 1u) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// four consecutive floats at src + i, zeros behind `count`; one 16-byte load when `vec` and all four exist
__device__ __forceinline__ void load4(const float* __restrict__ src, int i, int count, bool vec, float (&x)[4]) {
  if (vec && i + 4 <= count) {
    const float4 q = *reinterpret_cast<const float4*>(src + i);
    x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = i + j < count ? src[i + j] : 0.f;
  }
}
__device__ __forceinline__ void store4(float* __restrict__ dst, int i, int count, bool vec, const float (&x)[4]) {
  if (vec && i + 4 <= count) {
    *reinterpret_cast<float4*>(dst + i) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < count) dst[i + j] = x[j];
  }
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ------------------------------------------------------------------------------------------------------------------
// 1. gradient statistics
// ------------------------------------------------------------------------------------------------------------------
// partial record of workgroup b: partials[2 b] = the bits of its fp64 sum of squares, partials[2 b + 1] = 1 if it saw a
// not-finite g * inv_scale.  Workgroup b takes chunks b, b + grid, ...; a thread adds its elements in index order.
__global__ void __launch_bounds__(kThreads) optim_grad_stats_kernel(const sst_optim_tensor* __restrict__ tensors,
                                                                    const sst_optim_chunk* __restrict__ chunks, int64_t n_chunks,
                                                                    const OptimRecord* __restrict__ rec, int scale_mode,
                                                                    unsigned long long* __restrict__ partials) {
  __shared__ double wsum[1][kWaves];
  const double inv = inverse_scale(rec->scale, scale_mode);
  double acc = 0.0;
  int bad = 0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const sst_optim_chunk ck = chunks[c];
    const float* g = tensors[ck.tensor].g + ck.start;
    const bool vec = aligned16(g);
    for (int i = (int)threadIdx.x * 4; i < ck.count; i += kThreads * 4) {
      float x[4];
      load4(g, i, ck.count, vec, x);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double y = (double)x[j] * inv;   // a zero behind the chunk's end adds +0.0: the sum keeps its bits
        bad |= (int)not_finite((float)y);     // the unscaled gradient as fp32 holds it: inf, NaN or overflow
        acc += y * y;
      }
    }
  }
  const double w = sst_wave_sum(acc);
  const int any_bad = __syncthreads_or(bad);
  if (sst_lane() == 0) wsum[0][threadIdx.x >> 6] = w;
  __syncthreads();
  unsigned long long* rec_out = partials + 2 * (int64_t)blockIdx.x;
  sst_write_record<kWaves, 1>(wsum, rec_out);
  if (threadIdx.x == 0) rec_out[1] = any_bad ? 1ull : 0ull;
}

// ------------------------------------------------------------------------------------------------------------------
// 2. finalize
// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFinalizeThreads) optim_finalize_kernel(const sst_optim_tensor* __restrict__ tensors,
                                                                          int64_t n_tensors, int n_partials,
                                                                          const sst_optim_hyper h, float* __restrict__ steps,
                                                                          OptimRecord* __restrict__ rec,
                                                                          const unsigned long long* __restrict__ partials,
                                                                          TensorScalars* __restrict__ scalars) {
  __shared__ double part[kMaxPartials];
  int bad = 0;
  for (int i = threadIdx.x; i < n_partials; i += kFinalizeThreads) {
    part[i] = __longlong_as_double((long long)partials[2 * i]);
    bad |= (int)(partials[2 * i + 1] != 0);
  }
  const int found_inf = __syncthreads_or(bad) ? 1 : 0;   // also the barrier behind the writes of part[]
  const bool skip = found_inf && h.skip_nonfinite;

  if (threadIdx.x == 0) {
    // wave 0, lane 0: the partials in index order, the coefficient and the loss scale, while the other waves do the counters
    double s = 0.0;
    for (int i = 0; i < n_partials; ++i) s += part[i];
    const double total_norm = sqrt(s);
    double coef = 1.0;
    if (h.max_norm >= 0.0) {
      const double c = h.max_norm / (total_norm + 1e-6);
      coef = c < 1.0 ? c : (c != c ? c : 1.0);            // min(1, c) that lets a NaN through, as torch's clamp does
    }
    const float scale = rec->scale;
    float new_scale = scale;
    int tracker = rec->growth_tracker;
    if (h.scale_mode == SST_OPTIM_SCALE_DYNAMIC) {        // torch.amp.GradScaler.update (_amp_update_scale_)
      if (found_inf) {
        new_scale = scale * (float)h.backoff_factor;
        tracker = 0;
      } else if (++tracker == h.growth_interval) {
        const float grown = scale * (float)h.growth_factor;
        if (!not_finite(grown)) new_scale = grown;
        tracker = 0;
      }
    }
    rec->total_norm = total_norm;
    rec->clip_coef = (float)coef;
    rec->clip_coef64 = coef;
    rec->inv_scale64 = inverse_scale(scale, h.scale_mode);
    rec->inv_scale = (float)rec->inv_scale64;                // the scale this step's gradients carry
    rec->scale = new_scale;
    rec->found_inf = found_inf;
    rec->growth_tracker = tracker;
    rec->skipped_steps += skip ? 1 : 0;
  }
  if (threadIdx.x >= SST_WAVE) {
    for (int64_t i = threadIdx.x - SST_WAVE; i < n_tensors; i += kFinalizeThreads - SST_WAVE) {
      const sst_optim_tensor t = tensors[i];
      float step = steps[t.slot];
      if (!skip) steps[t.slot] = (step += 1.f);
      const unsigned n = step >= 1.f ? (unsigned)step : 1u;   // a skipped first step: its scalars are never read
      TensorScalars sc;
      sc.step_size = h.lr[t.group] / (1.0 - pow_int(h.b1[t.group], n));
      sc.bc2_sqrt = sqrt(1.0 - pow_int(h.b2[t.group], n));
      scalars[i] = sc;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// 3. AdamW
// ------------------------------------------------------------------------------------------------------------------
// One element.  The stated order of operations, each evaluated in fp64 on the fp32 operands and the fp64 scalars, and p, m, v
// rounded to fp32 once: every result is the correctly rounded value of the float64 restatement (half an fp32 ulp).  The same
// order in fp32 arithmetic - four or more roundings per quantity, and torch's own lerp_ form of m likewise - is up to 1.2 - 2 ulp
// off on a lone element, which the parity margin of a one-element tensor (1 ulp when torch's own error happens to be small) does
// not allow: measured, 74 respectively 1 of 4500 quantities of 1500 one-element tensors missed it.  The kernel
// moves 28 bytes per element; what the fp64 root and the two fp64 divisions cost beside that traffic is not measured apart.
struct GroupScalars {
  double decay, b1, omb1, b2, omb2, eps;
};

__device__ __forceinline__ void adamw_elem(float gf, float& pf, float& mf, float& vf, double inv, double coef,
                                           const GroupScalars& k, const TensorScalars& s) {
  const double g = (double)gf * inv * coef;
  double p = (double)pf * k.decay;
  const double m = k.b1 * (double)mf + k.omb1 * g;
  const double v = k.b2 * (double)vf + k.omb2 * g * g;
  p = p - s.step_size * m / (sqrt(v) / s.bc2_sqrt + k.eps);
  pf = (float)p, mf = (float)m, vf = (float)v;
}

__global__ void __launch_bounds__(kThreads) optim_adamw_kernel(const sst_optim_tensor* __restrict__ tensors,
                                                               const sst_optim_chunk* __restrict__ chunks, int64_t n_chunks,
                                                               const sst_optim_hyper h, const OptimRecord* __restrict__ rec,
                                                               const TensorScalars* __restrict__ scalars) {
  if (rec->found_inf && h.skip_nonfinite) return;   // a skipped step writes nothing
  const double inv = rec->inv_scale64, coef = rec->clip_coef64;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const sst_optim_chunk ck = chunks[c];
    const sst_optim_tensor t = tensors[ck.tensor];
    const TensorScalars s = scalars[ck.tensor];
    const int gi = t.group;
    GroupScalars k;
    k.decay = 1.0 - h.lr[gi] * h.wd[gi];
    k.b1 = h.b1[gi], k.omb1 = 1.0 - h.b1[gi];
    k.b2 = h.b2[gi], k.omb2 = 1.0 - h.b2[gi];
    k.eps = h.eps[gi];
    float* p = t.p + ck.start;
    const float* g = t.g + ck.start;
    float* m = t.m + ck.start;
    float* v = t.v + ck.start;
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
    for (int i = (int)threadIdx.x * 4; i < ck.count; i += kThreads * 4) {
      float xp[4], xg[4], xm[4], xv[4];
      load4(p, i, ck.count, vec, xp);
      load4(g, i, ck.count, vec, xg);
      load4(m, i, ck.count, vec, xm);
      load4(v, i, ck.count, vec, xv);
#pragma unroll
      for (int j = 0; j < 4; ++j) adamw_elem(xg[j], xp[j], xm[j], xv[j], inv, coef, k, s);
      store4(p, i, ck.count, vec, xp);
      store4(m, i, ck.count, vec, xm);
      store4(v, i, ck.count, vec, xv);
    }
  }
}

int element_grid(int64_t n_chunks) { return (int)(n_chunks < kMaxPartials ? n_chunks : kMaxPartials); }

}  // namespace

extern "C" {

int sst_optim_chunk_elems(void) { return kChunk; }
int sst_optim_max_groups(void) { return SST_OPTIM_MAX_GROUPS; }
int sst_optim_record_bytes(void) { return (int)sizeof(OptimRecord); }

int64_t sst_optim_workspace_bytes(int64_t n_tensors) {
  if (n_tensors < 0) return SST_ERR_ARG;
  sst_carver c(nullptr);
  c.take<unsigned long long>(2 * kMaxPartials);
  c.take<TensorScalars>(n_tensors);
  return c.off;
}

int sst_optim_step_f32(const sst_optim_tensor* d_tensors, int64_t n_tensors, const sst_optim_chunk* d_chunks, int64_t n_chunks,
                       const sst_optim_hyper* hyper, float* d_steps, void* d_record, void* d_workspace, void* stream) {
  if (!hyper || !d_record || !d_workspace || n_tensors < 0 || n_chunks < 0) return SST_ERR_ARG;
  if ((n_tensors > 0 && (!d_tensors || !d_steps)) || (n_chunks > 0 && (!d_chunks || n_tensors == 0))) return SST_ERR_ARG;
  if (n_tensors > INT32_MAX) return SST_ERR_UNSUPPORTED;
  if (hyper->n_groups < 1 || hyper->n_groups > SST_OPTIM_MAX_GROUPS) return SST_ERR_ARG;
  if (hyper->scale_mode < SST_OPTIM_SCALE_NONE || hyper->scale_mode > SST_OPTIM_SCALE_DYNAMIC) return SST_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  sst_carver c(d_workspace);
  unsigned long long* partials = c.take<unsigned long long>(2 * kMaxPartials);
  TensorScalars* scalars = c.take<TensorScalars>(n_tensors);
  OptimRecord* rec = (OptimRecord*)d_record;
  const int grid = element_grid(n_chunks);
  if (grid > 0) {
    optim_grad_stats_kernel<<<grid, kThreads, 0, s>>>(d_tensors, d_chunks, n_chunks, rec, hyper->scale_mode, partials);
    SST_LAUNCH_CHECK();
  }
  optim_finalize_kernel<<<1, kFinalizeThreads, 0, s>>>(d_tensors, n_tensors, grid, *hyper, d_steps, rec, partials, scalars);
  SST_LAUNCH_CHECK();
  if (grid > 0) {
    optim_adamw_kernel<<<grid, kThreads, 0, s>>>(d_tensors, d_chunks, n_chunks, *hyper, rec, scalars);
    SST_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"

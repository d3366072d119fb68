// fp32 arithmetic that must equal its numpy float32 restatement bit for bit, shared by the clustering kernels (cluster.hip,
// fps.hip) and, through head_math.h, by the head files.  What the build gives, not what the intrinsic names suggest:
//   - In this toolchain's __clang_hip_math.h, without OCML_BASIC_ROUNDED_OPERATIONS (which nothing here defines), __fadd_rn,
//     __fsub_rn, __fmul_rn and __fdiv_rn are the plain operators +, -, *, / and __fsqrt_rn is __ocml_native_sqrt_f32, a bare
//     v_sqrt_f32 with about one ulp of error.  The names pin nothing.
//   - The plain operators round each operation on its own exactly when the compiler may not contract them: the pragma below
//     covers every function of this header and the rest of a file that includes it, and the Makefile builds the files that
//     rely on it with -ffp-contract=off as well.  `/` on fp32 is the correctly rounded division under the compiler's default
//     (-fhip-fp32-correctly-rounded-divide-sqrt); no file here turns that off.
//   - The root is taken in fp64 and rounded once more, which is the correctly rounded fp32 root under any flags.
// Measured on an MI355X before this header existed (tests/test_gpu_cluster_boundary.py on the __fsqrt_rn kernels): the bare
// v_sqrt_f32 decided `sqrt(s) < t` wrongly at 81 of 262 thresholds t, always for the one s with sqrt_rn(s) == t exactly.
#pragma once
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

namespace {

// The correctly rounded fp32 root: the fp64 root of an fp32 number, rounded to fp32, is the exact rounding
// (53 >= 2 * 24 + 2 bits) whatever the build flags are.
__device__ __forceinline__ float sst_sqrt_rn(float v) { return (float)sqrt((double)v); }

// sqrt(dx * dx + dy * dy) of a - b in the xy plane as numpy evaluates it in float32: subtract, two products, one sum, each
// rounded on its own, then the correctly rounded root.  The edge tests `< dist`, `< thr2`, `< radius` compare this value.
__device__ __forceinline__ float sst_xy_dist(float ax, float ay, float bx, float by) {
  const float dx = ax - bx, dy = ay - by;
  const float xx = dx * dx, yy = dy * dy;
  return sst_sqrt_rn(xx + yy);
}

}  // namespace

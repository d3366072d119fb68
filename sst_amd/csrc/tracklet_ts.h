// The timestamp lookup of the CTRL tracklet kernels (tracklet.hip, tracklet_prep.hip): timestamps are int64 microseconds
// (about 1.5e15), ascending within a tracklet, and are compared as int64 - never through a float.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace {

// position of t in the ascending list ts[0 .. n), -1 if absent
__device__ __forceinline__ int find_ts(const int64_t* __restrict__ ts, int n, int64_t t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ts[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ts[lo] == t ? lo : -1;
}

}  // namespace

// The tile machinery of the segmented reduction over long, uneven groups, shared by seg_tiles_k (csrc/scatter.hip) and the fused
// SIR stage (csrc/sir_stage.hip): a workgroup owns a TILE of consecutive sorted positions of a grouping's CSR, whatever groups
// they belong to:
//   * a row lane walks kSegSpan consecutive sorted rows, reducing runs of equal group id (seg_span_walk); a run that begins and
//     ends strictly inside a lane's span is a whole group: written straight to the output;
//   * the first and the last run of every lane meet in LDS, where lane 0's threads merge them in order (seg_tile_merge): groups
//     that are whole inside the tile are written out; a run that began before the tile (record 0) or continues behind it
//     (record 1) goes to a global record;
//   * a group that crosses tiles is finished by the LAST of its tiles to arrive (seg_tile_finish: one atomic ticket per crossing
//     group and tile, in a per-grouping counter array that is zeroed once and cleans itself): that workgroup merges the group's
//     records with all its threads, in a fixed order.
// Deterministic: every merge order is fixed, MAX carries (value, row) and prefers the smaller row on ties.  No float atomics,
// nothing spins.
#pragma once
#include <math.h>
#include "common.h"

constexpr int kSegSpan = 8;       // rows per row lane
constexpr int kSegNone = -3;      // "no record" (group ids are >= -1: -1 = rows of a discarded group)

struct seg_rec {                  // partial result of a run, one channel vector
  float4 v;
  int4 a;
};

// Records travel between workgroups that may run on different XCDs, whose L2s are not coherent with each other: they are
// written and read with AGENT-scope accesses (`sc1`: the store writes through to, the load reads from, the point that is
// coherent for the whole device), 16 bytes at a time, and the writer waits for its stores (s_waitcnt vmcnt(0)) BEFORE the
// workgroup takes the group's ticket.  History: the relaxed atomic load / store builtins compiled to one scoped access
// followed by seven plain ones; word-wise atomic exchanges worked only once their results were consumed (a fire-and-forget
// exchange is not ordered before the ticket by a workgroup-scope fence, which is `s_waitcnt lgkmcnt(0)` on this target:
// 1-8 % of the launches at 50 000 x 256 gave one wrong group) and cost 8 atomics per lane and record (a 160 000-row
// reduction spent most of its 93 us in them); a device-scope FENCE (__threadfence) writes back the whole L2 of the XCD and
// serialised the launch (50 us for 10 MB).
__device__ __forceinline__ void seg_rec_store(seg_rec* p, const seg_rec& r) {
  typedef float seg_f4 __attribute__((ext_vector_type(4)));
  typedef int seg_i4 __attribute__((ext_vector_type(4)));
  const seg_f4 v = {r.v.x, r.v.y, r.v.z, r.v.w};
  const seg_i4 a = {r.a.x, r.a.y, r.a.z, r.a.w};
  asm volatile(
      "global_store_dwordx4 %0, %1, off sc1\n\t"
      "global_store_dwordx4 %0, %2, off offset:16 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      :
      : "v"(p), "v"(v), "v"(a)
      : "memory");
}
__device__ __forceinline__ seg_rec seg_rec_load(const seg_rec* p) {
  typedef float seg_f4 __attribute__((ext_vector_type(4)));
  typedef int seg_i4 __attribute__((ext_vector_type(4)));
  seg_f4 v;
  seg_i4 a;
  asm volatile(
      "global_load_dwordx4 %0, %2, off sc1\n\t"
      "global_load_dwordx4 %1, %2, off offset:16 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v), "=&v"(a)
      : "v"(p)
      : "memory");
  seg_rec r;
  r.v = make_float4(v.x, v.y, v.z, v.w);
  r.a = make_int4(a.x, a.y, a.z, a.w);
  return r;
}

// (v, a) <- merge((v, a), (w, b)); MAX: larger value, on ties the smaller row index (order-independent)
__device__ __forceinline__ void seg_merge(int mode, float4& v, int4& a, const float4& w, const int4& b) {
  if (mode == SST_REDUCE_MAX) {
    if (w.x > v.x || (w.x == v.x && b.x < a.x)) v.x = w.x, a.x = b.x;
    if (w.y > v.y || (w.y == v.y && b.y < a.y)) v.y = w.y, a.y = b.y;
    if (w.z > v.z || (w.z == v.z && b.z < a.z)) v.z = w.z, a.z = b.z;
    if (w.w > v.w || (w.w == v.w && b.w < a.w)) v.w = w.w, a.w = b.w;
  } else {
    v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
    a.x += b.x;                   // SUM / MEAN: a.x counts the rows merged so far
  }
}

template <int V>                  // channel vector width: 4 (16-byte accesses) or 1
__device__ __forceinline__ void seg_write(int mode, float* __restrict__ out, int32_t* __restrict__ argmax, int c, int64_t g,
                                          int ch, float4 v, int4 a) {
  if (mode == SST_REDUCE_MEAN) {
    const float cnt = (float)a.x;   // rows of the group (every row was merged exactly once)
    v.x = v.x / cnt, v.y = v.y / cnt, v.z = v.z / cnt, v.w = v.w / cnt;
  }
  if (V == 4) {
    *(float4*)(out + g * c + ch) = v;
    if (mode == SST_REDUCE_MAX && argmax != nullptr) *(int4*)(argmax + g * c + ch) = a;
  } else {
    out[g * c + ch] = v.x;
    if (mode == SST_REDUCE_MAX && argmax != nullptr) argmax[g * c + ch] = a.x;
  }
}

// One row lane's span of `cnt` <= kSegSpan sorted rows (row indices, group ids and values already in registers), channel vector
// q of cv: runs of equal group id inside the span: run 0 -> record 0, the last run (if there is a second one) -> record 1, the
// runs between them are whole groups.  lrec [lanes][2][cv], lgrp [lanes][2] in LDS.
template <int V>
__device__ __forceinline__ void seg_span_walk(int mode, int cnt, const uint32_t (&rows)[kSegSpan], const int (&grp)[kSegSpan],
                                              const float4 (&x)[kSegSpan], const float4 ident, const int4 noarg,
                                              float* out, int32_t* argmax, int c, int ch, int lane, int q,
                                              int cv, seg_rec* lrec, int* lgrp) {
  int cur = grp[0], n_closed = 0, first_grp = kSegNone;
  float4 acc = ident;
  int4 arg = noarg;
  seg_rec first;
  first.v = ident, first.a = noarg;
#pragma unroll
  for (int i = 0; i < kSegSpan; ++i) {
    if (i < cnt) {
      if (grp[i] != cur) {   // the run `cur` just ended
        if (n_closed == 0) {
          first.v = acc, first.a = arg, first_grp = cur;
        } else if (cur >= 0) {
          seg_write<V>(mode, out, argmax, c, cur, ch, acc, arg);
        }
        ++n_closed;
        cur = grp[i];
        acc = ident;
        arg = noarg;
      }
      const int r = mode == SST_REDUCE_MAX ? (int)rows[i] : 1;
      seg_merge(mode, acc, arg, x[i], make_int4(r, r, r, r));
    }
  }
  seg_rec last;
  last.v = acc, last.a = arg;
  int last_grp = cur;
  if (cnt == 0) {
    first_grp = last_grp = kSegNone;
  } else if (n_closed == 0) {   // the span is one run: its only record is record 0
    first = last;
    first_grp = cur;
    last_grp = kSegNone;
  }
  lrec[(lane * 2 + 0) * cv + q] = first;
  lrec[(lane * 2 + 1) * cv + q] = last;
  if (q == 0) {
    lgrp[lane * 2 + 0] = first_grp;
    lgrp[lane * 2 + 1] = last_grp;
  }
}

// Lane 0's threads merge the lane records of their channel vector in row order (call behind a barrier that follows the walks).
// before / behind: groups of the sorted rows right before / right behind the tile (kSegNone: none); tile_recs: the tile's two
// global records [2][cv]; tile_grp [2]: groups of the tile's two boundary records (preset to kSegNone).
template <int V>
__device__ __forceinline__ void seg_tile_merge(int mode, int lanes, int cv, int q, int ch, int c, const seg_rec* lrec,
                                               const int* lgrp, const int before, const int behind, const float4 ident,
                                               const int4 noarg, float* out, int32_t* argmax,
                                               seg_rec* tile_recs, int* tile_grp) {
  int cur = kSegNone;
  float4 acc = ident;
  int4 arg = noarg;
  bool first_run = true;
  auto close_run = [&](bool last_run) {
    const bool was_first = first_run;
    first_run = false;
    if (cur < 0) return;                 // nothing yet, or rows of a discarded group
    // the groups are contiguous in sorted order: a run goes on outside the tile iff the neighbouring row has its id
    const bool starts_here = !(was_first && cur == before), ends_here = !(last_run && cur == behind);
    if (starts_here && ends_here) {
      seg_write<V>(mode, out, argmax, c, cur, ch, acc, arg);
    } else {
      const int slot = starts_here ? 1 : 0;    // began before the tile: record 0; begins here and goes on: record 1
      seg_rec r;
      r.v = acc, r.a = arg;
      seg_rec_store(tile_recs + (int64_t)slot * cv + q, r);
      if (q == 0) tile_grp[slot] = cur;
    }
  };
  for (int l = 0; l < lanes; ++l) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int g = lgrp[l * 2 + h];
      if (g == kSegNone) continue;
      const seg_rec r = lrec[(l * 2 + h) * cv + q];
      if (cur == kSegNone) {
        cur = g;
        acc = r.v;
        arg = r.a;
      } else if (g != cur) {
        close_run(false);
        cur = g;
        acc = r.v;
        arg = r.a;
      } else {
        seg_merge(mode, acc, arg, r.v, r.a);
      }
    }
  }
  if (cur != kSegNone) close_run(true);
}

// Groups that cross tiles: the last of their tiles to arrive merges their records.  Called by EVERY thread of the workgroup
// (lane = tid / cv may be >= lanes).  recs [tiles][2][cv]; finish: int [3] in LDS.
template <int V>
__device__ __forceinline__ void seg_tile_finish(int mode, int lanes, int cv, int lane, int q, int ch, int c, int tile_rows,
                                                const int32_t* offsets, int32_t* counters,
                                                const seg_rec* recs, seg_rec* lrec, const int* tile_grp,
                                                int* finish, const float4 ident, const int4 noarg, float* out,
                                                int32_t* argmax) {
  // every record store above waited for its own completion (seg_rec_store); the barrier then orders all of them, in every
  // thread, before the tickets are taken
  __syncthreads();
#pragma unroll 1
  for (int slot = 0; slot < 2; ++slot) {
    const int g = tile_grp[slot];
    if (g < 0) continue;   // uniform
    if (threadIdx.x == 0) {
      const int ta = offsets[g] / tile_rows, tb = (offsets[g + 1] - 1) / tile_rows;
      const int before = atomicAdd(counters + g, 1);
      const int fin = before == tb - ta;       // tb - ta + 1 tiles hold a record of g
      if (fin) atomicExch(counters + g, 0);    // every other tile of g has already taken its ticket
      finish[0] = fin, finish[1] = ta, finish[2] = tb;
    }
    __syncthreads();
    if (finish[0]) {
      const int ta = finish[1], tb = finish[2];
      float4 acc = ident;
      int4 arg = noarg;
      if (lane < lanes) {
        for (int t = ta + lane; t <= tb; t += lanes) {
          const seg_rec r = seg_rec_load(recs + ((int64_t)t * 2 + (t == ta ? 1 : 0)) * cv + q);
          seg_merge(mode, acc, arg, r.v, r.a);
        }
        seg_rec r;
        r.v = acc, r.a = arg;
        lrec[lane * cv + q] = r;
      }
      __syncthreads();
      if (lane == 0) {
        for (int l = 1; l < lanes; ++l) {
          const seg_rec r = lrec[l * cv + q];
          seg_merge(mode, acc, arg, r.v, r.a);
        }
        seg_write<V>(mode, out, argmax, c, g, ch, acc, arg);
      }
    }
    __syncthreads();
  }
}

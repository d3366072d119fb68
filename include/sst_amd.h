/*
 * sst_amd.h — C ABI of libsst_amd.so: the MI355X (gfx950) implementation of the SST / FSD sparse
 * hot path (dynamic voxelization -> point->voxel scatter -> window bucketing -> Sparse Regional
 * Attention core -> SIR segmented max).
 *
 * Conventions
 *   - Every pointer named d_* is a DEVICE pointer (HBM). h_* pointers are host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream). All work is
 *     enqueued on that stream; no entry point synchronises the device unless its comment says so.
 *   - All buffers are owned by the caller (reference contract: tensors are caller/allocator owned,
 *     SURVEY.md §8b "Ownership"). Workspaces are sized with the matching *_workspace_bytes().
 *   - Return value: 0 on success, a positive hipError_t value if the HIP runtime reported an error,
 *     or a negative SST_ERR_* code for an argument the library refuses.
 *   - Row-major, contiguous unless a stride argument (in elements) is given.
 *
 * Each entry point cites the reference interface (file:line under the reference tree) it replaces.
 */
#ifndef SST_AMD_H
#define SST_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SST_OK 0
#define SST_ERR_ARG (-1)          /* invalid argument (null pointer, negative size, bad mode)        */
#define SST_ERR_UNSUPPORTED (-2)  /* shape outside what the kernels are built for                    */
#define SST_ERR_KEYSPACE (-3)     /* coordinates do not pack into 63 bits                             */

typedef enum { SST_REDUCE_SUM = 0, SST_REDUCE_MEAN = 1, SST_REDUCE_MAX = 2 } sst_reduce_t;

/* Library self-description: returns a static string "sst_amd <version> gfx950". */
const char* sst_version(void);

/* ------------------------------------------------------------------------------------------------
 * (a1) dynamic voxelization.
 * Replaces voxel_layer.dynamic_voxelize (mmdet3d/ops/voxel/src/voxelization.h:71-83 ->
 * dynamic_voxelize_gpu, voxelization_cuda.cu:332-375, kernel :24-65).
 *   c[d] = clamp((int)floorf((p[d] - range[d]) / voxel_size[d]), 0, grid[d]-1), fp32 subtract then
 *   fp32 IEEE divide; grid[d] = ceil((range[d+3]-range[d]) / voxel_size[d]) in fp32 (cuda.cu:355-357);
 *   THIS FORK clamps out-of-range points into the border voxel (cuda.cu:37-59).
 * d_points: [n, row_stride] fp32, columns 0..2 = x,y,z.  d_coors: [n, coors_stride] int32; columns
 * coors_col0..coors_col0+2 receive (z, y, x).  If batch_idx >= 0 and coors_col0 == 1, column 0 is
 * filled with batch_idx (fuses DynamicVoxelNet.voxelize's F.pad, detectors/dynamic_voxelnet.py:49-71).
 * ---------------------------------------------------------------------------------------------- */
int sst_dynamic_voxelize_f32(const float* d_points, int64_t n, int64_t row_stride,
                             const float voxel_size[3], const float coors_range[6],
                             int32_t* d_coors, int64_t coors_stride, int coors_col0, int batch_idx,
                             void* stream);
/* Host helper: the grid the kernel clamps to (fp32 ceil, as voxelization_cuda.cu:355-357). */
void sst_dynamic_voxelize_grid(const float voxel_size[3], const float coors_range[6], int32_t grid_xyz[3]);

/* ------------------------------------------------------------------------------------------------
 * Device primitives shared by the unique / bucketing steps (exported so they can be tested alone).
 * ---------------------------------------------------------------------------------------------- */
/* Exclusive prefix sum of int32.  d_out may alias d_in.  d_total (optional, device int32) receives
 * the grand total.  Workspace: sst_scan_workspace_bytes(n). */
int64_t sst_scan_workspace_bytes(int64_t n);
int sst_exclusive_scan_i32(const int32_t* d_in, int32_t* d_out, int64_t n, int32_t* d_total,
                           void* d_workspace, void* stream);

/* Stable LSD radix sort of (key, index) pairs on the low `key_bits` bits of 64-bit keys.
 * On return d_keys_out is sorted ascending and d_perm_out[i] is the original position of the i-th
 * smallest key (ties in ascending original position).  d_keys_in is clobbered (used as ping-pong).
 * Workspace: sst_sort_workspace_bytes(n). */
int64_t sst_sort_workspace_bytes(int64_t n);
int sst_sort_pairs_u64(uint64_t* d_keys_in, uint64_t* d_keys_out, uint32_t* d_perm_out, int64_t n,
                       int key_bits, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a3/a5) sorted-unique of integer coordinate rows — the part of
 *   dynamic_point_to_voxel_forward_gpu that calls at::unique_dim (scatter_points_cuda.cu:202-205) and of
 *   scatter_v2 that calls torch.unique(dim=0) (ops/sst/sst_ops.py:151-165).
 * Rows are packed into one 64-bit key  key = 1 + sum_j (c_j - mins[j]) * stride_j  (last column fastest),
 * so ascending key order == lexicographic row order.  With invalid_if_negative != 0, any row with a
 * negative entry gets key 0 (the reference's coors.masked_fill(any(<0), -1): all such rows collapse
 * into ONE group that sorts first, scatter_points_cuda.cu:200).
 * invalid_if_negative == 2 is the batched form (DynamicScatter.forward's per-sample loop,
 * ops/voxel/scatter_points.py:85-99, done in one pass): column 0 is the batch index, the validity test
 * looks at columns 1.., and an invalid row becomes (b,-1,-1,...) — pass mins[j>=1] = -1 so that it sorts
 * first inside its own sample.
 * coor_is_i64: 0 -> int32 rows, 1 -> int64 rows.   extents[j] = (max_j - mins[j] + 1) upper bound.
 * Outputs (all device, caller allocated):
 *   d_perm   [n]   uint32  row indices grouped by unique row, ascending row index inside a group
 *   d_inverse[n]   int32   group id of every input row (== torch.unique's inverse)
 *   d_offsets[n+1] int32   CSR offsets into d_perm; entries 0..M valid
 *   d_ukeys  [n]   uint64  packed key of each group; entries 0..M-1 valid
 *   d_num_unique   int32   M
 * Workspace: sst_unique_workspace_bytes(n).  No host synchronisation.
 * ---------------------------------------------------------------------------------------------- */
int64_t sst_unique_workspace_bytes(int64_t n);
int sst_unique_rows(const void* d_coors, int coor_is_i64, int64_t n, int ncols, int64_t row_stride,
                    const int64_t* h_mins, const int64_t* h_extents, int invalid_if_negative,
                    uint32_t* d_perm, int32_t* d_inverse, int32_t* d_offsets, uint64_t* d_ukeys,
                    int32_t* d_num_unique, void* d_workspace, void* stream);
/* Decode packed keys back into rows (int32 or int64 output); key 0 decodes to all -1. */
int sst_unpack_keys(const uint64_t* d_ukeys, int64_t m, int ncols, const int64_t* h_mins,
                    const int64_t* h_extents, void* d_rows_out, int out_is_i64, int64_t out_stride,
                    int out_col0, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a3/a5/a15) segmented reduce over the CSR produced above: one output row per group.
 * Replaces feats_reduce_kernel (scatter_points_cuda.cu:80-103, float-CAS atomics) and
 * torch_scatter.scatter_max / scatter(reduce=sum|mean) (call sites ops/sst/sst_ops.py:172-177).
 *   d_feats [n, c] fp32; group g reduces rows d_perm[d_offsets[g] .. d_offsets[g+1]).
 *   MAX of an empty group is -inf, SUM/MEAN is 0.  MEAN = sum / (float)count (cuda.cu:228-229).
 *   d_argmax (optional, [m, c] int32): row index of the FIRST (smallest index) row attaining the max
 *   (the tie rule of max_reduce_traceback_scatter_idx_kernel, cuda.cu:135-160); n for empty groups.
 *   d_group_index (optional, [m] int32): output row g reduces CSR group d_group_index[g] instead of group g (a negative
 *   entry: an empty group)
 *   (a subset / re-ordering of the groups without gathering the result: the batched DynamicScatter keeps all but
 *   the first sorted-unique row of every sample).
 * ---------------------------------------------------------------------------------------------- */
int sst_segment_reduce_fwd_f32(const float* d_feats, int64_t n, int c, const uint32_t* d_perm,
                               const int32_t* d_offsets, const int32_t* d_group_index, int64_t m, int mode,
                               float* d_out, int32_t* d_argmax, const int32_t* d_m_limit, void* stream);
/* sst_segment_reduce_fwd_work_f32: sst_segment_reduce_fwd_f32 made robust against a few very long groups among many short
 * ones (the voxels next to the sensor of a real LiDAR sweep hold thousands of points while the average voxel holds 1-10:
 * voxel_encoder.py:185-298 reduces them with the same DynamicScatter).  Groups of more than 32 rows are put on the work
 * list d_work by the element kernel - cut into chunks of 512 rows - and reduced by one workgroup per chunk in a second launch
 * of fixed size; a third merges the chunks of the groups that were cut, in chunk order; same tie rule, same results up to the
 * association of a cut group's sum.  d_work: int32 [work_capacity], 16-byte aligned, work_capacity >=
 * sst_segment_reduce_work_words(n, m, c), its first 8 entries ZEROED ONCE by the caller; the kernels leave them zeroed (reusable
 * by every later call on the same stream).  d_work == NULL: exactly
 * sst_segment_reduce_fwd_f32.  d_scale / d_shift (optional, [c], c % 4 == 0, with a work list): every value is read as
 * relu(x * scale + shift) - the BatchNorm + ReLU of DynamicVFE's last layer applied while its output is pooled
 * (voxel_encoder.py:286-296), whose activated [n, c] matrix is then never written. */
int64_t sst_segment_reduce_work_words(int64_t n, int64_t m, int c);
int sst_segment_reduce_fwd_work_f32(const float* d_feats, int64_t n, int c, const uint32_t* d_perm,
                                    const int32_t* d_offsets, const int32_t* d_group_index, int64_t m, int mode,
                                    float* d_out, int32_t* d_argmax, const int32_t* d_m_limit, int32_t* d_work,
                                    int64_t work_capacity, const float* d_scale, const float* d_shift, void* stream);
/* sst_segment_reduce_long_f32: the same reduction (all three modes, the arg-max tie rule) for groupings whose groups are
 * long and uneven (FSD's clusters, voxel_encoder.py:696-764 / backbones/sir.py:67-88: torch_scatter.scatter_max / scatter over
 * cluster ids): work is cut into tiles of sorted positions whatever group they belong to, groups inside a tile are written
 * directly, a group that crosses tiles is merged by the last of its tiles to arrive (one atomic ticket per crossing group and
 * tile; deterministic merge order; csrc/scatter.hip).  d_inverse [n] int32 = group of every point (+ inverse_shift; negative =
 * not reduced); every group with at least one point is written, groups without points are NOT.  d_scratch:
 * sst_segment_long_scratch_bytes(n, m, c) bytes, 256-byte aligned, its first 4 m bytes ZEROED ONCE by the caller; the kernel
 * leaves them zeroed (reusable by every later call on the same grouping without a fill).  c <= 256. */
int64_t sst_segment_long_scratch_bytes(int64_t n, int64_t m, int c);
int sst_segment_reduce_long_f32(const float* d_feats, int64_t n, int c, const uint32_t* d_perm, const int32_t* d_inverse,
                                int inverse_shift, const int32_t* d_offsets, int64_t m, int mode, void* d_scratch,
                                float* d_out, int32_t* d_argmax, void* stream);
/* sst_segment_reduce_profile_next(start, stop): one-shot hipEvent_t pair bound to the NEXT forward launch of this thread
 * (kernel start / stop; measurement hook of bench.py's FSD workloads, as sst_sra_attn_profile_next_fwd). */
int sst_segment_reduce_profile_next(void* start, void* stop);
/* Backward (scatter_points_cuda.cu:236-303).  d_grad_feats [n, c] is fully written (zero where no
 * gradient flows).  SUM/MEAN: g[i] = G[inv[i]] (/count); rows with d_inverse[i] < 0 get 0.
 * MAX: gradient goes to d_argmax[g, ch] only.  d_inverse may be shifted by the caller
 * (inverse_shift is added before use; the DynamicScatter "first row" quirk uses -1).  With d_group_index the
 * inverse map must already address OUTPUT rows; the group index is only used for the MEAN count.
 * d_m_limit (both directions, may be NULL): the number of output rows when it is only known on the device - `m`
 * is then an upper bound that sizes the launch and rows >= *d_m_limit are neither computed nor read. */
int sst_segment_reduce_bwd_f32(const float* d_grad_out, int64_t m, int c, const int32_t* d_inverse,
                               int inverse_shift, const int32_t* d_offsets, const int32_t* d_group_index,
                               const int32_t* d_argmax, int64_t n, int mode, float* d_grad_feats,
                               const int32_t* d_m_limit, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a15 / f1) d_out[i] = [ d_x[i, 0:c1] | d_g[d_idx[i], 0:c2] ]  ([n, c1 + c2] contiguous): the gather by the inverse map
 * + concatenation between the layers of DynamicVFE / DynamicScatterVFE / SIRLayer (voxel_encoders/voxel_encoder.py:
 * 288-291, 605-607, 745-750) in one coalesced pass.  d_idx[i] < 0 reads row 0.  c1, c2 multiples of 4, 16-byte rows.
 * ---------------------------------------------------------------------------------------------- */
int sst_concat_gather_f32(const float* d_x, int64_t ldx, int c1, const float* d_g, int64_t ldg, int c2,
                          const int32_t* d_idx, int64_t n, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a14) SSTv2.recover_bev (models/backbones/sst_v2.py:161-197): voxel features [m, c] + coordinates (b, z, y, x)
 * -> dense canvas of batch x ny x nx cells, written ONCE, cell by cell (the voxel's row or zeros), in CHANNELS-LAST
 * order: d_canvas is [batch, ny, nx, c] contiguous = the channels-last memory of the reference's logical
 * [batch, c, ny, nx] tensor (the host layer hands it on as that view).  c % 4 == 0, 16-byte aligned rows.
 *   d_cell_map [batch*ny*nx] int32 scratch (cell -> voxel, -1 empty); d_cell_of_voxel [m] int32 out: the cell each
 *   voxel was written to (-1: outside the canvas, or another voxel with the same cell was written instead - the
 *   reference's index assignment keeps one of them too).  Backward: rows of the canvas gradient at those cells.
 * ---------------------------------------------------------------------------------------------- */
int sst_recover_bev_f32(const float* d_feats, int64_t ldf, const void* d_coors, int coor_is_i64, int64_t ldc, int64_t m,
                        int batch, int ny, int nx, int c, int32_t* d_cell_map, int32_t* d_cell_of_voxel, float* d_canvas,
                        void* stream);
int sst_recover_bev_bwd_f32(const float* d_grad_canvas, const int32_t* d_cell_of_voxel, int64_t m, int c,
                            float* d_grad_feats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (f1) Decorate step of DynamicVFE / DynamicScatterVFE (voxel_encoders/voxel_encoder.py:252-271, :569-589) in one
 * launch: d_out[i] = [ point features (c) | xyz - mean xyz of the point's voxel, divided by cluster_div (3, if
 * with_cluster) | xyz - centre of the point's voxel (3, if with_center) ], bit-identical to the composed torch ops.
 *   d_inverse [n] int32 voxel of every point (< 0 reads voxel 0, like the reference's zero-initialised canvas);
 *   d_voxel_mean [m, >= 3] (row stride ldm); d_coors [n, 4] (b, z, y, x) int32 or int64 (row stride ldc);
 *   voxel_size / offsets: HOST float[3] (vx, vy, vz) and (v / 2 + range_min) per axis.
 * ---------------------------------------------------------------------------------------------- */
int sst_vfe_decorate_f32(const float* d_points, int64_t ldp, int64_t n, int c, const int32_t* d_inverse,
                         const float* d_voxel_mean, int64_t ldm, float cluster_div, const void* d_coors,
                         int coor_is_i64, int64_t ldc, const float* voxel_size, const float* offsets,
                         int with_cluster, int with_center, float* d_out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a7) in-group rank.  Replaces TorchEx ingroup_indices.forward(group_inds, out_inds)
 * (call site ops/sst/sst_ops.py:244-264).  d_rank[i] = number of j < i with group[j] == group[i]
 * (the stable choice; the reference leaves the order unspecified).  group ids must lie in [0, 2^key_bits).
 * Workspace: sst_ingroup_rank_workspace_bytes(n).
 * ---------------------------------------------------------------------------------------------- */
int64_t sst_ingroup_rank_workspace_bytes(int64_t n);
int sst_ingroup_rank_i64(const int64_t* d_group, int64_t n, int key_bits, int64_t* d_rank,
                         void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a6) window coordinates, both shifts in one launch.  Replaces get_window_coors
 * (ops/sst/sst_ops.py:266-314) called twice by SSTInputLayerV2.window_partition
 * (middle_encoders/sst_input_layer_v2.py:229-236).
 *   d_coors [m, 4] (b,z,y,x) int32 or int64.  sparse_shape = (sx,sy,sz), window_shape = (wx,wy,wz).
 *   d_win[s]   [m] int32     batch_win_inds for shift s (0: no shift, 1: half-window shift)
 *   d_ciw[s]   [m,3] int32   coors_in_win (z,y,x)
 * ---------------------------------------------------------------------------------------------- */
int sst_window_coors(const void* d_coors, int coor_is_i64, int64_t m, const int32_t sparse_shape[3],
                     const int32_t window_shape[3], int32_t* d_win0, int32_t* d_ciw0,
                     int32_t* d_win1, int32_t* d_ciw1, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a7-a9) region batching for both shifts: drop levels, voxel drop, in-window order, and the
 * window CSR ("plan") the SRA kernels consume.  Replaces SSTInputLayerV2.drop_voxel /
 * drop_single_shift (sst_input_layer_v2.py:128-226) and get_flat2win_inds (sst_ops.py:26-64).
 *   levels: n_levels rows of (max_tokens, lower, upper): level l applies when lower <= count < upper.
 *   Inputs d_win0/d_win1 [m] from sst_window_coors; win ids must be < 2^win_bits.
 * Outputs (device, caller allocated, sizes in elements):
 *   d_keep     [m] int32   1 if the voxel survives both shifts
 *   d_newidx   [m] int32   index among survivors (exclusive scan of keep)
 *   d_level[s] [m] int32   drop level of the voxel's window in shift s (-1 if no range matches)
 *   d_inner[s] [m] int32   rank among SURVIVORS of its window (valid where keep)
 *   d_flat2win[s] [m] int32  contiguous-window-id-within-level * max_tokens + inner (valid where keep)
 *   d_tok[s]   [m] int32   survivor indices (NEW numbering) grouped by window, ascending window id,
 *                           ascending inner; first M' entries valid
 *   d_winoff[s][m+1] int32 CSR offsets into d_tok[s] per non-empty window; first W_s+1 entries valid
 *   d_winlevel[s][m] int32 level of each non-empty window; first W_s valid
 *   d_counts   [8] int32   {M', W_0, W_1, T_0, T_1, 0...}: survivors, windows per shift, largest surviving window
 *                            population per shift (lets the caller pick the attention kernels' tile class)
 * Semantics follow the reference exactly: shift-1 levels are computed on the survivors of shift 0,
 * shift-0 levels are NOT recomputed after the second filter (sst_input_layer_v2.py:186-194).
 * Workspace: sst_region_batching_workspace_bytes(m).
 * ---------------------------------------------------------------------------------------------- */
int64_t sst_region_batching_workspace_bytes(int64_t m);
int sst_region_batching(const int32_t* d_win0, const int32_t* d_win1, int64_t m, int win_bits,
                        const int32_t* h_levels /*[n_levels,3]*/, int n_levels,
                        int32_t* d_keep, int32_t* d_newidx,
                        int32_t* d_level0, int32_t* d_level1, int32_t* d_inner0, int32_t* d_inner1,
                        int32_t* d_flat2win0, int32_t* d_flat2win1,
                        int32_t* d_tok0, int32_t* d_tok1, int32_t* d_winoff0, int32_t* d_winoff1,
                        int32_t* d_winlevel0, int32_t* d_winlevel1, int32_t* d_counts,
                        void* d_workspace, void* stream);
/* Launch order of the windows of a CSR for the register-resident attention kernels: d_order [n_windows] = window ids by ascending
 * token count (winoff[w + 1] - winoff[w] <= max_tokens), ties in id order - torch.sort(sizes, stable=True)[1] of the host layer
 * (the kernels dispatch from the end: largest windows first).  One launch.  SST_ERR_UNSUPPORTED: max_tokens >= 512. */
int sst_window_order_i32(const int32_t* d_winoff, int n_windows, int max_tokens, int32_t* d_order, void* stream);


/* ------------------------------------------------------------------------------------------------
 * (a2-a9 in one piece) Index plan of a frame batch without host round trips (csrc/frame_plan.hip): the same voxel
 * table / window bucketing / voxel drop / window CSR as sst_unique_rows + sst_window_coors + sst_region_batching,
 * from buffers sized by host-known upper bounds; the counts stay on the device (d_counts) and are read once.
 * Replaces, for the SST training path, DynamicScatter's per-sample unique bookkeeping (ops/voxel/scatter_points.py:
 * 85-99, src/scatter_points_cuda.cu:202-210) and SSTInputLayerV2.window_partition / drop_voxel / get_flat2win_inds
 * (middle_encoders/sst_input_layer_v2.py:128-236, ops/sst/sst_ops.py:26-64, 266-331).
 *
 * sst_frame_voxels_i32: from the sorted-unique groups of the point coordinates (sst_unique_rows with
 *   invalid_if_negative = 2, mins (0,-1,-1,-1), extents (B, gz+1, gy+1, gx+1); d_ukeys / d_inverse = its sorted keys and its
 *   point -> group map, d_num_groups = its device count):
 *   drop_mode 1: the first group of every sample is discarded (the reference's unconditional out_coors[1:]),
 *   drop_mode 0: only the group of invalid rows.  Kept groups are the voxels v = 0..M-1 (ascending key):
 *     d_vcoors [n_points, 4] int32 (b,z,y,x), d_gidx [n_points] group of voxel v, d_coors_map [n_points] voxel of every
 *     point (-1: dropped), d_grid [B*gz*gy*gx] dense cell -> voxel map (-1: empty), d_counts[0] = M,
 *     d_dropped_groups (optional, [B]): the discarded group of every sample, -1 where a sample has none (its points read
 *     voxel row 0 through map_voxel_center_to_point's zero-initialised canvas, voxel_encoder.py:246-270, and hand their
 *     gradient to that row: sst_segment_reduce_fwd_f32 with this array as d_group_index gives that sum without atomics).
 * sst_window_plan_i32: window / shifted-window bucketing, drop levels (h_levels: n_levels x (max_tokens, lo, hi)), the
 *   three passes of drop_voxel, window CSR.  seed = 0: survivors of an over-full window are its first voxels in
 *   ascending voxel order; seed != 0: a uniformly random subset (the reference's shuffle_voxels).  Outputs, kept voxels
 *   numbered window-major (position in the shift-0 CSR):
 *     d_feat_index / d_feat_index32 [n_upper] voxel v of every output row, d_out_coors [n_upper, 4] int64,
 *     d_winoff0 / d_winoff1 [n_windows + 1] CSR offsets of the non-empty windows (shift-0 tokens are 0..M'-1 in order),
 *     d_tok1 [n_upper] output rows grouped by shift-1 window, d_posidx0/1 [n_upper] row of the positional table
 *     ((z_in * wy + y_in) * wx + x_in); d_counts: [1] M', [2] W_0, [3] W_1, [4] / [5] largest window of each shift.
 *   n_windows = B * sst_frame_windows_per_sample(grid, window).  Limits: B <= 64, window <= 512 cells,
 *   B * cells <= 2^28 (otherwise SST_ERR_UNSUPPORTED: callers use the piecewise entry points).
 * ---------------------------------------------------------------------------------------------- */
int64_t sst_frame_windows_per_sample(const int32_t grid_zyx[3], const int32_t window_shape[3]);
int sst_frame_voxels_i32(const uint64_t* d_ukeys, const int32_t* d_inverse, const int32_t* d_num_groups, int64_t n_points, int batch_size, const int32_t grid_zyx[3],
                         int drop_mode, int32_t* d_vcoors, int32_t* d_gidx, int32_t* d_coors_map, int32_t* d_grid,
                         int32_t* d_counts, int32_t* d_dropped_groups, void* stream);
int64_t sst_window_plan_workspace_bytes(int64_t n_upper, int64_t n_windows);
int sst_window_plan_i32(const int32_t* d_vcoors, const int32_t* d_grid, int64_t n_upper, int batch_size,
                        const int32_t grid_zyx[3], const int32_t window_shape[3], const int32_t* h_levels, int n_levels,
                        uint32_t seed, int64_t* d_feat_index, int32_t* d_feat_index32, int64_t* d_out_coors,
                        int32_t* d_tok1, int32_t* d_winoff0, int32_t* d_winoff1, int32_t* d_posidx0, int32_t* d_posidx1,
                        int32_t* d_counts, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a12) Sparse Regional Attention core over variable-length windows (no padding, no key mask):
 *   for every window w (tokens tok[winoff[w] .. winoff[w+1])), every head h:
 *       S = (Q_h * scale) K_h^T ; P = softmax_rows(S) ; O_h = P V_h
 * Replaces the per-drop-level  flat2window -> nn.MultiheadAttention bmm/softmax/bmm -> window2flat
 * of WindowAttention.forward (models/sst/sst_basic_block_v2.py:41-75); the in/out projections stay
 * GEMM-library calls in the host layer; the cosine variant (cosine_msa.py:159-170) is sst_sra_attn_cos_{fwd,bwd}_f32
 * below (normalisation and 1 / clamp(tau) inside the kernels); for layouts those do not take the host layer normalises and
 * rescales Q,K before calling this with scale = 1.  head_dim is 16 (d_model/nhead =
 * 128/8, 192/12 in every SST config); n_heads must be a multiple of 4.
 * Q,K,V,O: [M, n_heads*16] fp32 with row strides ldq/ldk/ldv/ldo (elements, multiples of 4; base
 * pointers 16-byte aligned).  d_lse [M, n_heads] fp32: log-sum-exp of each softmax row (for backward).
 *   max_tokens: upper bound on tokens per window the caller guarantees (0 = unknown).  It must be an upper bound of EVERY
 *     window of the call (inclusive: a window of exactly max_tokens tokens is fine): it picks the register class of the
 *     launch, and a window longer than announced (but <= 144 tokens) is skipped by the register-resident kernels and picked
 *     up by no other - its output rows keep whatever the buffers held.  The bf16 and cosine calls below take the same bound.
 *   d_tok == NULL: the tokens of window w are the rows winoff[w] .. winoff[w+1] - 1 themselves (feature rows kept in
 *     window order, as sst_window_plan_i32 numbers them for the unshifted partition): no token list is read; taken by the
 *     register-resident kernels only (impl 0 / 3, 0 < max_tokens <= 144, aligned operands), else SST_ERR_UNSUPPORTED.
 *   impl: 0 = auto: register-resident MFMA kernels (wave = window x head, no LDS) for windows <= 144
 *             tokens, generic VALU kernel above that;
 *         1 = generic VALU kernel for every window (validation path);
 *         2 = LDS-staged MFMA kernels (K,V of a 4-head group in LDS; the first implementation);
 *         3 = forward as 0; backward as two register-resident launches (dQ, then dK / dV), kept for comparison.
 * ---------------------------------------------------------------------------------------------- */
int sst_sra_attn_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ldq, int64_t ldk,
                         int64_t ldv, const int32_t* d_tok, const int32_t* d_winoff, int64_t n_windows,
                         int n_heads, float scale, int max_tokens, int impl, float* d_o, int64_t ldo,
                         float* d_lse, void* stream);
/* Backward: given dO, recomputes P from (Q,K,LSE) and writes dQ, dK, dV for every token row listed in
 * d_tok (other rows untouched).  n_tokens = number of rows of the [M, *] tensors.  impl 0: ONE pass over
 * Q, K, V, O, dO per (window, head) wave (dQ, dK and dV from the same S / dP tiles; 8 x 64 B per token and
 * head of traffic); d_workspace may be NULL for it.
 * Workspace (impl 3): sst_sra_attn_bwd_workspace_bytes(n_tokens, n_heads) (rowsum(dO*O) per token, head). */
int64_t sst_sra_attn_bwd_workspace_bytes(int64_t n_tokens, int n_heads);
int sst_sra_attn_bwd_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_o,
                         const float* d_do, const float* d_lse, int64_t ldq, int64_t ldk, int64_t ldv,
                         int64_t ldo, int64_t lddo, const int32_t* d_tok, const int32_t* d_winoff,
                         int64_t n_windows, int64_t n_tokens, int n_heads, float scale, int max_tokens,
                         int impl, float* d_dq, float* d_dk, float* d_dv, int64_t lddq, int64_t lddk,
                         int64_t lddv, void* d_workspace, void* stream);

/* The same two calls with a LAUNCH ORDER of the windows: d_win_order (may be NULL) is a permutation of 0 .. n_windows - 1;
 * the workgroups are dispatched from its END (so: windows sorted by ascending token count = the largest windows first,
 * which shortens the tail of the launch: -5 % on the bench frame).  Results do not depend on it.  Used by the
 * register-resident kernels (impl 0 / 3 forward, impl 0 backward); the other kernels ignore it. */
int sst_sra_attn_fwd_ord_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ldq, int64_t ldk, int64_t ldv,
                             const int32_t* d_tok, const int32_t* d_winoff, const int32_t* d_win_order, int64_t n_windows,
                             int n_heads, float scale, int max_tokens, int impl, float* d_o, int64_t ldo, float* d_lse,
                             void* stream);
int sst_sra_attn_bwd_ord_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_o, const float* d_do,
                             const float* d_lse, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                             const int32_t* d_tok, const int32_t* d_winoff, const int32_t* d_win_order, int64_t n_windows,
                             int64_t n_tokens, int n_heads, float scale, int max_tokens, int impl, float* d_dq,
                             float* d_dk, float* d_dv, int64_t lddq, int64_t lddk, int64_t lddv, void* d_workspace,
                             void* stream);

/* Scaled cosine attention (CosineMultiheadAttention, models/sst/cosine_msa.py:123-185, 449-466; layer_cfg = dict(cosine=True,
 * tau_min=..) of configs/sst_refactor/sst_waymoD5_1x_3class_centerhead.py:75 and configs/fsd/fsd_waymoD1_1x_sst_encoder.py:70):
 *       S = normalize(Q_h) normalize(K_h)^T * head_scale[h] ; P = softmax_rows(S) ; O_h = P V_h
 * normalize = x / max(|x|_2, 1e-12) over the 16 channels of the head (torch.nn.functional.normalize), formed in the load
 * prologue of the register-resident kernels (one 4-lane reduction per row fragment).  d_head_scale: [n_heads] fp32 in DEVICE
 * memory = 1 / clamp(tau, tau_min) (a shared tau is passed expanded) - the parameter never visits the host.
 * Backward: d_dq / d_dk are the gradients of the UN-normalised q / k (d x = (d x^ - x^ (x^ . d x^)) / |x|, taken where the
 * row fragment is stored); d_r [n_tokens, n_heads] receives x^ . d x^ of the query side, whose column sum is the gradient of
 * the scale: d head_scale[h] = sum_rows d_r[:, h] / head_scale[h].  Same layouts and d_tok == NULL rule as above; windows of
 * <= 144 tokens, 16-byte aligned operands and n_heads % 4 == 0 only (else SST_ERR_UNSUPPORTED: the host layer then
 * normalises outside). */
int sst_sra_attn_cos_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t ldq, int64_t ldk, int64_t ldv,
                             const int32_t* d_tok, const int32_t* d_winoff, const int32_t* d_win_order, int64_t n_windows,
                             int n_heads, const float* d_head_scale, int max_tokens, float* d_o, int64_t ldo, float* d_lse,
                             void* stream);
int sst_sra_attn_cos_bwd_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_o, const float* d_do,
                             const float* d_lse, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                             const int32_t* d_tok, const int32_t* d_winoff, const int32_t* d_win_order, int64_t n_windows,
                             int64_t n_tokens, int n_heads, const float* d_head_scale, int max_tokens, float* d_dq, float* d_dk,
                             float* d_dv, int64_t lddq, int64_t lddk, int64_t lddv, float* d_r, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a12, reduced precision) The same attention core with bf16 storage: Q, K, V, O, dO, dQ, dK, dV are bf16 ([M, n_heads*16],
 * row strides in elements, multiples of 4; 8-byte aligned), the softmax, the log-sum-exp (fp32 [M, n_heads]) and every
 * accumulation are fp32; v_mfma_f32_16x16x16_bf16.  The reference's own training precision for these layers is fp16
 * (configs/sst_refactor/sst_waymoD5_1x_3class_8heads_v2.py:82).  Windows up to 144 tokens (max_tokens must say so, else
 * SST_ERR_UNSUPPORTED).  The backward is one pass per (window, head) wave (dQ, dK, dV from one read of Q, K, V, O, dO).
 * d_tok == NULL: the tokens of window w are the rows winoff[w] .. winoff[w+1] - 1 themselves (as for the fp32 kernels).
 * sst_sra_attn_bf16_profile_next(backward, start, stop): one-shot kernel-bound events, as for the fp32 kernels.
 * ---------------------------------------------------------------------------------------------- */
int sst_sra_attn_fwd_bf16(const void* d_q, const void* d_k, const void* d_v, int64_t ldq, int64_t ldk, int64_t ldv,
                          const int32_t* d_tok, const int32_t* d_winoff, int64_t n_windows, int n_heads, float scale,
                          int max_tokens, void* d_o, int64_t ldo, float* d_lse, void* stream);
int sst_sra_attn_bwd_bf16(const void* d_q, const void* d_k, const void* d_v, const void* d_o, const void* d_do,
                          const float* d_lse, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                          const int32_t* d_tok, const int32_t* d_winoff, int64_t n_windows, int n_heads, float scale,
                          int max_tokens, void* d_dq, void* d_dk, void* d_dv, int64_t lddq, int64_t lddk, int64_t lddv,
                          void* stream);
int sst_sra_attn_bf16_profile_next(int backward, void* start, void* stop);
/* with a launch order of the windows (see sst_sra_attn_fwd_ord_f32) */
int sst_sra_attn_fwd_ord_bf16(const void* d_q, const void* d_k, const void* d_v, int64_t ldq, int64_t ldk, int64_t ldv,
                              const int32_t* d_tok, const int32_t* d_winoff, const int32_t* d_win_order, int64_t n_windows,
                              int n_heads, float scale, int max_tokens, void* d_o, int64_t ldo, float* d_lse,
                              void* stream);
int sst_sra_attn_bwd_ord_bf16(const void* d_q, const void* d_k, const void* d_v, const void* d_o, const void* d_do,
                              const float* d_lse, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                              const int32_t* d_tok, const int32_t* d_winoff, const int32_t* d_win_order, int64_t n_windows,
                              int n_heads, float scale, int max_tokens, void* d_dq, void* d_dk, void* d_dv, int64_t lddq,
                              int64_t lddk, int64_t lddv, void* stream);
/* scaled cosine attention (cosine_msa.py:123-185) with bf16 storage: as sst_sra_attn_cos_{fwd,bwd}_f32 - normalisation in the
 * load prologue (the normalised rows rounded to bf16 before the products), d_head_scale [n_heads] fp32 in device memory =
 * 1 / clamp(tau, tau_min), gradients through the normalisation at the store, d_r [n_tokens, n_heads] fp32 = q^ . dq^ */
int sst_sra_attn_cos_fwd_bf16(const void* d_q, const void* d_k, const void* d_v, int64_t ldq, int64_t ldk, int64_t ldv,
                              const int32_t* d_tok, const int32_t* d_winoff, const int32_t* d_win_order, int64_t n_windows,
                              int n_heads, const float* d_head_scale, int max_tokens, void* d_o, int64_t ldo, float* d_lse,
                              void* stream);
int sst_sra_attn_cos_bwd_bf16(const void* d_q, const void* d_k, const void* d_v, const void* d_o, const void* d_do,
                              const float* d_lse, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo,
                              const int32_t* d_tok, const int32_t* d_winoff, const int32_t* d_win_order, int64_t n_windows,
                              int n_heads, const float* d_head_scale, int max_tokens, void* d_dq, void* d_dk, void* d_dv,
                              int64_t lddq, int64_t lddk, int64_t lddv, float* d_r, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row kernels of the reduced-precision encoder layer: bf16 storage, fp32 parameters / statistics / arithmetic.
 *   sst_add_layernorm_fwd_bf16: y = LN(x + res) * w + b  (res may be NULL); d_sum (optional) = x + res for the backward
 *     pass; d_stats [m, 2] fp32 (mean, rstd); optional second output d_y_plus_pos = y + pos_table[pos_idx[row]] - the
 *     next layer's q / k input "x + positional embedding" (sst_basic_block_v2.py:58-60; pos_table: fp32 [P, c], the
 *     distinct rows of SSTInputLayerV2.get_pos_embed).
 *   sst_add_layernorm_bwd_bf16: d(x + res) from dy (+ dy2, optional second gradient arriving at y) and dweight / dbias
 *     (fp32).  Workspace: sst_add_layernorm_bwd_workspace_bytes(m, c).
 *   sst_cast_add_pos_bf16: out(bf16) = x (fp32 or bf16) [+ pos_table[pos_idx]]: entry of the bf16 stack.
 * ---------------------------------------------------------------------------------------------- */
int sst_add_layernorm_fwd_bf16(const void* d_x, const void* d_res, const float* d_weight, const float* d_bias, int64_t m,
                               int c, float eps, void* d_y, void* d_sum, float* d_stats, const float* d_pos_table,
                               const int32_t* d_pos_idx, void* d_y_plus_pos, void* stream);
int sst_add_layernorm_bwd_bf16(const void* d_dy, const void* d_dy2, const void* d_sum, const float* d_stats,
                               const float* d_weight, int64_t m, int c, void* d_dx, float* d_dweight, float* d_dbias,
                               void* d_workspace, void* stream);
int sst_cast_add_pos_bf16(const void* d_x, int x_is_bf16, int64_t m, int c, const float* d_pos_table,
                          const int32_t* d_pos_idx, void* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense products of the reduced-precision encoder layer (csrc/dense_bf16.hip): bf16 operands, fp32 accumulation.
 * Replace F.linear / nn.MultiheadAttention's in_proj / out_proj and linear1 - activation - linear2 of
 * mmdet3d/models/sst/sst_basic_block_v2.py:41-75, 104-126 (forward and autograd's data / weight gradients).
 *   sst_tall_linear_bf16: y[m, n] (bf16) = epilogue(x[m, k] w[n, k]^T + bias);  (k, n) in {(128,128), (128,256), (256,128)};
 *     w bf16 row-major [n][k] contiguous, bias fp32 or NULL.  epilogue: 0 = bias; 1 / 2 = GELU(erf) / ReLU, the bf16
 *     pre-activation also written to d_aux_out (may be NULL); 3 / 4 = multiply by GELU' / ReLU' of d_aux_in (the stored
 *     pre-activation): the data gradient through the activation; 5 = add the bf16 [m, n] tensor d_aux_in (a residual
 *     branch's gradient).  ldaux = row stride of d_aux_in / d_aux_out (elements).
 *   sst_wgrad_group_bf16: for every problem, out_w[p][128] (fp32) = a[m, p]^T b[m, 128] with p = 128 or 256
 *     (transpose_out: out_w[128][p] instead - the operands of a [128][256] weight swapped), and out_b = column sums of a
 *     (bias_side 1, p values) or of b (bias_side 2, 128 values).  All problems (<= 8) run in ONE launch + one reduction.
 * ---------------------------------------------------------------------------------------------- */
int sst_tall_linear_bf16(const void* d_x, int64_t ldx, const void* d_w, const float* d_bias, int64_t m, int k, int n,
                         int epilogue, const void* d_aux_in, void* d_aux_out, int64_t ldaux, void* d_y, int64_t ldy,
                         void* stream);
/* The row partition of a sst_tall_linear_bf16 / sst_tall_linear_ln_bf16 (epi_is_ln) launch for m rows: workgroups (4 waves each,
 * 8 under SST_AMD_BF16_LINEAR_WAVES=8) and rows per wave (a multiple of 16).  Host arithmetic only. */
int sst_tall_linear_bf16_partition(int64_t m, int k, int n, int epi_is_ln, int64_t* blocks, int64_t* rows_per_wave);
/* sst_tall_linear_ln_bf16: y = LayerNorm(x w^T + bias + res) - `norm(src + src2)` (sst_basic_block_v2.py:113-118) in the
 * epilogue of the projection that produces src2 (out_proj, linear2): n = 128, k = 128 or 256.  Also written: d_sum (bf16
 * [m, 128], row stride ldres like d_res; the backward pass's input; may be NULL), d_stats [m, 2] fp32 (mean, rstd), and, when
 * the positional arguments are given, d_y_plus_pos = y + pos_table[pos_idx[row]] (the next layer's q / k input). */
int sst_tall_linear_ln_bf16(const void* d_x, int64_t ldx, const void* d_w, const float* d_bias, int64_t m, int k,
                            const void* d_res, int64_t ldres, const float* d_ln_weight, const float* d_ln_bias, float eps,
                            void* d_y, void* d_sum, float* d_stats, const float* d_pos_table, const int32_t* d_pos_idx,
                            void* d_y_plus_pos, void* stream);
typedef struct sst_wgrad_problem_bf16 {
  const void* a;   /* bf16 [m, p], row stride lda */
  const void* b;   /* bf16 [m, 128], row stride ldb */
  int64_t lda, ldb, m;
  float* out_w;    /* device, fp32 [p][128] (or [128][p]) contiguous */
  float* out_b;    /* device, fp32, or NULL */
  int32_t p, bias_side, transpose_out, reserved;
} sst_wgrad_problem_bf16;
int64_t sst_wgrad_group_workspace_bytes(const sst_wgrad_problem_bf16* problems, int n);
int sst_wgrad_group_bf16(const sst_wgrad_problem_bf16* problems, int n, void* d_workspace, void* stream);
/* sst_cast_group_bf16: the bf16 copies of the fp32 master weights the reduced-precision mode computes with, any number of
 * them in one launch (what mmcv's Fp16OptimizerHook.copy_params_to_fp16 does after every optimizer step for
 * configs/sst_refactor/sst_waymoD5_1x_3class_8heads_v2.py:82).  Problem = rows x cols block of an fp32 matrix with row stride
 * ld_src -> bf16 [rows][cols] contiguous, or, with transpose, [cols][rows] (the operand of a data gradient).  problems is a
 * HOST array. */
typedef struct sst_cast_problem_bf16 {
  const float* src; /* device */
  void* dst;        /* device, bf16, rows * cols elements */
  int64_t ld_src;
  int32_t rows, cols, transpose, reserved;
} sst_cast_problem_bf16;
int sst_cast_group_bf16(const sst_cast_problem_bf16* problems, int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a10/a14) row gather / scatter used by flat2window / window2flat / recover_bev.
 *   gather:  d_out[i, :] = idx[i] >= 0 ? d_src[idx[i], :] : fill
 *   scatter: d_out[idx[i], :] = d_src[i, :]      (idx unique; rows with idx < 0 skipped)
 * Replaces feat_3d[this_inds] = feat / feat[inds] (ops/sst/sst_ops.py:98, 124-125).
 * ---------------------------------------------------------------------------------------------- */
int sst_gather_rows_f32(const float* d_src, int64_t ld_src, const int32_t* d_idx, int64_t n_out, int c,
                        float fill, float* d_out, int64_t ld_out, void* stream);
/* out[i, :] = x[i, :] + table[idx[i], :]: q = k = feat + pos_embed of the first encoder layer (sst_basic_block_v2.py:62-66) with the
 * positional embedding kept as a table of the distinct in-window positions + a row index (sst_input_layer_v2.py:196-226 builds
 * the [M, C] tensor).  c % 4 == 0, 16-byte aligned rows. */
int sst_add_table_rows_f32(const float* d_x, int64_t ldx, const float* d_table, int64_t ld_table, const int32_t* d_idx, int64_t m,
                           int c, float* d_out, int64_t ld_out, void* stream);
int sst_scatter_rows_f32(const float* d_src, int64_t ld_src, const int32_t* d_idx, int64_t n_src, int c,
                         float* d_out, int64_t ld_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (a13, §8 f1) row-wise pieces of an encoder layer around the attention core.
 *   sst_add_layernorm_fwd_f32: y = LayerNorm(x + res) * weight + bias per row (res may be NULL);
 *     replaces `src = self.norm1(src + src2)` (models/sst/sst_basic_block_v2.py:113-118).  d_sum (optional)
 *     receives x + res (saved for backward), d_stats [m,2] receives (mean, rstd).  1 <= c <= 512 (16-byte accesses
 *     when c % 4 == 0 and the operands are 16-byte aligned, 4-byte accesses otherwise: FSD's SIR layers have C = 133 ...).
 *   sst_add_layernorm_bwd_f32: d_dx = gradient w.r.t. (x + res) (same tensor for both addends);
 *     d_dweight / d_dbias [c] are overwritten with the column reductions.
 *   sst_colsum_f32: out[c] = sum over rows of x[m, c] (row stride ld) — bias gradients of the
 *     projections / FFN.  c % 4 == 0, c <= 1024.
 * ---------------------------------------------------------------------------------------------- */
/*   sst_add_layernorm_act_{fwd,bwd}_f32: the same with an activation behind the norm in the same pass, y = act(LayerNorm(
 *     x + res)) - "Linear -> LN -> GELU" of FSD's SIR layers and MLPs (voxel_encoder.py:628-650, sst_ops.py:334-361).
 *     act: 0 none, 1 GELU (erf form), 2 ReLU.  The backward takes dy at the activation's OUTPUT and recomputes the norm's
 *     output from the saved sum and statistics (hence d_bias). */
int sst_add_layernorm_act_fwd_f32(const float* d_x, const float* d_res, const float* d_weight, const float* d_bias,
                                  int64_t m, int c, float eps, int act, float* d_y, float* d_sum, float* d_stats,
                                  void* stream);
int sst_add_layernorm_act_bwd_f32(const float* d_dy, const float* d_sum, const float* d_stats, const float* d_weight,
                                  const float* d_bias, int act, int64_t m, int c, float* d_dx, float* d_dweight,
                                  float* d_dbias, void* d_workspace, void* stream);
int sst_add_layernorm_fwd_f32(const float* d_x, const float* d_res, const float* d_weight, const float* d_bias,
                              int64_t m, int c, float eps, float* d_y, float* d_sum, float* d_stats,
                              void* stream);
/* the same with a second output d_y_plus_pos[row] = y[row] + d_pos_table[d_pos_idx[row]] (table rows of c floats): the next
 * encoder layer's q / k input (sst_basic_block_v2.py:56-58: q = k = feat + pos) without an add pass; c % 4 == 0 */
int sst_add_layernorm_pos_fwd_f32(const float* d_x, const float* d_res, const float* d_weight, const float* d_bias, int64_t m,
                                  int c, float eps, float* d_y, float* d_sum, float* d_stats, const float* d_pos_table,
                                  const int32_t* d_pos_idx, float* d_y_plus_pos, void* stream);
int64_t sst_add_layernorm_bwd_workspace_bytes(int64_t m, int c);
int sst_add_layernorm_bwd_f32(const float* d_dy, const float* d_sum, const float* d_stats,
                              const float* d_weight, int64_t m, int c, float* d_dx, float* d_dweight,
                              float* d_dbias, void* d_workspace, void* stream);
int64_t sst_colsum_workspace_bytes(int64_t m, int c);
int sst_colsum_f32(const float* d_x, int64_t m, int c, int64_t ld, float* d_out, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weight / bias gradient of a tall linear layer y = x W^T + b (projections and FFN of an encoder layer,
 * models/sst/sst_basic_block_v2.py:104-126; VFE / SIR linears): dW[out,in] = dY[M,out]^T X[M,in] as a
 * split-K fp32 MFMA kernel, d_db[out] = column sums of dY (optional, NULL to skip).  1 <= out, in <= 4096.
 * Row strides ld_dy / ld_x in elements.  Workspace: sst_weight_grad_workspace_bytes(m, out, in).
 * ---------------------------------------------------------------------------------------------- */
int64_t sst_weight_grad_workspace_bytes(int64_t m, int out, int in);
int sst_weight_grad_f32(const float* d_dy, const float* d_x, int64_t m, int out, int in, int64_t ld_dy,
                        int64_t ld_x, float* d_dw, float* d_db, void* d_workspace, void* stream);
/* The same for several problems (e.g. the five parameter gradients of an encoder layer): the split-K kernels one after
 * the other, ONE reduction launch for all.  dw [out, in] contiguous, db [out] or NULL. */
typedef struct sst_wgrad_problem_f32 {
  const float* dy;  /* [m, out], row stride ld_dy */
  const float* x;   /* [m, in], row stride ld_x */
  int64_t m, ld_dy, ld_x;
  float* dw;
  float* db;
  int32_t out, in;
  /* optional (both NULL or both set; exact-split group only, in a multiple of 128 as for every problem of that group): the X
   * operand is x + x_add_rows[x_add_index[token]] - rows fp32 [P][in] contiguous (row stride in) and 16-byte aligned, index
   * int32 [m] with values in [0, P): the weight gradient of q | k = (feat + pos) W (sst_basic_block_v2.py:56-60) without
   * "feat + pos" in memory.  sst_weight_grad_group_f32 returns SST_ERR_UNSUPPORTED when they are set. */
  const float* x_add_rows;
  const int32_t* x_add_index;
} sst_wgrad_problem_f32;
int64_t sst_weight_grad_group_workspace_bytes(const sst_wgrad_problem_f32* problems, int n);
int sst_weight_grad_group_f32(const sst_wgrad_problem_f32* problems, int n, void* d_workspace, void* stream);
/* The same gradients from the EXACT three-way bf16 split of both operands, six products on the bf16 matrix pipe with fp32
 * accumulation (csrc/wgrad_x6.hip; the arithmetic class of the fp32 kernel, see sst_tall_linear_epi_f32x6): ONE launch for all
 * problems (128 x 128 tiles of every dW x token slices) + one reduction.  All problems share m; out, in multiples of 128; row
 * strides % 4 == 0, 16-byte aligned operands; otherwise the workspace query returns SST_ERR_UNSUPPORTED (< 0) and the caller
 * uses sst_weight_grad_group_f32. */
int64_t sst_weight_grad_group_f32x6_workspace_bytes(const sst_wgrad_problem_f32* problems, int n);
int sst_weight_grad_group_f32x6(const sst_wgrad_problem_f32* problems, int n, void* d_workspace, void* stream);
/* Host only: the launch plan of that group, from the function the launch itself uses - 128 x 128 tiles over all problems, token
 * slices per tile, tokens per slice (a multiple of 32), and how many of the slices (the first ones) run their steady state in
 * the kernel's lean loop: full steps only, every requested row inside [0, m).  Outputs may be NULL.  SST_ERR_UNSUPPORTED as
 * the workspace query. */
int sst_weight_grad_group_f32x6_plan(const sst_wgrad_problem_f32* problems, int n, int* tiles, int* slices,
                                     int64_t* tokens_per_slice, int* lean_slices);

/* ------------------------------------------------------------------------------------------------
 * (a11/a12, §8 f1) BatchNorm1d (+ ReLU) of the point-wise "Linear -> norm -> ReLU" layers of DynamicVFE / SIR
 * (models/voxel_encoders/utils.py:107-144; norm = BN1d or naiveSyncBN1d, ops/norm.py:28-86) over tall
 * x[n, c] (row strides in elements, c % 4 == 0, c <= 1024, 16-byte aligned rows).  Replaces the library's
 * batch_norm statistics / backward-reduce kernels and the separate ReLU passes.
 *   sst_bn_stats_f32: d_mean[c], d_var[c] = column mean and BIASED variance E[x^2] - mean^2 (fp64 sums).
 *   sst_bn_act_fwd_f32: y = act(x * scale[c] + shift[c]); act 0 = identity, 1 = ReLU
 *     (scale = weight * rsqrt(var + eps), shift = bias - mean * scale; the [c]-sized algebra, running
 *      statistics and the cross-rank averaging of naiveSyncBN stay on the host side).
 *   sst_bn_act_bwd_reduce_f32: d_sum_g[c] = sum g, d_sum_gxhat[c] = sum g * xhat with g = dy masked by the
 *     activation and xhat = (x - mean) * invstd  (= dbias, dweight of the affine norm).
 *   sst_bn_act_bwd_apply_f32: dx = scale * (g - coef_scale * coef_a[c] - xhat * coef_scale * coef_b[c])
 *     (training: coef_a = sum_g, coef_b = sum_gxhat, coef_scale = 1 / count; eval: coef_scale = 0).
 * Workspace: sst_bn_workspace_bytes(n, c) for the stats / reduce calls.
 * ---------------------------------------------------------------------------------------------- */
int64_t sst_bn_workspace_bytes(int64_t n, int c);
int sst_bn_stats_f32(const float* d_x, int64_t n, int c, int64_t ld, float* d_mean, float* d_var,
                     void* d_workspace, void* stream);
int sst_bn_act_fwd_f32(const float* d_x, int64_t n, int c, int64_t ldx, const float* d_scale,
                       const float* d_shift, int act, float* d_y, int64_t ldy, void* stream);
int sst_bn_act_bwd_reduce_f32(const float* d_dy, const float* d_x, int64_t n, int c, int64_t lddy, int64_t ldx,
                              const float* d_mean, const float* d_invstd, const float* d_scale,
                              const float* d_shift, int act, float* d_sum_g, float* d_sum_gxhat,
                              void* d_workspace, void* stream);
int sst_bn_act_bwd_apply_f32(const float* d_dy, const float* d_x, int64_t n, int c, int64_t lddy, int64_t ldx,
                             const float* d_mean, const float* d_invstd, const float* d_scale,
                             const float* d_shift, const float* d_coef_a, const float* d_coef_b, float coef_scale,
                             int act, float* d_dx, int64_t lddx, void* stream);
/* Single-process training forward in one call: column moments of x, then d_out4 [4][c] = mean, invstd,
 * scale = weight * invstd, shift = bias - mean * scale, and running = (1 - factor) * running + factor * {mean,
 * var * n / (n - 1)} in place (nn.BatchNorm1d's bookkeeping; d_weight / d_bias / d_running_* may be NULL). */
int sst_bn_prepare_f32(const float* d_x, int64_t n, int c, int64_t ld, const float* d_weight, const float* d_bias,
                       float eps, float* d_running_mean, float* d_running_var, float factor, float* d_out4,
                       void* d_workspace, void* stream);
/*   sst_bn_prepare_tracked_f32: the same, and *d_num_batches_tracked += 1 (nn.BatchNorm1d's int64 counter; may be NULL)
 *     in the same launch. */
int sst_bn_prepare_tracked_f32(const float* d_x, int64_t n, int c, int64_t ld, const float* d_weight,
                               const float* d_bias, float eps, float* d_running_mean, float* d_running_var,
                               float factor, int64_t* d_num_batches_tracked, float* d_out4, void* d_workspace,
                               void* stream);
/* ------------------------------------------------------------------------------------------------
 * (f1) DynamicVFE's layer stack with its passes fused into their neighbours (voxel_encoder.py:185-298, utils.py:107-144:
 * per layer Linear(bias=False) -> BN -> ReLU -> scatter max -> cat with the pooled feature of the point's voxel).  Host side:
 * sst_amd/voxel_encoder.py FusedVFE2.
 *   sst_vfe_linear_moments_f32: first layer, y = x W^T for the K <= 16 decorated point channels (C % 4 == 0, C <= 256)
 *     and the block partials of the batch-norm moments of y in d_workspace (sst_bn_workspace_bytes(n, c)) from the same pass;
 *   sst_bn_prepare_from_partials_f32 / sst_bn_stats_from_partials_f32: the second halves of sst_bn_prepare_tracked_f32 /
 *     sst_bn_stats_f32 on those partials (the naiveSyncBN all-reduce of ops/norm.py:50-58 sits between the halves);
 *   sst_tall_linear_add_rows_f32x6 (below): second layer in its split-weight form;
 *   sst_segment_reduce_fwd_work_f32 with d_scale / d_shift: BN + ReLU of the last layer applied while it is pooled;
 *   sst_bn_act_pool_bwd_reduce_f32 / _apply_f32: sst_bn_act_bwd_reduce_f32 / _apply_f32 whose incoming gradient is
 *     d_dy (dense, may be NULL) + the gradient d_dpool [G, ldp] of the max pooling, routed to the recorded arg-max rows
 *     d_arg [G, c] through the point -> group map d_group [n] (negative: none): the dense matrix of the pooling's gradient
 *     (scatter_points_cuda.cu:135-179) is never written.
 * ---------------------------------------------------------------------------------------------- */
int sst_vfe_linear_moments_f32(const float* d_x, int64_t ldx, int64_t n, int k, const float* d_w, int64_t ldw, int c,
                               float* d_y, int64_t ldy, void* d_workspace, void* stream);
int sst_bn_prepare_from_partials_f32(int64_t n, int c, const float* d_weight, const float* d_bias, float eps,
                                     float* d_running_mean, float* d_running_var, float factor,
                                     int64_t* d_num_batches_tracked, float* d_out4, void* d_workspace, void* stream);
int sst_bn_stats_from_partials_f32(int64_t n, int c, float* d_mean, float* d_var, void* d_workspace, void* stream);
int sst_bn_act_pool_bwd_reduce_f32(const float* d_dy, const float* d_x, int64_t n, int c, int64_t lddy, int64_t ldx,
                                   const float* d_mean, const float* d_invstd, const float* d_scale, const float* d_shift,
                                   int act, const int32_t* d_group, const int32_t* d_arg, const float* d_dpool, int64_t ldp,
                                   float* d_sum_g, float* d_sum_gxhat, void* d_workspace, void* stream);
int sst_bn_act_pool_bwd_apply_f32(const float* d_dy, const float* d_x, int64_t n, int c, int64_t lddy, int64_t ldx,
                                  const float* d_mean, const float* d_invstd, const float* d_scale, const float* d_shift,
                                  const float* d_coef_a, const float* d_coef_b, float coef_scale, int act,
                                  const int32_t* d_group, const int32_t* d_arg, const float* d_dpool, int64_t ldp, float* d_dx,
                                  int64_t lddx, void* stream);
/* The residual tail of a sparse basic block (mmdet3d/ops/spconv/... sparse_block.py:127-139: bn2 -> += identity -> ReLU)
 * in the batch-norm passes: y = act(x * scale + shift + res).  The *_res_* entries are the calls above with the identity
 * branch d_res [n, c] (row stride ldr; NULL = none) inside the activation; the backward apply also writes the gradient of
 * the identity branch, d_dres = dy masked by the activation (NULL = not wanted). */
int sst_bn_act_res_fwd_f32(const float* d_x, int64_t n, int c, int64_t ldx, const float* d_res, int64_t ldr,
                           const float* d_scale, const float* d_shift, int act, float* d_y, int64_t ldy, void* stream);
int sst_bn_act_res_bwd_reduce_f32(const float* d_dy, const float* d_x, const float* d_res, int64_t n, int c,
                                  int64_t lddy, int64_t ldx, int64_t ldr, const float* d_mean, const float* d_invstd,
                                  const float* d_scale, const float* d_shift, int act, float* d_sum_g,
                                  float* d_sum_gxhat, void* d_workspace, void* stream);
int sst_bn_act_res_bwd_apply_f32(const float* d_dy, const float* d_x, const float* d_res, int64_t n, int c,
                                 int64_t lddy, int64_t ldx, int64_t ldr, const float* d_mean, const float* d_invstd,
                                 const float* d_scale, const float* d_shift, const float* d_coef_a,
                                 const float* d_coef_b, float coef_scale, int act, float* d_dres, int64_t lddres,
                                 float* d_dx, int64_t lddx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tall fp32 linear layer  y[m, n] (+)= x[m, k] W^T + bias  on the fp32 MFMA pipe with W resident in LDS
 * (projections / FFN of an encoder layer and their data gradients, models/sst/sst_basic_block_v2.py:41-75,
 * :104-126; replaces the library GEMM behind nn.Linear / F.linear for these shapes).
 *   trans_w = 0: d_w is [n][k] row-major (nn.Linear weight, forward).
 *   trans_w = 1: d_w is [k][n] row-major (data gradient dx = dy W of a layer whose weight is [out = k][in = n]).
 *   accumulate = 1: y += ... (residual / gradient accumulation rides on the product).
 * Supported: n == 128, k in {128, 256}; row strides in elements (multiples of 4, 16-byte aligned rows);
 * d_bias may be NULL.  Other shapes return SST_ERR_UNSUPPORTED (callers use the library GEMM for them).
 * ---------------------------------------------------------------------------------------------- */
int sst_tall_linear_f32(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, const float* d_bias,
                        int64_t m, int n, int k, int trans_w, int accumulate, float* d_y, int64_t ldy,
                        void* stream);
/* The same product (n == 128, k == 128) with the FFN's GELU (erf form, sst_basic_block_v2.py:116) in the epilogue:
 *   mode 0: y = x W^T + b and aux = gelu(y)   (linear1 + activation; both kept for the backward pass)
 *   mode 1: y = (x W [+ b]) * gelu'(aux)      (data gradient through linear2 times the activation's derivative at
 *                                              the pre-activation aux)
 * d_aux has the row stride ldy.  A 256-wide FFN is two calls on column halves of W / y / aux. */
/* sst_tall_linear_ln_f32: y = LayerNorm(x w^T + bias + res) in exact fp32 - `norm(src + src2)` (sst_basic_block_v2.py:113-118)
 * in the epilogue of the projection that produces src2 (out_proj, linear2; n = 128, k = 128 | 256; d_w [128][k] rows).  Also
 * written: d_sum ([m, 128], row stride ldres like d_res; may be NULL), d_stats [m, 2] (mean, rstd), and with the positional
 * arguments d_y_plus_pos = y + pos_table[pos_idx[row]].  sst_add_layernorm_bwd2_f32: the LayerNorm backward with an
 * optional SECOND upstream gradient d_dy2 (the one that arrives through y + pos), c = 128. */
int sst_tall_linear_ln_f32(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, const float* d_bias, int64_t m, int k,
                           const float* d_res, int64_t ldres, const float* d_ln_weight, const float* d_ln_bias, float eps,
                           float* d_y, float* d_sum, float* d_stats, const float* d_pos_table, const int32_t* d_pos_idx,
                           float* d_y_plus_pos, void* stream);
/* sst_tall_linear_epi_f32x3 / sst_tall_linear_ln_f32x3: the same two entry points (same arguments, fp32 tensors) with the
 * product evaluated on the bf16 matrix pipe from SPLIT operands, x w ~= x_hi w_hi + x_lo w_hi + x_hi w_lo, fp32 accumulation
 * (csrc/dense_f32x3.hip): ~1e-5 relative error per product - tighter than the TF32 the reference's nn.Linear ran on under
 * torch 1.8's default allow_tf32 = True on Ampere - at 3 / 16 of the fp32 pipe time.  Selected by SSTv2.set_precision('f32x3');
 * reported beside the exact-fp32 headline. */
int sst_tall_linear_epi_f32x3(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, int trans_w, const float* d_bias,
                              int64_t m, int k, int n, int epilogue, const float* d_aux_in, float* d_aux_out, int64_t ldaux,
                              float* d_y, int64_t ldy, void* stream);
int sst_tall_linear_ln_f32x3(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, const float* d_bias, int64_t m, int k,
                             const float* d_res, int64_t ldres, const float* d_ln_weight, const float* d_ln_bias, float eps,
                             float* d_y, float* d_sum, float* d_stats, const float* d_pos_table, const int32_t* d_pos_idx,
                             float* d_y_plus_pos, void* stream);
/* sst_tall_linear_epi_f32x6 / sst_tall_linear_ln_f32x6 (csrc/dense_f32x6.hip): the same two entry points again, fp32 tensors,
 * the product evaluated on the bf16 matrix pipe from an EXACT three-way split of both operands (x = x0 + x1 + x2, 8 + 8 + 8
 * significand bits) with the six products x_i w_j, i + j <= 2, accumulated in fp32: what is dropped is below 2^-24 |x w| per
 * product, i.e. below the rounding of an fp32 FMA chain - the arithmetic class of the reference's nn.Linear in fp32
 * (sst_basic_block_v2.py:41-126), at 6 x 16 instead of 8 x 32 matrix-pipe cycles per 16 x 16 x 32 block.  (k, n) in
 * {(128,128), (128,256), (128,384), (256,128)}; the LayerNorm entry takes k = 128 only (SST_ERR_UNSUPPORTED for 256: the
 * caller runs epilogue 5 + sst_add_layernorm_act_fwd_f32).  Selected by SSTv2.set_precision('f32x6').
 * sst_tall_linear_epi2_f32x6: the same with a second input matrix d_x2 (same ldx) for the output columns >= x2_from_col (a
 * multiple of 128): q | k | v of an encoder layer in ONE launch, q = k = (x + pos) W, v = x W (sst_basic_block_v2.py:56-62). */
int sst_tall_linear_epi_f32x6(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, int trans_w, const float* d_bias,
                              int64_t m, int k, int n, int epilogue, const float* d_aux_in, float* d_aux_out, int64_t ldaux,
                              float* d_y, int64_t ldy, void* stream);
int sst_tall_linear_epi2_f32x6(const float* d_x, const float* d_x2, int x2_from_col, int64_t ldx, const float* d_w, int64_t ldw,
                               int trans_w, const float* d_bias, int64_t m, int k, int n, int epilogue, const float* d_aux_in,
                               float* d_aux_out, int64_t ldaux, float* d_y, int64_t ldy, void* stream);
/* y = x W^T + rows[row_index[r]] (negative index: row 0), (k, n) = (64, 128) or (64, 64): DynamicVFE's second layer on [point feature |
 * pooled feature of the point's voxel] (voxel_encoder.py:286-294: cat + Linear(128 -> 128)) as point_feats W[:, :64]^T +
 * (pooled W[:, 64:]^T)[voxel of the point].  sst_tall_linear_epi_f32x6 also takes (k, n) = (64, 128), (64, 64) and (128, 64). */
int sst_tall_linear_add_rows_f32x6(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, int64_t m, int k, int n,
                                   const float* d_rows, int64_t ldrows, const int32_t* d_row_index, float* d_y, int64_t ldy,
                                   void* stream);
/* The in-projection of an SRA encoder layer from x alone (sst_basic_block_v2.py:56-62: q = k = feat + pos, v = feat):
 * y[m, 384] = [(x + rows[index]) W[:256]^T | x W[256:]^T] + bias; W [384][128] (in_proj_weight), rows = positional table fp32
 * [P][128], index int32 [m].  One launch; "x + pos" is formed in registers. */
int sst_inproj_pos_f32x6(const float* d_x, int64_t ldx, const float* d_rows, const int32_t* d_index, const float* d_w, int64_t ldw,
                         const float* d_bias, int64_t m, float* d_y, int64_t ldy, void* stream);
/* The row partition of the sst_tall_linear_*_f32x6 launches for m rows and `groups` column groups (1 - 3): row blocks per group
 * (8 waves each) and rows per wave (a multiple of 16).  Host arithmetic only. */
int sst_tall_linear_f32x6_partition(int64_t m, int groups, int64_t* row_blocks, int64_t* rows_per_wave);
int sst_tall_linear_ln_f32x6(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, const float* d_bias, int64_t m, int k,
                             const float* d_res, int64_t ldres, const float* d_ln_weight, const float* d_ln_bias, float eps,
                             float* d_y, float* d_sum, float* d_stats, const float* d_pos_table, const int32_t* d_pos_idx,
                             float* d_y_plus_pos, void* stream);
int sst_add_layernorm_bwd2_f32(const float* d_dy, const float* d_dy2, const float* d_sum, const float* d_stats,
                               const float* d_weight, int64_t m, int c, float* d_dx, float* d_dweight, float* d_dbias,
                               void* d_workspace, void* stream);
/* ------------------------------------------------------------------------------------------------
 * One post-norm SRA encoder layer (sst_basic_block_v2.py:41-126, d_model 128, 8 heads, feed-forward 256) as ONE call forward
 * and ONE call backward (csrc/layer_exec.hip): the entry points above issued in the order of
 * sst_amd/sst_basic_block.py FusedEncoderLayerFn in its exact-split mode - nothing but the launch sequence moves from the
 * interpreter into the library (15 foreign calls per layer and step become 2).  All tensors fp32, row-major, contiguous with
 * the widths given; tok may be NULL (rows in window order), order may be NULL.
 *   forward : qkv [m, 384] = [(xp W_q^T | xp W_k^T) | x W_v^T] + b_in;  o, lse = SRA(q, k, v);
 *             y1 = LN1(x + o W_o^T + b_o) (s1 = the sum, st1 [m, 2] = mean, rstd; s1 may be NULL when nothing is kept);
 *             pre = y1 W_1^T + b_1 [m, 256], h = act(pre) (act 1 = GELU(erf), 2 = ReLU);  s2 = y1 + h W_2^T + b_2;
 *             y2 = LN2(s2), st2; y2p = y2 + pos_table[pos_idx] when pos_table != NULL (the next layer's x + pos).
 *   backward: from dy2 (and dy2p, may be NULL) the gradients of every parameter and dx (returned in ds1: d(x) with the
 *             gradient of xp folded in, xp = x + a constant); ds2, dpre, ds1, d_o, dqkv [m, 384] are scratch outputs of the
 *             widths 128, 256, 128, 128, 384; workspace: sst_encoder_layer_bwd_workspace_bytes(m, n_heads), 256-byte aligned.
 *   head_scale (last field of both): NULL = softmax(q k^T * scale); else scaled cosine attention (sst_sra_attn_cos_*_f32),
 *             [n_heads] floats = 1 / clamp(tau, tau_min) in device memory, and the backward writes cos_r [m, n_heads]
 *             (d head_scale[h] = colsum(cos_r)[h] / head_scale[h], taken by the caller).
 *   xp      : x + positional rows as a tensor, or NULL with (xpos_table, xpos_idx): the in-projection and the weight gradient of
 *             W_q | W_k then add the table rows to x on load (sst_inproj_pos_f32x6, x_add_rows of sst_wgrad_problem_f32) and
 *             no [m, 128] "x + pos" tensor exists; a chain of layers passes pos_table = NULL (no y2p) in that mode.
 *   wpack   : the weight images of the one-kernel tail (csrc/layer_tail_x6.hip: out-projection -> norm1 -> feed-forward -> norm2),
 *             sst_encoder_layer_wpack_bytes() bytes of device memory: formed by the forward call, read by the backward call.
 *   Launches: forward 4 (in-projection, attention core, weight images, tail), backward 5 (tail, attention core, the five
 *             weight gradients + their reduction - which also finishes the LayerNorm parameter gradients -, in-projection's data
 *             gradient).  dy1 (a scratch field of the round-5 sequence) is ignored.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sst_encoder_layer_fwd_args {
  int64_t m, n_windows;
  int32_t n_heads, act, max_tokens, impl;
  float eps, scale;
  const float *x, *xp;
  const float *w_in, *b_in, *w_out, *b_out, *w1, *b1, *w2, *b2, *n1w, *n1b, *n2w, *n2b;
  const int32_t *tok, *winoff, *order;
  const float* pos_table;
  const int32_t* pos_idx;
  float *qkv, *o, *lse, *y1, *s1, *st1, *pre, *h, *s2, *y2, *st2, *y2p;
  const float* head_scale;
  void* wpack;   /* sst_encoder_layer_wpack_bytes() bytes, written by the forward call, read by the backward call of the SAME layer call;
                    with w_out = w1 = w2 = NULL: already formed by sst_encoder_tail_pack_f32x6_many, only read */
  const float* xpos_table;     /* with xp == NULL: x + pos is formed on load from the positional table [P][128] ... */
  const int32_t* xpos_idx;     /* ... and the table row of every token (int32 [m]); then pos_table / y2p are normally NULL */
  int32_t tail_flags;          /* the `flags` of the tail kernel (SST_TAIL_HANDOVER: s1, pre, s2 are hand-over buffers); same in both calls */
} sst_encoder_layer_fwd_args;
typedef struct sst_encoder_layer_bwd_args {
  int64_t m, n_windows;
  int32_t n_heads, act, max_tokens, impl;
  float eps, scale;
  const float *dy2, *dy2p;
  const float *x, *xp, *qkv, *o, *lse, *s1, *st1, *y1, *pre, *h, *s2, *st2;
  const float *w_in, *w_out, *w1, *w2, *n1w, *n2w;
  const int32_t *tok, *winoff, *order;
  float *ds2, *dpre, *ds1, *d_o, *dqkv;
  float *dw_in, *db_in, *dwo, *dbo, *dw1, *db1, *dw2, *db2, *dn1w, *dn1b, *dn2w, *dn2b;
  void* workspace;
  const float* head_scale;
  float* cos_r;
  float* dy1;    /* unused since round 6 (the gradient of y1 never leaves the registers of the tail kernel); may be NULL */
  const void* wpack;
  const float* xpos_table;     /* with xp == NULL (as in the forward call): the weight gradient of W_q | W_k reads x + table rows */
  const int32_t* xpos_idx;
  int32_t tail_flags;          /* as in the forward call */
} sst_encoder_layer_bwd_args;
int64_t sst_encoder_layer_bwd_workspace_bytes(int64_t m, int n_heads);
int64_t sst_encoder_layer_wpack_bytes(void);
int sst_encoder_layer_fwd_f32x6(const sst_encoder_layer_fwd_args* args, void* stream);
int sst_encoder_layer_bwd_f32x6(const sst_encoder_layer_bwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The part of that layer behind the attention core as ONE kernel per direction (csrc/layer_tail_x6.hip), exact-split
 * arithmetic, d_model 128, feed-forward 256 (sst_basic_block_v2.py:113-118 and their autograd): a wave carries 16 tokens
 * through out-projection -> + x -> norm1 -> linear1 -> act -> linear2 -> + y1 -> norm2 in registers; the weights pass
 * through LDS in 10 chunks.  All tensors fp32, contiguous, 16-byte aligned; widths: o, x, s1, y1, s2, y2, y2p, ds2, ds1,
 * d_o, dy2, dy2p 128; pre, h, dpre 256; st1, st2 [m, 2] (mean, rstd); w_out [128][128], w1 [256][128], w2 [128][256].
 *   pack    : `packed` (sst_encoder_tail_pack_bytes() bytes, device) = the three bf16 parts of the three weight matrices as the
 *             chunk images both kernels fetch with LDS-DMA; formed once per layer call (the weights of THIS forward pass: the
 *             backward pass must see the same buffer).
 *   forward : s1 = x + o W_o^T + b_o (s1 may be NULL), y1 = LN1(s1), pre = y1 W_1^T + b_1, h = act(pre) (act 1 = GELU(erf),
 *             2 = ReLU), s2 = y1 + h W_2^T + b_2 (s2 may be NULL), y2 = LN2(s2), y2p = y2 + pos_table[pos_idx] (all three NULL
 *             or all three given); biases may be NULL.
 *   backward: ds2 = LN2'(dy2 (+ dy2p, may be NULL)), dpre = (ds2 W_2) act'(pre), ds1 = LN1'(ds2 + dpre W_1), d_o = ds1 W_o;
 *             dn2w | dn2b | dn1w | dn1b [128] = the LayerNorm parameter gradients (m == 0: zeros).  workspace:
 *             sst_encoder_tail_bwd_workspace_bytes(m), 256-byte aligned.
 * The weight gradients of the three linears are the caller's (sst_weight_grad_group_f32x6 on (ds2, h), (dpre, y1), (ds1, o)).
 *   flags   : 0 = all tensors row-major, as described above.  SST_TAIL_HANDOVER (the same value in the forward and the
 *             backward call): s1, s2 and pre are a private hand-over between the two kernels.  Each is a buffer of
 *             sst_encoder_tail_handover_rows(m) rows (x 128 / 256 floats) in a tile-blocked layout nobody else should read
 *             (csrc/layer_tail_x6.hip; sst_amd/dense.py handover_to_rows undoes it for tests), and `pre` holds act'(pre), the
 *             derivative the backward kernel multiplies by.  Every other tensor, and every result, is what it is with flags 0.
 * ---------------------------------------------------------------------------------------------- */
#define SST_TAIL_HANDOVER 1
typedef struct sst_encoder_tail_fwd_args {
  int64_t m;
  int32_t act, flags;
  float eps, reserved_f;
  const float *o, *x;
  const void* packed;
  const float *b_out, *b1, *b2, *n1w, *n1b, *n2w, *n2b;
  const float* pos_table;
  const int32_t* pos_idx;
  float *s1, *st1, *y1, *pre, *h, *s2, *st2, *y2, *y2p;
} sst_encoder_tail_fwd_args;
typedef struct sst_encoder_tail_bwd_args {
  int64_t m;
  int32_t act, flags;
  const float *dy2, *dy2p, *s2, *st2, *pre, *s1, *st1;
  const void* packed;
  const float *n1w, *n2w;
  float *ds2, *dpre, *ds1, *d_o;
  float *dn2w, *dn2b, *dn1w, *dn1b;
  void* workspace;
} sst_encoder_tail_bwd_args;
int64_t sst_encoder_tail_handover_rows(int64_t m);   /* m rounded up to the rows of a workgroup; m < 0: SST_ERR_ARG */
int64_t sst_encoder_tail_pack_bytes(void);
int sst_encoder_tail_pack_f32x6(const float* d_w_out, const float* d_w1, const float* d_w2, void* d_packed, void* stream);
/* the images of n layers in ONE launch (arrays of n device pointers in HOST memory; d_packed[i]: sst_encoder_tail_pack_bytes()
 * bytes each): what a stack of layers does once per forward pass (sst_v2.py:118-133 runs its blocks back to back);
 * sst_encoder_layer_fwd_f32x6 takes such images with w_out = w1 = w2 = NULL in its arguments */
int sst_encoder_tail_pack_f32x6_many(const float* const* d_w_out, const float* const* d_w1, const float* const* d_w2,
                                     void* const* d_packed, int n, void* stream);
int64_t sst_encoder_tail_bwd_workspace_bytes(int64_t m);
int sst_encoder_tail_fwd_f32x6(const sst_encoder_tail_fwd_args* args, void* stream);
int sst_encoder_tail_bwd_f32x6(const sst_encoder_tail_bwd_args* args, void* stream);

/* The same one-kernel tail in the reduced-precision mode (csrc/layer_tail_bf16.hip): activations bf16 (o, x, s1, y1, s2, y2, y2p,
 * ds2, ds1, d_o, dy2, dy2p [m, 128]; pre, h, dpre [m, 256]), statistics / biases / LayerNorm parameters / their gradients fp32;
 * `packed` = sst_encoder_tail_pack_bf16_bytes() bytes written by sst_encoder_tail_pack_bf16 from the fp32 master weights
 * (w_out [128][128], w1 [256][128], w2 [128][256]): the bf16 images of both directions.  Field meaning as sst_encoder_tail_*_args. */
typedef struct sst_encoder_tail_fwd_bf16_args {
  int64_t m;
  int32_t act, reserved;
  float eps, reserved_f;
  const void *o, *x;
  const void* packed;
  const float *b_out, *b1, *b2, *n1w, *n1b, *n2w, *n2b;
  const float* pos_table;
  const int32_t* pos_idx;
  void* s1;
  float* st1;
  void *y1, *pre, *h, *s2;
  float* st2;
  void *y2, *y2p;
} sst_encoder_tail_fwd_bf16_args;
typedef struct sst_encoder_tail_bwd_bf16_args {
  int64_t m;
  int32_t act, reserved;
  const void *dy2, *dy2p, *s2;
  const float* st2;
  const void *pre, *s1;
  const float* st1;
  const void* packed;
  const float *n1w, *n2w;
  void *ds2, *dpre, *ds1, *d_o;
  float *dn2w, *dn2b, *dn1w, *dn1b;
  void* workspace;
} sst_encoder_tail_bwd_bf16_args;
int64_t sst_encoder_tail_pack_bf16_bytes(void);
int sst_encoder_tail_pack_bf16(const float* d_w_out, const float* d_w1, const float* d_w2, void* d_packed, void* stream);
/* the images of n layers in one launch: host arrays of device pointers (a whole encoder stack per forward pass) */
int sst_encoder_tail_pack_bf16_many(const float* const* d_w_out, const float* const* d_w1, const float* const* d_w2,
                                    void* const* d_packed, int n, void* stream);
int64_t sst_encoder_tail_bwd_bf16_workspace_bytes(int64_t m);
int sst_encoder_tail_fwd_bf16(const sst_encoder_tail_fwd_bf16_args* args, void* stream);
int sst_encoder_tail_bwd_bf16(const sst_encoder_tail_bwd_bf16_args* args, void* stream);

/* The same layer in the reduced-precision mode (bf16 storage, fp32 accumulation / softmax / LayerNorm statistics, fp32 master
 * weights: what the reference's fp16 training of these layers - configs/sst_refactor/sst_waymoD5_1x_3class_8heads_v2.py:82 -
 * corresponds to), one call per direction: the launch sequence of sst_amd/bf16.py EncoderLayerBF16Fn issued from C (6 launches
 * forward, 10 + the grouped weight gradients backward; same kernels, same order, same bits).  d_model 128, feed-forward 256,
 * 8 heads.  Activations are bf16 [m, *]; wqk [256][128], wv / wout [128][128], w1 [256][128], w2 [128][256] are the bf16 copies
 * of the fp32 parameters (sst_cast_group_bf16), the *_t ones their transposes; biases, LayerNorm parameters, statistics
 * (st1, st2 [m, 2]) and lse [m, 8] are fp32.  Backward: dx / dxp (bf16) are the gradients of x and of xp = x + positional rows;
 * ds2, dpre, dy1, ds1, d_o, dqkv are scratch of widths 128, 256, 128, 128, 128, 384; parameter gradients fp32; workspace:
 * sst_encoder_layer_bwd_bf16_workspace_bytes(m), 256-byte aligned.  head_scale (last fields): NULL = standard attention, else
 * scaled cosine attention (sst_sra_attn_cos_*_bf16) and the backward writes cos_r [m, 8] fp32. */
typedef struct sst_encoder_layer_fwd_bf16_args {
  int64_t m, n_windows;
  int32_t n_heads, act, max_tokens, reserved;
  float eps, scale;
  const void *x, *xp;
  const void *wqk, *wv, *wout, *w1, *w2;
  const float *b_in, *b_out, *b1, *b2, *n1w, *n1b, *n2w, *n2b;
  const int32_t *tok, *winoff, *order;
  const float* pos_table;
  const int32_t* pos_idx;
  void *qk, *v, *o;
  float* lse;
  void *y1, *s1;
  float* st1;
  void *pre, *h, *s2;
  float* st2;
  void *y2, *y2p;
  const float* head_scale;
  const void* wpack;   /* sst_encoder_tail_pack_bf16 images of this layer's out_proj / linear1 / linear2 (fp32 masters) */
} sst_encoder_layer_fwd_bf16_args;
typedef struct sst_encoder_layer_bwd_bf16_args {
  int64_t m, n_windows;
  int32_t n_heads, act, max_tokens, reserved;
  float eps, scale;
  const void *dy2, *dy2p;
  const void *x, *xp, *qk, *v, *o;
  const float* lse;
  const void* s1;
  const float* st1;
  const void *y1, *pre, *h, *s2;
  const float* st2;
  const void *wqk_t, *wv_t, *wout_t, *w1_t, *w2_t;
  const float *n1w, *n2w;
  const int32_t *tok, *winoff, *order;
  void *ds2, *dpre, *dy1, *ds1, *d_o, *dqkv, *dxp, *dx;
  float *dw_in, *db_in, *dwo, *dbo, *dw1, *db1, *dw2, *db2, *dn1w, *dn1b, *dn2w, *dn2b;
  void* workspace;
  const float* head_scale;
  float* cos_r;
  const void* wpack;   /* as in the forward arguments */
} sst_encoder_layer_bwd_bf16_args;
int64_t sst_encoder_layer_bwd_bf16_workspace_bytes(int64_t m);
int sst_encoder_layer_fwd_bf16(const sst_encoder_layer_fwd_bf16_args* args, void* stream);
int sst_encoder_layer_bwd_bf16(const sst_encoder_layer_bwd_bf16_args* args, void* stream);

/* sst_tall_linear_epi_f32 (csrc/dense_f32.hip): y[m, n] = epilogue(x[m, k] W^T + bias), exact fp32 (v_mfma_f32_16x16x4_f32),
 * the whole weight matrix resident in LDS; (k, n) in {(128,128), (128,256), (256,128)}.  trans_w = 0: d_w holds W as [n][k]
 * rows (F.linear's weight); trans_w = 1: d_w holds [k][n] rows - the data gradient dy[m, out] w[out, in] of a layer with
 * parameter w (sst_basic_block_v2.py:41-75, 104-126 and their autograd).  epilogue: 0 = bias; 1 / 2 = GELU(erf) / ReLU with
 * the pre-activation also written to d_aux_out (may be NULL); 3 / 4 = multiply by GELU' / ReLU' of d_aux_in; 5 = add
 * d_aux_in (may alias d_y: in-place accumulation of a residual branch's gradient). */
int sst_tall_linear_epi_f32(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, int trans_w, const float* d_bias,
                            int64_t m, int k, int n, int epilogue, const float* d_aux_in, float* d_aux_out, int64_t ldaux,
                            float* d_y, int64_t ldy, void* stream);
int sst_tall_linear_gelu_f32(const float* d_x, int64_t ldx, const float* d_w, int64_t ldw, const float* d_bias,
                             int64_t m, int n, int k, int trans_w, int mode, float* d_aux, float* d_y, int64_t ldy,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py `roofline`): HIP events attached to ONE launch of the register-resident SRA forward
 * kernel.  sst_sra_attn_profile_next_fwd(start, stop) arms the next sst_sra_attn_fwd_f32 call (impl 0, windows
 * <= 144 tokens): the kernel is launched with hipExtLaunchKernelGGL so that `start` / `stop` carry the kernel's own
 * begin / end timestamps on the launch stream.  Events come from sst_event_create (plain hipEventCreate).
 * ---------------------------------------------------------------------------------------------- */
void* sst_event_create(void);
void sst_event_destroy(void* ev);
float sst_event_elapsed_ms(void* start, void* stop); /* synchronises on `stop`; < 0 on error */
int sst_sra_attn_profile_next_fwd(void* start, void* stop);
/* the same for the one-pass backward kernel (the next sst_sra_attn_bwd_f32 call with impl 0); both hooks are
 * one-shot and local to the calling thread */
int sst_sra_attn_profile_next_bwd(void* start, void* stop);

/* ------------------------------------------------------------------------------------------------
 * (§8 f2) Connected components of the graph "same sample and xy distance < dist" over n points — FSD's
 * ClusterAssigner.  Replaces find_connected_componets (models/detectors/single_stage_fsd.py:45-68): dense N x N
 * distance matrix, `.cpu()`, scipy.sparse.csgraph.connected_components per sample, running label base.
 *   d_points [n, >= 2] fp32 (x, y first; row stride ld elements), d_batch [n] int32 sample index (samples stored
 *   one after the other, as the sorted-unique that produces the centres leaves them).
 *   d_labels [n] int32: components numbered by their smallest point index (scipy's order of first appearance;
 *   with contiguous samples = the reference's per-sample numbering + running base).  Bit-exact: the edge test
 *   uses the reference's fp32 operations (sub, mul, add, sqrt, <).  d_num_components (optional, device int32).
 * Workspace: sst_connected_components_workspace_bytes(n).
 * ---------------------------------------------------------------------------------------------- */
int64_t sst_connected_components_workspace_bytes(int64_t n);
int sst_connected_components_xy_f32(const float* d_points, int64_t ld, const int32_t* d_batch, int64_t n, float dist,
                                    int32_t* d_labels, int32_t* d_num_components, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (§8 f3) Dynamic point pool — the RoI extractor in front of FSD's second-stage SIR layers.  Replaces
 * dynamic_point_pool_ext.forward(rois, pts, extra_wlh, max_inbox_point, out_pts_idx, out_roi_idx, out_pts_feats)
 * (mmdet3d/ops/dynamic_point_pool_op.py:36) and dynamic_point_pool_ext.dynamic_point_pool_mixed_gpu (:86-88); that
 * extension (TorchEx) is not in the reference tree: PARITY UNPINNED beyond the box convention of
 * ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-50 and the invariants asserted in
 * models/roi_heads/roi_extractors/dynamic_point_roi_extractor.py:96-105.
 *   d_rois [n_rois, 7] fp32 (x, y, z of the bottom centre, w, l, h, rz); d_pts [n_pts, >= 3] fp32, row stride ld_pts.
 *   d_rois_batch / d_pts_batch: both NULL (one sample) or int32 sample indices (a pair needs equal indices).
 *   extra_wlh: HOST pointer to 3 floats added to (w, l, h) for the membership test.
 *   Outputs (caller-allocated, max_all_pts rows; rows >= *d_num_out are left untouched): d_out_pts_idx,
 *   d_out_roi_idx int64; d_out_feats [max_all_pts, 13] = point xyz, box-frame xyz, distances to the six faces of the
 *   un-enlarged box (+x, +y, +z side sums give l, w, h), 1.0 if the point lies only in the enlarged margin.
 *   Deterministic: pairs sorted by (RoI, point index); a RoI keeps its first max_inbox_point points, the output
 *   its first max_all_pts pairs (the reference's atomics make the surviving subset and the order race-dependent).
 *   d_num_out: device int64.  Workspace: sst_dynamic_point_pool_workspace_bytes(n_rois, n_pts).
 * ---------------------------------------------------------------------------------------------- */
int64_t sst_dynamic_point_pool_workspace_bytes(int64_t n_rois, int64_t n_pts);
int sst_dynamic_point_pool_f32(const float* d_rois, const int32_t* d_rois_batch, int64_t n_rois, const float* d_pts,
                               int64_t ld_pts, const int32_t* d_pts_batch, int64_t n_pts, const float* extra_wlh,
                               int max_inbox_point, int64_t max_all_pts, int64_t* d_out_pts_idx,
                               int64_t* d_out_roi_idx, float* d_out_feats, int64_t* d_num_out, void* d_workspace,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * (§8 f4, first part) Sparse 3-D convolution: rulebook + convolution.  Replaces the reference's vendored spconv for
 * 3-D int32 indices: getIndicePair<3> (mmdet3d/ops/spconv/include/spconv/spconv_ops.h:26-150; kernel-offset and
 * position arithmetic include/spconv/geometry.h:24-151) and indiceConv / indiceConvBackward (spconv_ops.h:256-446).
 * All index tensors are int32; d_coors rows are (batch, z, y, x), contiguous, 16-byte aligned; shapes / ksize /
 * stride / padding / dilation are HOST arrays of 3 int32 (z, y, x).  Kernel offset k = (kz * ksize_y + ky) * ksize_x
 * + kx (the `offset` of geometry.h:66-70); K = ksize_z * ksize_y * ksize_x <= 4096.
 *
 * The rulebook is two dense maps, in2out [K, n] and out2in [K, m] (-1 = no partner), plus the reference's pair lists
 * (indice_pairs [K, 2, n] filled with -1 behind the valid entries, indice_num [K]; pairs ordered by input row).
 *   sst_spconv_candidates_i32: regular / transposed convolution, rows [K * n + 1, 4] = output voxel (b, z, y, x) touched
 *     by (offset k, input row j) at row k * n + j, or four -1; the last row is always invalid.  Feed them to
 *     sst_unique_rows(invalid_if_negative = 1): the sorted groups 1.. are the output voxels in ascending (b, z, y, x)
 *     order (the order of the reference's GPU path, torch::_unique of the linear indices, spconv_ops.h:128), and
 *     sst_spconv_inverse_to_map_i32 turns its inverse into in2out (group - 1).
 *   sst_spconv_subm_map_i32: submanifold convolution (stride 1, padding ksize / 2, spconv_ops.h:74-77): outputs =
 *     inputs.  d_sorted_keys / d_perm: ukeys and perm of sst_unique_rows over the n input rows with mins = 0,
 *     extents = (batch, shape) and invalid_if_negative = 0 (key = 1 + linear index).
 *   sst_spconv_invert_map_i32: out2in from in2out.   sst_spconv_pair_lists_i32: pair lists from in2out.
 *   sst_spconv_gather_gemm_f32: Y[r, :] = sum_k X[map[k][r], :] W[k] (+ bias), r < m; W[k] is [cin, cout] row-major, or
 *     [cout, cin] with trans_w (data gradient on the forward weights).  Forward: map = out2in; data gradient and
 *     inverse convolution: map = in2out.  Every row of Y is written.  form: 0 = automatic, 1 = every row of a 64 x 128
 *     tile times every offset present in the tile, 2 = MFMAs over the compacted rows that have a partner (K <= 32,
 *     W not transposed; best when few of the K offsets are populated).
 *   sst_spconv_wgrad_f32: dW[k] = sum over the pairs p < num[k] of X[pairs[k][x_side][p]]^T dY[pairs[k][1 - x_side][p]];
 *     pair_ld = row length of the pair lists (n); total_pairs = sum of d_num if the caller knows it on the host (it bounds
 *     the launch and the workspace), -1 otherwise.  Workspace: sst_spconv_wgrad_workspace_bytes (same arguments).
 * ---------------------------------------------------------------------------------------------- */
int sst_spconv_candidates_i32(const int32_t* d_coors, int64_t n, const int32_t* in_shape, const int32_t* out_shape,
                              const int32_t* ksize, const int32_t* stride, const int32_t* padding,
                              const int32_t* dilation, int transpose, int32_t* d_rows, void* stream);
int sst_spconv_inverse_to_map_i32(const int32_t* d_inverse, int64_t total, int32_t* d_in2out, void* stream);
/*   Dense-grid builders of the SAME rulebooks (getIndicePair<3>, spconv_ops.h:26-150; identical numbering): a cell -> row
 *     grid over batch x shape replaces the sort / binary search when the grid fits (cells <= 2^31).
 *     sst_spconv_grid_subm_i32: d_grid [batch * prod(shape)] int32 scratch -> in2out AND out2in [K, n].
 *     sst_spconv_grid_conv_count_i32: regular / transposed convolution, pass 1: flags the output cells, scans them,
 *     *d_num_out = number of output voxels (device int32: the caller reads it back to size pass 2's outputs);
 *     workspace sst_spconv_grid_conv_workspace_bytes(batch * prod(out_shape)), handed on to
 *     sst_spconv_grid_conv_maps_i32: d_outids [m, 4] (b, z, y, x) ascending, in2out [K, n], out2in [K, m]. */
int sst_spconv_grid_subm_i32(const int32_t* d_coors, int64_t n, int batch, const int32_t* shape, const int32_t* ksize,
                             const int32_t* dilation, int32_t* d_grid, int32_t* d_in2out, int32_t* d_out2in,
                             void* stream);
int64_t sst_spconv_grid_conv_workspace_bytes(int64_t cells);
int sst_spconv_grid_conv_count_i32(const int32_t* d_coors, int64_t n, int batch, const int32_t* in_shape,
                                   const int32_t* out_shape, const int32_t* ksize, const int32_t* stride,
                                   const int32_t* padding, const int32_t* dilation, int transpose, void* d_workspace,
                                   int32_t* d_num_out, void* stream);
int sst_spconv_grid_conv_maps_i32(const int32_t* d_coors, int64_t n, int batch, const int32_t* in_shape,
                                  const int32_t* out_shape, const int32_t* ksize, const int32_t* stride,
                                  const int32_t* padding, const int32_t* dilation, int transpose, void* d_workspace,
                                  int64_t m, int32_t* d_outids, int32_t* d_in2out, int32_t* d_out2in, void* stream);
int sst_spconv_subm_map_i32(const int32_t* d_coors, int64_t n, const int32_t* shape, const int32_t* ksize,
                            const int32_t* dilation, const uint64_t* d_sorted_keys, const uint32_t* d_perm,
                            int32_t* d_in2out, void* stream);
int sst_spconv_invert_map_i32(const int32_t* d_in2out, int kvol, int64_t n, int64_t m, int32_t* d_out2in,
                              void* stream);
int64_t sst_spconv_pair_lists_workspace_bytes(int kvol, int64_t n);
int sst_spconv_pair_lists_i32(const int32_t* d_in2out, int kvol, int64_t n, int32_t* d_pairs, int32_t* d_num,
                              void* d_workspace, void* stream);
int sst_spconv_gather_gemm_f32(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol,
                               const float* d_w, int cin, int cout, int trans_w, const float* d_bias, float* d_y,
                               int64_t ldy, int form, void* stream);
/*   sst_spconv_maxpool_{fwd,bwd}_f32: indiceMaxPool / indiceMaxPoolBackward (include/spconv/pool_ops.h:24-97,
 *     src/maxpool.cc:22-63) on the maps: y[i] = max(0, max_k x[out2in[k][i]]) (the reference's zero-filled start);
 *     dx[j] = sum of dy[i] over the outputs i = in2out[k][j] whose value equals x[j] (ties all receive). */
int sst_spconv_maxpool_fwd_f32(const float* d_x, int64_t ldx, const int32_t* d_out2in, int64_t m, int kvol, int c,
                               float* d_y, int64_t ldy, void* stream);
int sst_spconv_maxpool_bwd_f32(const float* d_x, int64_t ldx, const float* d_y, int64_t ldy, const float* d_dy,
                               int64_t lddy, const int32_t* d_in2out, int64_t n, int kvol, int c, float* d_dx,
                               int64_t lddx, void* stream);
/*   sst_spconv_conv_os_f32: the same contraction as sst_spconv_gather_gemm_f32 (indiceConv and the data gradient of
 *     indiceConvBackward, spconv_ops.h:256-446) as an output-stationary implicit GEMM: W[k] packed into MFMA-fragment
 *     order (d_workspace, sst_spconv_conv_os_workspace_bytes) and staged through LDS, partner rows gathered straight into
 *     MFMA operands, XCD-aware tile numbering (csrc/spconv_os.hip).  K <= 32, cin % 4 == 0, ldx % 4 == 0, d_x 16-byte
 *     aligned; SST_ERR_UNSUPPORTED otherwise (use sst_spconv_gather_gemm_f32).  trans_w as above.  tile_cfg: 0 = tile
 *     shape chosen from m and cout, else 10 * (column tiles of 16: 4 | 8) + (16-row blocks per wave: 1 | 2).
 *     d_tile_order (may be NULL): a permutation of the ceil(m / tile_rows) row tiles, the order in which they are launched -
 *     heaviest first evens out the end of the launch; tile_rows = sst_spconv_conv_os_tile_rows(m, cout, tile_cfg) (64 or
 *     128), and sst_spconv_os_tile_work_i32 writes work[tile] = populated (16-row block, offset) slots of the tile, the key
 *     to sort by (descending).  The result does not depend on the order. */
int64_t sst_spconv_conv_os_workspace_bytes(int kvol, int cin, int cout);
int sst_spconv_conv_os_tile_rows(int64_t m, int cout, int tile_cfg);
int sst_spconv_os_tile_work_i32(const int32_t* d_map, int64_t m, int kvol, int tile_rows, int32_t* d_work, void* stream);
int sst_spconv_conv_os_f32(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                           int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy,
                           int tile_cfg, const int32_t* d_tile_order, void* d_workspace, void* stream);
/*   sst_spconv_conv_os_f32x3: sst_spconv_conv_os_f32 in SPLIT precision - every fp32 product as three bf16 products of split
 *     operands (x w ~= x_hi w_hi + x_lo w_hi + x_hi w_lo) on v_mfma_f32_16x16x32_bf16, fp32 accumulation, fp32 in memory
 *     (csrc/spconv_os_x3.hip; ~1e-5 of the output scale).  Same arguments, workspace size and launch order; tile_cfg = 0. */
int sst_spconv_conv_os_f32x3(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                             int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                             const int32_t* d_tile_order, void* d_workspace, void* stream);
/*   sst_spconv_conv_os_f32x6: the same contraction from the EXACT three-way bf16 split of both operands, six products per
 *     fp32 product on v_mfma_f32_16x16x32_bf16 with fp32 accumulation in two accumulator sets (csrc/spconv_os_x6.hip; the
 *     arithmetic class of the fp32 kernel: error vs float64 <= 2 x its error, tests/test_gpu_spconv.py).  Same arguments and
 *     launch order; workspace: sst_spconv_conv_os_f32x6_workspace_bytes (6 bytes per packed weight element); tile_cfg = 0. */
int64_t sst_spconv_conv_os_f32x6_workspace_bytes(int kvol, int cin, int cout);
int sst_spconv_conv_os_f32x6(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                             int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                             const int32_t* d_tile_order, void* d_workspace, void* stream);
/* sst_spconv_conv_os_rows_f32x6: the same call, told the size of its workspace.  With
 * sst_spconv_conv_os_f32x6_workspace_bytes_rows(kvol, cin, cout, m) bytes (packed weights + partial tiles) a THIN level - a few
 * thousand rows: 30-200 (row tile, column group) units for 256 CUs, each walking all 27 offsets alone - has its offsets dealt
 * out over up to 8 workgroups per unit, whose partial tiles are added in a fixed order by a second launch (deterministic; same
 * results up to the association of the per-offset sums).  d_workspace 256-byte aligned. */
int64_t sst_spconv_conv_os_f32x6_workspace_bytes_rows(int kvol, int cin, int cout, int64_t m);
int sst_spconv_conv_os_rows_f32x6(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                                  int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                                  const int32_t* d_tile_order, void* d_workspace, int64_t workspace_bytes, void* stream);
/*   sst_spconv_conv_os_rows_bf16: the same contraction with bf16 OPERANDS - the gathered rows and the weights are rounded to
 *     bf16 once (round to nearest even), one v_mfma_f32_16x16x32_bf16 product per pair, fp32 accumulation, fp32 result, fp32 in
 *     memory (csrc/spconv_os_bf16.hip): the contraction of round_bf16(x) and round_bf16(w) up to the fp32 summation order, i.e. what
 *     the f32x6 entries return on operands rounded beforehand.  The 'bf16' mode of sst_amd.spconv.SparseConvolution.  Argument
 *     list, restrictions, launch order and offset split of sst_spconv_conv_os_rows_f32x6; the packed weights take 2 bytes per
 *     element.  sst_spconv_conv_os_bf16_workspace_bytes_rows(kvol, cin, cout, m): packed weights + the partial tiles of the split
 *     the call chooses for m rows (m = 0: the packed weights alone, the least a call accepts - SST_ERR_ARG below it; between the
 *     two the split is halved until its partial tiles fit).  d_workspace 256-byte aligned.  Deterministic. */
int64_t sst_spconv_conv_os_bf16_workspace_bytes_rows(int kvol, int cin, int cout, int64_t m);
int sst_spconv_conv_os_rows_bf16(const float* d_x, int64_t ldx, const int32_t* d_map, int64_t m, int kvol, const float* d_w,
                                 int cin, int cout, int trans_w, const float* d_bias, float* d_y, int64_t ldy, int tile_cfg,
                                 const int32_t* d_tile_order, void* d_workspace, int64_t workspace_bytes, void* stream);
/*   sst_spconv_conv_os_plan: what a call of one of the five entries above would launch (host only, nothing runs): rows per
 *     tile (64 | 128), columns per workgroup (64 | 128), the offset split the call really uses (after the rows entry's own
 *     halving against workspace_bytes; 1 for the others, which ignore workspace_bytes) and the workgroups launched (the
 *     padded grid).  Computed by the functions the launches call.  Same error codes as the entry for m, kvol, cin, cout,
 *     tile_cfg and workspace_bytes; m >= 1. */
#define SST_SPCONV_OS_ENTRY_F32 0
#define SST_SPCONV_OS_ENTRY_F32X3 1
#define SST_SPCONV_OS_ENTRY_F32X6 2
#define SST_SPCONV_OS_ENTRY_ROWS_F32X6 3
#define SST_SPCONV_OS_ENTRY_ROWS_BF16 4
int sst_spconv_conv_os_plan(int entry, int64_t m, int kvol, int cin, int cout, int tile_cfg, int64_t workspace_bytes,
                            int32_t* tile_rows, int32_t* cols, int32_t* n_split, int64_t* workgroups);
/*   sst_spconv_wgrad_os_f32: the same filter gradient as sst_spconv_wgrad_f32 (indiceConvBackward, spconv_ops.h:359-446)
 *     with the gathered rows staged through LDS transposed, 64 x 64 blocks of dW[k], 2048-pair chunks (csrc/spconv_os.hip).
 *     cin % 4 == 0, cout % 4 == 0, row strides % 4 == 0, 16-byte aligned operands; SST_ERR_UNSUPPORTED otherwise. */
int64_t sst_spconv_wgrad_os_workspace_bytes(int kvol, int64_t pair_ld, int64_t total_pairs, int cin, int cout);
int sst_spconv_wgrad_os_f32(const float* d_x, int64_t ldx, const float* d_dy, int64_t lddy, const int32_t* d_pairs,
                            int64_t pair_ld, int64_t total_pairs, int x_side, const int32_t* d_num, int kvol, int cin,
                            int cout, float* d_dw, void* d_workspace, void* stream);
/*   sst_spconv_wgrad_os_plan: pairs per chunk (512 .. 2048) and the chunk slots (workgroups along x, partials in the
 *     workspace) of a call of sst_spconv_wgrad_os_f32 / _f32x6 with these arguments (host only). */
int sst_spconv_wgrad_os_plan(int kvol, int64_t pair_ld, int64_t total_pairs, int cin, int cout, int32_t* chunk_pairs,
                             int64_t* chunk_slots);
/*   sst_spconv_wgrad_os_f32x6: the same gradient from the exact three-way bf16 split of both gathered operands (six products on the
 *   bf16 matrix pipe, fp32 accumulation, two accumulator sets; csrc/spconv_os.hip sp_wgrad_os_x6_k): the filter-gradient half of
 *   the 'f32x6' convolution precision.  Same arguments and workspace as sst_spconv_wgrad_os_f32. */
int sst_spconv_wgrad_os_f32x6(const float* d_x, int64_t ldx, const float* d_dy, int64_t lddy, const int32_t* d_pairs,
                            int64_t pair_ld, int64_t total_pairs, int x_side, const int32_t* d_num, int kvol, int cin,
                            int cout, float* d_dw, void* d_workspace, void* stream);
/*   sst_spconv_wgrad_os_bf16: the same gradient with both gathered operands (x and dy) rounded to bf16 once, one product per pair on
 *   the bf16 matrix pipe, fp32 accumulation, fp32 result (csrc/spconv_os_bf16.hip sp_wgrad_os_bf16_k): the filter-gradient half of
 *   the 'bf16' convolution precision.  Same arguments, chunking (sst_spconv_wgrad_os_plan) and workspace as sst_spconv_wgrad_os_f32. */
int sst_spconv_wgrad_os_bf16(const float* d_x, int64_t ldx, const float* d_dy, int64_t lddy, const int32_t* d_pairs,
                             int64_t pair_ld, int64_t total_pairs, int x_side, const int32_t* d_num, int kvol, int cin,
                             int cout, float* d_dw, void* d_workspace, void* stream);
int64_t sst_spconv_wgrad_workspace_bytes(int kvol, int64_t pair_ld, int64_t total_pairs, int cin, int cout);
int sst_spconv_wgrad_f32(const float* d_x, int64_t ldx, const float* d_dy, int64_t lddy, const int32_t* d_pairs,
                         int64_t pair_ld, int64_t total_pairs, int x_side, const int32_t* d_num, int kvol, int cin,
                         int cout, float* d_dw, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rotated-box ops of the heads and the FSD training step (csrc/box_ops.hip).  fp32 only; deterministic (no atomics);
 * everything on `stream`.  BEV boxes are [x1, y1, x2, y2, ry] (the reference's xywhr2xyxyr form), LiDAR boxes
 * [x, y, z_bottom, w, l, h, rz].
 * ---------------------------------------------------------------------------------------------- */
#define SST_BOX_OVERLAP 0   /* overlap area of the rotated boxes                                       */
#define SST_BOX_IOU 1       /* rotated IoU, overlap / max(area_a + area_b - overlap, 1e-8)              */
#define SST_BOX_IOU_AXIS 2  /* axis-aligned IoU, ry ignored (iou_normal)                                */
#define SST_PIB_FIRST 0       /* points in boxes: smallest index of a box holding the point, else -1   */
#define SST_PIB_MEMBERSHIP 1  /* points in boxes: 0 / 1 per (point, box)                               */

/* Pairwise BEV overlap matrix.  Replaces iou3d_cuda.boxes_overlap_bev_gpu (mode SST_BOX_OVERLAP) and
 * iou3d_cuda.boxes_iou_bev_gpu (mode SST_BOX_IOU) of mmdet3d/ops/iou3d/src/iou3d.cpp:34-78 (kernels
 * iou3d_kernel.cu:127-282); SST_BOX_IOU_AXIS is the pairwise form of iou_normal (:335-343).
 *   d_a [n_a, 5], d_b [n_b, 5] fp32; d_out [n_a, n_b] fp32, caller-owned, every element written.  No workspace.
 *   PARITY: the arithmetic is restated from iou3d_kernel.cu (same operations and order, no contraction) and pinned to
 *   the reference's own known-answer tests (tests/golden/box_ops_kat.npz), not to a run of that kernel. */
int sst_boxes_overlap_bev_f32(const float* d_a, int64_t n_a, const float* d_b, int64_t n_b, int mode, float* d_out,
                              void* stream);

/* Aligned (1-to-1) BEV overlap: d_out[i] = value(d_a[i], d_b[i]) for the modes above.  Stands for TorchEx
 * boxes_overlap_1to1 as called from core/bbox/structures/lidar_box3d.py:404-449, 505-549 (mode SST_BOX_OVERLAP).
 *   d_a, d_b [n, 5] fp32; d_out [n] fp32, caller-owned.  Bit-identical to the diagonal of sst_boxes_overlap_bev_f32.
 *   PARITY: the TorchEx contract inferred from lidar_box3d.py (its source is absent from the reference tree); the
 *   per-pair arithmetic is that of sst_boxes_overlap_bev_f32. */
int sst_boxes_overlap_aligned_f32(const float* d_a, const float* d_b, int64_t n, int mode, float* d_out, void* stream);

/* NMS over boxes sorted by descending score.  Replaces iou3d_cuda.nms_gpu (rotated != 0) and nms_normal_gpu
 * (rotated == 0) of mmdet3d/ops/iou3d/src/iou3d.cpp:95-185 (mask kernels iou3d_kernel.cu:284-333, 345-): box i
 * suppresses a later box j when IoU(i, j) > threshold strictly; a box never suppresses itself.  Only the 64 x 64
 * tiles on or above the diagonal of the mask are computed; the greedy sweep (the reference's host loop) runs on the
 * device in one workgroup, so the mask never leaves the device.
 *   d_sorted_boxes [n, 5] fp32.  d_group: NULL (one group, threshold `thresh`) or int32 [n] group ids: boxes suppress
 *   only within their group, with the threshold h_group_thresh[g] (HOST fp32 [n_groups], 1 <= n_groups <= 64, passed
 *   to the kernel as an argument; +inf = no suppression, no IoU computed; an id outside [0, n_groups) suppresses
 *   nothing).
 *   d_keep [n] int64 (caller-owned): the kept positions in ascending order, first *d_num_keep entries written.
 *   d_num_keep: device int32 (the one value a caller reads back).  Workspace: sst_nms_bev_workspace_bytes(n)
 *   (the [n, ceil(n / 64)] mask).  n <= 516096, else SST_ERR_UNSUPPORTED.
 *   PARITY: the IoU arithmetic is restated from iou3d_kernel.cu and pinned to the reference's own known-answer tests
 *   (tests/golden/box_ops_kat.npz, test_parta2_bbox_head.py's multi_class_nms), not to a run of that kernel. */
int64_t sst_nms_bev_workspace_bytes(int64_t n);
int sst_nms_bev_f32(const float* d_sorted_boxes, const int32_t* d_group, int64_t n, float thresh,
                    const float* h_group_thresh, int n_groups, int rotated, int64_t* d_keep, int32_t* d_num_keep,
                    void* d_workspace, void* stream);

/* Points in boxes.  Replaces roiaware_pool3d_ext.points_in_boxes_gpu (mode SST_PIB_FIRST) and
 * points_in_boxes_batch (mode SST_PIB_MEMBERSHIP) of mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-105.
 *   d_boxes [batch, n_boxes, 7] fp32 LiDAR boxes, d_pts [batch, n_pts, 3] fp32.
 *   d_out int32, caller-owned, every element written: [batch, n_pts] (first box index or -1) or
 *   [batch, n_pts, n_boxes] (0 / 1).  No workspace.
 *   PARITY: the membership test is dpp_classify of the dynamic point pool (csrc/pib_test.h), pinned to the reference's
 *   compiled CPU routine points_in_boxes_cpu (tests/golden/point_pool.npz). */
int sst_points_in_boxes_f32(const float* d_boxes, const float* d_pts, int batch, int64_t n_boxes, int64_t n_pts,
                            int mode, int32_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Furthest point sampling and FSD's SSG cluster assignment (csrc/fps.hip).  fp32, deterministic, everything on `stream`.
 * ---------------------------------------------------------------------------------------------- */
#define SST_SSG_MULTI_BALL 1     /* status: some point lay in more than one ball                                  */
#define SST_SSG_EMPTY_SEGMENT 2  /* status: some non-empty segment assigned no point                              */
#define SST_SSG_BAD_KEYPOINT 4   /* status: a keypoint index outside its segment was skipped                      */

/* Furthest point sampling inside each of n_segments segments of a point array.  Replaces
 * furthest_point_sample_ext.furthest_point_sampling_wrapper of mmdet3d/ops/furthest_point_sample/src/
 * furthest_point_sample.cpp (kernel furthest_point_sample_cuda.cu:25-141), one segment per batch entry, and the
 * `if num_fps >= len(points)` branch of ssg_single_sample (detectors/single_stage_fsd.py:103-106).
 *   d_points [n_points, >= 3] fp32 with row stride ld (columns 0..2 are read).
 *   Segments: d_seg_offsets int32 [n_segments + 1] on the device, or NULL for n_segments segments of uniform_len points.
 *   d_idx int32 [n_segments, m]: sample j of segment s, RELATIVE to the segment's first point.  Sample 0 is point 0,
 *   sample j the arg-max of temp[k] = min(temp[k], d(k, sample j-1)), temp starting at 1e10 and
 *   d = (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1) evaluated left to right, every operation rounded on its own.
 *   Among equal distances the reference's winner is kept: the k with the smallest
 *   (bitreverse_{log2 B}(k mod B), k div B), B = max(min(2^floor(log2 n_s), 1024), 1) from the segment's length n_s.
 *   identity_if_short != 0: a segment with n_s <= m gets 0 .. n_s-1 in order (then -1), d_count[s] = n_s.  Otherwise the
 *   recurrence simply runs on when m > n_s (repeats, as in the reference) and d_count[s] = m.  An empty segment: a row of
 *   -1 and d_count[s] = 0.  d_count (int32 [n_segments]) may be NULL.
 *   d_temp fp32 [n_points]: workspace of the segments longer than 16 384 points (initialised here, used for the points
 *   behind the first 12 288 of such a segment); shorter ones keep their state in registers and leave it untouched.  No
 *   launch when n_segments == 0 or m == 0.
 *   NaN / infinite coordinates are outside the contract. */
int sst_fps_segmented_f32(const float* d_points, int64_t ld, int64_t n_points, const int32_t* d_seg_offsets,
                          int64_t uniform_len, int64_t n_segments, int m, int identity_if_short, float* d_temp,
                          int32_t* d_idx, int32_t* d_count, void* stream);

/* The same selection with the distance to the last sample read from row `old` of a [batch, n, n] matrix (values >= 0).
 * Replaces furthest_point_sampling_with_dist_wrapper (furthest_point_sample_cuda.cu:213-331).  d_temp fp32 [batch, n],
 * d_idx int32 [batch, m]. */
int sst_fps_with_dist_f32(const float* d_dist, int64_t batch, int64_t n, int m, float* d_temp, int32_t* d_idx,
                          void* stream);

/* Everything after the sampling in ssg_single_sample (detectors/single_stage_fsd.py:108-142) and the running base of
 * ssg() (:83-97), for all segments at once.  Keypoint j of segment s is the point d_key_idx[s * m + j] (relative to the
 * segment), j < d_key_count[s] (the outputs of sst_fps_segmented_f32).
 *   Pruning: keypoint j falls if ANY earlier keypoint i < j of its segment - fallen ones included - has
 *   sqrt(dx*dx + dy*dy) < thr2.  Numbering: a surviving keypoint's id = its rank among the survivors of its segment + the
 *   survivors of all earlier segments.  Assignment: d_cluster_id[p] = the id of the one surviving keypoint of p's segment
 *   with sqrt(dx*dx + dy*dy) < radius, or -1 if there is none or more than one.  thr2 and radius are the reference's
 *   Python scalars (radius * 2 + 0.01, radius) rounded to fp32 by the caller; sum and square root are computed as written,
 *   correctly rounded.
 *   d_points [n_points, >= 2] fp32 with row stride ld; d_seg_offsets int32 [n_segments + 1] (n_segments <= 65535).
 *   d_cluster_id int32 [n_points]; d_n_clusters, d_status: device int32 (SST_SSG_* bits; the first two are the
 *   reference's asserts :125 and :128).  Workspace: sst_ssg_assign_workspace_bytes(n_segments, m). */
int64_t sst_ssg_assign_workspace_bytes(int64_t n_segments, int m);
int sst_ssg_assign_f32(const float* d_points, int64_t ld, int64_t n_points, const int32_t* d_seg_offsets,
                       int64_t n_segments, const int32_t* d_key_idx, const int32_t* d_key_count, int m, float thr2,
                       float radius, int32_t* d_cluster_id, int32_t* d_n_clusters, int32_t* d_status, void* d_workspace,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * The fused SIR stage (csrc/sir_stage.hip): one stage of FSD's SIRLayer - Linear without bias, LayerNorm, activation and the
 * max pooling over the points of a cluster - in one launch forward and one backward.  Replaces, per stage of
 * voxel_encoders/voxel_encoder.py:738-750 (layer: voxel_encoders/utils.py:147-189; stack: backbones/sir.py:67-88; pooling:
 * torch_scatter.scatter_max through ops/sst/sst_ops.py:172-177), a GEMM, sst_add_layernorm_act_fwd_f32,
 * sst_segment_reduce_long_f32 and sst_concat_gather_f32.  fp32, c == 128, 1 <= k <= 256, deterministic, no float atomics.
 *   Forward, for every row r of d_x [n, k] (contiguous; rows need not be 16-byte aligned) with group g = d_inverse[r]:
 *     d_pre[r]   = d_x[r] . d_weight^T (+ d_add_rows[g])    d_weight [128, k] with row stride ldw >= k (a column slice of a
 *                  wider matrix is passed as it lies); the product is exact fp32 (v_mfma_f32_16x16x4_f32)
 *     d_y[r]     = act(LayerNorm(d_pre[r]; d_gamma, d_beta, eps)),  act: 0 none, 1 GELU (erf form), 2 ReLU
 *     d_stats[r] = (mean, rstd), the layout of sst_add_layernorm_act_fwd_f32
 *     d_pooled[g], d_argmax[g] = max over the group's rows of d_y and the SMALLEST row index attaining it, per column.
 *   d_add_rows (optional, [m, 128]): the split-weight form of the second stage, whose input the reference builds as
 *   cat([point_feats, pooled[unq_inv]]) (voxel_encoder.py:744-747): x W^T = point_feats W[:, :128]^T +
 *   (pooled W[:, 128:]^T)[unq_inv], so the [n, 256] matrix is never formed; the caller computes the small second product.
 *   The grouping is the CSR of a sorted-unique (d_perm [n], d_inverse [n], d_offsets [m + 1], as sst_segment_reduce_long_f32
 *   takes them); groups without rows are NOT written.  d_scratch: sst_segment_long_scratch_bytes(n, m, 128) bytes, 256-byte
 *   aligned, its first 4 m bytes ZEROED ONCE by the caller; the kernel leaves them zeroed.  d_pre, d_y, d_pooled, d_argmax,
 *   d_add_rows, d_gamma and d_beta must be 16-byte aligned.  NaN / Inf inputs are outside the contract.
 *   sst_sir_stage_tile_rows(): sorted positions per workgroup (a group crossing a multiple of it is merged across workgroups).
 *   Backward: d_dpre = gradient of d_pre given d_dy (at d_y, [n, 128]) and d_dpooled (at d_pooled, [m, 128]), either of which
 *   may be NULL: dy_total[r, c] = dy[r, c] + (argmax[inverse[r], c] == r ? dpooled[inverse[r], c] : 0) is formed on load and
 *   goes through the row arithmetic of sst_add_layernorm_act_bwd_f32; d_dgamma / d_dbeta [128] are overwritten.  d_workspace:
 *   sst_sir_gather_segmax_bwd_workspace_bytes(n) bytes.  The gradients of x, W and d_add_rows are products / a segmented sum
 *   of d_dpre and stay with the caller.
 *   Errors (nothing is launched): SST_ERR_UNSUPPORTED for c != 128, k outside 1..256 or an unknown act; SST_ERR_ARG for a
 *   NULL required pointer, a misaligned operand or ldw < k.
 * ---------------------------------------------------------------------------------------------- */
int sst_sir_stage_tile_rows(void);
int sst_sir_gather_segmax_fwd_f32(const float* d_x, int64_t n, int k, const float* d_weight, int64_t ldw, int c,
                                  const float* d_add_rows, const float* d_gamma, const float* d_beta, float eps, int act,
                                  const uint32_t* d_perm, const int32_t* d_inverse, const int32_t* d_offsets, int64_t m,
                                  void* d_scratch, float* d_pre, float* d_stats, float* d_y, float* d_pooled, int32_t* d_argmax,
                                  void* stream);
int64_t sst_sir_gather_segmax_bwd_workspace_bytes(int64_t n);
int sst_sir_gather_segmax_bwd_f32(const float* d_dy, const float* d_dpooled, const int32_t* d_argmax, const int32_t* d_inverse,
                                  const float* d_pre, const float* d_stats, const float* d_gamma, const float* d_beta, int act,
                                  int64_t n, int c, int64_t m, float* d_dpre, float* d_dgamma, float* d_dbeta, void* d_workspace,
                                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training side of VoteSegHead (csrc/seg_loss.hip): point targets of a batch, the decode / vote losses with the logged
 * statistics, and their backward.  fp32 data, everything on `stream`, no float atomics, no host read-back, bit-reproducible.
 * Replaces VoteSegHead.get_targets / get_point_labels / get_vote_target / encode_vote_targets and losses of
 * mmdet3d/models/decode_heads/segmentation_head.py:106-275 (and autograd's backward of the latter).
 *
 * Targets, one launch for all samples:
 *   d_points [n, ld >= 3] fp32 (columns 0..2 are read), sample s = rows d_pt_offsets[s] .. d_pt_offsets[s + 1] (device int32
 *   [batch + 1]); d_boxes [n_boxes, 7] fp32 (x, y, z_bottom, w, l, h, rz) of all samples, d_box_labels int64 [n_boxes], sample
 *   s = boxes d_box_offsets[s] .. d_box_offsets[s + 1].  A point belongs to the FIRST box of its own sample with label >= 0
 *   that holds it (dpp_box / dpp_classify of csrc/pib_test.h != 0) with w and l enlarged by (float)(2.0 * extra_width) when
 *   has_extra_width (enlarged_box_hw, lidar_box3d.py:331-346: for a negative width a box whose enlarged w or l would be <= 0
 *   keeps its own extents); boxes with label < 0 are skipped.  Outputs, every element written: d_inbox int32 [n] (index into
 *   d_boxes or -1), d_labels int64 [n] (the box's label or bg_label), d_vote_mask uint8 [n] (inbox >= 0), d_vote_targets
 *   [n, 3] = sign(delta) * sqrt(|delta|) with delta = centre - point, centre = (x, y, z_bottom + h * 0.5) or
 *   d_centers[inbox] (optional, [n_boxes, 3]); 0 for background rows.  Every operation is rounded once, the root correctly.
 *   sst_seg_targets_box_tile(): boxes per LDS tile.
 *
 * Losses.  d_logits [n, c], d_vote_preds [n, 3c], d_labels int64 [n], d_vote_targets [n, 3], d_vote_mask uint8 [n],
 * 1 <= c <= 32, n >= 1.  With z = logit_scale * logit:
 *   SST_SEG_SIGMOID_FOCAL  t[i, k] = (labels[i] == k) (label c = background: all zero), p = sigmoid(z),
 *                          e = (max(z, 0) - t z + log1p(exp(-|z|))) * (alpha t + (1 - alpha)(1 - t)) * |t - p|^gamma,
 *                          loss_sem = sum(e) / (n c)      (py_sigmoid_focal_loss, mmdet3d/models/losses/focal_loss.py:13-67)
 *   SST_SEG_SOFTMAX_CE     e_i = -w[labels[i]] * log_softmax(z_i)[labels[i]] (w = 1 when d_class_weight is NULL; the last
 *                          class is the background), loss_sem = sum(e) / n
 *   vote loss, both modes  over the points with d_vote_mask and 0 <= labels[i] < c:
 *                          loss_vote = sum_d |vote_preds[i, 3 labels[i] + d] - vote_targets[i, d]| / (3 num_valid), 0 without any
 *   statistics             d_score_thresh (device, NULL: none).  Sigmoid: c thresholds, tp[k] = #(p[i, k] > thr[k] and
 *                          labels[i] == k).  Cross entropy: n_groups thresholds and d_class_group int32 [c - 1] (the group of
 *                          each non-background class, anything else: in no group): group_score[g] = sum of the softmax over
 *                          the classes of g, pred[g] = group_score[g] > thr[g], num_fg = sum_g #pred[g], tp[k] = #(pred[group
 *                          of k] and labels[i] == k).  real[k] = #(labels[i] == k), recall = tp / (real + 1e-5).
 *   d_out float [2 + c + 1]: loss_sem, loss_vote (neither multiplied by a loss weight), recall per class, num_fg.
 *   d_counts int64 [2 + 2c]: num_valid, status, tp per class, real per class.  status bit 0: a label outside [0, c] (sigmoid)
 *   or [0, c) (cross entropy) - the row contributes nothing; bit 1: a masked point whose label is no class - no vote term.
 *   Forward = a launch writing one record per sst_seg_loss_tile_rows() rows into d_workspace
 *   (sst_seg_loss_workspace_bytes(n, c)) and a one-workgroup launch adding the records in index order; sums are carried in
 *   fp64 from the lane on.  Backward = one launch: d_g[2] (device: upstream gradient x loss weight of loss_sem, loss_vote)
 *   and the forward's d_counts -> d_dlogits [n, c] and d_dvote_preds [n, 3c], every element written; recomputed from the
 *   logits.  The L1 gradient is sign(pred - target) / (3 num_valid), sign(0) = 0.
 *   Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer, n < 1 or gamma < 0; SST_ERR_UNSUPPORTED for c
 *   outside 1..32, an unknown mode, or statistics over 32 classes in more than 28 groups (LDS).
 * ---------------------------------------------------------------------------------------------- */
#define SST_SEG_SIGMOID_FOCAL 0
#define SST_SEG_SOFTMAX_CE 1
int sst_seg_targets_box_tile(void);
int sst_seg_targets_f32(const float* d_points, int64_t ld, int64_t n, const int32_t* d_pt_offsets, int batch,
                        const float* d_boxes, const int64_t* d_box_labels, const int32_t* d_box_offsets, int64_t n_boxes,
                        int has_extra_width, double extra_width, int64_t bg_label, const float* d_centers, int32_t* d_inbox,
                        int64_t* d_labels, float* d_vote_targets, uint8_t* d_vote_mask, void* stream);
int sst_seg_loss_tile_rows(void);
int64_t sst_seg_loss_workspace_bytes(int64_t n, int c);
int sst_seg_loss_fwd_f32(const float* d_logits, const float* d_vote_preds, const int64_t* d_labels, const float* d_vote_targets,
                         const uint8_t* d_vote_mask, int64_t n, int c, int mode, float logit_scale, float gamma, float alpha,
                         const float* d_class_weight, const float* d_score_thresh, const int32_t* d_class_group, int n_groups,
                         float* d_out, int64_t* d_counts, void* d_workspace, void* stream);
int sst_seg_loss_bwd_f32(const float* d_logits, const float* d_vote_preds, const int64_t* d_labels, const float* d_vote_targets,
                         const uint8_t* d_vote_mask, int64_t n, int c, int mode, float logit_scale, float gamma, float alpha,
                         const float* d_class_weight, const float* d_g, const int64_t* d_counts, float* d_dlogits,
                         float* d_dvote_preds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training and decoding side of CenterHead (csrc/center_head.hip).  fp32 data, everything on `stream`, no float atomics, no
 * host read-back, bit-reproducible.
 *
 * Targets - replaces CenterHead.get_targets / get_targets_single (mmdet3d/models/dense_heads/centerpoint_head.py:385-560, a
 * Python loop over every box of every sample), gaussian_radius / draw_heatmap_gaussian / gaussian_2d
 * (mmdet3d/core/utils/gaussian.py:5-85) and LiDARInstance3DBoxes.gravity_center.  One memset over d_out and one launch for all
 * samples and tasks.
 *   d_boxes [n_boxes, box_cols] fp32, box_cols 7 or 9: (x, y, z_bottom, w, l, h, rz [, vx, vy]) of all samples, d_labels int64
 *   [n_boxes], sample s = boxes d_box_offsets[s] .. d_box_offsets[s + 1] (device int32 [batch + 1]).  task_table: HOST int32
 *   [n_tasks][2] = (first class, class count), n_tasks <= SST_CENTER_MAX_TASKS.  The feature map is W = grid_x /
 *   out_size_factor by H = grid_y / out_size_factor; point_cloud_range and voxel_size are HOST float arrays of which [0], [1]
 *   are read.  Slot k of a task is the box's rank in the reference's class-grouped list (all boxes of the task's first class in
 *   input order, then the second ...; labels outside the task are not in it); ranks >= max_objs do not exist.  A box whose w or
 *   l is <= 0 in cells keeps its rank and is skipped, so is a box whose centre cell (truncation toward zero of
 *   (x - pc_range) / voxel_size / out_size_factor, so a coordinate in (-1, 0) is cell 0) lies outside the map.
 *   radius = max(min_radius, (int)gaussian_radius((l, w) in cells, gaussian_overlap)) in the reference's fp32 operation order,
 *   roots correctly rounded; heatmap[class] = max(heatmap[class], exp(-(dx^2 + dy^2) / (2 sigma^2))), sigma = (2 radius + 1) /
 *   6, over the patch clipped to the map, evaluated in fp64 and rounded to fp32.
 *   d_out: one allocation of sst_center_targets_layout(...) bytes; that call also fills HOST offsets[4 * n_tasks] with the byte
 *   offsets (multiples of 256) of each task's heatmap [batch, classes, H, W] fp32, anno_box [batch, max_objs, 10] fp32
 *   (x - cell, y - cell, z_bottom + h * 0.5, log(w, l, h) when norm_bbox else w, l, h, sin rz, cos rz, vx, vy; 0 velocities for
 *   7 columns), ind [batch, max_objs] int64 (y * W + x) and mask [batch, max_objs] uint8.  Empty slots are zero.
 *   sst_center_targets_box_tile(): boxes per workgroup.
 *
 * Losses of one task - replaces CenterHead.loss :563-610 (clip_sigmoid, GaussianFocalLoss, the concatenation / permute /
 * _gather_feat :360-383 of the regression maps, L1Loss) and autograd's backward of it.
 *   d_logits, d_heatmap [batch, classes, H, W] (hw = H * W): p = clamp(sigmoid(z), 1e-4, 1 - 1e-4),
 *     loss_heatmap = weight_cls * sum(-log(p + 1e-12) (1 - p)^2 [t == 1] - log(1 - p + 1e-12) p^2 (1 - t)^4) / max(#(t == 1), 1)
 *   (mmdet 2.x gaussian_focal_loss, alpha 2, gamma 4; mmdet is not in the reference tree).  The logits are not modified.
 *   d_heads: HOST array of 5 device pointers (reg, height, dim, rot, vel), NCHW with head_channels[5] (HOST; 0 = absent, at most
 *   10 in all); channel c of their concatenation is compared with column c of d_anno [batch, max_objs, 10] at cell d_ind[b, k]:
 *     loss_bbox = weight_bbox * sum(|pred - target| mask code_weights[c]) / (sum(mask) + 1e-4),   code_weights: HOST float[10]
 *   (the denominator is formed in fp32, as the reference's avg_factor = mask.float().sum() + 1e-4 is)
 *   A masked slot whose ind is outside [0, hw) adds nothing (the reference's gather raises).  Targets are assumed finite.
 *   d_out float [2]: loss_heatmap, loss_bbox.  d_counts int64 [2]: #(t == 1), sum(mask).
 *   Forward = a launch writing one record per sst_center_loss_tile_cells() cells into d_workspace
 *   (sst_center_loss_workspace_bytes(batch * classes * hw)) and a one-workgroup launch that adds the records in index order and
 *   computes the box loss; sums are carried in fp64 from the lane on.  Backward: d_g_heatmap, d_g_bbox (device scalars, the
 *   upstream gradients of the two losses; NULL = zero) and the forward's d_counts -> d_dlogits (every element written; zero where the clamp is active) and d_dheads, one allocation of
 *   batch * sum(head_channels) * hw floats holding the gradients of the present heads one after the other: a memset, the
 *   element-wise heatmap launch and one launch with a workgroup per sample, in which the lowest slot of each cell adds the
 *   contributions sign(pred - target) weight / denominator of all slots naming that cell in slot order (sign(0) = 0).
 *   max_objs <= sst_center_loss_max_objs() in the backward.
 *
 * Decoding - replaces CenterPointBBoxCoder.decode (mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py:115-227) after its
 * _topk.  d_inds int64 / d_scores fp32 [batch, k]: cell indices in [0, hw) and scores.  d_maps: HOST array of 6 device pointers
 * (reg 2 channels, height 1, dim 3, rot_sine 1, rot_cosine 1, vel 2; reg and vel may be NULL), each with channels hw floats
 * apart and samples batch_strides[m] floats apart (HOST int64 [6]).  Per index: x = ((cell % W) + reg0 [or 0.5]) *
 * out_size_factor * voxel_size[0] + pc_range[0], y likewise with (int)((float)cell / W), z = height, dim (exp when norm_bbox),
 * atan2(sine, cosine), vel -> d_boxes [batch, k, 9 or 7 without vel]; d_keep uint8 [batch, k] = (score > score_threshold when
 * has_score_threshold) and (post_center_range[0..2] <= (x, y, z) <= post_center_range[3..5] when given; HOST float[6]).  An index
 * outside the map gives a zero box that is not kept.
 *
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer or a size < 1; SST_ERR_UNSUPPORTED for box_cols other
 * than 7 / 9, more than 10 head channels, a map of 2^31 cells or more, or max_objs above the backward's limit.
 * ---------------------------------------------------------------------------------------------- */
#define SST_CENTER_MAX_TASKS 8
int sst_center_targets_box_tile(void);
int64_t sst_center_targets_layout(int batch, int n_tasks, const int32_t* task_table, int grid_x, int grid_y,
                                  int out_size_factor, int max_objs, int64_t* offsets);
int sst_center_targets_f32(const float* d_boxes, int box_cols, const int64_t* d_labels, const int32_t* d_box_offsets,
                           int64_t n_boxes, int batch, const int32_t* task_table, int n_tasks, int grid_x, int grid_y,
                           const float* point_cloud_range, const float* voxel_size, int out_size_factor,
                           double gaussian_overlap, int min_radius, int max_objs, int norm_bbox, void* d_out, void* stream);
int sst_center_loss_tile_cells(void);
int sst_center_loss_max_objs(void);
int64_t sst_center_loss_workspace_bytes(int64_t n_cells);
int sst_center_loss_fwd_f32(const float* d_logits, const float* d_heatmap, int batch, int classes, int64_t hw,
                            const float* const* d_heads, const int32_t* head_channels, const float* d_anno,
                            const int64_t* d_ind, const uint8_t* d_mask, int max_objs, const float* code_weights,
                            float weight_cls, float weight_bbox, float* d_out, int64_t* d_counts, void* d_workspace,
                            void* stream);
int sst_center_loss_bwd_f32(const float* d_logits, const float* d_heatmap, int batch, int classes, int64_t hw,
                            const float* const* d_heads, const int32_t* head_channels, const float* d_anno,
                            const int64_t* d_ind, const uint8_t* d_mask, int max_objs, const float* code_weights,
                            float weight_cls, float weight_bbox, const float* d_g_heatmap, const float* d_g_bbox,
                            const int64_t* d_counts, float* d_dlogits, float* d_dheads, void* stream);
int sst_center_decode_f32(const int64_t* d_inds, const float* d_scores, int batch, int k, int grid_w, int64_t hw,
                          const float* const* d_maps, const int64_t* batch_strides, int out_size_factor,
                          const float* voxel_size, const float* pc_range, int norm_bbox, int has_score_threshold,
                          float score_threshold, const float* post_center_range, float* d_boxes, uint8_t* d_keep,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training and decoding side of the FSD cluster heads, SparseClusterHeadV2 and FSDV2Head (csrc/cluster_head.hip).  fp32 data,
 * everything on `stream`, no float atomics, no host read-back, bit-reproducible.
 *
 * Targets - replaces, for ALL tasks and ALL samples in one launch, the per-task per-sample Python loop of
 * mmdet3d/models/dense_heads/sparse_cluster_head_v2.py:299-405 (modify_gt_for_single_task(_single_sample), get_targets,
 * get_targets_single), fsd_v2_head.py:277-395 (the same, with xyz_for_assign of centroid_assign), sparse_cluster_head.py:269-289
 * (split_by_batch / combine_by_batch) and :364-397 (assign_single), LiDARInstance3DBoxes.enlarged_box
 * (core/bbox/structures/lidar_box3d.py:269-285) and BasePointBBoxCoder.encode (core/bbox/coders/base_point_bbox_coder.py:36-58).
 *   d_xyz_assign, d_xyz_base [n, 3] fp32: the points tested for membership and the points the regression is relative to (the
 *   same pointer unless centroid_assign).  Row i belongs to sample d_batch_idx[i * batch_idx_stride] (int64; rows of different
 *   samples may interleave; an index outside [0, batch) gives a background row).  d_boxes [n_boxes, box_cols] fp32, box_cols 7,
 *   9 or 10: (x, y, z_bottom, w, l, h, rz [, vx, vy [, copy-paste flag]]), d_box_labels int64, sample s = boxes
 *   d_box_offsets[s] .. d_box_offsets[s + 1] (device int32 [batch + 1]).  class_table: HOST int32 [n_classes][2] = (task or -1,
 *   class index within the task), n_classes <= 64; task_classes: HOST int32 [n_tasks], n_tasks <= SST_CLUSTER_MAX_TASKS, at most
 *   32 classes each.  A box with label < 0, >= n_classes or of a class in no task is in no list.  Membership: dpp_box /
 *   dpp_classify of csrc/pib_test.h != 0 on the box enlarged by has_enlarge_width ? enlarge_width : nothing (w, l, h +=
 *   (float)(2 width), z -= (float)width; for a negative width a box whose enlarged w, l or h would be <= 0 keeps its own
 *   extents).  Per task the assigned box is the hit with the smallest (class index within the task, box index): the first
 *   hit of the reference's class-regrouped list.
 *   d_out: one allocation of sst_cluster_targets_layout(n, n_tasks, code_size, offsets) bytes; the call fills HOST
 *   offsets[4 * n_tasks] with the byte offsets (multiples of 256) of each task's labels int64 [n] (class index within the task,
 *   or the task's class count for background), bbox_targets fp32 [n, code_size] (box xyz - base, each one rounded subtraction;
 *   logf(dim + 1e-6f); sinf / cosf of rz; vx, vy when code_size is 10), bbox_weights fp32 [n, code_size] (1 on positive rows, the
 *   last two columns = box column 9 when box_cols is 10: sparse_cluster_head_v2.py:393-398) and assigned int32 [n] (index into
 *   d_boxes or -1).  Rows without a hit are zero.  code_size 8 goes with 7 box columns, 10 with 9 or 10 (SST_ERR_ARG otherwise).
 *   sst_cluster_targets_box_tile(): boxes per LDS tile.
 *   sst_cluster_encode_f32: BasePointBBoxCoder.encode on n boxes and n base points.
 *
 * Losses of all tasks - replaces loss_single_task (sparse_cluster_head_v2.py:192-297, fsd_v2_head.py:168-275) per task:
 * FocalLoss (sigmoid; py_sigmoid_focal_loss of mmdet3d/models/losses/focal_loss.py:13-67, sum / avg_factor), the nonzero() of
 * pos_inds, the three or four gathered L1Loss calls, and autograd's backward.  tasks: HOST array of n_tasks
 * sst_cluster_loss_task (device pointers: logits [n, classes], reg_preds / bbox_targets / bbox_weights [n, code_size], labels
 * int64 [n]; d_logits / d_reg_preds: the backward's outputs), n >= 1, classes <= 32.  code_weight: HOST float [code_size] or NULL;
 * loss_weights: HOST float [5] (cls, center, size, rot, vel); smooth_l1_beta: HOST float [5] in the same order or NULL - a
 * regression loss with beta > 0 is mmdet's SmoothL1Loss (0.5 d^2 / beta below beta, |d| - 0.5 beta above; configs/fsdv2/
 * fsdv2_argo_2x.py), with 0 its L1Loss ([0] is not read).  Positive rows: 0 <= label < classes; label == classes:
 * background (all-zero targets).
 *   loss_cls = w_cls * sum(focal) / cls_avg;  loss_center / size / rot = w * sum(|pred - target| weight code_weight over columns
 *   0-2 / 3-5 / 6-7 of the positive rows) / reg_avg;  loss_vel = w_vel * sum(columns 8-9) / (2 num_pos) (the reference gives
 *   loss_vel no avg_factor: the mean over elements).  The four regression losses are exactly 0 without a positive row.
 *   d_out float [n_tasks][5]; d_counts double [n_tasks][4] = (num_pos, status, cls_avg, reg_avg).  status bit 0: a label outside
 *   [0, classes] - the row contributes nothing; bit 1: a weight of column 8 / 9 of a positive row other than 0 or 1.
 *   Forward, phases = SST_CLUSTER_LOSS_COUNTS | SST_CLUSTER_LOSS_FINISH: a launch (grid = sst_cluster_loss_tile_rows() row
 *   tiles x tasks) writing one record per workgroup into d_workspace (sst_cluster_loss_workspace_bytes(n, n_tasks)) and a
 *   one-workgroup launch that adds the records in index order, writes d_counts with cls_avg = n, reg_avg = num_pos and the
 *   losses.  With phases = COUNTS alone the second launch only writes d_counts; with FINISH alone it reads cls_avg / reg_avg
 *   FROM d_counts - so a caller can average the factors over processes on the device between the two calls (reduce_mean).
 *   Sums are carried in fp64 from the lane on.  Backward = one launch (grid = 256-row tiles x tasks): d_g float [n_tasks][5]
 *   (device: upstream gradients) and the forward's d_counts -> every element of every task's d_logits and d_reg_preds;
 *   recomputed from the logits; the L1 gradient is sign(pred - target) weight code_weight w / avg, sign(0) = 0
 *   ((pred - target) / beta in its place below a SmoothL1Loss's beta).
 *
 * Decoding of one task - BasePointBBoxCoder.decode (base_point_bbox_coder.py:60-82): d_boxes [n, code_size - 1] = (base + d,
 * expf(dims) - 1e-6f, atan2f(sin, cos) [, vx, vy]); optionally d_scores [n, classes + 1] = sigmoid(d_logits [n, classes]) with a
 * zero last column (sparse_cluster_head_v2.py:534, :552-554) and d_bev [n, 5] = (x - w / 2, y - l / 2, x + w / 2, y + l / 2, yaw),
 * the rows xywhr2xyxyr(boxes.bev) gives for the NMS.
 *
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer, a bad size or table; SST_ERR_UNSUPPORTED for a count
 * beyond the limits above.
 * ---------------------------------------------------------------------------------------------- */
#define SST_CLUSTER_MAX_TASKS 8
#define SST_CLUSTER_LOSS_COUNTS 1
#define SST_CLUSTER_LOSS_FINISH 2
typedef struct sst_cluster_loss_task {
  const float* logits;
  const float* reg_preds;
  const int64_t* labels;
  const float* bbox_targets;
  const float* bbox_weights;
  float* d_logits;
  float* d_reg_preds;
  int32_t classes;
  int32_t reserved;
} sst_cluster_loss_task;
int sst_cluster_max_tasks(void);
int sst_cluster_targets_box_tile(void);
int sst_cluster_loss_tile_rows(void);
int64_t sst_cluster_targets_layout(int64_t n, int n_tasks, int code_size, int64_t* offsets);
int sst_cluster_targets_f32(const float* d_xyz_assign, const float* d_xyz_base, int64_t n, const int64_t* d_batch_idx,
                            int64_t batch_idx_stride, int batch, const float* d_boxes, int box_cols,
                            const int64_t* d_box_labels, const int32_t* d_box_offsets, int64_t n_boxes,
                            const int32_t* class_table, int n_classes, const int32_t* task_classes, int n_tasks, int code_size,
                            int has_enlarge_width, double enlarge_width, void* d_out, void* stream);
int sst_cluster_encode_f32(const float* d_boxes, int box_cols, const float* d_base, int64_t n, int code_size, float* d_out,
                           void* stream);
int64_t sst_cluster_loss_workspace_bytes(int64_t n, int n_tasks);
int sst_cluster_loss_fwd_f32(const sst_cluster_loss_task* tasks, int n_tasks, int64_t n, int code_size, float gamma, float alpha,
                             const float* code_weight, const float* loss_weights, const float* smooth_l1_beta, int phases,
                             float* d_out, double* d_counts, void* d_workspace, void* stream);
int sst_cluster_loss_bwd_f32(const sst_cluster_loss_task* tasks, int n_tasks, int64_t n, int code_size, float gamma, float alpha,
                             const float* code_weight, const float* loss_weights, const float* smooth_l1_beta, const float* d_g,
                             const double* d_counts, void* stream);
int sst_cluster_decode_f32(const float* d_reg_preds, const float* d_base, const float* d_logits, int64_t n, int code_size,
                           int classes, float* d_boxes, float* d_scores, float* d_bev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The second stage of FSD / FSDv2 around its network, GroupCorrectionHead with FullySparseBboxHead (csrc/roi_head.hip).  fp32
 * data, everything on `stream`, no float atomics, no host read-back, bit-reproducible.  Boxes are (x, y, z_bottom, w, l, h, rz
 * [, vx, vy]); proposals have 7 or 9 columns, ground truth 7 or more (the first 7 are read).  Sample s owns proposals
 * prop_offsets[s] .. prop_offsets[s + 1] and boxes gt_offsets[s] .. gt_offsets[s + 1] (device int32 [batch + 1]).
 *
 * sst_roi_assign_f32 - replaces, for ALL samples and classes in one launch, the loop of mmdet3d/models/roi_heads/
 * fsd_roi_head.py:229-289 (_assign_and_sample: per sample and class two boolean compactions and an IoU launch) and
 * BboxOverlaps3D / BaseInstance3DBoxes.overlaps (core/bbox/structures/base_box3d.py:395-450).  Per proposal (one lane each,
 * sst_roi_assign_block() per workgroup, the sample's boxes through LDS tiles of sst_roi_assign_gt_tile()): the 3-D IoU with the
 * boxes of its sample and, when class_mask != 0 (the list of per-class assigners), of its own predicted class - the BEV overlap
 * of csrc/bev_clip.h x the clamped height overlap / the clamped union, the operation order of box_ops.boxes3d_overlaps_lidar.
 * A box with a label outside [0, num_classes) and a proposal with such a label match nothing.
 *   iou fp32 [n_props, ld]: column j = box gt_offsets[s] + j of the proposal's sample, -1 where masked or past the sample's
 *   boxes (every element is written); ld >= the largest box count of a sample.  max_iou fp32 [n_props]: the row maximum, 0
 *   without a match; argmax int32 [n_props]: the first box (index into gts) that attains it, -1 without a match.
 *
 * sst_roi_sample_targets_f32 - one launch, one workgroup per sample; replaces mmdet's MaxIoUAssigner.assign_wrt_overlaps (the
 * Python loop over boxes of gt_max_assign_all), core/bbox/samplers/iou_neg_piecewise_sampler.py:46-164 (nonzero, randperm,
 * unique) and bbox_heads/fsd_bbox_head.py:343-543 (get_targets, _get_target_single, get_multi_class_soft_label) with
 * core/bbox/coders/delta_xyzwhlr_bbox_coder.py:20-56 (encode).  Thresholds are indexed by the proposal's (box's) class when
 * class_mask != 0, else [0].
 *   Assignment: background where 0 <= max < neg_iou_thr, positive (argmax) where max >= pos_iou_thr, ignored between; then for
 *   every box in index order whose column maximum is >= min_pos_iou, every proposal whose IoU equals that maximum goes to it
 *   (the last box wins).  Sampling: min(positives, num_expected_pos) positives; num - that many negatives: all when there are
 *   no more, else piece k = [piece_thr[k + 1], piece_thr[k]) (the last from 0) takes (int)(expected * piece_frac[k]) + the
 *   shortfall carried from the pieces before it (the last piece: what is left).  "k of a pool" = its k smallest (keys[i], i).
 *   Outputs per sample, num rows each, positives first, each group in ascending proposal index, zero / -1 padding:
 *   rois fp32 [batch * num, 1 + prop_cols] = (sample, box), src int32 (proposal index), gt_index int32 (index into gts, -1 off
 *   the positives), labels int64 (-1 off the positives), iou_out fp32 (row maximum), soft_label fp32 (get_multi_class_soft_label
 *   on cls_pos_thr / cls_neg_thr of the box's class; 0 on negatives), reg_mask uint8, targets fp32 [batch * num, 7]
 *   (_get_target_single; 0 off the positives), counts int32 [batch, 2] = (positives, negatives), (-1, -1) for a sample with
 *   more than sst_roi_sample_max_proposals() proposals (SST_ERR_UNSUPPORTED when max_props_per_sample says so up front).
 *   assigned: int32 [n_props] workspace (-1 background, -2 ignored, else the box).  Every element is written.
 *
 * sst_roi_loss_fwd_f32 / _bwd_f32 - replaces FullySparseBboxHead.loss, filter_pos_assigned_but_empty_rois and
 * get_corner_loss_lidar (fsd_bbox_head.py:207-341, :546-579) over n >= 1 RoI rows:
 *   loss_cls = w_cls * sum over nonempty rows of BCE-with-logits(cls_score, soft_label) / cls_avg;
 *   loss_bbox = w_reg * sum over rows with reg_mask & nonempty of loss(bbox_pred - targets) * code_weight / reg_avg, loss = |d|
 *   (beta == 0) or mmdet's smooth L1;  loss_corner = w_corner * mean over 8 corners x the kept rows of Huber(min(distance to the
 *   box's corners, to the corners of the box turned by pi)) of the prediction decoded against the zero-centred RoI, turned by
 *   roi_ry + pi / 2 and moved to the RoI centre; kept rows = those of loss_bbox with labels == car_index (all when car_index < 0);
 *   with_corner == 0: no corner loss.  loss_bbox and loss_corner are exactly 0 without a row.
 *   d_out float [5] = (loss_cls, loss_bbox, loss_corner, num_pos_rois, num_neg_rois); d_counts double [4] = (num_pos, corner
 *   rows, cls_avg = n, reg_avg = num_pos).  phases: SST_ROI_LOSS_COUNTS | SST_ROI_LOSS_FINISH as for sst_cluster_loss_fwd_f32
 *   (two launches; COUNTS alone stops after d_counts, FINISH alone reads the averaging factors from d_counts).  Workspace:
 *   sst_roi_loss_workspace_bytes(n).  Sums are fp64 from the lane on, in a fixed order.
 *   Backward, one launch: d_g float [3] (device; upstream gradients of the three losses) and d_counts -> every element of
 *   d_dcls [n] and d_dbbox [n, 7], with the corner loss's gradient through the decode derived by hand.
 *
 * sst_roi_decode_f32 - fsd_bbox_head.py:609, :634-653: d_boxes [n, roi_cols - 1] = decode_from_rois (velocity columns of a
 * 9-column RoI pass through), d_scores [n] = sigmoid(d_cls_score) (optional), d_bev [n, 5] = the xyxyr NMS rows (optional).
 * ---------------------------------------------------------------------------------------------- */
#define SST_ROI_MAX_CLASSES 16
#define SST_ROI_MAX_PIECES 8
#define SST_ROI_LOSS_COUNTS 1
#define SST_ROI_LOSS_FINISH 2
typedef struct sst_roi_assign_args {
  const float* props;
  const int64_t* prop_labels;
  const int32_t* prop_offsets;
  const float* gts;
  const int64_t* gt_labels;
  const int32_t* gt_offsets;
  float* iou;
  float* max_iou;
  int32_t* argmax;
  int64_t n_props, n_gts, ld;
  int32_t prop_cols, gt_cols, batch, num_classes, class_mask, reserved;
} sst_roi_assign_args;
typedef struct sst_roi_sample_args {
  const float* props;
  const int64_t* prop_labels;
  const int32_t* prop_offsets;
  const float* gts;
  const int64_t* gt_labels;
  const int32_t* gt_offsets;
  const float* iou;
  const float* max_iou;
  const int32_t* argmax;
  const float* keys;
  int32_t* assigned;
  float* rois;
  int32_t* src;
  int32_t* gt_index;
  int64_t* labels;
  float* iou_out;
  float* soft_label;
  uint8_t* reg_mask;
  float* targets;
  int32_t* counts;
  int64_t n_props, n_gts, ld, max_props_per_sample;
  int32_t prop_cols, gt_cols, batch, num_classes, class_mask, num, num_expected_pos, n_pieces;
  float pos_iou_thr[SST_ROI_MAX_CLASSES], neg_iou_thr[SST_ROI_MAX_CLASSES], min_pos_iou[SST_ROI_MAX_CLASSES];
  float piece_thr[SST_ROI_MAX_PIECES];
  double cls_pos_thr[SST_ROI_MAX_CLASSES], cls_neg_thr[SST_ROI_MAX_CLASSES];
  double piece_frac[SST_ROI_MAX_PIECES];
} sst_roi_sample_args;
typedef struct sst_roi_loss_args {
  const float* cls_score;
  const float* bbox_pred;
  const uint8_t* nonempty;
  const float* rois;
  const float* soft_label;
  const uint8_t* reg_mask;
  const float* targets;
  const int32_t* gt_index;
  const int64_t* labels;
  const float* gts;
  int64_t n, n_gts;
  int32_t roi_cols, gt_cols, with_corner, car_index;
  float beta, w_cls, w_reg, w_corner;
  float code_weight[7];
  float reserved;
} sst_roi_loss_args;
int sst_roi_assign_gt_tile(void);
int sst_roi_assign_block(void);
int sst_roi_sample_max_proposals(void);
int sst_roi_assign_f32(const sst_roi_assign_args* args, void* stream);
int sst_roi_sample_targets_f32(const sst_roi_sample_args* args, void* stream);
int64_t sst_roi_loss_workspace_bytes(int64_t n);
int sst_roi_loss_fwd_f32(const sst_roi_loss_args* args, int phases, float* d_out, double* d_counts, void* d_workspace,
                         void* stream);
int sst_roi_loss_bwd_f32(const sst_roi_loss_args* args, const float* d_g, const double* d_counts, float* d_dcls, float* d_dbbox,
                         void* stream);
int sst_roi_decode_f32(const float* d_rois, int roi_cols, const float* d_bbox_pred, const float* d_cls_score, int64_t n,
                       float* d_boxes, float* d_scores, float* d_bev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Anchor3DHead around its three 1 x 1 convolutions (csrc/anchor_head.hip).  fp32 data, everything on `stream`, no float atomics,
 * no host read-back, bit-reproducible.  No anchor tensor is read: anchor a = ((h * W + w) * n_sizes + s) * n_rots + r of a sample
 * (the reference's flattening of its [1, H, W, n_sizes, n_rots, 7] tensor) is (centers.x[s][w], centers.y[s][h], centers.z[s],
 * sizes[s], rots[r]).  centers: device fp32, xs [n_sizes, W], then ys [n_sizes, H], then zs [n_sizes] - the generator's own
 * torch.linspace tables, so every centre is bit-equal to the reference's.  Boxes are (x, y, z_bottom, w, l, h, rz, ...) with
 * gt_cols >= 7 columns; sample b owns boxes gt_offsets[b] .. gt_offsets[b + 1] (device int32 [batch + 1]).
 *
 * sst_anchor_targets_f32 - one memset and two launches for all samples and sizes; replaces anchor_target_3d_single
 * (mmdet3d/models/dense_heads/train_mixins.py:101-314) with a list of MaxIoUAssigner (one per size; pos_iou_thr / neg_iou_thr /
 * min_pos_iou are host arrays [n_sizes], all > 0 but neg), BboxOverlapsNearest3D('lidar') (iou3d_calculator.py:94-140,
 * nearest_bev of lidar_box3d.py:123-141, mmdet bbox_overlaps: every step one correctly rounded fp32 operation) and
 * PseudoSampler.  The anchors of size s meet the sample's boxes - those with label s when assign_per_class.  Per anchor: the
 * maximum IoU and its first arg-max; background where max < neg_iou_thr, the arg-max where max >= pos_iou_thr, ignored between;
 * then for every box in index order whose largest IoU over the size's anchors is >= min_pos_iou, every anchor whose IoU equals
 * it goes to the box (the last box wins).
 *   d_assigned int32 [batch, H * W * n_sizes * n_rots]: the box index within the sample, -1 background, -2 ignored (every
 *   element is written).  d_state int32 [n_sizes * n_gts + batch]: the float bits of the largest IoU per (size, box), then the
 *   positives per sample.  A workgroup is a tile of sst_anchor_block() cells; the boxes pass through LDS in chunks of
 *   sst_anchor_targets_gt_chunk().
 *
 * sst_anchor_loss_fwd_f32 / _bwd_f32 - replaces Anchor3DHead.loss / loss_single (dense_heads/anchor3d_head.py:197-379) with
 * sigmoid FocalLoss, L1Loss (smooth_l1 == 0) or SmoothL1Loss(beta), softmax CrossEntropyLoss of the direction, all 'mean' with
 * avg_factor = sum over samples of max(positives, 1).  cls_score [B, n_a * C, H, W], bbox_pred [B, n_a * 7, H, W], dir_pred
 * [B, n_a * 2, H, W] or NULL (no direction classifier), n_a = n_sizes * n_rots: read where they lie.  The target of a positive
 * anchor is formed in the kernel: DeltaXYZWLHRBBoxCoder.encode, get_direction_target(dir_offset), add_sin_difference when
 * sin_diff.  The weight of a class term: 0 ignored, pos_weight (> 0) or 1 positive, 1 background.
 *   Forward, two launches: d_out float [4] = (loss_cls, loss_bbox, loss_dir, avg_factor); workspace
 *   sst_anchor_loss_workspace_bytes(batch, H, W).  Sums are fp64 from the lane on, in a fixed order.
 *   Backward, one launch: d_g_* (device scalars, NULL = no upstream gradient) and d_out -> every element of the three gradient
 *   maps, zeros included.
 *
 * sst_anchor_decode_f32 - one sample: get_bboxes_single :465-530 after its topk.  d_inds int64 [n] anchor indices (NULL: 0 ..
 * n - 1); d_boxes [n, 7] = DeltaXYZWLHRBBoxCoder.decode against the analytic anchor, d_scores [n, C + 1] = sigmoid with the zero
 * background column, d_dir int64 [n] = the direction arg-max (0 at a tie, 0 without dir_pred), d_bev [n, 5] = xyxyr NMS rows.
 * ---------------------------------------------------------------------------------------------- */
#define SST_ANCHOR_MAX_SIZES 8
#define SST_ANCHOR_MAX_ROTS 4
typedef struct sst_anchor_grid {
  const float* centers;
  int32_t H, W, n_sizes, n_rots;
  float sizes[SST_ANCHOR_MAX_SIZES][3];
  float rots[SST_ANCHOR_MAX_ROTS];
} sst_anchor_grid;
typedef struct sst_anchor_loss_args {
  const float* cls_score;
  const float* bbox_pred;
  const float* dir_pred;
  const int32_t* assigned;
  const float* gts;
  const int64_t* gt_labels;
  const int32_t* gt_offsets;
  const int32_t* pos_counts;
  int64_t n_gts;
  int32_t gt_cols, batch, num_classes, smooth_l1, sin_diff, reserved;
  float gamma, alpha, w_cls, w_bbox, w_dir, beta, pos_weight, dir_offset;
  float code_weight[7];
  float reserved_f;
} sst_anchor_loss_args;
int sst_anchor_targets_gt_chunk(void);
int sst_anchor_block(void);
int sst_anchor_targets_f32(const sst_anchor_grid* grid, const float* d_gts, int gt_cols, const int64_t* d_gt_labels,
                           const int32_t* d_gt_offsets, int64_t n_gts, int batch, int assign_per_class, const float* pos_iou_thr,
                           const float* neg_iou_thr, const float* min_pos_iou, int32_t* d_assigned, int32_t* d_state,
                           void* stream);
int64_t sst_anchor_loss_workspace_bytes(int batch, int grid_h, int grid_w);
int sst_anchor_loss_fwd_f32(const sst_anchor_grid* grid, const sst_anchor_loss_args* args, float* d_out, void* d_workspace,
                            void* stream);
int sst_anchor_loss_bwd_f32(const sst_anchor_grid* grid, const sst_anchor_loss_args* args, const float* d_out,
                            const float* d_g_cls, const float* d_g_bbox, const float* d_g_dir, float* d_dcls, float* d_dbbox,
                            float* d_ddir, void* stream);
int sst_anchor_decode_f32(const sst_anchor_grid* grid, const float* d_cls_score, const float* d_bbox_pred,
                          const float* d_dir_pred, const int64_t* d_inds, int64_t n, int num_classes, float* d_boxes,
                          float* d_scores, int64_t* d_dir, float* d_bev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FSD foreground sampling (csrc/fg_sample.hip): the stage between the segmentor and the clustering.
 *
 * sst_fg_sample_f32 - replaces SingleStageFSD.sample, get_fg_mask and get_sample_beg_position
 * (mmdet3d/models/detectors/single_stage_fsd.py:698-797) for all classes and all samples of a batch: three launches and one
 * memset, no host read.  mask[c][i] = sigmoid_f32(logits[i][c]) > thresholds[c], ORed with extra_mask[c][i] (bool [C, n] or
 * NULL; logits may be NULL, then extra_mask alone decides).  batch_idx (int32, or int64 when batch_is_i64) must be
 * non-decreasing with values in [0, batch); a value outside is counted nowhere and sets bit 0 of the status word.  With
 * apply_rule, class c gets the first point of EVERY present sample whenever some sample up to the largest one present has no
 * selected point of class c (:725-727; the decision is taken on the device).
 *   Outputs: slot int32 [C, n] (the row within the class, or -1), mask bool [C, n], and in concatenated layout (class after
 *   class, class c from row class_off[c]) src int32 (the point of every row), centers [.., 3] = points[:, :3] + votes[:, 3c:3c+3]
 *   (one fp32 add), batch_out (the type of batch_idx), points_out [.., point_cols]; the last three may be NULL.  Each holds up
 *   to C * n rows; a row at or beyond max_rows is not written.  With sample_major the rows are ordered by sample and, inside a
 *   sample, class after class (inside a class in point order): slot then holds that output row, and aux int32 [C, n] (or
 *   NULL) rides along: aux_out[row] = aux[c][i], aux_inv[aux[c][i]] = row where aux is in [0, aux_rows).  info int32 [sst_fg_sample_info_words(C)] = totals[C] | rule[C] | class_off[C + 1] | status: what the host
 *   reads, once.  num_classes <= SST_FG_MAX_CLASSES, else SST_ERR_UNSUPPORTED.
 *
 * sst_fg_slot2_i32 - update_sample_results_by_mask (:571-586) for the masks: d_keep int64 [keep_offsets[C]] are the rows of
 * every class that pass the cluster filter, ascending within a class, class after class (keep_offsets: C + 1 HOST values);
 * d_slot2 int32 [C, n] = the row in the combined output or -1, d_final_mask bool [C, n] = slot2 >= 0.
 *
 * sst_fg_gather_cat_fwd_f32 - the per-class indexing of seg_logits / seg_vote_preds / seg_feats / seg_points (:738-744), the
 * second indexing by the valid mask (:584), combine_classes (:588-593) and the column concatenation (:532) as one gather
 * through idx int32 [m] into the n source rows: out [m, c_logits + c_votes + c_feats], points_out [m, c_points]; an index
 * outside [0, n) gives zeros.
 * sst_fg_roi_cat_fwd_f32 - the rows of FSD.prepare_multi_class_roi_input / prepare_roi_input
 * (mmdet3d/models/detectors/two_stage_fsd.py:108-178): d_out [rows, cluster_cols + feat_cols] = (cluster_feats[d_row[g]], zeros
 * where d_row[g] is outside [0, n_cluster) | seg_feats[d_src[g]], zeros where d_src[g] is outside [0, n_points)), d_src == NULL:
 * the identity.
 * sst_fg_gather_cat_bwd_f32 - d_feats_grad[i][f] = sum over the classes in ascending order of
 * d_out_grad[slot2[c][i]][col0 + f] (d_out_grad has `rows` rows; a slot outside them adds nothing), zeros where no class holds the point: every element written, no float atomic.
 * ---------------------------------------------------------------------------------------------- */
#define SST_FG_MAX_CLASSES 32
typedef struct sst_fg_sample_args {
  const float* logits;
  const float* votes;
  const float* points;
  const void* batch_idx;
  const uint8_t* extra_mask;
  int32_t* slot;
  uint8_t* mask;
  int32_t* src;
  float* centers;
  void* batch_out;
  float* points_out;
  int32_t* info;
  const int32_t* aux;
  int32_t* aux_out;
  int32_t* aux_inv;
  int64_t n, ld_logits, ld_votes, ld_points, max_rows, aux_rows;
  int32_t num_classes, point_cols, batch, batch_is_i64, apply_rule, sample_major;
  float thresholds[SST_FG_MAX_CLASSES];
} sst_fg_sample_args;
typedef struct sst_fg_gather_args {
  const int32_t* idx;
  const float* logits;
  const float* votes;
  const float* feats;
  const float* points;
  float* out;
  float* points_out;
  int64_t m, n, ld_logits, ld_votes, ld_feats, ld_points;
  int32_t c_logits, c_votes, c_feats, c_points;
} sst_fg_gather_args;
int64_t sst_fg_sample_workspace_bytes(int64_t n, int num_classes, int batch);
int sst_fg_sample_info_words(int num_classes);
int sst_fg_sample_f32(const sst_fg_sample_args* args, void* d_workspace, void* stream);
int sst_fg_slot2_i32(const int32_t* d_slot, int64_t n, int num_classes, const int64_t* d_keep, const int64_t* keep_offsets,
                     int32_t* d_slot2, uint8_t* d_final_mask, void* stream);
int sst_fg_gather_cat_fwd_f32(const sst_fg_gather_args* args, void* stream);
int sst_fg_roi_cat_fwd_f32(const int32_t* d_src, const int32_t* d_row, int64_t rows, int64_t n_points, int64_t n_cluster,
                           const float* d_cluster_feats, int64_t ld_cluster, int cluster_cols, const float* d_seg_feats,
                           int64_t ld_feats, int feat_cols, float* d_out, void* stream);
int sst_fg_gather_cat_bwd_f32(const float* d_out_grad, int64_t rows, int64_t ld_out, int col0, const int32_t* d_slot2, int64_t n,
                              int num_classes, int feat_cols, float* d_feats_grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FSDv2 grouped foreground sampling (csrc/fg_group_sample.hip): the stage between the segmentor and the
 * virtual voxels.
 *
 * sst_fg_group_sample_f32 - replaces SingleStageFSDV2.batched_group_sample / group_sample with get_fg_mask,
 * gather_group_by_names, get_sample_beg_position and get_offset_weight
 * (mmdet3d/models/detectors/single_stage_fsd_v2.py:656-705, 726-891) for all groups and all samples of a batch: three launches
 * and one memset, no host read.  logits [n, num_logits] (K = C + 1 columns, the background among them) go through an fp32
 * softmax (row maximum subtracted, expf, sum in ascending column order, one division per probability); the score of group g is
 * the sum of the probabilities of group_class[group_begin[g] .. group_begin[g + 1]) in that order (:879-891);
 * mask[g][i] = score > thresholds[g] (+inf: never), ORed with extra_mask[g][i] (bool [G, n] or NULL; logits may be NULL when
 * centers is NULL, then extra_mask alone decides).  batch_idx and the at-least-one-point rule are those of sst_fg_sample_f32
 * (:820-822; with batch = 1 also `fg_mask[0] = True` of :756-757).  Outputs as there, class after class read as group after
 * group: slot int32 [G, n], mask bool [G, n], src, batch_out, points_out, and
 *   centers[row] = points[i][:3] + offset_scale * sum over the group's classes k, in listed order, of votes[i][3k:3k+3] * w_k,
 *   w_k = (|logits[i][k] - m| < 1e-6f) / (number of such k), m the maximum of the group's logits (:826-839, :855-861);
 *   every product, quotient and sum is rounded on its own (no fused multiply-add).
 * info int32 [sst_fg_sample_info_words(G)] = totals[G] | rule[G] | group_off[G + 1] | status.  num_groups <=
 * SST_FG_MAX_CLASSES and num_logits <= SST_FG_MAX_LOGITS, else SST_ERR_UNSUPPORTED; a class listed twice is SST_ERR_ARG.
 *
 * sst_fg_virtual_rows_fwd_f32 - the input rows of the virtual-point projector (SingleStageFSDV2.extract_feat :164-176 with
 * clip_points :124-129) gathered once through src int32 [m] (the point of every sampled row):
 *   out [m, c_feats + 3 + c_logits + (c_points - 3)] = (feats[i] | (clip(centers[j]) - points[i][:3]) / 10 | logits[i] |
 *   points[i][3:]), clipped [m, 3] = clip(centers[j]) = min(max(., lo), hi); an index outside [0, n) gives zeros.  The division
 *   is one fp32 subtraction and one fp32 product with fl32(1 / 10), as torch divides a device tensor by a scalar.
 * sst_fg_virtual_rows_bwd_f32 - d_feats_grad[i][f] = sum over the groups in ascending order of
 * d_out_grad[offsets[g] + slot[g][i]][f] (slot int32 [G, n]: the row within the group or -1; offsets: G + 1 HOST values),
 * zeros where no group holds the point: every element written, no float atomic.
 * ---------------------------------------------------------------------------------------------- */
#define SST_FG_MAX_LOGITS 64
typedef struct sst_fg_group_sample_args {
  const float* logits;
  const float* votes;
  const float* points;
  const void* batch_idx;
  const uint8_t* extra_mask;
  int32_t* slot;
  uint8_t* mask;
  int32_t* src;
  float* centers;
  void* batch_out;
  float* points_out;
  int32_t* info;
  int64_t n, ld_logits, ld_votes, ld_points, max_rows;
  int32_t num_groups, num_logits, point_cols, batch, batch_is_i64, apply_rule;
  float offset_scale;
  float thresholds[SST_FG_MAX_CLASSES];
  uint8_t group_begin[SST_FG_MAX_CLASSES + 1];
  uint8_t group_class[SST_FG_MAX_LOGITS];
} sst_fg_group_sample_args;
typedef struct sst_fg_virtual_rows_args {
  const int32_t* src;
  const float* centers;
  const float* feats;
  const float* logits;
  const float* points;
  float* out;
  float* clipped;
  int64_t m, n, ld_feats, ld_logits, ld_points;
  int32_t c_feats, c_logits, c_points, reserved;
  float lo[3], hi[3];
} sst_fg_virtual_rows_args;
typedef struct sst_fg_group_offsets {
  int64_t off[SST_FG_MAX_CLASSES + 1];
} sst_fg_group_offsets;
int64_t sst_fg_group_sample_workspace_bytes(int64_t n, int num_groups, int batch);
int sst_fg_group_sample_f32(const sst_fg_group_sample_args* args, void* d_workspace, void* stream);
int sst_fg_virtual_rows_fwd_f32(const sst_fg_virtual_rows_args* args, void* stream);
int sst_fg_virtual_rows_bwd_f32(const float* d_out_grad, int64_t rows, int64_t ld_out, const int32_t* d_slot,
                                const sst_fg_group_offsets* offsets, int64_t n, int num_groups, int feat_cols, float* d_feats_grad,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Deformable convolution v1 (csrc/deform_conv.hip), fp32, NCHW, everything on `stream`, no float atomics: two runs agree bit
 * for bit.  The operator of mmcv's deform_conv2d (DCN of CenterHead's DCNSeparateHead, centerpoint_head.py:123-239), restated
 * from its published kernel; nothing compiled from mmcv was available to compare with.
 *   input [B, Cin, H, W], offset [B, deform_groups * 2 * kh * kw, Ho, Wo], weight [Cout, Cin / groups, kh, kw],
 *   out [B, Cout, Ho, Wo], Ho = (H + 2 pad_h - (dil_h (kh - 1) + 1)) / stride_h + 1, Wo likewise.
 *   For output pixel (ho, wo) and tap (i, j): h = ho stride_h - pad_h + i dil_h + off_h, w = wo stride_w - pad_w + j dil_w + off_w,
 *   off_h = channel 2 (i kw + j) and off_w = channel 2 (i kw + j) + 1 of the block of deformable group c / (Cin / deform_groups).
 *   The sample is 0 unless h > -1 && w > -1 && h < H && w < W, otherwise the bilinear value over the cell (floor(h), floor(w))
 *   with corners outside the image contributing 0.  Column order c kh kw + i kw + j; no bias, no modulation mask.  The
 *   derivative in an offset is that of the cell floor() selects, and 0 where the sample is 0.
 * Forward: one launch, no workspace.  Backward: d_workspace of sst_deform_conv_bwd_workspace_bytes(shape) bytes (an int64 image
 * of the input for the order-independent fixed-point sum of the input gradient, and one weight partial per block of the weight
 * gradient's grid: sst_deform_conv_wgrad_blocks(tiles) blocks, block x taking the tiles x, x + blocks, ...; a tile is
 * sst_deform_conv_tile_pixels() consecutive output pixels of one sample).  All three gradients are always written.
 * kh, kw <= 3 and Ho Wo kh kw <= 2^22 in the backward, else SST_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sst_deform_conv_shape {
  int32_t batch, in_channels, height, width, out_channels, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w,
      groups, deform_groups, reserved;
} sst_deform_conv_shape;
int sst_deform_conv_tile_pixels(void);
int sst_deform_conv_wgrad_blocks(int64_t total_tiles);
int sst_deform_conv_out_size(const sst_deform_conv_shape* shape, int32_t* out_h, int32_t* out_w);
int64_t sst_deform_conv_bwd_workspace_bytes(const sst_deform_conv_shape* shape);
int sst_deform_conv_fwd_f32(const sst_deform_conv_shape* shape, const float* d_input, const float* d_offset,
                            const float* d_weight, float* d_out, void* stream);
int sst_deform_conv_bwd_f32(const sst_deform_conv_shape* shape, const float* d_input, const float* d_offset,
                            const float* d_weight, const float* d_out_grad, float* d_input_grad, float* d_offset_grad,
                            float* d_weight_grad, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The training update (csrc/optim.hip), fp32: what the reference's runner does through mmcv's OptimizerHook /
 * Fp16OptimizerHook and torch.optim.AdamW after the backward pass.  At most three launches on `stream` for ALL tensors, no host
 * read, no device allocation, no float atomics: two runs agree bit for bit.
 *   d_tensors [n_tensors]: one entry per tensor that has a gradient this step.  p and g at any 4-byte aligned address; m and
 *     v (the optimizer's moments) likewise, 16-byte accesses are used for a chunk whose four addresses allow them and give the
 *     same bits as the 4-byte path.  group < hyper->n_groups; slot = index of the tensor's step counter in d_steps.
 *   d_chunks [n_chunks]: the tensors cut into slices of at most sst_optim_chunk_elems() elements, `start` a multiple of it,
 *     in any fixed order (the order is part of the sum's order).  A tensor of numel 0 has an entry and no chunk.
 *   hyper: by value per call.  lr, wd, b1, b2, eps per group; max_norm < 0 = no clipping; scale_mode SST_OPTIM_SCALE_*;
 *     skip_nonfinite != 0: a step whose gradients hold an inf or NaN writes no p, m, v and moves no counter.
 *   d_steps: fp32 step counters (torch's own type for `step`: exact to 2^24), advanced for the listed tensors only.
 *   d_record: sst_optim_record_bytes() bytes, 8-byte aligned, kept by the caller between calls:
 *     double total_norm @0 | float clip_coef @8 | float inv_scale @12 (the one this step used) | float scale @16 (after this
 *     step's bookkeeping; the caller initialises it, 1 without loss scaling) | int32 found_inf @20 | int32 growth_tracker @24 |
 *     int32 skipped_steps @28 (running count) | double clip_coef @32 and double inv_scale @40 as the update uses them | reserved.
 *   d_workspace: sst_optim_workspace_bytes(n_tensors) bytes.
 * Arithmetic per element, in this order, evaluated in fp64 on the fp32 operands with fp64 scalars and rounded to fp32 once
 * per result, so that p, m and v are the correctly rounded values of the float64 restatement (half an fp32 ulp):
 *     g = g * inv_scale * clip_coef;  p = p * (1 - lr wd);  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;
 *     p = p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *   total_norm = sqrt(fp64 sum of (g * inv_scale)^2), clip_coef = min(1, max_norm / (total_norm + 1e-6)); the scale follows
 *   torch.amp.GradScaler.update.
 * sst_optim_step_f32 replaces GradScaler.unscale_ + clip_grad_norm_ + AdamW.step + GradScaler.update.
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer, a negative count, n_groups outside
 * 1..SST_OPTIM_MAX_GROUPS or an unknown scale_mode; SST_ERR_UNSUPPORTED for n_tensors above 2^31 - 1.
 * ---------------------------------------------------------------------------------------------- */
#define SST_OPTIM_MAX_GROUPS 8
#define SST_OPTIM_SCALE_NONE 0     /* no loss scale: inv_scale = 1, the record's scale is neither read nor written */
#define SST_OPTIM_SCALE_FIXED 1    /* the record's scale is used and never changed (Fp16OptimizerHook)    */
#define SST_OPTIM_SCALE_DYNAMIC 2  /* GradScaler: backoff on a not-finite step, growth after an interval  */
typedef struct sst_optim_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t numel;
  int32_t group, slot;
} sst_optim_tensor;
typedef struct sst_optim_chunk {
  int64_t start;
  int32_t tensor, count;
} sst_optim_chunk;
typedef struct sst_optim_hyper {
  double lr[SST_OPTIM_MAX_GROUPS], wd[SST_OPTIM_MAX_GROUPS], b1[SST_OPTIM_MAX_GROUPS], b2[SST_OPTIM_MAX_GROUPS],
      eps[SST_OPTIM_MAX_GROUPS];
  double max_norm, growth_factor, backoff_factor;
  int32_t growth_interval, scale_mode, skip_nonfinite, n_groups;
} sst_optim_hyper;
/* elements per chunk (replaces nothing: the layout constant of d_chunks) */
int sst_optim_chunk_elems(void);
/* SST_OPTIM_MAX_GROUPS as the library was built (replaces nothing) */
int sst_optim_max_groups(void);
/* bytes of the device record (replaces GradScaler's _scale / _growth_tracker / found_inf tensors) */
int sst_optim_record_bytes(void);
/* bytes of the per-call workspace (replaces the per-step temporaries of clip_grad_norm_ and the foreach AdamW) */
int64_t sst_optim_workspace_bytes(int64_t n_tensors);
/* the update (replaces GradScaler.unscale_ + clip_grad_norm_ + AdamW.step + GradScaler.update) */
int sst_optim_step_f32(const sst_optim_tensor* d_tensors, int64_t n_tensors, const sst_optim_chunk* d_chunks, int64_t n_chunks,
                       const sst_optim_hyper* hyper, float* d_steps, void* d_record, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The CTRL tracklet family (csrc/tracklet.hip): TrackletRoIHead's training targets and the input rows of its box head.
 * fp32 data, int64 timestamps and offsets, no float atomics, no host read-back, bit-reproducible.
 *
 * sst_tracklet_targets_f32 - one launch for the whole batch, one workgroup (sst_tracklet_targets_block() threads) per tracklet.
 *   Replaces tracklet_roi_head.py:333-347 (_select_one2one_candidates: one aligned_iou_3d launch, one .sum() and one host
 *   tensor per candidate, torch.argmax(...).item()), :287-331 (_assign_and_sample per tracklet), tracklet_assigner.py:14-55
 *   (TrackletAssigner.assign: Python timestamp walks, overlaps[i].item() per box), lidar_tracklet.py:278-299 (self_ious /
 *   intersection_ious), mmdet's PseudoSampler and fsd_bbox_head.py:343-543 (get_targets / _get_target_single /
 *   get_multi_class_soft_label per tracklet).  Every output size follows from the tracklet lengths the host knows.
 *   Inputs: boxes [n_rows, 7] tracklet-major in frame order, ts int64 [n_rows] ascending within a tracklet, scores [n_rows],
 *   trk_offsets int64 [n_tracklets + 1] (rows), cand_boxes [n_cand_rows, 7], cand_ts int64 [n_cand_rows] ascending within a
 *   candidate, cand_offsets int64 [n_cands + 1] (candidate rows), trk_cand_offsets int64 [n_tracklets + 1] (candidates of a
 *   tracklet), trk_class int64 [n_tracklets] in [0, num_classes).  Offsets are clamped to their arrays.
 *   Candidate choice: per candidate the number of shared timestamps whose aligned 3-D IoU is > candidate_thresh (strict); the
 *   chosen one is the FIRST with the maximal count - what torch.argmax returns on the reference's int64 host tensor (checked
 *   on the CPU: torch.argmax(torch.tensor([2, 5, 5, 1])) == 1, and tests/test_tracklet_host.py pins it); chosen[t] = its index
 *   into the candidates, -1 for a tracklet without candidates (the reference's empty ground-truth tracklet).
 *   Per row in frame order: matched int32 (index of the chosen candidate's box with the same timestamp within that candidate,
 *   -1 if none = get_index_from_ts), overlaps (the IoU with it, 0 if none = self_ious), assigned_gt_inds int64 (matched + 1;
 *   with object_centric only where IoU > iou_thr, else 0).  The IoU is the device function sst_boxes_overlap_aligned_f32 uses
 *   (bev_clip.h) x the height overlap over the union volume: bit-equal to aligned_iou_3d built on that entry point.
 *   Per row in PseudoSampler's order (positives in frame order, then negatives in frame order; ranks by wave ballots and a scan
 *   over the waves, no atomics), rows of tracklet t at trk_offsets[t] ..: the layout of sst_roi_sample_targets_f32 without
 *   padding - rois [n_rows, 8] = (t, box), src int32 (input row), gt_index int32 (row of cand_boxes, -1 off the positives),
 *   labels int64 (the tracklet's class, -1 off the positives), iou_out, soft_label (cls_pos_thr / cls_neg_thr of the class; 0
 *   on negatives), reg_mask uint8, targets [n_rows, 7] (_get_target_single; 0 off the positives) - and frame_inds int64
 *   (bboxes_frame_inds), scores_out, pos_gt_bboxes [n_rows, 7] (the matched box, 0 off the positives); counts int32
 *   [n_tracklets, 2] = (positives, negatives).  Every element is written.
 *
 * sst_tracklet_rows_fwd_f32 / _bwd_f32 - tracklet_roi_head.py:247-258, the gathers and cats in front of the box head:
 *   out[i] = (feats[p_i, 0 : feat_cols] | is_cur_frame_i if combined | roi_scores[r_i] if with_roi_scores), xyz_out[i] =
 *   xyz[p_i, 0 : xyz_cols] (optional), p = pts_inds int64 [m], r = roi_inds int64 [m], is_cur_frame = pts_frame_inds[p] ==
 *   roi_frame_inds[r].  A negative index counts from the end as Python's does (-1, the pool's fake row, reads the last row);
 *   an index outside the array reads zeros.  feat_cols need not be a multiple of 4: the 16-byte-aligned part of a source row is
 *   read as float4; the rows of a workgroup are staged in LDS and leave as one contiguous span, consecutive lanes on consecutive
 *   floats.  Backward (replaces autograd's index_put): d_feats[p] = the sum of d_out[row, 0 : feat_cols] over the output rows of
 *   p in ascending row order.  sst_tracklet_rows_keys_i64 writes key[i] = p_i * m + i (INT64_MAX for a row that names no point);
 *   the caller sorts the keys (any sort: they are distinct); sst_tracklet_rows_bwd_f32 zeroes d_feats [n_points, feat_cols] (one
 *   memset) and walks every run of the sorted keys once.  No float atomic; two runs are bit-equal.
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer or a negative size, SST_ERR_UNSUPPORTED for num_classes
 * outside 1..SST_ROI_MAX_CLASSES or sizes above 2^31 - 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sst_tracklet_targets_args {
  const float* boxes;
  const int64_t* ts;
  const float* scores;
  const int64_t* trk_offsets;
  const float* cand_boxes;
  const int64_t* cand_ts;
  const int64_t* cand_offsets;
  const int64_t* trk_cand_offsets;
  const int64_t* trk_class;
  int32_t* chosen;
  int32_t* counts;
  int32_t* matched;
  float* overlaps;
  int64_t* assigned_gt_inds;
  float* rois;
  int32_t* src;
  int64_t* frame_inds;
  int32_t* gt_index;
  int64_t* labels;
  float* iou_out;
  float* scores_out;
  float* soft_label;
  uint8_t* reg_mask;
  float* targets;
  float* pos_gt_bboxes;
  int64_t n_rows, n_cand_rows, n_cands, n_tracklets;
  int32_t num_classes, object_centric;
  float candidate_thresh, iou_thr;
  double cls_pos_thr[SST_ROI_MAX_CLASSES], cls_neg_thr[SST_ROI_MAX_CLASSES];
} sst_tracklet_targets_args;
typedef struct sst_tracklet_rows_args {
  const float* feats;
  const float* xyz;
  const int64_t* pts_frame_inds;
  const int64_t* pts_inds;
  const int64_t* roi_inds;
  const int64_t* roi_frame_inds;
  const float* roi_scores;
  float* out;
  float* xyz_out;
  int64_t m, n_points, n_rois, ld_feats, ld_xyz;
  int32_t feat_cols, xyz_cols, combined, with_roi_scores;
} sst_tracklet_rows_args;
/* threads of a workgroup of the targets kernel (replaces nothing: the launch constant the tests size their cases by) */
int sst_tracklet_targets_block(void);
int sst_tracklet_targets_f32(const sst_tracklet_targets_args* args, void* stream);
int sst_tracklet_rows_fwd_f32(const sst_tracklet_rows_args* args, void* stream);
int sst_tracklet_rows_keys_i64(const int64_t* d_pts_inds, int64_t m, int64_t n_points, int64_t* d_keys, void* stream);
int sst_tracklet_rows_bwd_f32(const float* d_out_grad, int64_t m, int64_t ld_out, int feat_cols, const int64_t* d_sorted_keys,
                              int64_t n_points, float* d_feats_grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The FSD++ incremental point stage (csrc/incremental.hip): the input stage of TwoStageFSDPP for a whole batch - seed-box
 * crops of the previous frames, capped per box, and the points of the current frame (and of frame -1) that fall into voxels
 * no base frame occupies.  fp32 points, int64 frame indices, integer atomics only, bit-reproducible.
 *
 * Voxel coordinates everywhere below: incremental_ops.py:14-18 (voxelize_single), torch.div(p - lo, vs, rounding_mode =
 * 'floor').int() in fp32 - torch's fmod-based floor division (c10::div_floor_floating), NOT floorf((p - lo) / vs): a = p - lo;
 * mod = fmodf(a, vs); div = (a - mod) / vs; div -= 1 where mod != 0 and its sign differs from vs's; floor(div), + 1 where
 * div - floor(div) > 0.5; a signed zero where div == 0.  Every operation is rounded on its own.
 *
 * sst_incr_voxel_coors_f32 - incremental_ops.py:14-18: d_points [n, >= 3] rows ld floats apart -> d_coors int32 [n, 3].
 *
 * sst_incr_mask_i32 - the TorchEx op incremental_points_mask(coors1, coors2, spatial_size) (call sites incremental_ops.py:62,
 *   :121), with the set semantics of incremental_ops.py:20-34, :83-97 (find_delta_unq_coors + find_delta_pc_mask): mask[j] = 1
 *   iff no row of coors1 equals row j of coors2.  An occupancy bitmap of spatial[0] * spatial[1] * spatial[2] bits (32-bit
 *   atomicOr, skipped where the bit is already set); rows of coors1 outside the grid go to an overflow list (capacity n1) that
 *   out-of-grid rows of coors2 are compared with exactly, so the answer is exact for every int32 triple.  One memset, two
 *   launches.  Workspace: sst_incr_mask_workspace_bytes(n1, spatial) (< 0: the grid is refused).
 *
 * sst_incr_delta_mask_f32 - incremental_ops.py:45-63 (find_delta_points_by_voxelization) and :99-123
 *   (find_delta_points_by_voxelization_list_v3) without the concatenation and the compactions: up to SST_INCR_MAX_CLOUDS base
 *   clouds by value, one query cloud; mask[j] = 1 iff point j of the query falls into a voxel no base point falls into.
 *   lower_bound != 0: v3's filter - points of either side that are not strictly above lo on every axis neither occupy nor
 *   are new.  Workspace: sst_incr_mask_workspace_bytes(total base points, grid).
 *
 * sst_incr_plan_f32 + sst_incr_rows_f32 - two_stage_fsdpp.py:460-503 (generate_points), :592-635 (get_old_points), :637-678
 *   (crop_and_process_points), :738-745 (get_delta_points) for every sample and frame of a batch.
 *   Inputs: per sample s points[s] [n_points[s], cols] contiguous and frame_inds[s] int64 (0 = current, -k = k frames back);
 *   boxes [n_boxes, 7] (already enlarged), box_offsets int32 [n_samples * n_frames + 1]: the boxes of (sample s, frame -(i + 1))
 *   are rows box_offsets[s * n_frames + i] ..; keys uint32, one per point of the batch in sample order (NULL: the key is the
 *   point's index); queries q < n_queries: the points with frame index q_inc[q] are tested against the points with frame
 *   index in [q_lo[q], q_hi[q]] of the SAME sample (one bitmap per (sample, query)); a (sample, query) without a single base
 *   point yields no delta row (get_delta_points, :740-743: an empty base cloud gives an empty result).
 *   plan: one memset; mark (bits, overflow lists, the first box of its own (sample, frame) that holds a point - the inside test
 *   of csrc/pib_test.h with the boxes staged in LDS, bit-equal to sst_points_in_boxes_f32 - and integer counts per box); with
 *   max_crop_points > 0 a scan of the box counts, ONE sst_sort_pairs_u64 of (box << 32 | key) (stable: ties by point index) and
 *   a rank launch (kept: rank in its box < max_crop_points = randperm + get_inner_win_inds < max_n for the permutation
 *   argsort(keys)); flags and per-workgroup counts; a scan per (sample, segment).  It leaves counts int32
 *   [n_samples, n_frames + n_queries] on the device: crop rows per frame, delta rows per query.
 *   rows (after the caller has read counts and laid out the segments): out [M, cols + 1]; the rows of (sample s, segment b)
 *   start at row seg_base[s * (n_frames + n_queries) + b], in ascending point index; the appended column is
 *   float(-i - 1) / 10 for crop segment i (:626) and q_tag[q] for delta segment q (:483, :491).  Rows are staged in LDS and
 *   leave as contiguous spans.  Workspace (the same buffer for both calls): sst_incr_workspace_bytes.
 *
 * sst_points_frame_transform_f32 - incremental_ops.py:175-186 (points_frame_transform) for up to SST_INCR_MAX_CLOUDS clouds
 *   in one launch: dst[i] = (((x * m0 + y * m1) + z * m2) + m3 per row of the cloud's 3 x 4 matrix | the other columns), every
 *   product and sum rounded on its own.  The matrix inv(cur_pose) @ pre_pose is formed by the caller.
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer, a negative size or a non-positive voxel size,
 * SST_ERR_UNSUPPORTED for counts above the SST_INCR_* limits, cols outside 3..SST_INCR_MAX_COLS, a grid of more than 2^33
 * cells or sizes above 2^31 - 1.
 * ---------------------------------------------------------------------------------------------- */
#define SST_INCR_MAX_SAMPLES 16
#define SST_INCR_MAX_FRAMES 16
#define SST_INCR_MAX_QUERIES 4
#define SST_INCR_MAX_CLOUDS 8
#define SST_INCR_MAX_COLS 15
typedef struct sst_incr_args {
  const float* points[SST_INCR_MAX_SAMPLES];
  const int64_t* frame_inds[SST_INCR_MAX_SAMPLES];
  int64_t n_points[SST_INCR_MAX_SAMPLES];
  const float* boxes;
  const int32_t* box_offsets;
  const uint32_t* keys;
  int32_t* counts;
  float* out;
  void* workspace;
  int64_t workspace_bytes;
  int64_t seg_base[SST_INCR_MAX_SAMPLES * (SST_INCR_MAX_FRAMES + SST_INCR_MAX_QUERIES)];
  int32_t n_samples, cols, n_frames, n_queries, n_boxes, max_crop_points, lower_bound;
  int32_t q_inc[SST_INCR_MAX_QUERIES], q_lo[SST_INCR_MAX_QUERIES], q_hi[SST_INCR_MAX_QUERIES];
  float q_tag[SST_INCR_MAX_QUERIES];
  float lo[3], vs[3];
  int32_t grid[3];
} sst_incr_args;
typedef struct sst_incr_delta_args {
  const float* base[SST_INCR_MAX_CLOUDS];
  int64_t n_base[SST_INCR_MAX_CLOUDS], ld_base[SST_INCR_MAX_CLOUDS];
  const float* query;
  int64_t n_query, ld_query;
  uint8_t* mask;
  void* workspace;
  int64_t workspace_bytes;
  int32_t n_clouds, lower_bound;
  float lo[3], vs[3];
  int32_t grid[3];
} sst_incr_delta_args;
typedef struct sst_frame_transform_args {
  const float* src[SST_INCR_MAX_CLOUDS];
  float* dst[SST_INCR_MAX_CLOUDS];
  int64_t n[SST_INCR_MAX_CLOUDS];
  float mat[SST_INCR_MAX_CLOUDS][12];
  int32_t n_clouds, cols;
} sst_frame_transform_args;
int sst_incr_voxel_coors_f32(const float* d_points, int64_t n, int64_t ld, const float* lo3, const float* vs3, int32_t* d_coors,
                             void* stream);
int64_t sst_incr_mask_workspace_bytes(int64_t n_base, const int32_t* spatial3);
int sst_incr_mask_i32(const int32_t* d_coors1, int64_t n1, const int32_t* d_coors2, int64_t n2, const int32_t* spatial3,
                      void* d_workspace, int64_t workspace_bytes, uint8_t* d_mask, void* stream);
int sst_incr_delta_mask_f32(const sst_incr_delta_args* args, void* stream);
int64_t sst_incr_workspace_bytes(const sst_incr_args* args);
int sst_incr_plan_f32(const sst_incr_args* args, void* stream);
int sst_incr_rows_f32(const sst_incr_args* args, void* stream);
int sst_points_frame_transform_f32(const sst_frame_transform_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training augmentation of points and boxes (csrc/augment.hip): what a shipped train_pipeline does after
 * db_sampler.sample_all - ObjectSample's point removal (mmdet3d/datasets/pipelines/transforms_3d.py:262-279, :332-334),
 * RandomFlip3D (:95-172), GlobalRotScaleTrans (:564-676), PointsRangeFilter, ObjectRangeFilter and PointShuffle - for a packed
 * batch.  fp32, every operation rounded on its own (no contraction), integer atomics only, bit-reproducible.
 *
 * sst_augment_params - one record per sample: flags flip_h, flip_v, rotate, shuffle; cos, sin of the fp32 angle, scale, the
 *   angle itself (boxes: yaw += angle); trans[3]; range[6] = (x0, y0, z0, x1, y1, z1); the 64-bit shuffle seed.
 *
 * sst_augment_points_f32 - points [n_total, cols] (3 <= cols <= SST_AUG_MAX_COLS, 16-byte aligned), sample after sample, inside
 *   a sample the n_pasted[s] pasted rows first (points.cat([sampled_points, points]), :334); row_offsets int64 [batch + 1];
 *   block_offsets int32 [batch + 1]: the prefix sums of ceil(rows of the sample / 256) (n_blocks = the last one);
 *   planes [n_planes, 6, 4] = (a, b, c, d) of the pasted boxes' faces with the normals pointing inwards (surface_equ_3d,
 *   mmdet3d/core/bbox/box_np_ops.py:693-714), plane_offsets int32 [batch + 1].  Per row, in this order:
 *     1. removal (rows at or after n_pasted[s] only): sgn = ((x * a + y * b) + z * c) + d for the six faces of every pasted
 *        box of the sample; inside iff all six are < 0 (sgn >= 0 is outside, box_np_ops.py:745-751); a row inside any box is
 *        dropped.  The planes are staged in LDS, sst_augment_plane_chunk() boxes at a time.
 *     2. flip_h: y = -y; flip_v: x = -x (lidar_box3d.py:195-227).
 *     3. rotate: x' = x * cos + y * sin, y' = x * (-sin) + y * cos (lidar_box3d.py:166-190, base_points.py:155-177).
 *     4. x, y, z *= scale.   5. x, y, z += trans.
 *     6. kept iff x > r0 && y > r1 && z > r2 && x < r3 && y < r4 && z < r5 (base_points.py:223-228): a NaN is dropped.
 *     7. the other columns are copied; a column k >= 3 named in norm_mask leaves as (v - norm_mean[k]) / norm_std[k], each
 *        operation in fp32 (NormalizePoints, mmdet3d/datasets/pipelines/loading.py:1026-1050).
 *   out [n_total, cols]: the survivors packed, sample after sample; counts int32 [batch] (zeroed by the call).  Inside a
 *   sample: without `shuffle` the input order; with it the order of the STABLE sort by the 32-bit key
 *     x = seed + 0x9E3779B97F4A7C15 * (((sample << 32) | row) + 1);  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;
 *     x *= 0x94D049BB133111EB;  x ^= x >> 31;  key = x >> 32       (splitmix64; row = the index inside the sample, 64-bit
 *   wrap-around arithmetic).  One memset, a classify launch, one sst_sort_pairs_u64 of (dropped | sample | key), a gather
 *   launch.  Workspace: sst_augment_workspace_bytes(n_total, batch), 16-byte aligned.
 *
 * sst_augment_boxes_f32 - boxes [n_boxes, cols] (cols 7 or 9), box_offsets int32 [batch + 1], labels int64 or NULL.  In order:
 *   flips (flip_h: columns 1 and 8 negated, yaw = -yaw + (float)pi; flip_v: columns 0 and 7, yaw = -yaw; lidar_box3d.py:210-216),
 *   rotation (centre and columns 7:9 as points, yaw += angle; applied where the record's `rotate` is set or always_rotate),
 *   scale (columns 0:6 and 7:, base_box3d.py:222-231), translation (0:3); with `filter`: in_range_bev strict on the centre
 *   (lidar_box3d.py:244-247), the kept rows compacted in their order to boxes_out / labels_out rows box_offsets[s] .., counts
 *   int32 [batch], and yaw = yaw - floor(yaw / (float)(2 pi) + 0.5f) * (float)(2 pi) (limit_yaw, base_box3d.py:233-245).
 *   Without `filter` (the seed boxes of the FSD++ loaders) every row is written and the yaw is not limited.  One launch.
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer, a negative size, a misaligned buffer or a workspace
 * that is too small; SST_ERR_UNSUPPORTED for cols outside the limits or n_total above 2^31 - 257.
 * ---------------------------------------------------------------------------------------------- */
#define SST_AUG_MAX_COLS 8
typedef struct sst_augment_params {
  int32_t flip_h, flip_v, rotate, shuffle;
  float cos, sin, scale, angle;
  float trans[3];
  float reserved;
  float range[6];
  uint64_t seed;
} sst_augment_params;
typedef struct sst_augment_args {
  const float* points;
  const int64_t* row_offsets;
  const int32_t* n_pasted;
  const int32_t* block_offsets;
  const sst_augment_params* params;
  const float* planes;
  const int32_t* plane_offsets;
  float* out;
  int32_t* counts;
  void* workspace;
  int64_t workspace_bytes;
  int64_t n_total;
  int32_t batch, cols, n_blocks, n_planes;
  int32_t norm_mask, reserved;           /* bit k (k >= 3): column k leaves as (v - norm_mean[k]) / norm_std[k] */
  float norm_mean[SST_AUG_MAX_COLS], norm_std[SST_AUG_MAX_COLS];
} sst_augment_args;
typedef struct sst_augment_box_args {
  const float* boxes;
  const int64_t* labels;
  const int32_t* box_offsets;
  const sst_augment_params* params;
  float* boxes_out;
  int64_t* labels_out;
  int32_t* counts;
  int32_t batch, cols, n_boxes, filter, always_rotate, reserved;
} sst_augment_box_args;
int sst_augment_plane_chunk(void);
int64_t sst_augment_workspace_bytes(int64_t n_total, int batch);
int sst_augment_points_f32(const sst_augment_args* args, void* stream);
int sst_augment_boxes_f32(const sst_augment_box_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The points of a CTRL tracklet pipeline (csrc/tracklet_augment.hip): TrackletPoseTransform
 * (mmdet3d/datasets/pipelines/tracklet_pipelines.py:149-208), PointDecoration (:455-506), TrackletRandomFlip (:414-439),
 * TrackletGlobalRotScaleTrans (:329-355), PointsRangeFilter and PointShuffle for a packed batch of tracklets.  fp32, every
 * operation rounded on its own (no contraction), integer atomics only, bit-reproducible.
 *
 * sst_tracklet_augment_points_f32 - points [n_total, cols] (3 <= cols <= SST_AUG_MAX_COLS, 16-byte aligned), sample after
 *   sample and inside a sample frame after frame; frame_rows int32 [n_frames + 1]: the first row of every frame of the batch
 *   (an empty frame repeats its successor's); sample_frames int32 [batch + 1]: the first frame of every sample (at most
 *   SST_TRK_AUG_MAX_FRAMES frames per sample, max_frames = the largest count); block_offsets int32 [batch + 1]: the prefix sums
 *   of ceil(rows of the sample / 256) (n_blocks = the last one); frames [n_frames, 12 + deco]: rows 0..2 of the frame's 4 x 4
 *   matrix m (row-major, 12 values), then the deco (0 <= deco <= SST_TRK_AUG_MAX_DECO) values appended to every row of the
 *   frame; frame_values int32 [n_frames]: what out_frame_inds holds for a row of the frame; params: one sst_augment_params per
 *   sample.  Per row, in this order:
 *     1. its frame: the first frame f of the sample with frame_rows[f + 1] > row (a binary search over the sample's frame
 *        offsets, staged in LDS).
 *     2. x' = ((m00 * x + m01 * y) + m02 * z) + m03, y' and z' likewise from rows 1 and 2 of m.
 *     3. steps 2 to 6 of sst_augment_points_f32 with the sample's record (flips, rotation, scale, translation, the strict range
 *        test): the same device function.
 *     4. the other columns are copied; the frame's deco values are appended.
 *   out [n_total, cols + deco] and out_frame_inds int32 [n_total]: the survivors packed, sample after sample; counts int32
 *   [batch] (zeroed by the call).  Inside a sample: without `shuffle` the input order, with it the order of the stable sort by
 *   the key of sst_augment_points_f32 (row = the index inside the sample).  One memset, a classify launch, one
 *   sst_sort_pairs_u64, a gather launch.  Workspace: sst_tracklet_augment_workspace_bytes(n_total, batch), 16-byte aligned.
 *   The boxes of the tracklets and their candidates go through sst_augment_boxes_f32 with filter = 0 and always_rotate = 1.
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer, a negative size, a misaligned buffer or a workspace
 * that is too small; SST_ERR_UNSUPPORTED for cols, deco or max_frames outside the limits or n_total above 2^31 - 257.
 * ---------------------------------------------------------------------------------------------- */
#define SST_TRK_AUG_MAX_DECO 8
#define SST_TRK_AUG_MAX_FRAMES 2048
typedef struct sst_tracklet_augment_args {
  const float* points;
  const int32_t* frame_rows;
  const int32_t* sample_frames;
  const int32_t* block_offsets;
  const float* frames;
  const int32_t* frame_values;
  const sst_augment_params* params;
  float* out;
  int32_t* out_frame_inds;
  int32_t* counts;
  void* workspace;
  int64_t workspace_bytes;
  int64_t n_total;
  int32_t batch, cols, deco, n_blocks, n_frames, max_frames;
} sst_tracklet_augment_args;
int64_t sst_tracklet_augment_workspace_bytes(int64_t n_total, int batch);
int sst_tracklet_augment_points_f32(const sst_tracklet_augment_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Test-time augmentation of the CTRL tracklet family (csrc/tracklet_tta.hip).  fp32 with every operation
 * rounded on its own (no contraction), the merge in fp64; integer atomics only, bit-reproducible.
 *
 * sst_tracklet_tta_views_f32 - the n_views views of a packed batch of tracklets in one pass.  Replaces, per view, the deep copy
 *   and the transforms of MultiScaleFlipAug3D (mmdet3d/datasets/pipelines/test_time_aug.py:88-109): TrackletGlobalRotScaleTrans
 *   (tracklet_pipelines.py:329-355), TrackletRandomFlip (:414-439), PointsRangeFilter and PointShuffle, behind
 *   TrackletPoseTransform (:149-208) and PointDecoration (:455-506).  The inputs are those of sst_tracklet_augment_points_f32;
 *   params holds one sst_augment_params per (view, sample), view-major [n_views * batch].  Per INPUT row, once: its frame (the
 *   binary search over the LDS-staged offsets), x' = ((m00 x + m01 y) + m02 z) + m03 (y', z' likewise), the copied columns and
 *   the frame's deco values.  Then per view, in the reference's order: rotation (x' = x cos + y sin, y' = x (-sin) + y cos,
 *   where `rotate` is set), x, y, z *= scale, += trans, flip_h (y = -y), flip_v (x = -x), the strict range test of
 *   sst_augment_points_f32.  (sst_augment_points_f32 flips FIRST: its order is not this one.)
 *   out [n_views * n_total, cols + deco], out_frame_inds int32 [n_views * n_total]: the survivors packed view after view and,
 *   inside a view, sample after sample; counts int32 [n_views * batch] (zeroed by the call).  Inside a (view, sample): without
 *   `shuffle` the input order, with it the stable sort by the key of sst_augment_points_f32 with seed + v * 0xD6E8FEB86659FD93
 *   in place of the seed (view 0 keeps the sample's seed).  One memset, a classify launch, ONE sst_sort_pairs_u64 of
 *   (dropped | view | sample | key), a gather launch.  Workspace: sst_tracklet_tta_views_workspace_bytes(n_total, batch, n_views,
 *   cols + deco), 16-byte aligned (0 for sizes the call refuses).
 * sst_tracklet_tta_boxes_f32 - boxes [n_boxes, cols] (cols 7 or 9), box_offsets int32 [batch + 1] -> boxes_out
 *   [n_views, n_boxes, cols] in the same order: rotation (centre and columns 7:9, yaw += angle), scale (0:6, 7:), translation
 *   (0:3), flip_h (columns 1 and 8 negated, yaw = -yaw + (float)pi), flip_v (columns 0 and 7, yaw = -yaw).  One launch.
 *   sst_augment_boxes_f32 is untouched.
 * sst_tracklet_tta_finish - what TrackletRoIHead.inverse_aug (mmdet3d/models/roi_heads/tracklet_roi_head.py:168-179),
 *   LiDARTracklet.update_from_prediction (mmdet3d/core/bbox/structures/lidar_tracklet.py:403-445) and LiDARTracklet.merge_augs
 *   (:548-602) do, for every tracklet row of the batch in one launch.  boxes [n_views, n_rows, 7], scores [n_views, n_rows],
 *   valid uint8 [n_views, n_rows]: the decoded boxes of every view; old_boxes [n_rows, 7] (un-augmented, in the shared pose),
 *   old_scores double [n_rows]; mats [n_rows, 12]: rows 0..2 of inv(pose_i) @ shared_pose; views[k]: flip_h, flip_v, rotate,
 *   the fp32 angle, its cos and sin.  Per view, fp32: flip_h undone (y = -y, yaw = -yaw + (float)pi), flip_v undone (x = -x,
 *   yaw = -yaw), rotate(-angle) (x' = x cos + y (-sin), y' = x sin + y cos, yaw += -angle), then the centre by the matrix as
 *   above and yaw' = atan2(m00 sin yaw + m01 cos yaw, m10 sin yaw + m11 cos yaw); where valid is 0: the old box through the
 *   matrix and the old score.  Merge in fp64 over k = 0 .. n_views - 1 in this order: MAX - the first view with the largest
 *   score; WEIGHTED - box[:6] = sum(box_k[:6] * s_k) / sum(s_k), yaw = the median of the fp32 yaws (even n_views: (lower +
 *   upper) / 2 in fp32), score = sum(s_k) / n_views; IOU_CLAMPED - WEIGHTED with s_k *= (aligned 3-D IoU of view 0's box and
 *   view k's > iou_merge_thresh ? 1 : 0), the IoU of sst_tracklet_targets_f32, view 0's forced to 1.  0 / 0 follows IEEE.
 *   merged_boxes double [n_rows, 7], merged_scores double [n_rows]; view_boxes [n_views, n_rows, 7] and view_scores double
 *   [n_views, n_rows] (the effective scores): both or neither; without them a workspace of
 *   sst_tracklet_tta_finish_workspace_bytes(n_rows, n_views) bytes, 16-byte aligned, holds them.
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer, a negative size, n_views < 1, a misaligned buffer or a
 *   workspace that is too small; SST_ERR_UNSUPPORTED for n_views above SST_TRK_TTA_MAX_VIEWS, cols / deco / max_frames outside
 *   the limits, an unknown merge mode, or more than 2^31 - 257 (view, row) pairs.
 * ---------------------------------------------------------------------------------------------- */
#define SST_TRK_TTA_MAX_VIEWS 32
#define SST_TRK_TTA_MERGE_MAX 0
#define SST_TRK_TTA_MERGE_WEIGHTED 1
#define SST_TRK_TTA_MERGE_IOU_CLAMPED 2
typedef struct sst_tracklet_tta_views_args {
  const float* points;
  const int32_t* frame_rows;
  const int32_t* sample_frames;
  const int32_t* block_offsets;
  const float* frames;
  const int32_t* frame_values;
  const sst_augment_params* params;       /* [n_views * batch], view-major */
  float* out;
  int32_t* out_frame_inds;
  int32_t* counts;                        /* [n_views * batch] */
  void* workspace;
  int64_t workspace_bytes;
  int64_t n_total;
  int32_t batch, cols, deco, n_blocks, n_frames, max_frames, n_views, reserved;
} sst_tracklet_tta_views_args;
typedef struct sst_tracklet_tta_box_args {
  const float* boxes;
  const int32_t* box_offsets;
  const sst_augment_params* params;       /* [n_views * batch], view-major */
  float* boxes_out;
  int32_t batch, cols, n_boxes, n_views;
} sst_tracklet_tta_box_args;
typedef struct sst_tracklet_tta_view {
  int32_t flip_h, flip_v, rotate;
  float angle, cos, sin;
  float reserved[2];
} sst_tracklet_tta_view;
typedef struct sst_tracklet_tta_finish_args {
  const float* boxes;
  const float* scores;
  const uint8_t* valid;
  const float* old_boxes;
  const double* old_scores;
  const float* mats;
  double* merged_boxes;
  double* merged_scores;
  float* view_boxes;
  double* view_scores;
  void* workspace;
  int64_t workspace_bytes;
  int64_t n_rows;
  int32_t n_views, mode;
  float iou_merge_thresh;
  int32_t reserved;
  sst_tracklet_tta_view views[SST_TRK_TTA_MAX_VIEWS];
} sst_tracklet_tta_finish_args;
int64_t sst_tracklet_tta_views_workspace_bytes(int64_t n_total, int batch, int n_views, int width);
int sst_tracklet_tta_views_f32(const sst_tracklet_tta_views_args* args, void* stream);
int sst_tracklet_tta_boxes_f32(const sst_tracklet_tta_box_args* args, void* stream);
int64_t sst_tracklet_tta_finish_workspace_bytes(int64_t n_rows, int n_views);
int sst_tracklet_tta_finish(const sst_tracklet_tta_finish_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Class-batched cluster assignment (csrc/cluster_classes.hip): ClusterAssigner.forward's per-class loop
 * (mmdet3d/models/detectors/single_stage_fsd.py:922-999: per class a cluster-voxel grouping of the voted centres, the
 * occupancy filter with its "nothing survives, so keep every point" rule, the centroids, their connected components and the
 * point -> component map) for ALL classes of a step in one pass over their concatenated votes, with nothing read back in
 * between.  The rows of class c are rows class_off[c] .. class_off[c + 1] - 1 of the concatenation.
 *
 *   sst_cluster_classes_keys_f32: one launch.  d_rows [n, 5] int32 = (class, sample, cell x, y, z) of every vote, the cell
 *     being torch.div(p - origin, cell[class], rounding_mode='floor').int() bit for bit.  The caller groups these rows with
 *     sst_unique_rows over the FIXED key layout of sst_cluster_classes_key_layout (nothing is read back to size the keys) and
 *     takes the segmented mean of the votes over that grouping.  A sample index outside [0, SST_CCL_MAX_SAMPLES) or a cell
 *     outside the layout is clamped into it and recorded in d_status (int32 [1], OR-ed: SST_CCL_STATUS_*; the caller zeroes it
 *     and hands it on to sst_cluster_classes_f32): the result of such a call is not the reference's and must be refused.
 *   sst_cluster_classes_f32: from that grouping (d_perm, d_offsets, d_inverse, d_num_groups = its device count; the group
 *     means d_centroids [n, 3], rows >= *d_num_groups unread) to
 *       d_inds [n, 3] int32   (class, sample, component) of the surviving votes, class after class, inside a class in vote
 *                             order; the components are numbered from 0 inside every class by their smallest centroid
 *       d_keep [n] int64      index of every surviving vote INSIDE its class, same order
 *       d_mask [n] uint8      1 where the vote survives (concatenation order)
 *       d_sizes [2 * n_classes + 4] int32: surviving votes per class, surviving cluster voxels per class, then the status
 *                             word, the surviving voxels of all classes, and the 256 x 256 tile pairs of the edge test that
 *                             were staged and that left early (counted only with count_tiles != 0).
 *     The edge test is sst_connected_components_xy_f32's (same partition && sqrt(dx*dx + dy*dy) < dist[class], every operation
 *     rounded on its own); the partition of a centroid is (class, sample) with per_sample, else (class).  A tile pair whose
 *     partition ranges cannot meet (the centroids are sorted by partition) leaves before it stages anything.
 *   Integer atomics only (counters, union-find hooks onto the smaller root): bit-reproducible.  Every argument of these entry
 *   points is checked before the first launch; the three scans in between are called with n >= 1 and carved buffers, the
 *   only things sst_exclusive_scan_i32 itself refuses.  Workspace: sst_cluster_classes_workspace_bytes(n).
 * ---------------------------------------------------------------------------------------------- */
#define SST_CCL_MAX_CLASSES 32
#define SST_CCL_MAX_SAMPLES 256
#define SST_CCL_STATUS_CELL_RANGE 1   /* a cluster-voxel coordinate does not fit the fixed key layout */
#define SST_CCL_STATUS_SAMPLE_RANGE 2 /* a sample index outside [0, SST_CCL_MAX_SAMPLES) */
typedef struct sst_cluster_classes_params {
  int32_t n_classes;                           /* 1 .. SST_CCL_MAX_CLASSES */
  int32_t per_sample;                          /* 1: partition (class, sample) - training; 0: (class) - test */
  int32_t min_points;
  int32_t count_tiles;
  int32_t class_off[SST_CCL_MAX_CLASSES + 1];  /* ascending, class_off[0] = 0, class_off[n_classes] = n */
  float cell[SST_CCL_MAX_CLASSES][3];          /* cluster voxel size (x, y, z) per class, > 0 */
  float dist[SST_CCL_MAX_CLASSES];             /* connected_dist per class */
  float origin[3];
  int32_t reserved;
} sst_cluster_classes_params;
int sst_cluster_classes_max(void);
/* mins / extents (5 each) of the (class, sample, x, y, z) rows for sst_unique_rows */
int sst_cluster_classes_key_layout(int n_classes, int64_t* h_mins, int64_t* h_extents);
int sst_cluster_classes_keys_f32(const float* d_points, int64_t ld, const int32_t* d_batch, int64_t n,
                                 const sst_cluster_classes_params* params, int32_t* d_rows, int32_t* d_status, void* stream);
int64_t sst_cluster_classes_workspace_bytes(int64_t n);
int sst_cluster_classes_f32(const float* d_centroids, const int32_t* d_rows, const uint32_t* d_perm, const int32_t* d_offsets,
                            const int32_t* d_inverse, const int32_t* d_num_groups, int64_t n,
                            const sst_cluster_classes_params* params, const int32_t* d_status, int32_t* d_inds, int64_t* d_keep,
                            uint8_t* d_mask, int32_t* d_sizes, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CTRL's offline stage (csrc/tracklet_prep.hip): the compute loops of the reference's tools/ctrl/ scripts, each
 * for a whole batch in one launch.  fp32 data, int64 timestamps, integer atomics only, no order that depends on scheduling: two
 * runs are bit-equal.
 *
 * sst_tracklet_affinity_f32 - replaces the pair loop of tools/ctrl/generate_candidates.py:39-66 (tracklet_assign: per predicted
 *   tracklet a Python loop over the ground-truth tracklets of its segment) with LiDARTracklet.max_iou
 *   (mmdet3d/core/bbox/structures/lidar_tracklet.py:210-229: a set intersection, two cats, two .cuda() copies, one
 *   aligned_iou_3d launch and one .item() per pair).  One wave per pair, sst_tracklet_affinity_pairs_per_block() pairs of one
 *   predicted tracklet per workgroup.
 *   Inputs: pd_boxes [n_pd_rows, 7] and pd_ts int64 [n_pd_rows] (ascending within a tracklet) of the predicted tracklets with
 *   pd_offsets int64 [n_pd + 1]; gt_boxes / gt_ts / gt_offsets [n_gt + 1] likewise; pd_gt_begin / pd_gt_end int64 [n_pd]: the
 *   half-open range of ground-truth tracklets predicted tracklet p is paired with (its own segment's: the tracklets are sorted
 *   by segment on the host); out_offsets int64 [n_pd + 1]: the offset of p's row in the ragged output (out_offsets[p + 1] -
 *   out_offsets[p] >= its range); block_offsets int64 [n_pd + 1]: the cumulative number of workgroups, ceil(range /
 *   pairs_per_block) per predicted tracklet; n_blocks = block_offsets[n_pd].  Offsets and ranges are clamped to their arrays.
 *   Output: affinity [n_out] fp32, affinity[out_offsets[p] + (g - pd_gt_begin[p])] = the maximum over the shared timestamps of
 *   LiDARInstance3DBoxes.aligned_iou_3d(pd box, gt box) (lidar_box3d.py:404-450, the value of sst_tracklet_targets_f32 bit for
 *   bit; a NaN wins the maximum, as in torch.max), 0 without a shared timestamp.  Elements outside every range are not written.
 *
 * sst_box_crops_count_f32 / sst_box_crops_fill_f32 - replace the per-box loop of tools/ctrl/generate_track_input.py:88-101
 *   (extract_and_save_point: per frame and box one points_in_boxes launch chain on the whole cloud, a boolean mask, an index
 *   and a copy to the host) and, with the count alone, tools/ctrl/remove_empty.py:82-134 (process_single_frame /
 *   get_grouping_mask with group_size = 1: "does this box hold a point").  A batch of n_frames frames: points [n_points, cols]
 *   (cols >= 3, xyz first) frame after frame with pt_offsets int64 [n_frames + 1]; boxes [n_boxes, 7] ([x, y, z_bottom, w, l, h,
 *   ry], already modified by the caller) with box_offsets int64 [n_frames + 1].  Every box is tested alone against every point
 *   of its frame with the inside test of csrc/pib_test.h (dpp_box(roi, 0, 0, 0), dpp_classify == 1: sst_points_in_boxes_f32's).
 *   A workgroup takes a tile of sst_box_crops_tile() consecutive points of one frame: tile_offsets int64 [n_frames + 1] = the
 *   cumulative number of tiles, ceil(N_f / tile) per frame (n_tiles = its last element); cell_offsets int64 [n_frames + 1] =
 *   the cumulative B_f * T_f (n_cells = its last element): cell (f, b, t) = cell_offsets[f] + b * T_f + t.
 *   count: counts int32 [n_boxes] = points inside every box (zeroed here; integer atomics over the tiles).  With tile_counts
 *     (int32 [n_cells]) also the per-cell counts, their exclusive scan tile_starts (int32 [n_cells], sst_exclusive_scan_i32) and
 *     total int32 [1] - the one value the caller reads to size the fill; workspace: sst_box_crops_workspace_bytes(n_cells).
 *     With tile_counts == NULL: the count-only entry, one launch.
 *   fill: rows [n_rows, cols] = the points inside, in (frame, box, ascending point index) order - the order
 *     pc[inbox_inds == 0] gives the reference - and src int64 [n_rows] = the point's index in its frame.  Only cells with a
 *     non-zero count are tested again; a row's slot is tile_starts[cell] + its ballot rank.  Rows of any width are copied
 *     float by float (24-byte rows are not 16-byte aligned).
 * Errors (nothing is launched): SST_ERR_ARG for a NULL required pointer, a negative size or cols < 3; SST_ERR_UNSUPPORTED for
 * sizes above 2^31 - 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sst_tracklet_affinity_args {
  const float* pd_boxes;
  const int64_t* pd_ts;
  const int64_t* pd_offsets;
  const float* gt_boxes;
  const int64_t* gt_ts;
  const int64_t* gt_offsets;
  const int64_t* pd_gt_begin;
  const int64_t* pd_gt_end;
  const int64_t* out_offsets;
  const int64_t* block_offsets;
  float* affinity;
  int64_t n_pd_rows, n_gt_rows, n_pd, n_gt, n_out, n_blocks;
} sst_tracklet_affinity_args;
typedef struct sst_box_crops_args {
  const float* points;
  const float* boxes;
  const int64_t* pt_offsets;
  const int64_t* box_offsets;
  const int64_t* tile_offsets;
  const int64_t* cell_offsets;
  int32_t* counts;
  int32_t* tile_counts;
  int32_t* tile_starts;
  int32_t* total;
  float* rows;
  int64_t* src;
  void* workspace;
  int64_t workspace_bytes, n_points, n_boxes, n_tiles, n_cells, n_rows;
  int32_t n_frames, cols;
} sst_box_crops_args;
int sst_tracklet_affinity_pairs_per_block(void);
int sst_tracklet_affinity_f32(const sst_tracklet_affinity_args* args, void* stream);
int sst_box_crops_tile(void);
int sst_box_crops_box_chunk(void);   /* boxes staged in LDS at a time by the count kernel */
int64_t sst_box_crops_workspace_bytes(int64_t n_cells);
int sst_box_crops_count_f32(const sst_box_crops_args* args, void* stream);
int sst_box_crops_fill_f32(const sst_box_crops_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SST_AMD_H */

"""Furthest point sampling (mmdet3d/ops/furthest_point_sample/furthest_point_sample.py) and the device half of FSD's SSG
cluster assignment (detectors/single_stage_fsd.py:83-142).

Names, arguments and return values of ``furthest_point_sample`` / ``furthest_point_sample_with_dist`` are the reference's:
int32 indices, non-differentiable, contiguous device fp32 input.  ``fps_segmented`` samples inside every segment of one
point array in a single launch (one workgroup per segment) and ``ssg_assign`` prunes, numbers and assigns for all segments
at once; both are what ``sst_amd.cluster.ssg`` and the SSG / hybrid assigners are made of.  The work runs in csrc/fps.hip
behind the C ABI of include/sst_amd.h.

Selection rule (pinned by tests/fps_ref.py): sample 0 is point 0; every later sample is the arg-max of the running minimum
squared distance, computed in fp32 with every product and sum rounded on its own; among EQUAL distances the reference
kernel's winner is kept, which is not the lowest index (include/sst_amd.h).  Inputs holding NaN or infinity are outside
the contract.
"""
import struct

import torch

from . import _lib

SSG_MULTI_BALL, SSG_EMPTY_SEGMENT, SSG_BAD_KEYPOINT = 1, 2, 4


def _check_f32(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f'sst_amd.{what}: CUDA tensors required (no CPU fallback)')
    if t.dtype != torch.float32:
        raise RuntimeError(f'sst_amd.{what}: float32 expected, got {t.dtype}')


def _check_out(t, shape, dtype, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f'sst_amd.{what}: a contiguous device {dtype} tensor of shape {tuple(shape)} is expected')


def _fps_into(points_xyz, num_points, temp, out, what='furthest_point_sample'):
    """points_xyz [B, N, 3] -> out [B, num_points] (int32), both caller-owned; temp [B, N] fp32 workspace"""
    _check_f32(points_xyz, what)
    if points_xyz.dim() != 3 or points_xyz.size(2) != 3 or not points_xyz.is_contiguous():
        raise RuntimeError(f'sst_amd.{what}: a contiguous [B, N, 3] tensor is expected, got {tuple(points_xyz.shape)}')
    b, n = points_xyz.shape[:2]
    m = int(num_points)
    if m < 0 or (m > 0 and n == 0):
        raise RuntimeError(f'sst_amd.{what}: cannot take {m} samples of {n} points')
    _check_out(temp, (b, n), torch.float32, what + ' (temp)')
    _check_out(out, (b, m), torch.int32, what + ' (output)')
    if b and m:
        rc = _lib.load().sst_fps_segmented_f32(_lib.ptr(points_xyz), 3, b * n, None, n, b, m, 0, _lib.ptr(temp),
                                               _lib.ptr(out), None, _lib.stream_ptr())
        _lib.check(rc, 'sst_fps_segmented_f32')
    return out


def _fps_with_dist_into(points_dist, num_points, temp, out, what='furthest_point_sample_with_dist'):
    _check_f32(points_dist, what)
    if points_dist.dim() != 3 or points_dist.size(1) != points_dist.size(2) or not points_dist.is_contiguous():
        raise RuntimeError(f'sst_amd.{what}: a contiguous [B, N, N] tensor is expected, got {tuple(points_dist.shape)}')
    b, n = points_dist.shape[:2]
    m = int(num_points)
    if m < 0 or (m > 0 and n == 0):
        raise RuntimeError(f'sst_amd.{what}: cannot take {m} samples of {n} points')
    _check_out(temp, (b, n), torch.float32, what + ' (temp)')
    _check_out(out, (b, m), torch.int32, what + ' (output)')
    if b and m:
        rc = _lib.load().sst_fps_with_dist_f32(_lib.ptr(points_dist), b, n, m, _lib.ptr(temp), _lib.ptr(out),
                                               _lib.stream_ptr())
        _lib.check(rc, 'sst_fps_with_dist_f32')
    return out


def furthest_point_sample(points_xyz, num_points):
    """[B, N, 3] fp32 -> int32 [B, num_points] indices (FurthestPointSampling.forward, furthest_point_sample.py:15-35).
    num_points > N is allowed, as in the reference kernel: the recurrence runs on and repeats come out."""
    _check_f32(points_xyz, 'furthest_point_sample')
    if points_xyz.dim() != 3:
        raise RuntimeError('sst_amd.furthest_point_sample: a [B, N, 3] tensor is expected')
    b, n = points_xyz.shape[:2]
    out = torch.empty((b, int(num_points)), dtype=torch.int32, device=points_xyz.device)
    temp = torch.empty((b, n), dtype=torch.float32, device=points_xyz.device)   # initialised by the kernel where it is used
    return _fps_into(points_xyz, num_points, temp, out)


def furthest_point_sample_with_dist(points_dist, num_points):
    """[B, N, N] fp32 pairwise distances (>= 0) -> int32 [B, num_points] (FurthestPointSamplingWithDist.forward, :50-70)"""
    _check_f32(points_dist, 'furthest_point_sample_with_dist')
    if points_dist.dim() != 3:
        raise RuntimeError('sst_amd.furthest_point_sample_with_dist: a [B, N, N] tensor is expected')
    b, n = points_dist.shape[:2]
    out = torch.empty((b, int(num_points)), dtype=torch.int32, device=points_dist.device)
    temp = torch.empty((b, n), dtype=torch.float32, device=points_dist.device)
    return _fps_with_dist_into(points_dist, num_points, temp, out)


def _check_segments(points, seg_offsets, what, min_cols):
    _check_f32(points, what)
    if points.dim() != 2 or points.size(1) < min_cols or (points.size(0) > 0 and points.stride(1) != 1):
        raise RuntimeError(f'sst_amd.{what}: points of shape [N, >= {min_cols}] with unit column stride expected')
    if (not torch.is_tensor(seg_offsets) or not seg_offsets.is_cuda or seg_offsets.dtype != torch.int32
            or seg_offsets.dim() != 1 or seg_offsets.numel() < 1 or not seg_offsets.is_contiguous()):
        raise RuntimeError(f'sst_amd.{what}: seg_offsets must be a contiguous device int32 tensor [S + 1]')
    return seg_offsets.numel() - 1


def fps_segmented(points, seg_offsets, m, identity_if_short=False):
    """Furthest point sampling inside every segment [seg_offsets[s], seg_offsets[s+1]) of ``points`` [N, >= 3] (row-strided
    views are fine; columns 0..2 are read), one launch for all segments.

    -> (idx int32 [S, m], count int32 [S]): indices RELATIVE to the segment's first point.  identity_if_short: a segment
    with at most m points yields 0 .. n_s-1 in order, then -1, count = n_s (ssg_single_sample's ``num_fps >= len(points)``
    branch); otherwise count = m and a short segment repeats points.  An empty segment: -1 everywhere, count 0.  The
    offsets must be ascending and end at or below N; they are not read back."""
    s = _check_segments(points, seg_offsets, 'fps_segmented', 3)
    m = int(m)
    if m < 0:
        raise RuntimeError('sst_amd.fps_segmented: m must not be negative')
    dev = points.device
    n = points.size(0)
    idx = torch.empty((s, m), dtype=torch.int32, device=dev)
    count = torch.zeros(s, dtype=torch.int32, device=dev)
    if s and m:
        temp = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        rc = _lib.load().sst_fps_segmented_f32(_lib.ptr(points), points.stride(0) if n else 3, n, _lib.ptr(seg_offsets), 0, s,
                                               m, 1 if identity_if_short else 0, _lib.ptr(temp), _lib.ptr(idx),
                                               _lib.ptr(count), _lib.stream_ptr())
        _lib.check(rc, 'sst_fps_segmented_f32')
    return idx, count


def f32_scalar(v):
    """a Python scalar as torch compares it against an fp32 tensor: rounded to fp32 once, on the host"""
    return struct.unpack('f', struct.pack('f', float(v)))[0]


def ssg_assign(points, seg_offsets, key_idx, key_count, thr2, radius):
    """Pruning, numbering and assignment of ssg_single_sample / ssg (single_stage_fsd.py:83-142) for all segments.

    points [N, >= 2] fp32, seg_offsets int32 [S + 1], key_idx int32 [S, m] / key_count int32 [S] as fps_segmented returns
    them.  thr2 / radius: the two thresholds (``radius * 2 + 0.01`` and ``radius`` in the reference), rounded to fp32 here.
    -> (cluster_id int32 [N] (-1: in no ball or in several), n_clusters int32 [1], status int32 [1]); all on the device,
    nothing is read back.  status bits: SSG_MULTI_BALL, SSG_EMPTY_SEGMENT (the reference's two asserts), SSG_BAD_KEYPOINT."""
    s = _check_segments(points, seg_offsets, 'ssg_assign', 2)
    dev = points.device
    if (not torch.is_tensor(key_idx) or key_idx.dtype != torch.int32 or key_idx.dim() != 2 or key_idx.size(0) != s
            or not key_idx.is_cuda or not key_idx.is_contiguous()):
        raise RuntimeError('sst_amd.ssg_assign: key_idx must be a contiguous device int32 tensor [S, m]')
    _check_out(key_count, (s,), torch.int32, 'ssg_assign (key_count)')
    m = key_idx.size(1)
    n = points.size(0)
    cluster_id = torch.empty(n, dtype=torch.int32, device=dev)
    n_clusters = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _lib.workspace(lib.sst_ssg_assign_workspace_bytes(s, m), dev)
    rc = lib.sst_ssg_assign_f32(_lib.ptr(points), points.stride(0) if n else 2, n, _lib.ptr(seg_offsets), s, _lib.ptr(key_idx),
                                _lib.ptr(key_count), m, f32_scalar(thr2), f32_scalar(radius), _lib.ptr(cluster_id),
                                _lib.ptr(n_clusters), _lib.ptr(status), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, 'sst_ssg_assign_f32')
    return cluster_id, n_clusters, status


def raise_on_status(status):
    """the reference's asserts (single_stage_fsd.py:125, :128) for a status word already on the host"""
    status = int(status)
    assert not status & SSG_MULTI_BALL, 'ssg: a point lies in more than one ball'
    assert not status & SSG_EMPTY_SEGMENT, 'ssg: a sample assigned no point'
    assert not status & SSG_BAD_KEYPOINT, 'ssg: a keypoint index outside its segment'

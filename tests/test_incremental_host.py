"""The incremental stage without a GPU: the C entry points reject bad arguments before anything is launched, CPU tensors raise,
the packing of seed_info (offsets, empty frames, numpy labels, class-wise widths), the host matrix inv(cur) @ pre in float64,
the grid size as the reference computes it and the delta queries of the shipped settings."""
import ctypes

import numpy as np
import pytest
import torch

from sst_amd import _lib
from sst_amd import incremental as I

ARG, UNSUPPORTED = _lib.SST_ERR_ARG, _lib.SST_ERR_UNSUPPORTED


def _stage_args(**over):
    a = _lib.IncrArgs()
    a.n_samples, a.cols, a.n_frames, a.n_queries, a.n_boxes = 1, 5, 1, 1, 0
    a.n_points[0] = 0
    a.q_inc[0], a.q_lo[0], a.q_hi[0] = 0, -2, -1
    a.lo, a.vs, a.grid = I._f3([0, 0, 0]), I._f3([1, 1, 1]), _lib.i32array([4, 4, 4])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_stage_entry_points_reject_bad_arguments():
    lib = _lib.load()
    assert lib.sst_incr_plan_f32(None, None) == ARG and lib.sst_incr_rows_f32(None, None) == ARG
    assert lib.sst_incr_workspace_bytes(None) == ARG
    assert lib.sst_incr_workspace_bytes(ctypes.byref(_stage_args())) > 0
    for bad, rc in ((dict(n_samples=17), UNSUPPORTED), (dict(n_frames=17), UNSUPPORTED), (dict(n_queries=5), UNSUPPORTED),
                    (dict(cols=2), UNSUPPORTED), (dict(cols=16), UNSUPPORTED), (dict(n_samples=-1), ARG), (dict(n_boxes=-1), ARG),
                    (dict(vs=I._f3([0, 1, 1])), ARG), (dict(grid=_lib.i32array([0, 4, 4])), ARG),
                    (dict(grid=_lib.i32array([4096, 4096, 1024])), UNSUPPORTED), (dict(n_boxes=3), ARG)):
        a = _stage_args(**bad)
        assert lib.sst_incr_workspace_bytes(ctypes.byref(a)) == rc, bad
        assert lib.sst_incr_plan_f32(ctypes.byref(a), None) == rc, bad
        assert lib.sst_incr_rows_f32(ctypes.byref(a), None) == rc, bad
    a = _stage_args()
    a.n_points[0] = 10                                    # points announced, none given
    assert lib.sst_incr_plan_f32(ctypes.byref(a), None) == ARG
    a = _stage_args()                                     # no counts, no workspace
    assert lib.sst_incr_plan_f32(ctypes.byref(a), None) == ARG
    a = _stage_args()
    a.q_lo[0], a.q_hi[0] = -1, 0                          # a frame among its own base frames
    buf = (ctypes.c_char * 4096)()
    a.counts = a.workspace = ctypes.addressof(buf)
    a.workspace_bytes = 4096
    assert lib.sst_incr_plan_f32(ctypes.byref(a), None) == ARG
    a = _stage_args()
    a.counts = a.workspace = ctypes.addressof(buf)
    a.workspace_bytes = 16                                # a workspace that is too small
    assert lib.sst_incr_plan_f32(ctypes.byref(a), None) == ARG


def test_mask_coors_and_transform_entry_points_reject_bad_arguments():
    lib = _lib.load()
    sp = _lib.i32array([4, 4, 4])
    one = I._f3([1, 1, 1])
    assert lib.sst_incr_voxel_coors_f32(None, -1, 3, one, one, None, None) == ARG
    assert lib.sst_incr_voxel_coors_f32(None, 4, 2, one, one, None, None) == ARG
    assert lib.sst_incr_voxel_coors_f32(None, 4, 3, one, I._f3([1, 0, 1]), None, None) == ARG
    assert lib.sst_incr_voxel_coors_f32(None, 4, 3, one, one, None, None) == ARG
    assert lib.sst_incr_voxel_coors_f32(None, 0, 3, one, one, None, None) == 0
    assert lib.sst_incr_mask_workspace_bytes(10, sp) > 0 and lib.sst_incr_mask_workspace_bytes(-1, sp) == ARG
    assert lib.sst_incr_mask_workspace_bytes(10, _lib.i32array([4096, 4096, 1024])) == UNSUPPORTED
    assert lib.sst_incr_mask_i32(None, 0, None, 4, sp, None, 0, None, None) == ARG
    assert lib.sst_incr_mask_i32(None, -1, None, 4, sp, None, 0, None, None) == ARG
    assert lib.sst_incr_mask_i32(None, 0, None, 0, sp, None, 0, None, None) == 0
    assert lib.sst_incr_delta_mask_f32(None, None) == ARG
    d = _lib.IncrDeltaArgs()
    d.n_clouds, d.n_query, d.ld_query = 9, 4, 5
    d.vs, d.grid = one, sp
    assert lib.sst_incr_delta_mask_f32(ctypes.byref(d), None) == UNSUPPORTED
    d.n_clouds = 0
    assert lib.sst_incr_delta_mask_f32(ctypes.byref(d), None) == ARG          # a query without pointers
    d.ld_query = 2
    assert lib.sst_incr_delta_mask_f32(ctypes.byref(d), None) == ARG
    assert lib.sst_points_frame_transform_f32(None, None) == ARG
    t = _lib.FrameTransformArgs()
    t.n_clouds, t.cols = 9, 5
    assert lib.sst_points_frame_transform_f32(ctypes.byref(t), None) == UNSUPPORTED
    t.n_clouds, t.cols = 1, 2
    assert lib.sst_points_frame_transform_f32(ctypes.byref(t), None) == UNSUPPORTED
    t.cols = 5
    t.n[0] = 7
    assert lib.sst_points_frame_transform_f32(ctypes.byref(t), None) == ARG
    t.n[0] = 0
    assert lib.sst_points_frame_transform_f32(ctypes.byref(t), None) == 0


def test_cpu_tensors_raise():
    cfg = dict(voxel_size=(0.25, 0.25, 0.4), point_cloud_range=[-80, -80, -2, 80, 80, 4], extra_width=1.0)
    pts = torch.zeros(8, 5)
    seed = [[dict(gt_bboxes_3d=np.zeros((0, 7), np.float32), gt_labels_3d=np.zeros(0), scores=np.zeros(0, np.float32))]]
    with pytest.raises(RuntimeError):
        I.generate_points([pts], [torch.zeros(8, dtype=torch.long)], seed, cfg, True)
    with pytest.raises(RuntimeError):
        I.voxel_coors(pts, cfg['voxel_size'], cfg['point_cloud_range'])
    with pytest.raises(RuntimeError):
        I.incremental_points_mask(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.int32), (4, 4, 4))
    with pytest.raises(RuntimeError):
        I.find_delta_points_by_voxelization(pts, pts, cfg['voxel_size'], cfg['point_cloud_range'])
    with pytest.raises(RuntimeError):
        I.find_delta_points_by_voxelization_list_v3([pts], pts, cfg['voxel_size'], cfg['point_cloud_range'])
    with pytest.raises(RuntimeError):
        I.points_frame_transform(pts[:, :3], np.eye(4), np.eye(4))
    with pytest.raises(RuntimeError):
        I.seed_crop(pts, torch.zeros(1, 7))


def test_seed_info_packing():
    class Boxes(object):                                   # anything with .tensor
        def __init__(self, t):
            self.tensor = t

    b3 = torch.arange(27.).reshape(3, 9)                  # boxes with velocities: the first 7 columns travel
    frames0 = [dict(gt_bboxes_3d=Boxes(b3), gt_labels_3d=np.asarray([2, 0, 1]), scores=np.ones(3, np.float32)),
               dict(gt_bboxes_3d=torch.zeros(0, 7), gt_labels_3d=np.zeros(0), scores=np.zeros(0, np.float32)),
               dict(gt_bboxes_3d=np.ones((2, 7), np.float32), gt_labels_3d=torch.tensor([1., 1.]), scores=torch.ones(2))]
    frames1 = [dict(gt_bboxes_3d=torch.full((1, 7), 5.0), gt_labels_3d=np.asarray([0]), scores=np.ones(1, np.float32))]
    cfg = dict(extra_width=dict([(0, 0.5), (1, 0.25), (2, 1.0)]))
    rows, off = I.pack_seed_info([frames0, frames1], cfg, 3)
    assert off.dtype == np.int32 and off.tolist() == [0, 3, 3, 5, 6, 6, 6]
    assert rows.dtype == np.float32 and rows.shape == (6, 8)
    assert np.array_equal(rows[:3, :7], b3[:, :7].numpy()) and rows[:, 7].tolist() == [1.0, 0.5, 0.25, 0.25, 0.25, 0.5]
    rows, off = I.pack_seed_info([frames0, frames1], dict(extra_width=1.5), 2)
    assert off.tolist() == [0, 3, 3, 4, 4] and rows[:, 7].tolist() == [1.5] * 4
    rows, off = I.pack_seed_info([[], []], cfg, 0)
    assert rows.shape == (0, 8) and off.tolist() == [0]
    # the enlargement on the packed rows is LiDARInstance3DBoxes.enlarged_box's arithmetic
    rows, _ = I.pack_seed_info([frames0], dict(extra_width=0.3), 1)
    got = I.modify_boxes(torch.from_numpy(rows), dict(center_noise=0.0, dim_noise=0.0, yaw_noise=0.0), training=True)
    want = b3[:, :7].clone()
    want[:, 3:6] += 0.3 * 2
    want[:, 2] -= 0.3
    assert torch.equal(got, want)
    torch.manual_seed(0)
    noisy = I.modify_boxes(torch.from_numpy(rows), dict(center_noise=0.1, dim_noise=0.1, yaw_noise=0.1), training=True)
    assert not torch.equal(noisy, want) and torch.equal(I.modify_boxes(torch.from_numpy(rows), dict(center_noise=0.1), False), want)


def test_host_matrix_is_the_float64_product():
    g = np.random.default_rng(0)

    def pose():
        yaw = g.uniform(-3, 3)
        m = np.eye(4)
        m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        m[:3, 3] = g.uniform(-5000, 5000, 3)
        return m.astype(np.float32)

    pre, cur = pose(), pose()
    want = (np.linalg.inv(cur.astype(np.float64)) @ pre.astype(np.float64)).astype(np.float32)
    assert np.array_equal(I.frame_matrix(pre, cur), want)
    assert np.array_equal(I.frame_matrix(torch.from_numpy(pre), torch.from_numpy(cur)), want)
    inv = np.linalg.inv(cur.astype(np.float64))
    assert np.array_equal(I.frame_matrix(pre, None, cur_pose_inv=inv), want)
    # box_frame_transform_gpu keeps the kind it is given and moves centres and headings (host tensors: torch ops only)
    boxes = torch.tensor([[1.0, 2.0, 0.5, 2.0, 4.0, 1.5, 0.3, 1.0, 0.0]])
    out = I.box_frame_transform_gpu(boxes, pre, cur)
    m = torch.from_numpy(want)
    assert out.shape == (1, 9) and torch.allclose(out[0, :3], m[:3, :3] @ boxes[0, :3] + m[:3, 3], atol=1e-3)
    assert torch.equal(out[:, 3:6], boxes[:, 3:6]) and I.box_frame_transform_gpu(boxes[:0], pre, cur).shape == (0, 9)


def test_grid_and_queries_of_the_shipped_settings():
    cfg = dict(voxel_size=(0.25, 0.25, 0.4), point_cloud_range=[-80, -80, -2, 80, 80, 4], num_previous_frames=6, num_base_frame=5,
               max_age=1)
    assert I.spatial_size(cfg['voxel_size'], cfg['point_cloud_range']) == (641, 641, 16)
    assert I.spatial_size(cfg['voxel_size'], cfg['point_cloud_range'], fp32=False) == (641, 641, 16)
    assert I.queries_of(cfg, 6) == [(0, -5, -1, 0.0), (-1, -5, -2, -0.1)]
    assert I.queries_of(dict(cfg, max_age=0), 6) == [(0, -5, -1, 0.0)]
    assert I.queries_of(dict(cfg, num_base_frame=9), 6)[0] == (0, -6, -1, 0.0)
    assert I.queries_of(dict(cfg, disable_incremental=True), 6) == []

"""tests/golden/incremental.npz: the reference's own incremental point stage run on the CPU from its source text.

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_incremental.py

Loaded from detectors/incremental_ops.py: voxelize_single, find_delta_unq_coors, find_delta_pc_mask,
find_delta_points_by_voxelization, find_delta_points_by_voxelization_list_v2 / _v3, points_frame_transform,
box_frame_transform_gpu; from TwoStageFSDPP (detectors/two_stage_fsdpp.py): generate_points, get_old_points,
crop_and_process_points, modify_previous_boxes, channel_padding, get_delta_points, generate_points_list, get_old_points_list_v2,
get_delta_points_list.  Stand-ins for what cannot run here:
    incremental_points_mask (TorchEx, no source in the tree)  the in-tree set semantics: find_delta_unq_coors + find_delta_pc_mask
                                                              as find_delta_points_by_voxelization_list_v2 composes them
    get_inner_win_inds                                        oracle.ref_loader.stable_ingroup_rank
    torch.randperm                                            argsort of the stored keys (stable); a point's key is its column 4,
                                                              an integer below 2^24, exact in float32
    LiDARInstance3DBoxes.points_in_boxes                      the first hit of the reference's compiled points_in_boxes_cpu
                                                              (oracle/_ref); enlarged_box / classwise_enlarged_box / noisy_box are
                                                              the reference's arithmetic (lidar_box3d.py:269-329) on the tensor
Points are drawn at least 1e-3 away from every face of every enlarged box of their frame, so the CPU and GPU inside tests agree.
Every float case runs in float32 and in float64 (default dtype switched) and the gap is stored.  The clouds of the transform cases
are re-drawn until, in float64, no transformed coordinate lies within max(1e-4, 10 x gap) of a voxel boundary, so the masks after
the transform are the same in either precision.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))

OPS_PY = 'mmdet3d/models/detectors/incremental_ops.py'
DET_PY = 'mmdet3d/models/detectors/two_stage_fsdpp.py'
RANGE = [-80, -80, -2, 80, 80, 4]
VS = (0.25, 0.25, 0.4)


def load_ops():
    from oracle import ref_loader as L
    ops = {}
    glb = dict(F=F)
    for name in ('voxelize_single', 'find_delta_unq_coors', 'find_delta_pc_mask'):
        ops[name] = L.load_reference_function(OPS_PY, name, dict(glb))

    def incremental_points_mask(coors1, coors2, spatial_size):
        unq2, inv2 = torch.unique(coors2, return_inverse=True, dim=0)
        delta = ops['find_delta_unq_coors'](torch.unique(coors1, dim=0), unq2)
        _, _, counts = torch.unique(torch.cat([unq2, delta], 0), sorted=True, return_counts=True, return_inverse=True, dim=0)
        return (counts > 1)[inv2] if len(coors2) else torch.zeros(0, dtype=torch.bool)

    ops['incremental_points_mask'] = incremental_points_mask
    glb.update(ops)
    for name in ('find_delta_points_by_voxelization', 'find_delta_points_by_voxelization_list_v2',
                 'find_delta_points_by_voxelization_list_v3', 'points_frame_transform'):
        ops[name] = L.load_reference_function(OPS_PY, name, dict(glb))
    ops['box_frame_transform_gpu'] = L.load_reference_function(OPS_PY, 'box_frame_transform_gpu', dict(glb, LiDARInstance3DBoxes=Boxes))
    return ops


class Boxes(object):
    """the part of LiDARInstance3DBoxes the stage touches, on one tensor"""
    pib = None
    last_points = None

    def __init__(self, tensor, box_dim=7):
        self.tensor = tensor

    @property
    def heading_unit_vector(self):
        yaw = self.tensor[:, 6]
        return torch.stack([torch.sin(yaw), torch.cos(yaw), torch.zeros_like(yaw)], -1)        # lidar_box3d.py:109-114

    def __len__(self):
        return self.tensor.size(0)

    def to(self, device):
        return self

    def clone(self):
        return Boxes(self.tensor.clone())

    def new_box(self, t):
        return Boxes(t)

    def noisy_box(self, center_noise, dim_noise, yaw_noise):
        assert center_noise == 0 and dim_noise == 0 and yaw_noise == 0     # the shipped values: the identity
        return Boxes(self.tensor.clone())

    def enlarged_box(self, extra_width):
        b = self.tensor.clone()
        b[:, 3:6] += extra_width * 2
        b[:, 2] -= extra_width
        return Boxes(b)

    def classwise_enlarged_box(self, extra_width_dict, labels):
        ew = self.tensor.new_ones(len(self.tensor))
        for l in torch.unique(labels).tolist():
            ew[labels == l] = extra_width_dict[l]
        b = self.tensor.clone()
        b[:, 3:6] += ew[:, None] * 2
        b[:, 2] -= ew
        return Boxes(b)

    def points_in_boxes(self, xyz):
        Boxes.last_points = xyz._base if xyz._base is not None else xyz
        n, p = self.tensor.size(0), xyz.size(0)
        flags = torch.zeros((n, p), dtype=torch.int32)
        Boxes.pib.points_in_boxes_cpu(self.tensor[:, :7].float().contiguous(), xyz.float().contiguous(), flags)
        first = torch.where(flags.bool().any(0), flags.argmax(0), torch.full((p,), -1, dtype=torch.long))
        Boxes.last_mask = first > -1
        return first


class TorchProxy(object):
    """``torch`` for the detector's methods: randperm is argsort of the keys of the points last cropped"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def randperm(n):
        keys = Boxes.last_points[:, 4][Boxes.last_mask]
        assert keys.numel() == n
        return torch.sort(keys.long(), stable=True)[1]


class Stage(object):
    def __init__(self, cfg, training, methods):
        self.incremental_cfg, self.training = cfg, training
        self.max_pre_frames = cfg.get('num_previous_frames', 4)
        for k, fn in methods.items():
            setattr(self, k, fn.__get__(self))


def load_methods(ops):
    from oracle import ref_loader as L
    glb = dict(F=F, np=np, torch=TorchProxy(), get_inner_win_inds=L.stable_ingroup_rank, set_trace=lambda: None,
               find_delta_points_by_voxelization=ops['find_delta_points_by_voxelization'],
               find_delta_points_by_voxelization_list_v3=ops['find_delta_points_by_voxelization_list_v3'],
               points_frame_transform=ops['points_frame_transform'])
    return {k: L.load_reference_method(DET_PY, 'TwoStageFSDPP', k, dict(glb))
            for k in ('generate_points', 'get_old_points', 'crop_and_process_points', 'modify_previous_boxes', 'channel_padding',
                      'get_delta_points', 'generate_points_list', 'get_old_points_list_v2', 'get_delta_points_list')}


def clearance_ok(xyz, boxes, margin=1e-3):
    """every point at least ``margin`` from every face of every box (float64)"""
    ok = np.ones(len(xyz), bool)
    for b in boxes.astype(np.float64):
        rot = b[6] + np.pi / 2
        dx, dy = xyz[:, 0] - b[0], xyz[:, 1] - b[1]
        lx = dx * np.cos(rot) - dy * np.sin(rot)
        ly = dx * np.sin(rot) + dy * np.cos(rot)
        lz = xyz[:, 2] - (b[2] + b[5] / 2)
        d = np.minimum(np.minimum(np.abs(np.abs(lx) - b[4] / 2), np.abs(np.abs(ly) - b[3] / 2)), np.abs(np.abs(lz) - b[5] / 2))
        ok &= d >= margin
    return ok


def stage_case(g, cfg, n_samples=2, n_frames=3, per_frame=400, n_boxes=(9, 1, 4)):
    """clouds with 5 columns (column 4 = the key), frame indices, seeds; dense clumps so that the cap applies"""
    ew = cfg['extra_width']
    pts, finds, seeds = [], [], []
    for s in range(n_samples):
        frames, clouds, fr = [], [], []
        for i in range(n_frames):
            nb = n_boxes[(i + s) % len(n_boxes)]
            b = np.concatenate([g.uniform(-20, 20, (nb, 2)), g.uniform(-1, 0, (nb, 1)), g.uniform(1, 5, (nb, 3)), g.uniform(-3, 3, (nb, 1))], 1)
            labels = g.integers(0, 3, nb)
            frames.append(dict(gt_bboxes_3d=b.astype(np.float32), gt_labels_3d=labels.astype(np.int64), scores=g.uniform(0, 1, nb).astype(np.float32)))
            big = b.astype(np.float32).astype(np.float64).copy()
            w = np.asarray([ew[int(l)] for l in labels]) if isinstance(ew, dict) else np.full(nb, ew)
            big[:, 3:6] += (w * 2)[:, None]
            big[:, 2] -= w
            xyz = np.concatenate([g.uniform(-25, 25, (per_frame, 2)), g.uniform(-2, 3, (per_frame, 1))], 1)
            clump = b[g.integers(0, nb, 200), :3] + g.uniform(-0.4, 0.4, (200, 3)) + [0, 0, 0.6]       # > cap points in some box
            xyz = np.concatenate([xyz, clump], 0).astype(np.float32)
            while True:
                bad = ~clearance_ok(xyz.astype(np.float64), big)
                if not bad.any():
                    break
                xyz[bad] = (xyz[bad] + g.uniform(-0.05, 0.05, (int(bad.sum()), 3))).astype(np.float32)
            clouds.append(xyz)
            fr.append(np.full(len(xyz), -i - 1))
        cur = np.concatenate([g.uniform(-30, 30, (per_frame, 2)), g.uniform(-3, 5, (per_frame, 1))], 1).astype(np.float32)
        clouds.append(cur)
        fr.append(np.zeros(len(cur)))
        xyz = np.concatenate(clouds, 0)
        f = np.concatenate(fr).astype(np.int64)
        keys = g.integers(0, 2 ** 24, len(xyz))
        keys[:30] = keys[30:60]
        p = np.concatenate([xyz, g.uniform(0, 1, (len(xyz), 1)).astype(np.float32), keys[:, None].astype(np.float32)], 1)
        perm = g.permutation(len(p))
        pts.append(p[perm])
        finds.append(f[perm])
        seeds.append(frames)
    return pts, finds, seeds


def run_stage(methods, cfg, pts, finds, seeds, dtype):
    torch.set_default_dtype(dtype)
    try:
        st = Stage(cfg, True, methods)
        seed_info = [[dict(gt_bboxes_3d=Boxes(torch.as_tensor(f['gt_bboxes_3d'], dtype=dtype)), gt_labels_3d=f['gt_labels_3d'],
                           scores=f['scores']) for f in frames] for frames in seeds]
        outs, nd = st.generate_points([torch.as_tensor(p, dtype=dtype) for p in pts], [torch.as_tensor(f) for f in finds], seed_info)
        return [o.numpy() for o in outs], nd
    finally:
        torch.set_default_dtype(torch.float32)


def sequential_case(methods, g, cfg, dtype):
    """one frame of the sequential path (generate_points_list, :528-565): two previous clouds already in the current frame, two
    previous crops in their own frames with their poses, three seeds (so the current frame joins the base clouds and is cropped
    by the newest seed: the warm-up), no shuffle"""
    def cloud(n):
        return np.concatenate([g.uniform(-25, 25, (n, 2)), g.uniform(-2, 3, (n, 1)), g.uniform(0, 1, (n, 2))], 1).astype(np.float32)
    cur, pre = cloud(900), [cloud(800), cloud(700)]
    poses = [pose(g, 30) for _ in range(3)]
    crops = [cloud(150), cloud(120)]
    b = np.concatenate([g.uniform(-20, 20, (6, 2)), g.uniform(-1, 0, (6, 1)), g.uniform(3, 8, (6, 3)), g.uniform(-3, 3, (6, 1))], 1).astype(np.float32)
    big = b.astype(np.float64).copy()
    big[:, 3:6] += cfg['extra_width'] * 2
    big[:, 2] -= cfg['extra_width']
    while True:
        bad = ~clearance_ok(cur[:, :3].astype(np.float64), big)
        if not bad.any():
            break
        cur[bad, :3] += g.uniform(-0.05, 0.05, (int(bad.sum()), 3)).astype(np.float32)
    seed = dict(gt_bboxes_3d=b, gt_labels_3d=g.integers(0, 3, 6).astype(np.int64), scores=g.uniform(0, 1, 6).astype(np.float32))
    empty = dict(gt_bboxes_3d=np.zeros((0, 7), np.float32), gt_labels_3d=np.zeros(0, np.int64), scores=np.zeros(0, np.float32))
    outs = {}
    for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        torch.set_default_dtype(dt)
        try:
            st = Stage(cfg, False, methods)
            st.previous_cropped_pc = [torch.as_tensor(c, dtype=dt) for c in crops]
            st.previous_pose = [torch.as_tensor(p, dtype=dt) for p in poses[:2]]
            st.previous_delta_pc = []
            seeds = [dict(gt_bboxes_3d=Boxes(torch.as_tensor(f['gt_bboxes_3d'], dtype=dt)), gt_labels_3d=f['gt_labels_3d'], scores=f['scores'])
                     for f in (seed, empty, empty)]
            res, nd = st.generate_points_list(torch.as_tensor(cur, dtype=dt), [torch.as_tensor(c, dtype=dt) for c in pre], seeds,
                                              torch.as_tensor(poses[2], dtype=dt))
            outs[tag] = (res[0].numpy(), nd[0])
        finally:
            torch.set_default_dtype(torch.float32)
    assert outs['f32'][0].shape == outs['f64'][0].shape and outs['f32'][1] == outs['f64'][1]
    return dict(cur=cur, pre0=pre[0], pre1=pre[1], crop0=crops[0], crop1=crops[1], pose0=poses[0], pose1=poses[1], cur_pose=poses[2],
                boxes=b, labels=seed['gt_labels_3d'], scores=seed['scores'], out_f32=outs['f32'][0], out_f64=outs['f64'][0],
                num_delta=np.int64(outs['f32'][1]), gap=np.float64(np.abs(outs['f32'][0] - outs['f64'][0]).max()), cfg=np.asarray(repr(cfg)))


def box_transform_case(ops, g):
    b = np.concatenate([g.uniform(-60, 60, (40, 2)), g.uniform(-2, 1, (40, 1)), g.uniform(0.5, 8, (40, 3)), g.uniform(-3, 3, (40, 1)),
                        g.uniform(-10, 10, (40, 2))], 1).astype(np.float32)
    pre_pose, cur_pose = pose(g), pose(g)
    out = {}
    for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        for cols in (7, 9):
            r = ops['box_frame_transform_gpu'](Boxes(torch.as_tensor(b[:, :cols], dtype=dt)), torch.as_tensor(pre_pose, dtype=dt),
                                               torch.as_tensor(cur_pose, dtype=dt))
            out[f'out{cols}_{tag}'] = r.tensor.numpy()
    out.update(boxes=b, pre_pose=pre_pose, cur_pose=cur_pose,
               gap=np.float64(max(np.abs(out[f'out{c}_f32'] - out[f'out{c}_f64']).max() for c in (7, 9))))
    return out


def pose(g, far=300):
    yaw, t = g.uniform(-3, 3), g.uniform(-far, far, 3)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    m[:3, 3] = t
    return m.astype(np.float32)


def transform_case(ops, g, n):
    """a cloud of the previous frame, the poses, its image in the current frame in float32 and float64, the gap, and the masks
    of the image against a base cloud (and of the base against the image)"""
    pre_pose, cur_pose = pose(g), pose(g)
    m64 = np.linalg.inv(cur_pose.astype(np.float64)) @ pre_pose.astype(np.float64)
    inv64 = np.linalg.inv(m64)
    base = np.concatenate([g.uniform(-30, 30, (600, 2)), g.uniform(-1.5, 3.5, (600, 1))], 1).astype(np.float32)
    lo, vs = np.asarray(RANGE[:3], np.float64), np.asarray(np.asarray(VS, np.float32), np.float64)
    def draw(k):
        tgt = np.concatenate([g.uniform(-30, 30, (k, 2)), g.uniform(-1.5, 3.5, (k, 1))], 1)
        return (np.concatenate([tgt, np.ones((k, 1))], 1) @ inv64.T)[:, :3].astype(np.float32)      # lands inside the range

    src = draw(n)
    for _ in range(200):                                  # the points too close to a voxel boundary are drawn again
        t32 = ops['points_frame_transform'](torch.from_numpy(src), torch.from_numpy(pre_pose), torch.from_numpy(cur_pose)).numpy()
        t64 = ops['points_frame_transform'](torch.from_numpy(src).double(), torch.from_numpy(pre_pose).double(),
                                            torch.from_numpy(cur_pose).double()).numpy()
        gap = float(np.abs(t32 - t64).max())
        q = (t64 - lo) / vs
        close = ((np.abs(q - np.round(q)) * vs) <= max(1e-4, 10 * gap)).any(1)
        if not close.any():
            break
        src[close] = draw(int(close.sum()))
    else:
        raise RuntimeError('no clear draw')
    t_img = torch.from_numpy(t64.astype(np.float32))
    new_img = ops['find_delta_points_by_voxelization'](torch.from_numpy(base), torch.cat([t_img, torch.arange(n)[:, None].float()], 1), VS, RANGE)
    new_base = ops['find_delta_points_by_voxelization'](t_img, torch.cat([torch.from_numpy(base), torch.arange(600)[:, None].float()], 1), VS, RANGE)
    mask_img, mask_base = np.zeros(n, bool), np.zeros(600, bool)
    mask_img[new_img[:, 3].long().numpy()] = True
    mask_base[new_base[:, 3].long().numpy()] = True
    return dict(src=src, pre_pose=pre_pose, cur_pose=cur_pose, out_f32=t32, out_f64=t64, gap=np.float64(gap), base=base,
                mask_img=mask_img, mask_base=mask_base)


def main():
    from oracle import build_ref
    build_ref.build_points_in_boxes()
    Boxes.pib = build_ref.load_points_in_boxes()
    ops, g, out = load_ops(), np.random.default_rng(7), {}
    methods = load_methods(ops)
    # 1. the mask on integer triples: inside the grid, on its faces and beyond them, duplicates
    grid = (7, 5, 16)
    for k, (n1, n2) in enumerate(((0, 300), (1, 1), (255, 257), (257, 255), (5000, 5000))):
        c1 = np.stack([g.integers(-2, d + 2, n1) for d in grid], 1).astype(np.int32).reshape(n1, 3)
        c2 = np.stack([g.integers(-2, d + 2, n2) for d in grid], 1).astype(np.int32).reshape(n2, 3)
        out[f'mask{k}_c1'], out[f'mask{k}_c2'] = c1, c2
        out[f'mask{k}_out'] = ops['incremental_points_mask'](torch.from_numpy(c1), torch.from_numpy(c2), grid).numpy()
    out['mask_grid'], out['mask_cases'] = np.asarray(grid), np.int64(5)
    # 2. the points-level functions: plain and the list form v3 with its lower-bound filter (clouds reaching over the range)
    rng = [-10, -10, -2, 10, 10, 4]
    bases = [np.concatenate([g.uniform(-13, 13, (n, 2)), g.uniform(-4, 6, (n, 1)), g.uniform(0, 1, (n, 2))], 1).astype(np.float32) for n in (300, 2000)]
    query = np.concatenate([g.uniform(-13, 13, (3000, 2)), g.uniform(-4, 6, (3000, 1)), g.uniform(0, 1, (3000, 1)), np.arange(3000)[:, None]], 1).astype(np.float32)
    for dtype, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        torch.set_default_dtype(dtype)
        b, q = [torch.as_tensor(x, dtype=dtype) for x in bases], torch.as_tensor(query, dtype=dtype)
        for name, res in (('plain', ops['find_delta_points_by_voxelization'](torch.cat(b, 0), q, VS, rng)),
                          ('v2', ops['find_delta_points_by_voxelization_list_v2'](b, q, VS, rng)),
                          ('v3', ops['find_delta_points_by_voxelization_list_v3'](b, q, VS, rng))):
            m = np.zeros(3000, bool)
            m[res[:, 4].long().numpy()] = True
            out[f'delta_{name}_{tag}'] = m
        torch.set_default_dtype(torch.float32)
    assert np.array_equal(out['delta_plain_f32'], out['delta_v2_f32'])
    out['delta_bases0'], out['delta_bases1'], out['delta_query'], out['delta_range'] = bases[0], bases[1], query, np.asarray(rng, np.float64)
    # 3. the stage of a batch, the shipped settings (class-wise widths in the second case, no shuffle and cap 1 in the third)
    cfgs = [dict(voxel_size=VS, point_cloud_range=RANGE, center_noise=0.0, dim_noise=0.0, yaw_noise=0.0, extra_width=1.0,
                 num_previous_frames=3, crop_frames=3, max_crop_points=128, crop_shuffle=True, max_age=1, num_base_frame=2),
            dict(voxel_size=VS, point_cloud_range=RANGE, center_noise=0.0, dim_noise=0.0, yaw_noise=0.0,
                 extra_width={0: 0.5, 1: 0.25, 2: 0.75}, num_previous_frames=3, crop_frames=2, max_crop_points=16, crop_shuffle=True,
                 max_age=1, num_base_frame=3),
            dict(voxel_size=VS, point_cloud_range=RANGE, center_noise=0.0, dim_noise=0.0, yaw_noise=0.0, extra_width=0.5,
                 num_previous_frames=3, crop_frames=3, max_crop_points=1, crop_shuffle=False, max_age=0, num_base_frame=3)]
    out['stage_cases'] = np.int64(len(cfgs))
    for k, cfg in enumerate(cfgs):
        pts, finds, seeds = stage_case(g, cfg)
        o32, nd32 = run_stage(methods, cfg, pts, finds, seeds, torch.float32)
        o64, nd64 = run_stage(methods, cfg, pts, finds, seeds, torch.float64)
        assert nd32 == nd64
        gap = 0.0
        for s in range(len(pts)):
            out[f'stage{k}_points{s}'], out[f'stage{k}_finds{s}'] = pts[s], finds[s]
            out[f'stage{k}_out{s}'] = o32[s]
            assert o32[s].shape == o64[s].shape
            gap = max(gap, float(np.abs(o32[s] - o64[s]).max()))
            for i, f in enumerate(seeds[s]):
                out[f'stage{k}_boxes{s}_{i}'], out[f'stage{k}_labels{s}_{i}'], out[f'stage{k}_scores{s}_{i}'] = \
                    f['gt_bboxes_3d'], f['gt_labels_3d'], f['scores']
        out[f'stage{k}_num_delta'], out[f'stage{k}_gap'] = np.asarray(nd32, np.int64), np.float64(gap)
        out[f'stage{k}_cfg'] = np.asarray(repr(cfg))
    # 4. the frame transform
    for k, n in enumerate((1, 64, 65, 700)):
        for name, v in transform_case(ops, g, n).items():
            out[f'tf{k}_{name}'] = v
    out['tf_cases'] = np.int64(4)
    # 5. one frame of the sequential path, 6. box_frame_transform_gpu
    seq_cfg = dict(voxel_size=VS, point_cloud_range=RANGE, center_noise=0.0, dim_noise=0.0, yaw_noise=0.0, extra_width=1.0,
                   num_previous_frames=3, crop_frames=3, max_crop_points=16, crop_shuffle=False, max_age=1, num_base_frame=3)
    for name, v in sequential_case(methods, g, seq_cfg, None).items():
        out[f'seq_{name}'] = v
    for name, v in box_transform_case(ops, g).items():
        out[f'boxtf_{name}'] = v
    path = os.path.join(HERE, 'incremental.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', {k: float(out[k]) for k in out if k.endswith('_gap')})


if __name__ == '__main__':
    main()

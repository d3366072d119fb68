"""The FSD++ incremental point stage on the GPU (csrc/incremental.hip, sst_amd/incremental.py) against its restatement with torch
ops on the device (tests/incremental_ref.py): voxel coordinates equal to torch's floor division, the delta mask equal to the set
semantics at every size and on every side of the grid, the seed-box crops and their caps, the row layout, the frame transform
bit for bit in its stated order, and the whole stage of a batch bit for bit; two runs give equal bits."""
import numpy as np
import pytest
import torch

import incremental_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RANGE = [-80, -80, -2, 80, 80, 4]
VS = (0.25, 0.25, 0.4)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what=''):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b)), what


# ---- coordinates -------------------------------------------------------------------------------------------------------------

def _torch_coors(p, lo, vs):
    return torch.div(p[:, :3] - torch.tensor(lo, device=DEV)[None], torch.tensor(vs, device=DEV)[None], rounding_mode='floor').int()


@pytest.mark.parametrize('vs', [0.4, 0.25])
def test_coordinates_at_every_cell_boundary(vs):
    from sst_amd import incremental as I
    lo = [-80.0, -80.0, -2.0]
    cols = []
    for c in range(3):
        v = np.float32(lo[c]) + np.arange(17, dtype=np.float32) * np.float32(vs)
        vals = [v]
        up, dn = v.copy(), v.copy()
        for _ in range(3):
            up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
            vals += [up.copy(), dn.copy()]
        cols.append(np.concatenate(vals))
    n = len(cols[0])
    pts = np.zeros((3 * n, 3), np.float32)
    for c in range(3):
        pts[c * n:(c + 1) * n, c] = cols[c]
    p = torch.from_numpy(pts).to(DEV)
    got = I.voxel_coors(p, (vs, vs, vs), lo + [0, 0, 0])
    assert torch.equal(got, _torch_coors(p, lo, (vs, vs, vs)))


def test_coordinates_where_floor_of_the_quotient_differs():
    from sst_amd import incremental as I
    vals = torch.tensor([2.0, 3.5999999, 5.5999999, 6.0], dtype=torch.float32)
    p = torch.zeros(12, 3)
    for c in range(3):
        p[4 * c:4 * c + 4, c] = vals
    p = p.to(DEV)
    got = I.voxel_coors(p, (0.4, 0.4, 0.4), [0, 0, 0, 1, 1, 1])
    want = _torch_coors(p, [0.0, 0.0, 0.0], (0.4, 0.4, 0.4))
    assert torch.equal(got, want)
    # torch's floor division is not floor(a / b) at these values: the kernel follows torch
    assert got[:2, 0].tolist() == [4, 8]
    assert torch.floor(p[:4, 0] / torch.tensor(0.4, device=DEV)).int().tolist() != want[:4, 0].tolist()


def test_coordinates_of_a_million_random_values():
    from sst_amd import incremental as I
    g = torch.Generator().manual_seed(3)
    p = (torch.rand(1000000, 3, generator=g) * torch.tensor([170.0, 170.0, 8.0]) + torch.tensor([-85.0, -85.0, -3.0])).to(DEV)
    assert torch.equal(I.voxel_coors(p, VS, RANGE), _torch_coors(p, [-80.0, -80.0, -2.0], VS))
    q = torch.cat([p, p[:, :2]], 1)[:, 1:4]          # rows 12 bytes into 20-byte rows: a strided view
    assert torch.equal(I.voxel_coors(q, VS, RANGE), _torch_coors(q.contiguous(), [-80.0, -80.0, -2.0], VS))


# ---- the integer mask --------------------------------------------------------------------------------------------------------

GRID = (7, 5, 16)
SIZES = (0, 1, 255, 256, 257, 5000)


def _coors(n, seed):
    """triples over the grid and two cells beyond it on every side: duplicates, hits, misses, equal out-of-grid triples"""
    g = torch.Generator().manual_seed(seed)
    c = torch.stack([torch.randint(-2, d + 2, (n,), generator=g) for d in GRID], 1).int()
    return c.to(DEV)


@pytest.mark.parametrize('n1', SIZES)
def test_mask_at_every_size(n1):
    from sst_amd import incremental as I
    for n2 in SIZES:
        c1, c2 = _coors(n1, 10 + n1), _coors(n2, 20 + n2)
        got = I.incremental_points_mask(c1, c2, GRID)
        assert got.dtype == torch.bool and torch.equal(got, R.incremental_points_mask(c1, c2)), (n1, n2)
        assert torch.equal(got, I.incremental_points_mask(c1, c2, GRID))


def test_mask_word_boundaries_and_outside_triples():
    from sst_amd import incremental as I
    # linear index (x * 5 + y) * 16 + z: cells 31 | 32 and 63 | 64 sit on both sides of a 32-bit word boundary
    base = torch.tensor([[0, 1, 15], [0, 4, 0], [-1, 0, 0], [7, 0, 0], [0, -1, 3], [0, 5, 3], [2, 2, -1], [2, 2, 16], [-1, 0, 0],
                         [2147483647, -2147483648, 5]], dtype=torch.int32, device=DEV)
    query = torch.tensor([[0, 1, 15], [0, 2, 0], [0, 3, 15], [0, 4, 0], [-1, 0, 0], [7, 0, 0], [0, -1, 3], [0, 5, 3], [2, 2, -1],
                          [2, 2, 16], [-1, 0, 1], [7, 0, 1], [2147483647, -2147483648, 5], [2147483647, -2147483648, 4],
                          [6, 4, 15], [0, 0, 0]], dtype=torch.int32, device=DEV)
    got = I.incremental_points_mask(base, query, GRID)
    want = [False, True, True, False, False, False, False, False, False, False, True, True, False, True, True, True]
    assert got.tolist() == want and torch.equal(got, R.incremental_points_mask(base, query))
    # nothing in the base: everything is new; nothing to ask: an empty mask
    assert bool(I.incremental_points_mask(base[:0], query, GRID).all())
    assert I.incremental_points_mask(base, query[:0], GRID).shape == (0,)


def _cloud(n, seed, cols=5, spread=(30.0, 30.0, 5.0), centre=(0.0, 0.0, 1.0)):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, cols, generator=g)
    p[:, :3] = (p[:, :3] - 0.5) * torch.tensor(spread) + torch.tensor(centre)
    return p.to(DEV)


@pytest.mark.parametrize('lower_bound', [False, True])
def test_points_level_mask(lower_bound):
    """find_delta_points_by_voxelization and the list form v3 (strict lower-bound filter on both sides): clouds that reach over
    the range on every side"""
    import sst_amd
    from sst_amd import incremental as I
    rng = [-10, -10, -2, 10, 10, 4]
    bases = [_cloud(n, 40 + i, spread=(26.0, 26.0, 9.0)) for i, n in enumerate((257, 0, 3000))]
    query = _cloud(5000, 50, spread=(26.0, 26.0, 9.0))
    query[:7, :3] = torch.tensor([-10.0, 0.0, 0.0], device=DEV)      # on the lower bound itself: not strictly above
    if lower_bound:
        want = R.find_delta_points_by_voxelization_list_v3(bases, query, VS, rng, return_mask=True)
        got = I.delta_mask(bases, query, VS, rng, lower_bound=True)
        _same(sst_amd.find_delta_points_by_voxelization_list_v3(bases, query, VS, rng), query[want])
    else:
        want = R.find_delta_points_by_voxelization(torch.cat(bases, 0), query, VS, rng, return_mask=True)
        got = I.delta_mask(bases, query, VS, rng)
        _same(sst_amd.find_delta_points_by_voxelization(torch.cat(bases, 0), query, VS, rng), query[want])
    assert torch.equal(got, want) and 0 < int(got.sum()) < got.numel()
    assert torch.equal(got, I.delta_mask(bases, query, VS, rng, lower_bound=lower_bound))


def test_two_queries_two_samples_no_leak():
    """queries 0 and 1 in one launch over two samples whose occupancy is mirrored: a base point of sample 0 must not mask a
    point of sample 1"""
    from sst_amd import incremental as I
    cfg = dict(voxel_size=VS, point_cloud_range=RANGE, num_previous_frames=3, num_base_frame=3, max_age=1, extra_width=0.5)
    left = dict(spread=(20.0, 20.0, 5.0), centre=(-15.0, 0.0, 1.0))
    right = dict(spread=(20.0, 20.0, 5.0), centre=(15.0, 0.0, 1.0))
    pts, finds = [], []
    for s, (pre, cur) in enumerate(((left, right), (right, left))):
        p = torch.cat([_cloud(700, 60 + s, **cur), _cloud(600, 62 + s, **pre), _cloud(500, 64 + s, **pre), _cloud(400, 66 + s, **cur)], 0)
        f = torch.cat([torch.full((n,), v) for n, v in ((700, 0), (600, -1), (500, -2), (400, -3))]).long().to(DEV)
        perm = torch.randperm(len(p), generator=torch.Generator().manual_seed(70 + s)).to(DEV)     # frames interleaved
        pts.append(p[perm].contiguous())
        finds.append(f[perm].contiguous())
    seeds = [[dict(gt_bboxes_3d=np.zeros((0, 7), np.float32), gt_labels_3d=np.zeros(0), scores=np.zeros(0, np.float32))] * 3] * 2
    outs, num_delta = I.generate_points(pts, finds, seeds, cfg, training=False)
    want, want_delta, segs = R.generate_points(pts, finds, seeds, cfg)
    assert num_delta == want_delta and min(num_delta) > 0
    for s in range(2):
        _same(outs[s], want[s], f'sample {s}')
        assert [n for n, _ in segs[s]] == ['fallback', 'delta0', 'delta1'] and all(len(r) for _, r in segs[s])
    # the leak would show: with both samples' bases in one bitmap fewer points of either are new
    both = R.find_delta_points_by_voxelization(torch.cat([p[f < 0] for p, f in zip(pts, finds)]), pts[1][finds[1] == 0], VS, RANGE)
    assert len(both) < dict(segs[1])['delta0'].size(0)
    again, _ = I.generate_points(pts, finds, seeds, cfg, training=False)
    for a, b in zip(outs, again):
        _same(a, b, 'second run')


# ---- crops and rows ----------------------------------------------------------------------------------------------------------

def _box(x, y, yaw=0.3, size=(1.0, 2.0, 1.0)):
    return [x, y, 0.0, size[0], size[1], size[2], yaw]


def _inside(box, n, seed):
    """n points well inside a box (within a tenth of its size of the centre)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, 3, generator=g) * 0.1 - 0.05
    p[:, 0] += box[0]
    p[:, 1] += box[1]
    p[:, 2] += box[2] + box[5] / 2
    return p


def _crop_scene(cap, cols):
    """sample 0: frame -1 with 33 boxes (box 0 empty, box 1 holding cap points, box 2 holding cap + 1, the others a few), frame -2
    with one box, frame -3 with none; sample 1: frame -1 with boxes and no points, frame -2 with two overlapping boxes (the first
    wins), frame -3 with a box nothing lies in"""
    def rows(xyz, frame, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.cat([xyz, torch.rand(len(xyz), cols - 3, generator=g)], 1), torch.full((len(xyz),), frame, dtype=torch.long)

    boxes0 = [_box(4.0 * (k % 8) - 14.0, 6.0 * (k // 8) - 10.0, yaw=0.2 * k) for k in range(33)]
    chunks = [rows(_inside(boxes0[1], cap, 1), -1, 2), rows(_inside(boxes0[2], cap + 1, 3), -1, 4)]
    for k in range(3, 33):
        chunks.append(rows(_inside(boxes0[k], 1 + k % 4, 100 + k), -1, 200 + k))
    lone = _box(30.0, 30.0, yaw=1.0, size=(2.0, 2.0, 2.0))
    chunks.append(rows(_inside(lone, 40, 5), -2, 6))
    chunks.append(rows(_inside(lone, 30, 7), -3, 8))                       # frame -3 has no box: nothing cropped there
    chunks.append(rows(_inside(lone, 25, 9), -1, 10))                      # frame -1 has no box there: not cropped
    chunks.append(rows(torch.rand(300, 3, generator=torch.Generator().manual_seed(11)) * 60 - 30, 0, 12))
    chunks.append(rows(torch.rand(200, 3, generator=torch.Generator().manual_seed(13)) * 60 - 30, -2, 14))
    p0, f0 = torch.cat([c[0] for c in chunks], 0), torch.cat([c[1] for c in chunks], 0)
    perm = torch.randperm(len(p0), generator=torch.Generator().manual_seed(15))
    p0, f0 = p0[perm], f0[perm]
    a, b = _box(-5.0, 5.0, yaw=0.0, size=(3.0, 3.0, 2.0)), _box(-4.5, 5.0, yaw=0.7, size=(3.0, 3.0, 2.0))
    far = _box(60.0, -60.0)
    chunks = [rows(_inside(a, 50, 16), -2, 17), rows(_inside(b, 50, 18), -2, 19),
              rows(torch.rand(400, 3, generator=torch.Generator().manual_seed(20)) * 40 - 20, 0, 21),
              rows(torch.rand(100, 3, generator=torch.Generator().manual_seed(22)) * 40 - 20, -3, 23)]
    p1, f1 = torch.cat([c[0] for c in chunks], 0), torch.cat([c[1] for c in chunks], 0)

    def seed(boxes):
        n = len(boxes)
        return dict(gt_bboxes_3d=torch.tensor(boxes, dtype=torch.float32).reshape(n, 7), gt_labels_3d=np.arange(n) % 3,
                    scores=np.ones(n, np.float32))
    seeds = [[seed(boxes0), seed([lone]), seed([])], [seed([a, b]), seed([a, b]), seed([far])]]
    return [p0.to(DEV), p1.to(DEV)], [f0.to(DEV), f1.to(DEV)], seeds, (a, b)


@pytest.mark.parametrize('cap', [128, 1])
@pytest.mark.parametrize('shuffle', [True, False])
@pytest.mark.parametrize('cols', [5, 4])
def test_crops_caps_and_rows(cap, shuffle, cols):
    from sst_amd import incremental as I
    pts, finds, seeds, (a, b) = _crop_scene(cap, cols)
    cfg = dict(voxel_size=VS, point_cloud_range=RANGE, num_previous_frames=3, crop_frames=3, num_base_frame=2, max_age=1,
               extra_width=dict([(0, 0.2), (1, 0.3), (2, 0.25)]), max_crop_points=cap, crop_shuffle=shuffle,
               center_noise=0.0, dim_noise=0.0, yaw_noise=0.0)
    total = sum(len(p) for p in pts)
    keys = torch.randint(0, 2 ** 32, (total,), generator=torch.Generator().manual_seed(31), dtype=torch.int64).to(DEV)
    keys[:40] = keys[40:80]                                                  # equal keys: the tie goes to the smaller index
    per_sample = [keys[:len(pts[0])], keys[len(pts[0]):]]
    outs, num_delta = I.generate_points(pts, finds, seeds, cfg, training=True, keys=keys)
    want, want_delta, segs = R.generate_points(pts, finds, seeds, cfg, keys=per_sample)
    assert num_delta == want_delta
    for s in range(2):
        assert outs[s].shape[1] == cols + 1
        _same(outs[s], want[s], f'sample {s}')
    names0, names1 = [n for n, _ in segs[0]], [n for n, _ in segs[1]]
    assert names0 == ['crop0', 'crop1', 'delta0', 'delta1'] and names1 == ['crop1', 'delta0', 'delta1']
    seg0 = dict(segs[0])
    # box 1 holds cap points and keeps them all, box 2 holds cap + 1 and loses one, the small boxes keep min(count, cap)
    expect = cap + cap + sum(min(1 + k % 4, cap) for k in range(3, 33))
    assert seg0['crop0'].size(0) == expect and seg0['crop1'].size(0) == min(40, cap)
    # the appended column: float(-i - 1) / 10 for the crops, 0 and -0.1 for the delta points, in the reference's segment order
    col = outs[0][:, -1]
    n0, n1, d0 = seg0['crop0'].size(0), seg0['crop1'].size(0), seg0['delta0'].size(0)
    assert bool((col[:n0] == float(-1) / 10).all()) and bool((col[n0:n0 + n1] == float(-2) / 10).all())
    assert bool((col[n0 + n1:n0 + n1 + d0] == 0).all()) and bool((col[n0 + n1 + d0:] == torch.tensor(-0.1).item()).all())
    assert seg0['delta1'].size(0) > 0 and d0 > 0
    # overlapping boxes: a point in both belongs to the first, so with cap 1 one row survives where both boxes hold points
    if cap == 1:
        import sst_amd
        fr = pts[1][finds[1] == -2]
        eb = R.enlarged(torch.tensor([a, b], device=DEV), cfg['extra_width'], torch.tensor([0.0, 1.0], device=DEV))
        first = sst_amd.points_in_boxes_gpu(fr[None, :, :3].contiguous(), eb[None])[0]
        assert dict(segs[1])['crop1'].size(0) == len(torch.unique(first[first >= 0]))
    again, _ = I.generate_points(pts, finds, seeds, cfg, training=True, keys=keys)
    for x, y in zip(outs, again):
        _same(x, y, 'second run')


def test_fallback_when_nothing_is_cropped():
    """a sample whose seed boxes hold no point gets rows 1 .. 199 of its previous-frame points with -num_pre_frames / 10"""
    from sst_amd import incremental as I
    pts = [_cloud(900, 80), _cloud(150, 81)]
    finds = [(torch.arange(900, device=DEV) % 3 - 2).long(), (torch.arange(150, device=DEV) % 3 - 2).long()]
    far = dict(gt_bboxes_3d=np.asarray([_box(70.0, 70.0)], np.float32), gt_labels_3d=np.zeros(1), scores=np.ones(1, np.float32))
    cfg = dict(voxel_size=VS, point_cloud_range=RANGE, num_previous_frames=2, crop_frames=2, extra_width=0.5, max_crop_points=16,
               crop_shuffle=False, disable_incremental=True)
    outs, num_delta = I.generate_points(pts, finds, [[far, far], [far, far]], cfg, training=False)
    want, _, segs = R.generate_points(pts, finds, [[far, far], [far, far]], cfg)
    assert num_delta == [] and [n for n, _ in segs[0]] == ['fallback']
    assert outs[0].shape == (199, 6) and outs[1].shape == (99, 6) and bool((outs[0][:, -1] == float(-2) / 10).all())
    for s in range(2):
        _same(outs[s], want[s])


def test_seed_crop_without_a_cap_and_empty_inputs():
    from sst_amd import incremental as I
    p = _cloud(3000, 90, spread=(10.0, 10.0, 2.0))
    boxes = torch.tensor([_box(0.0, 0.0, size=(4.0, 4.0, 3.0)), _box(3.0, 3.0, size=(4.0, 4.0, 3.0))], device=DEV)
    got = I.seed_crop(p, boxes)
    idx = R.crop_indices(p, boxes)
    _same(got, p[idx])
    assert 0 < len(got) < len(p)
    capped = I.seed_crop(p, boxes, 7)
    _same(capped, p[R.crop_indices(p, boxes, 7)])
    assert capped.size(0) == 14
    assert I.seed_crop(p[:0], boxes, 7).shape == (0, 5) and I.seed_crop(p, boxes[:0], 7).shape == (0, 5)


# ---- frame transform ---------------------------------------------------------------------------------------------------------

def _pose(seed):
    g = np.random.default_rng(seed)
    yaw, t = g.uniform(-3, 3), g.uniform(-200, 200, 3)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    m[:3, 3] = t
    return m.astype(np.float32)


@pytest.mark.parametrize('n_clouds', [1, 7])
def test_frame_transform_in_its_stated_order(n_clouds):
    from sst_amd import incremental as I
    sizes = [1, 64, 65, 0, 300, 257, 5][:n_clouds]
    cur = _pose(1)
    clouds = [_cloud(n, 100 + i, spread=(120.0, 120.0, 6.0)) for i, n in enumerate(sizes)]
    mats = [I.frame_matrix(_pose(10 + i), cur) for i in range(n_clouds)]
    outs = I.transform_clouds(clouds, mats)
    for c, m, o in zip(clouds, mats, outs):
        _same(o, R.frame_transform(c, m))
    # points_frame_transform: [n, 3] in, [n, 3] out; against float64 within a few ulp at these magnitudes
    for n in (1, 64, 65):
        p = _cloud(n, 120 + n, spread=(120.0, 120.0, 6.0))
        got = I.points_frame_transform(p[:, :3], _pose(12), cur)
        m64 = np.linalg.inv(cur.astype(np.float64)) @ _pose(12).astype(np.float64)
        ref = (np.concatenate([p[:, :3].cpu().numpy().astype(np.float64), np.ones((n, 1))], 1) @ m64.T)[:, :3]
        assert got.shape == (n, 3)
        # one fp32 rounding of the matrix (relative 2^-24 on terms up to ~400 m) and four roundings of the sums
        assert float(np.abs(got.cpu().numpy() - ref).max()) <= 8 * 400 * 2.0 ** -24


# ---- the whole stage ---------------------------------------------------------------------------------------------------------

def test_whole_stage_of_a_batch():
    """batch of 2, three previous frames, about 2 000 points per frame, the shipped settings"""
    from sst_amd import incremental as I
    cfg = dict(voxel_size=VS, point_cloud_range=RANGE, center_noise=0.0, dim_noise=0.0, yaw_noise=0.0, extra_width=1.0,
               num_previous_frames=3, crop_frames=3, max_crop_points=128, crop_shuffle=True, max_age=1, num_base_frame=2)
    pts, finds, seeds = [], [], []
    for s in range(2):
        n = 2000 - 37 * s
        p = torch.cat([_cloud(n, 130 + 4 * s + f, spread=(60.0, 60.0, 5.0)) for f in range(4)], 0)
        f = torch.arange(4).repeat_interleave(n).neg().long().to(DEV)
        g = np.random.default_rng(140 + s)
        frames = []
        for i in range(3):
            nb = 12 - 5 * i
            b = np.concatenate([g.uniform(-25, 25, (nb, 2)), g.uniform(-1, 0, (nb, 1)), g.uniform(2, 8, (nb, 3)), g.uniform(-3, 3, (nb, 1))], 1)
            frames.append(dict(gt_bboxes_3d=b.astype(np.float32), gt_labels_3d=g.integers(0, 3, nb), scores=g.uniform(0, 1, nb).astype(np.float32)))
        pts.append(p)
        finds.append(f)
        seeds.append(frames)
    total = sum(len(p) for p in pts)
    keys = torch.randint(0, 2 ** 32, (total,), generator=torch.Generator().manual_seed(150), dtype=torch.int64).to(DEV)
    outs, num_delta = I.generate_points(pts, finds, seeds, cfg, training=True, keys=keys)
    want, want_delta, segs = R.generate_points(pts, finds, seeds, cfg, keys=[keys[:len(pts[0])], keys[len(pts[0]):]])
    assert num_delta == want_delta
    for s in range(2):
        assert [n for n, _ in segs[s]] == ['crop0', 'crop1', 'crop2', 'delta0', 'delta1']
        assert all(len(r) > 0 for _, r in segs[s])
        _same(outs[s], want[s], f'sample {s}')
    assert outs[0].data_ptr() + outs[0].numel() * 4 == outs[1].data_ptr()      # views of one buffer
    again, _ = I.generate_points(pts, finds, seeds, cfg, training=True, keys=keys)
    for a, b in zip(outs, again):
        _same(a, b, 'second run')
    # the keys default to a draw on the device: the crops change, the delta points do not
    rand, rand_delta = I.generate_points(pts, finds, seeds, cfg, training=True)
    assert rand_delta == num_delta and [len(r) for r in rand] == [len(o) for o in outs]

"""Training augmentation of points and boxes on the device (csrc/augment.hip): the ``train_pipeline`` of a
shipped config between ``db_sampler.sample_all`` and the collate.

Reference: mmdet3d/datasets/pipelines/transforms_3d.py - ``ObjectSample`` (:238-352, the part after ``sample_all``),
``RandomFlip3D`` (:20-186), ``GlobalRotScaleTrans`` (:520-676), ``PointShuffle`` (:679-700), ``ObjectRangeFilter`` (:745-790),
``PointsRangeFilter`` (:793-851), ``ObjectNameFilter`` (:854-889), ``NormalizePoints`` (loading.py:1026-1050) and
``MultiScaleFlipAug3D`` (test_time_aug.py) around them.  The reference runs them per sample in data-loader workers; here the
random numbers are drawn on the host (``draw_params``, the reference's ``np.random`` calls in its source order), the database
sampler stays on the host, and everything per point and per box is three launches and a sort for the whole batch.

What stays on the host: file loading, ``DataBaseSampler`` (pickles, files, its greedy collision test), ``ObjectNameFilter``
(a comparison of a few labels) and the six plane equations of each pasted box.

Deviations, all stated where they arise:
  * the plane equations are formed from the pasted boxes converted to float32 (``box_planes``); the reference computes them in
    the dtype the database pickles carry - if that is float64 its plane tests run in float64 and a point within rounding
    distance of a face may fall the other way;
  * a row with a NaN coordinate is dropped by the range comparisons (every comparison with a NaN is false); it is also never
    inside a pasted box (the reference's ``sign >= 0`` test would call it inside and remove it: the row is gone either way when
    a range filter is in the chain; without one the comparisons against +-inf still drop it);
  * ``PointShuffle`` is a stable sort by a counter-based hash (splitmix64 of the seed, the sample and the row's index), not
    ``torch.randperm``: the order is reproducible from ``params.seed`` alone;
  * the outputs are views of buffers this object owns: they are valid until its next call.

There is no eager fall-back: ``__call__`` needs a GPU."""
import ctypes

import numpy as np
import torch

from . import _lib

WHERE = 'sst_amd.augment'
MAX_COLS = 8
_BLOCK = 256

PARAMS_DTYPE = np.dtype([('flip_h', '<i4'), ('flip_v', '<i4'), ('rotate', '<i4'), ('shuffle', '<i4'), ('cos', '<f4'),
                         ('sin', '<f4'), ('scale', '<f4'), ('angle', '<f4'), ('trans', '<f4', (3,)), ('reserved', '<f4'),
                         ('range', '<f4', (6,)), ('seed', '<u8')])
assert PARAMS_DTYPE.itemsize == ctypes.sizeof(_lib.AugmentParams) == 80

_SKIPPED = ('DefaultFormatBundle3D', 'DefaultFormatBundle', 'Collect3D')
# position of a step in the order the kernels apply, and the streams it acts on (points, boxes): a box-only step and a
# point-only step commute (fsdv2_nusc puts ObjectRangeFilter behind PointShuffle)
_ORDER = {'ObjectSample': (0, 'pb'), 'RandomFlip3D': (1, 'pb'), 'GlobalRotScaleTrans': (2, 'pb'), 'PointsRangeFilter': (3, 'p'),
          'ObjectRangeFilter': (3, 'b'), 'PointShuffle': (4, 'p')}


def _refuse(name, why):
    raise NotImplementedError(f'{WHERE}: {name} is not supported ({why})')


def box_planes(boxes):
    """The six face planes (a, b, c, d), normals pointing inwards, of LiDAR boxes [S, >= 7] -> float32 [S, 6, 4]: a numpy
    restatement of ``center_to_corner_box3d(origin=(0.5, 0.5, 0), axis=2)`` -> ``corner_to_surfaces_3d`` -> ``surface_equ_3d``
    (mmdet3d/core/bbox/box_np_ops.py:205-234, :403-422, :693-714) as ``points_in_rbbox`` (:425-445) chains them.  The boxes are
    converted to float32 first (see the module docstring)."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, np.shape(boxes)[-1] if np.ndim(boxes) == 2 else 7)[:, :7]
    s = b.shape[0]
    if s == 0:
        return np.zeros((0, 6, 4), np.float32)
    unit = np.stack(np.unravel_index(np.arange(8), [2, 2, 2]), axis=1).astype(np.float32)[[0, 1, 3, 2, 4, 5, 7, 6]]
    unit = unit - np.array((0.5, 0.5, 0), dtype=np.float32)
    corners = b[:, 3:6].reshape(-1, 1, 3) * unit.reshape(1, 8, 3)
    sin, cos = np.sin(b[:, 6]), np.cos(b[:, 6])
    ones, zeros = np.ones_like(cos), np.zeros_like(cos)
    rot_t = np.stack([[cos, -sin, zeros], [sin, cos, zeros], [zeros, zeros, ones]])
    corners = np.einsum('aij,jka->aik', corners, rot_t)
    corners += b[:, :3].reshape(-1, 1, 3)
    c = corners
    faces = np.array([[c[:, 0], c[:, 1], c[:, 2], c[:, 3]], [c[:, 7], c[:, 6], c[:, 5], c[:, 4]],
                      [c[:, 0], c[:, 3], c[:, 7], c[:, 4]], [c[:, 1], c[:, 5], c[:, 6], c[:, 2]],
                      [c[:, 0], c[:, 4], c[:, 5], c[:, 1]], [c[:, 3], c[:, 2], c[:, 6], c[:, 7]]]).transpose([2, 0, 1, 3])
    edge = faces[:, :, :2, :] - faces[:, :, 1:3, :]
    normal = np.cross(edge[:, :, 0, :], edge[:, :, 1, :])
    d = np.einsum('aij, aij->ai', normal, faces[:, :, 0, :])
    return np.concatenate([normal, -d[..., None]], axis=-1).astype(np.float32)


class AugmentParams(object):
    """What one call applies, per sample: ``flip_h`` / ``flip_v`` bool [B]; ``angle``, ``scale`` float64 [B] and ``trans``
    float64 [B, 3] as drawn (the kernels get them rounded to float32 once; ``cos`` / ``sin`` are ``torch.cos`` / ``torch.sin``
    of the float32 angle on the CPU, as lidar_box3d.py:158-168 computes them); ``seed`` uint64 [B].  A plain record: fill it by
    hand to replay a batch."""

    def __init__(self, batch_size):
        self.flip_h = np.zeros(batch_size, bool)
        self.flip_v = np.zeros(batch_size, bool)
        self.angle = np.zeros(batch_size, np.float64)
        self.scale = np.ones(batch_size, np.float64)
        self.trans = np.zeros((batch_size, 3), np.float64)
        self.seed = np.zeros(batch_size, np.uint64)

    def __len__(self):
        return len(self.seed)

    def records(self, rotate, point_range, shuffle):
        """-> the kernels' records (PARAMS_DTYPE [B]); ``rotate`` bool [B]: is the sample rotated at all (the empty-box quirk)"""
        rec = np.zeros(len(self), PARAMS_DTYPE)
        angle = torch.from_numpy(self.angle.astype(np.float32))
        rec['flip_h'], rec['flip_v'], rec['rotate'], rec['shuffle'] = self.flip_h, self.flip_v, rotate, bool(shuffle)
        rec['cos'], rec['sin'], rec['angle'] = torch.cos(angle).numpy(), torch.sin(angle).numpy(), angle.numpy()
        rec['scale'], rec['trans'] = self.scale.astype(np.float32), self.trans.astype(np.float32)
        rec['range'] = np.asarray(point_range, np.float32)[None]
        rec['seed'] = self.seed
        return rec


class TrainAugment(object):
    """The augmentation steps of a shipped ``train_pipeline`` / ``test_pipeline`` (see ``from_pipeline``) as one device call."""

    def __init__(self):
        self.object_sample = False
        self.flip = None              # (ratio_h, ratio_v), or 'off' inside MultiScaleFlipAug3D(flip=False)
        self.rst = None               # (rot_range, scale_ratio_range, translation_std)
        self.fixed_scale = None       # MultiScaleFlipAug3D's pts_scale_ratio: pcd_scale_factor is set, nothing is drawn
        self.point_range = None
        self.box_range = None
        self.shuffle = False
        self.name_filter = None       # (number of classes, is it applied before GlobalRotScaleTrans)
        self.norm = None              # (dims, mean, std) of NormalizePoints
        self.flip_before_rst = False
        self._buf = {}

    # ------------------------------------------------------------------ the pipeline's text
    @classmethod
    def from_pipeline(cls, pipeline):
        """``pipeline``: the list of dicts of a shipped ``train_pipeline`` or ``test_pipeline``.  Accepted: ObjectSample,
        RandomFlip3D(sync_2d=False), GlobalRotScaleTrans, PointsRangeFilter, ObjectRangeFilter, PointShuffle, ObjectNameFilter,
        NormalizePoints and MultiScaleFlipAug3D(flip=False, one scale) around accepted ones; ``Load*``, ``DefaultFormatBundle3D``
        and ``Collect3D`` are skipped (loading and collation stay where they are).  Everything else raises NotImplementedError
        with the transform's name."""
        self = cls()
        self._parse(list(pipeline), inside_tta=False)
        if self.point_range is not None and self.box_range is not None and \
                not np.array_equal(self.point_range, self.box_range):
            _refuse('ObjectRangeFilter', 'its point_cloud_range differs from PointsRangeFilter\'s: the kernels take one range '
                                         'per sample')
        return self

    def _parse(self, pipeline, inside_tta):
        last = {'p': -1, 'b': -1}
        for step in pipeline:
            step = dict(step)
            name = step.pop('type')
            if name.startswith('Load') or name in _SKIPPED:
                continue
            if name.startswith('Tracklet'):
                _refuse(name, 'the tracklet pipelines of the CTRL configs are not point-cloud augmentation')
            if name in _ORDER:
                # the kernels apply removal, flips, rotation / scale / translation, the range and the shuffle in this order
                pos, streams = _ORDER[name]
                if any(pos < last[k] for k in streams) and not (inside_tta and name == 'RandomFlip3D'):
                    _refuse(name, 'it comes after a step the kernels apply later: the order is ObjectSample, RandomFlip3D, '
                                  'GlobalRotScaleTrans, the range filters, PointShuffle')
                for k in streams:
                    last[k] = max(last[k], pos)
            if name == 'ObjectSample':
                if step.get('sample_2d', False):
                    _refuse('ObjectSample(sample_2d=True)', 'images are not handled')
                self.object_sample = True
            elif name == 'RandomFlip3D':
                if inside_tta:
                    self.flip = 'off'      # MultiScaleFlipAug3D(flip=False) has set flip = False: nothing is drawn or flipped
                elif step.get('sync_2d', True):
                    _refuse('RandomFlip3D(sync_2d=True)', 'the flip would follow an image flip drawn by mmdet\'s RandomFlip')
                else:
                    self.flip = (float(step.get('flip_ratio_bev_horizontal', 0.0)), float(step.get('flip_ratio_bev_vertical', 0.0)))
                self.flip_before_rst = self.rst is None
            elif name == 'GlobalRotScaleTrans':
                if step.get('shift_height', False):
                    _refuse('GlobalRotScaleTrans(shift_height=True)', 'no height attribute column is scaled')
                rot = step.get('rot_range', [-0.78539816, 0.78539816])
                rot = [-rot, rot] if not isinstance(rot, (list, tuple, np.ndarray)) else list(rot)
                std = step.get('translation_std', [0, 0, 0])
                std = [std] * 3 if not isinstance(std, (list, tuple, np.ndarray)) else list(std)
                self.rst = (rot, list(step.get('scale_ratio_range', [0.95, 1.05])), std)
            elif name == 'PointsRangeFilter':
                self.point_range = np.array(step['point_cloud_range'], dtype=np.float32)
            elif name == 'ObjectRangeFilter':
                self.box_range = np.array(step['point_cloud_range'], dtype=np.float32)
            elif name == 'PointShuffle':
                self.shuffle = True
            elif name == 'ObjectNameFilter':
                self.name_filter = (len(step['classes']), self.rst is None)
            elif name == 'NormalizePoints':
                dims, mean, std = step.get('dims', [3]), step.get('mean', [0]), step.get('std', [255])
                if min(dims) < 3 or max(dims) >= MAX_COLS or not len(dims) == len(mean) == len(std):
                    _refuse('NormalizePoints', f'dims {dims}: attribute columns 3..{MAX_COLS - 1} with one mean and std each')
                self.norm = (list(dims), [float(m) for m in mean], [float(s) for s in std])
            elif name == 'MultiScaleFlipAug3D':
                if inside_tta:
                    _refuse('MultiScaleFlipAug3D', 'nested')
                ratio = step.get('pts_scale_ratio', 1)
                ratio = list(ratio) if isinstance(ratio, (list, tuple)) else [ratio]
                if step.get('flip', False) or step.get('pcd_horizontal_flip', False) or step.get('pcd_vertical_flip', False):
                    _refuse('MultiScaleFlipAug3D(flip=True)', 'test-time flip augmentation makes several outputs per sample')
                if len(ratio) != 1:
                    _refuse('MultiScaleFlipAug3D', f'pts_scale_ratio {ratio}: several outputs per sample')
                self.fixed_scale = float(ratio[0])
                self._parse(step.get('transforms', []), inside_tta=True)
            else:
                _refuse(name, 'not one of the transforms this module restates' if name not in (
                    'ObjectNoise', 'RandomJitterPoints', 'BackgroundPointsFilter', 'RandomPointDrop')
                    else 'no shipped config of the SST / FSD families uses it')

    # ------------------------------------------------------------------ the random numbers
    def draw_params(self, batch_size, rng=np.random):
        """The reference's draws, per sample in its source order: ``rand()`` for the horizontal and ``rand()`` for the vertical
        flip (transforms_3d.py:149-155), ``uniform(*rot_range)`` (:600), ``uniform(*scale_ratio_range)`` (:657),
        ``normal(scale=translation_std, size=3)`` (:577).  The 64-bit shuffle seeds (two ``randint(0, 2**32)`` each) are drawn
        AFTER the last sample's transform draws, so that the stream of the transform draws is the one the reference's
        transforms consume when they run sample after sample (its PointShuffle draws from torch's generator, not from
        ``np.random``).  ``rng``: ``np.random`` or a ``RandomState``."""
        p = AugmentParams(batch_size)
        for i in range(batch_size):
            if self.flip is not None and self.flip != 'off':
                p.flip_h[i] = rng.rand() < self.flip[0]
                p.flip_v[i] = rng.rand() < self.flip[1]
            if self.rst is not None:
                rot, scale, std = self.rst
                p.angle[i] = rng.uniform(rot[0], rot[1])
                p.scale[i] = self.fixed_scale if self.fixed_scale is not None else rng.uniform(scale[0], scale[1])
                p.trans[i] = rng.normal(scale=np.array(std, dtype=np.float32), size=3).T
        for i in range(batch_size):
            p.seed[i] = (int(rng.randint(0, 2 ** 32)) << 32) | int(rng.randint(0, 2 ** 32))
        return p

    # ------------------------------------------------------------------ host-side assembly
    @staticmethod
    def _np(t, dtype):
        t = getattr(t, 'tensor', t)
        if torch.is_tensor(t):
            t = t.detach().cpu().numpy()
        return np.ascontiguousarray(np.asarray(t), dtype=dtype)

    def assemble(self, gt_bboxes_3d, gt_labels_3d, sampled, batch_size):
        """ObjectSample's concatenations (transforms_3d.py:314-330) and ObjectNameFilter on the host -> per sample (boxes float32
        [G, D], labels int64 [G], pasted boxes [S, 7] or None, rotate: is the sample rotated at all)."""
        out = []
        for i in range(batch_size):
            if gt_bboxes_3d is None:
                # test mode: no box field when GlobalRotScaleTrans runs -> the points are rotated (:603-606); after RandomFlip3D the
                # field 'empty_box3d' exists (:107-110) and its empty tensor keeps the points from being rotated (:609-614)
                out.append((None, None, None, not (self.flip is not None and self.flip_before_rst)))
                continue
            boxes = self._np(gt_bboxes_3d[i], np.float32)
            boxes = boxes.reshape(-1, boxes.shape[-1] if boxes.ndim == 2 else 7)
            labels = self._np(gt_labels_3d[i], np.int64).reshape(-1)
            if boxes.shape[1] not in (7, 9):
                raise RuntimeError(f'{WHERE}: gt_bboxes_3d must have 7 or 9 columns, got {boxes.shape[1]}')
            pasted = None
            s = sampled[i] if sampled is not None else None
            if s is not None:
                if not self.object_sample:
                    raise RuntimeError(f'{WHERE}: sampled objects were given but the pipeline has no ObjectSample')
                pasted = self._np(s['gt_bboxes_3d'], np.float32)
                pasted = pasted.reshape(-1, pasted.shape[-1] if pasted.ndim == 2 else 7)
                if boxes.shape[1] == 9 and pasted.shape[1] == 7:
                    # transforms_3d.py:321-326 pads the pasted boxes with three zero columns and the ground truth with a flag column
                    # of ones: 10 columns.  Reached only with Waymo velocity boxes, which no shipped config of the five families loads.
                    _refuse('ObjectSample with 9-column ground truth and 7-column pasted boxes',
                            'the reference pads both to 10 columns (transforms_3d.py:321-326), reached only with Waymo velocity '
                            'boxes, which no shipped SST / FSD / FSDv2 / CTRL / FSD++ config loads')
                if pasted.shape[1] != boxes.shape[1]:
                    raise RuntimeError(f'{WHERE}: pasted boxes have {pasted.shape[1]} columns, ground truth {boxes.shape[1]}')
                boxes = np.concatenate([boxes, pasted])
                labels = np.concatenate([labels, self._np(s['gt_labels_3d'], np.int64).reshape(-1)])
            count_at_rotation = boxes.shape[0]
            if self.name_filter is not None:
                keep = (labels >= 0) & (labels < self.name_filter[0])        # ObjectNameFilter: label in range(len(classes))
                boxes, labels = boxes[keep], labels[keep]
                if self.name_filter[1]:
                    count_at_rotation = boxes.shape[0]
            # the reference rotates points and boxes only inside `if len(input_dict[key].tensor) != 0` (transforms_3d.py:609-614):
            # a sample whose box tensor is empty is NOT rotated at all, points included
            out.append((boxes, labels, pasted, count_at_rotation > 0))
        return out

    def records(self, params, asm):
        """the kernels' records of a batch: ``params`` with the pipeline's range and shuffle flag and, per sample of ``asm``
        (``assemble``), whether it is rotated at all"""
        rng6 = self.point_range if self.point_range is not None else self.box_range
        if rng6 is None:
            rng6 = np.array([-np.inf] * 3 + [np.inf] * 3, np.float32)
        return params.records(np.array([bool(a[3]) and self.rst is not None for a in asm]), rng6, self.shuffle)

    # ------------------------------------------------------------------ buffers (no allocation after the first call of a size)
    def _buffer(self, key, nbytes_or_shape, dtype, dev, pin=False):
        shape = (int(nbytes_or_shape),) if not isinstance(nbytes_or_shape, tuple) else nbytes_or_shape
        need = int(np.prod(shape))
        cur = self._buf.get(key)
        if cur is None or cur.numel() < need or cur.dtype != dtype or (not pin and cur.device != dev):
            grow = max(need, 1)
            cur = torch.empty(grow, dtype=dtype, pin_memory=True) if pin else torch.empty(grow, dtype=dtype, device=dev)
            self._buf[key] = cur
        return cur[:need].view(shape)

    # ------------------------------------------------------------------ the call
    def __call__(self, points, gt_bboxes_3d=None, gt_labels_3d=None, sampled=None, seed_boxes=None, params=None):
        """points: list of [N_i, C] float32 host or device tensors (3 <= C <= 8; further per-point values, such as the frame
        index of the multi-frame loaders, ride along as columns).  gt_bboxes_3d / gt_labels_3d: per sample [G_i, 7 | 9] and
        int64 [G_i] (tensors, arrays or box objects with ``.tensor``), or None (test pipelines).  sampled: per sample None or
        what ``db_sampler.sample_all`` returned (``gt_bboxes_3d``, ``gt_labels_3d``, ``points``).  seed_boxes: per sample a
        list of [K, 7 | 9] box sets (the ``seed_info`` boxes of the FSD++ loaders): transformed, never filtered.  params: an
        ``AugmentParams`` (default: ``draw_params(len(points))``).

        -> dict(points: per-sample VIEWS of the packed output, points_packed [M, C], offsets (list, B + 1), gt_bboxes_3d,
        gt_labels_3d: lists of device tensors as ``forward_train`` of sst_amd.detectors takes them (None without boxes),
        seed_boxes, params, and per sample what the reference records: pcd_horizontal_flip, pcd_vertical_flip, pcd_rotation
        (rot_mat_T, None where the sample was not rotated), pcd_scale_factor, pcd_trans).  One host read (the counts)."""
        if not torch.cuda.is_available():
            raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
        batch = len(points)
        if batch < 1:
            raise RuntimeError(f'{WHERE}: an empty batch')
        if batch >= 2 ** 31:
            raise NotImplementedError(f'{WHERE}: {batch} samples; the sample field of the sort key holds 2^31 - 1')
        pts = [getattr(p, 'tensor', p) for p in points]
        cols = int(pts[0].shape[1])
        if cols < 3 or cols > MAX_COLS:
            raise NotImplementedError(f'{WHERE}: {cols} point columns; the kernels take 3 to {MAX_COLS} (SST_AUG_MAX_COLS)')
        on_device = all(torch.is_tensor(p) and p.is_cuda for p in pts)
        if not on_device:
            pts = [self._np(p, np.float32) for p in pts]
        for p in pts:
            if p.ndim != 2 or p.shape[1] != cols or (on_device and p.dtype != torch.float32):
                raise RuntimeError(f'{WHERE}: points must be float32 [N, {cols}], got {tuple(p.shape)}')
        dev = pts[0].device if on_device else torch.device('cuda', torch.cuda.current_device())
        if params is None:
            params = self.draw_params(batch)
        if len(params) != batch:
            raise RuntimeError(f'{WHERE}: params for {len(params)} samples, {batch} given')
        asm = self.assemble(gt_bboxes_3d, gt_labels_3d, sampled, batch)
        with_boxes = gt_bboxes_3d is not None
        box_cols = asm[0][0].shape[1] if with_boxes else 7
        if with_boxes and any(a[0].shape[1] != box_cols for a in asm):
            raise RuntimeError(f'{WHERE}: the samples of a batch must have the same number of box columns')
        rec = self.records(params, asm)

        pasted_pts = [self._np(sampled[i]['points'], np.float32).reshape(-1, cols) if (sampled is not None and sampled[i] is not None)
                      else np.zeros((0, cols), np.float32) for i in range(batch)]
        planes = [box_planes(a[2]) if a[2] is not None else np.zeros((0, 6, 4), np.float32) for a in asm]
        n_pasted = np.array([p.shape[0] for p in pasted_pts], np.int32)
        rows = np.array([int(p.shape[0]) for p in pts], np.int64) + n_pasted
        row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        blk_off = np.concatenate([[0], np.cumsum((rows + _BLOCK - 1) // _BLOCK)]).astype(np.int32)
        plane_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in planes])]).astype(np.int32)
        n_total = int(row_off[-1])
        if n_total > 2 ** 31 - 1 - _BLOCK:
            raise NotImplementedError(f'{WHERE}: {n_total} rows in a batch; the kernels index 2^31 - 257')
        boxes = [a[0] for a in asm] if with_boxes else []
        box_off = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])]).astype(np.int32) if with_boxes \
            else np.zeros(batch + 1, np.int32)
        seeds = []
        if seed_boxes is not None:
            n_sets = max(len(s) for s in seed_boxes)
            for k in range(n_sets):
                sets = [self._np(s[k], np.float32).reshape(-1, box_cols) if k < len(s) else np.zeros((0, box_cols), np.float32)
                        for s in seed_boxes]
                seeds.append((sets, np.concatenate([[0], np.cumsum([b.shape[0] for b in sets])]).astype(np.int32)))

        # one host buffer, one copy: [points of the batch | offsets | records | planes | boxes | labels | seed boxes]
        parts, cursor = [], [0]

        def place(arr):
            arr = np.ascontiguousarray(arr)
            at = cursor[0]
            parts.append((at, arr))
            cursor[0] = (at + max(arr.nbytes, 1) + 255) // 256 * 256
            return at

        at_points = None
        if not on_device:
            at_points = cursor[0]
            for i in range(batch):
                parts.append((at_points + int(row_off[i]) * cols * 4, pasted_pts[i]))
                parts.append((at_points + (int(row_off[i]) + int(n_pasted[i])) * cols * 4, pts[i]))
            cursor[0] = (at_points + max(n_total * cols * 4, 1) + 255) // 256 * 256
        else:
            at_pasted = place(np.concatenate(pasted_pts))
        at_row, at_np, at_blk, at_pl = place(row_off), place(n_pasted), place(blk_off), place(plane_off)
        at_rec, at_planes, at_boff = place(rec), place(np.concatenate(planes)), place(box_off)
        at_boxes = place(np.concatenate(boxes)) if with_boxes else None
        at_labels = place(np.concatenate([a[1] for a in asm])) if with_boxes else None
        at_seeds = [(place(np.concatenate(sets)), place(off)) for sets, off in seeds]
        nbytes = cursor[0]
        host = self._buffer('host', nbytes, torch.uint8, None, pin=True)
        host_np = host.numpy()
        for at, arr in parts:
            if arr.nbytes:
                host_np[at:at + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        stage = self._buffer('stage', nbytes, torch.uint8, dev)
        stage.copy_(host, non_blocking=True)
        base = stage.data_ptr()
        at = lambda off: ctypes.c_void_p(base + off)

        if on_device:
            packed = self._buffer('points_in', (n_total, cols), torch.float32, dev)
            staged = stage[at_pasted:at_pasted + int(n_pasted.sum()) * cols * 4].view(torch.float32).view(int(n_pasted.sum()), cols)
            done = 0
            for i in range(batch):
                r0, k = int(row_off[i]), int(n_pasted[i])
                packed[r0:r0 + k].copy_(staged[done:done + k])
                packed[r0 + k:int(row_off[i + 1])].copy_(pts[i])
                done += k
            points_ptr = _lib.ptr(packed)
        else:
            points_ptr = at(at_points)

        n_counts = batch * (2 + len(seeds))
        counts = self._buffer('counts', n_counts, torch.int32, dev)
        out = self._buffer('out', (n_total, cols), torch.float32, dev)
        lib = _lib.load()
        ws_bytes = lib.sst_augment_workspace_bytes(n_total, batch)
        ws = self._buffer('workspace', max(ws_bytes, 256), torch.uint8, dev)
        a = _lib.AugmentArgs()
        a.points, a.row_offsets, a.n_pasted, a.block_offsets = points_ptr, at(at_row), at(at_np), at(at_blk)
        a.params, a.planes, a.plane_offsets = at(at_rec), at(at_planes), at(at_pl)
        a.out, a.counts, a.workspace, a.workspace_bytes = _lib.ptr(out), _lib.ptr(counts), _lib.ptr(ws), ws.numel()
        a.n_total, a.batch, a.cols, a.n_blocks, a.n_planes = n_total, batch, cols, int(blk_off[-1]), int(plane_off[-1])
        if self.norm is not None:
            for k, m, s in zip(*self.norm):
                if k < cols:
                    a.norm_mask |= 1 << k
                    a.norm_mean[k], a.norm_std[k] = m, s
        _lib.check(lib.sst_augment_points_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_augment_points_f32')

        boxes_out = labels_out = None
        seed_out = []
        if with_boxes or seeds:
            b = _lib.AugmentBoxArgs()
            b.params, b.batch, b.cols = at(at_rec), batch, box_cols
        if with_boxes:
            n_boxes = int(box_off[-1])
            boxes_out = self._buffer('boxes_out', (n_boxes, box_cols), torch.float32, dev)
            labels_out = self._buffer('labels_out', n_boxes, torch.int64, dev)
            b.boxes, b.labels, b.box_offsets = at(at_boxes), at(at_labels), at(at_boff)
            b.boxes_out, b.labels_out = _lib.ptr(boxes_out), _lib.ptr(labels_out)
            b.counts = ctypes.c_void_p(counts.data_ptr() + 4 * batch)
            b.n_boxes, b.filter, b.always_rotate = n_boxes, int(self.box_range is not None), 0
            _lib.check(lib.sst_augment_boxes_f32(ctypes.byref(b), _lib.stream_ptr()), 'sst_augment_boxes_f32')
        for k, ((sets, off), (at_b, at_o)) in enumerate(zip(seeds, at_seeds)):
            n_boxes = int(off[-1])
            so = self._buffer(f'seed_out{k}', (n_boxes, box_cols), torch.float32, dev)
            b.boxes, b.labels, b.box_offsets, b.boxes_out, b.labels_out = at(at_b), None, at(at_o), _lib.ptr(so), None
            b.counts = ctypes.c_void_p(counts.data_ptr() + 4 * batch * (2 + k))
            # seed['gt_bboxes_3d'].rotate is guarded by the seed set's own length (transforms_3d.py:616-619), not the ground truth's
            b.n_boxes, b.filter, b.always_rotate = n_boxes, 0, int(self.rst is not None)
            _lib.check(lib.sst_augment_boxes_f32(ctypes.byref(b), _lib.stream_ptr()), 'sst_augment_boxes_f32')
            seed_out.append((so, off))

        got = counts[:2 * batch].tolist()                                       # the one host read of the call
        offsets = [0]
        for c in got[:batch]:
            offsets.append(offsets[-1] + c)
        result = dict(points=[out[offsets[i]:offsets[i + 1]] for i in range(batch)], points_packed=out[:offsets[-1]],
                      offsets=offsets, params=params, gt_bboxes_3d=None, gt_labels_3d=None, seed_boxes=None)
        if with_boxes:
            result['gt_bboxes_3d'] = [boxes_out[int(box_off[i]):int(box_off[i]) + got[batch + i]] for i in range(batch)]
            result['gt_labels_3d'] = [labels_out[int(box_off[i]):int(box_off[i]) + got[batch + i]] for i in range(batch)]
        if seeds:
            result['seed_boxes'] = [[so[int(off[i]):int(off[i + 1])] for so, off in seed_out][:len(seed_boxes[i])]
                                    for i in range(batch)]
        result['pcd_horizontal_flip'] = [bool(v) for v in params.flip_h]
        result['pcd_vertical_flip'] = [bool(v) for v in params.flip_v]
        result['pcd_scale_factor'] = [float(v) for v in params.scale]
        result['pcd_trans'] = [params.trans[i].copy() for i in range(batch)]
        result['pcd_rotation'] = [rot_mat_t(rec['cos'][i], rec['sin'][i]) if rec['rotate'][i] else None
                                  for i in range(batch)]
        return result


def rot_mat_t(cos, sin):
    """``rot_mat_T`` of lidar_box3d.py:166-168 from the float32 cosine and sine"""
    return torch.tensor([[cos, -sin, 0], [sin, cos, 0], [0, 0, 1]], dtype=torch.float32)

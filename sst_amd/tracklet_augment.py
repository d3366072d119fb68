"""The ``train_pipeline`` / ``test_pipeline`` of a shipped CTRL config between the file load and the collate, for a whole batch
of tracklets on the device (csrc/tracklet_augment.hip) - the sibling of sst_amd.augment for the tracklet family.

Reference: mmdet3d/datasets/pipelines/tracklet_pipelines.py - ``TrackletCutting`` (:105-138), ``TrackletPoseTransform``
(:149-208), ``TrackletNoise`` (:550-562 with lidar_tracklet.py:495-546), ``PointDecoration`` (:455-506), ``TrackletRandomFlip``
(:414-439), ``TrackletGlobalRotScaleTrans`` (:329-355), then ``PointsRangeFilter`` and ``PointShuffle`` of transforms_3d.py.  The
reference runs them per sample in data-loader workers, frame by frame; here the random numbers are drawn on the host
(``draw_params``: the reference's ``np.random`` and ``torch.rand`` calls in its source order), everything per BOX runs on the host
once per batch (a few hundred rows: the cut, the frame matrices, the noise, the decoration values), and everything per POINT is
one packed copy, two launches and a sort; the boxes then go through the box kernel of sst_amd.augment.

Quirks of the reference that are reproduced:
  * the frame indices of a cut tracklet keep the values they had before the cut: they start at ``head`` (:126-127);
  * ``TrackletCutting`` draws its first ``np.random.rand()`` only when ``len(tracklet) >= min_length`` (a short-circuit, :108);
  * the candidates are neither cut nor noised, and go through ``frame_transform`` with their own poses;
  * ``yaw / 3.1415`` and ``len / 100`` are Python double divisions rounded to float32 once, ``size / 10`` is a float32 division;
  * the points are rotated by ``-angle`` through ``BasePoints.rotate`` and the boxes by ``angle``: the same 2 x 2 product.
One thing the reference cannot do is defined here: ``add_yaw_noise(consistent=True)`` adds a [1] tensor to a 0-d element in
place (lidar_tracklet.py:542), which torch refuses; here one number is drawn, shape (1,), and added to every frame's yaw.

Deviations, as in sst_amd.augment: ``PointShuffle`` is the stable sort by the counter-based hash of DESIGN.md 3.26, not
``torch.randperm``; the outputs are views of buffers this object owns, valid until its next call; the points of every frame go
through ``((m0 x + m1 y) + m2 z) + m3`` in float32 where the reference calls a matrix product of unspecified summation order
(the bar: DESIGN.md 3.27).  The tracklets and candidates handed in are modified in place, as the reference's transforms modify
theirs.  There is no eager fall-back: ``__call__`` needs a GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .augment import AugmentParams, MAX_COLS
from .tracklet import LiDARTracklet

WHERE = 'sst_amd.tracklet_augment'
MAX_DECO = 8
MAX_FRAMES = 2048
_BLOCK = 256

_SKIPPED = ('LoadTrackletAnnotations', 'TrackletFormatBundle', 'Collect3D')
_ORDER = ('TrackletCutting', 'TrackletPoseTransform', 'TrackletNoise', 'PointDecoration', 'TrackletRandomFlip',
          'TrackletGlobalRotScaleTrans', 'PointsRangeFilter', 'PointShuffle')
_DECO_WIDTH = dict(yaw=1, size=3, score=1, length=1)


def _refuse(name, why):
    raise NotImplementedError(f'{WHERE}: {name} is not supported ({why})')


class TrackletParams(AugmentParams):
    """What one call applies, per sample: ``AugmentParams`` (flips, angle, scale, translation, shuffle seed) and ``cut`` (head,
    tail: the frames dropped at either end), ``center_noise`` / ``size_noise`` / ``yaw_noise``: the ``torch.rand`` draws of
    lidar_tracklet.py:495-546 as float32 arrays ([n, 3], [n, 3], [n], or [3], [3], [1] when consistent), None where nothing is
    drawn.  A plain record: fill it by hand to replay a batch."""

    def __init__(self, batch_size):
        super().__init__(batch_size)
        self.cut = [(0, 0)] * batch_size
        self.center_noise = [None] * batch_size
        self.size_noise = [None] * batch_size
        self.yaw_noise = [None] * batch_size


def frame_matrices(center_pose, poses):
    """``inv(center_pose)[None] @ stack(poses)`` in float32: the expression of ``LiDARTracklet.frame_transform``"""
    if len(poses) == 0:
        return torch.zeros((0, 4, 4), dtype=torch.float32)
    stacked = torch.stack([p if torch.is_tensor(p) else torch.as_tensor(p) for p in poses], 0).to(torch.float32)
    return torch.linalg.inv(torch.as_tensor(center_pose, dtype=torch.float32))[None] @ stacked


def apply_noise(boxes, max_noise, draws, kind):
    """lidar_tracklet.py:495-546 on host boxes [n, 7] (in place): ``noise = (u - 0.5) * 2 * max_noise``; the centre and the yaw
    are raised by it, the size is multiplied by ``1 + noise``"""
    if boxes.size(0) == 0 or draws is None:
        return
    u = torch.as_tensor(draws, dtype=boxes.dtype)
    if kind == 'yaw':
        boxes[:, 6] += (u - 0.5) * 2 * max_noise
        return
    mx = torch.tensor(max_noise, dtype=boxes.dtype)
    if kind == 'center':
        boxes[:, :3] += (u - 0.5) * 2 * (mx[None, :] if u.dim() == 2 else mx)
    else:
        assert (mx < 0.5).all(), 'noise range is [1 - max_noise, 1 + max_noise], usually smaller than 0.5'
        boxes[:, 3:6] *= 1 + (u - 0.5) * 2 * (mx[None, :] if u.dim() == 2 else mx)


def decoration_values(boxes, scores, properties, length):
    """the columns PointDecoration appends to every point of a frame (tracklet_pipelines.py:474-506) -> float32 [n, D]: ``yaw``
    is ``yaw.item() / 3.1415`` and ``length`` is ``len / 100`` (Python doubles, rounded to float32 by ``F.pad``), ``size`` is
    ``tensor[:, 3:6] / 10`` in float32, ``score`` the frame's score"""
    n = boxes.size(0)
    cols = []
    for pro in properties:
        if pro == 'yaw':
            cols.append(torch.tensor([y / 3.1415 for y in boxes[:, 6].tolist()], dtype=torch.float64).to(torch.float32)[:, None])
        elif pro == 'size':
            cols.append(boxes[:, 3:6] / 10)
        elif pro == 'score':
            cols.append(torch.tensor([float(s) for s in scores], dtype=torch.float64).to(torch.float32).reshape(n, 1))
        else:
            cols.append(torch.full((n, 1), length / 100, dtype=torch.float64).to(torch.float32))
    return torch.cat(cols, 1) if cols else torch.zeros((n, 0), dtype=torch.float32)


class TrackletAugment(object):
    """The steps of a shipped CTRL ``train_pipeline`` / ``test_pipeline`` (see ``from_pipeline``) as one device call."""

    def __init__(self):
        self.use_dim = None
        self.cutting = None           # (min_length, ratio, max_cut_ratio, max_length)
        self.pose = False
        self.noise = None             # (center cfg, size cfg, yaw cfg), each None or (max_noise, consistent)
        self.properties = ()
        self.flip = None              # (ratio_h, ratio_v)
        self.rst = None               # (rot_range, scale_ratio_range, translation_std)
        self.point_range = None
        self.shuffle = False
        self._buf = {}

    @property
    def deco(self):
        return sum(_DECO_WIDTH[p] for p in self.properties)

    # ------------------------------------------------------------------ the pipeline's text
    @classmethod
    def from_pipeline(cls, pipeline):
        """``pipeline``: the list of dicts of a shipped CTRL ``train_pipeline`` or ``test_pipeline``.  Accepted, in this order:
        TrackletCutting, TrackletPoseTransform(centering=False), TrackletNoise, PointDecoration(yaw, size, score, length),
        TrackletRandomFlip, TrackletGlobalRotScaleTrans, PointsRangeFilter, PointShuffle.  LoadTrackletPoints (its ``use_dim`` is
        checked against the input; ``max_points`` stays with the loader), LoadTrackletAnnotations, TrackletFormatBundle and
        Collect3D are skipped.  Everything else raises NotImplementedError with the transform's name."""
        self = cls()
        last = -1
        for step in pipeline:
            step = dict(step)
            name = step.pop('type')
            if name == 'LoadTrackletPoints':
                self.use_dim = step.get('use_dim', 5)
                continue
            if name in _SKIPPED:
                continue
            if name == 'FrameDropout':
                _refuse(name, 'no shipped CTRL config uses it; LiDARTracklet.random_frame_drop is not built')
            if name == 'TrackletScaling':
                _refuse(name, 'no shipped CTRL config uses it (it needs scipy.signal.medfilt per tracklet)')
            if name == 'MultiScaleFlipAug3D':
                _refuse(name, 'test-time augmentation: the detectors refuse aug_test')
            if name not in _ORDER:
                _refuse(name, 'not one of the transforms this module restates')
            pos = _ORDER.index(name)
            if pos <= last:
                _refuse(name, 'it comes after a step the kernels apply later, or twice: the order is ' + ', '.join(_ORDER))
            last = pos
            if name == 'TrackletCutting':
                self.cutting = (int(step.get('min_length', 5)), float(step.get('ratio', 0.5)), float(step.get('max_cut_ratio', 0.5)),
                                int(step.get('max_length', 200)))
            elif name == 'TrackletPoseTransform':
                if step.get('centering', False):
                    _refuse('TrackletPoseTransform(centering=True)', 'no shipped CTRL config centres the tracklet')
                self.pose = True
            elif name == 'TrackletNoise':
                cfgs = []
                for key in ('center_noise_cfg', 'size_noise_cfg', 'yaw_noise_cfg'):
                    c = step.get(key)
                    if c is None:
                        cfgs.append(None)
                        continue
                    mx = c['max_noise']
                    if key != 'yaw_noise_cfg' and len(mx) != 3:
                        raise RuntimeError(f'{WHERE}: TrackletNoise {key}: three max_noise values expected')
                    cfgs.append(([float(v) for v in mx] if key != 'yaw_noise_cfg' else float(mx), bool(c.get('consistent', False))))
                self.noise = tuple(cfgs)
            elif name == 'PointDecoration':
                props = list(step['properties'])
                if 'center_offset' in props:
                    _refuse('PointDecoration(center_offset)', 'its columns differ from point to point; no shipped CTRL config lists it')
                for p in props:
                    if p not in _DECO_WIDTH:
                        _refuse(f'PointDecoration({p})', 'yaw, size, score and length are restated')
                self.properties = tuple(props)
                if self.deco > MAX_DECO:
                    _refuse('PointDecoration', f'{self.deco} appended columns; the kernels take {MAX_DECO} (SST_TRK_AUG_MAX_DECO)')
            elif name == 'TrackletRandomFlip':
                self.flip = (float(step.get('flip_ratio_bev_horizontal', 0.0)), float(step.get('flip_ratio_bev_vertical', 0.0)))
            elif name == 'TrackletGlobalRotScaleTrans':
                if step.get('shift_height', False):
                    _refuse('TrackletGlobalRotScaleTrans(shift_height=True)', 'no height attribute column is scaled')
                rot = step.get('rot_range', [-0.78539816, 0.78539816])
                rot = [-rot, rot] if not isinstance(rot, (list, tuple, np.ndarray)) else list(rot)
                std = step.get('translation_std', [0, 0, 0])
                std = [std] * 3 if not isinstance(std, (list, tuple, np.ndarray)) else list(std)
                self.rst = (rot, list(step.get('scale_ratio_range', [0.95, 1.05])), std)
            elif name == 'PointsRangeFilter':
                self.point_range = np.array(step['point_cloud_range'], dtype=np.float32)
            elif name == 'PointShuffle':
                self.shuffle = True
        if not self.pose:
            _refuse('a pipeline without TrackletPoseTransform', 'PointDecoration and the detector need the shared pose')
        return self

    # ------------------------------------------------------------------ the random numbers
    def cut_of(self, length, rng):
        """TrackletCutting's decision for a tracklet of ``length`` frames (tracklet_pipelines.py:105-124) -> (head, tail)"""
        if self.cutting is None:
            return 0, 0
        min_length, ratio, max_cut_ratio, max_length = self.cutting
        if length < min_length or (rng.rand() > ratio and length < max_length):     # the draw happens only when length >= min_length
            return 0, 0
        cut_len = length - max_length if length > max_length else int(length * max_cut_ratio * rng.rand())
        if cut_len < 1:
            return 0, 0
        head = int(rng.randint(0, cut_len))
        return head, cut_len - head

    def draw_params(self, tracklets, rng=np.random, generator=None):
        """The reference's draws, per sample in its source order: the cutting (``rand()`` unless short-circuited, ``rand()`` for
        the cut length of a tracklet below ``max_length``, ``randint(0, cut_len)``), the noise (``torch.rand`` of (n, 3), (n, 3),
        (n,) - or (3,), (3,), (1,) when consistent - with ``generator``, n the length after the cut; nothing for an empty
        tracklet), ``rand()`` twice for the flips, ``uniform`` for the angle and the scale, ``normal(size=3)`` for the translation;
        steps the pipeline lacks draw nothing.  The 64-bit shuffle seeds are drawn after the last sample's draws, as
        sst_amd.augment draws them, so that the stream is the one the reference's transforms consume sample after sample.
        ``tracklets``: the batch's tracklets, or their lengths."""
        lens = [t if isinstance(t, (int, np.integer)) else len(t) for t in tracklets]
        p = TrackletParams(len(lens))
        for i, length in enumerate(lens):
            p.cut[i] = self.cut_of(int(length), rng)
            n = int(length) - sum(p.cut[i])
            if self.noise is not None and n > 0:
                for key, cfg, shape in (('center_noise', self.noise[0], (n, 3)), ('size_noise', self.noise[1], (n, 3)),
                                        ('yaw_noise', self.noise[2], (n,))):
                    if cfg is not None:
                        shape = (shape[1:] or (1,)) if cfg[1] else shape
                        getattr(p, key)[i] = torch.rand(shape, dtype=torch.float32, generator=generator).numpy()
            if self.flip is not None:
                p.flip_h[i] = rng.rand() < self.flip[0]
                p.flip_v[i] = rng.rand() < self.flip[1]
            if self.rst is not None:
                rot, scale, std = self.rst
                p.angle[i] = rng.uniform(rot[0], rot[1])
                p.scale[i] = rng.uniform(scale[0], scale[1])
                p.trans[i] = rng.normal(scale=np.array(std, dtype=np.float32), size=3).T
        for i in range(len(lens)):
            p.seed[i] = (int(rng.randint(0, 2 ** 32)) << 32) | int(rng.randint(0, 2 ** 32))
        return p

    def records(self, params):
        """the kernels' per-sample records (PARAMS_DTYPE): TrackletGlobalRotScaleTrans always rotates; a pipeline without it
        scales by 1 and adds -0.0, which keeps every bit"""
        rng6 = self.point_range if self.point_range is not None else np.array([-np.inf] * 3 + [np.inf] * 3, np.float32)
        rec = params.records(np.full(len(params), self.rst is not None), rng6, self.shuffle)
        if self.rst is None:
            rec['trans'] = np.float32(-0.0)
        return rec

    # ------------------------------------------------------------------ host side, once per batch
    def prepare_boxes(self, tracklets, candidates, params):
        """the cut, the pose transform of every tracklet and candidate (ONE batched product), the noise and the decoration values
        -> per sample (frame matrices [n, 4, 4], decoration values [n, D], frame values int32 [n], (head, n): the frames kept),
        and the host boxes [total, 7 | 9] of the batch with their row ranges: per sample the tracklet's, then its candidates'"""
        per_sample, groups, src, mms = [], [], [], []
        for i, trk in enumerate(tracklets):
            if not getattr(trk, 'frozen', False):
                raise RuntimeError(f'{WHERE}: tracklets must be frozen (freeze())')
            if getattr(trk, 'shared_pose', None) is not None:
                raise RuntimeError(f'{WHERE}: tracklet {i} has a shared pose already: the pose transform runs once')
            if getattr(trk, 'pose_list', None) is None:
                raise RuntimeError(f'{WHERE}: tracklet {i} has no pose_list (set_poses)')
            full = len(trk)
            head, tail = params.cut[i]
            if head or tail:
                trk.remove(trk.ts_list[:head] + trk.ts_list[full - tail:])
            n = len(trk)
            if n == 0:
                raise RuntimeError(f'{WHERE}: tracklet {i} has no frame')
            center = torch.as_tensor(trk.pose_list[n // 2], dtype=torch.float32)
            mm = frame_matrices(center, trk.pose_list)
            members = [trk] + list(candidates[i] if candidates is not None else [])
            for c in members[1:]:
                if getattr(c, 'shared_pose', None) is not None:
                    raise RuntimeError(f'{WHERE}: a candidate of tracklet {i} has a shared pose already')
            for m in members:
                b = m.boxes.detach().cpu().to(torch.float32)
                src.append(b)
                mms.append(mm if m is trk else frame_matrices(center, m.pose_list))
            groups.append(members)
            per_sample.append([mm, None, np.arange(head, head + n, dtype=np.int32), (head, n), center])
        width = src[0].size(1)
        if any(b.size(1) != width for b in src) or width not in (7, 9):
            raise RuntimeError(f'{WHERE}: the boxes of a batch must all have 7 or all have 9 columns')
        moved = LiDARTracklet._apply_poses(torch.cat(src, 0), torch.cat(mms, 0))
        ranges, at = [], 0
        for i, members in enumerate(groups):
            rows = []
            for m in members:
                rows.append((at, at + len(m)))
                at += len(m)
            ranges.append(rows)
            t0, t1 = rows[0]
            own = moved[t0:t1]
            if self.noise is not None:
                for kind, cfg, draws in zip(('center', 'size', 'yaw'), self.noise,
                                            (params.center_noise[i], params.size_noise[i], params.yaw_noise[i])):
                    if cfg is not None:
                        apply_noise(own, cfg[0], draws, kind)
            per_sample[i][1] = decoration_values(own, members[0].score_list, self.properties, len(members[0]))
        return per_sample, moved, ranges

    def _buffer(self, key, nbytes_or_shape, dtype, dev, pin=False):
        shape = (int(nbytes_or_shape),) if not isinstance(nbytes_or_shape, tuple) else nbytes_or_shape
        need = int(np.prod(shape))
        cur = self._buf.get(key)
        if cur is None or cur.numel() < need or cur.dtype != dtype or (not pin and cur.device != dev):
            grow = max(need, 1)
            cur = torch.empty(grow, dtype=dtype, pin_memory=True) if pin else torch.empty(grow, dtype=dtype, device=dev)
            self._buf[key] = cur
        return cur[:need].view(shape)

    @staticmethod
    def _frames_of(sample, cols_hint=None):
        """one sample's points -> (rows [N, C] host array or device tensor, frame lengths int64 [n]); ``sample`` is the list (or
        object array) of per-frame [n_f, C] arrays / tensors, or (one concatenated [N, C] array / tensor, the frame lengths)"""
        if isinstance(sample, tuple) and len(sample) == 2 and not (torch.is_tensor(sample[1]) and sample[1].dim() == 2) \
                and not (isinstance(sample[1], np.ndarray) and sample[1].ndim == 2):
            rows, lens = sample
            rows = getattr(rows, 'tensor', rows)
            lens = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens, dtype=np.int64).reshape(-1)
            if not (torch.is_tensor(rows) and rows.is_cuda):
                rows = np.ascontiguousarray(rows.detach().numpy() if torch.is_tensor(rows) else np.asarray(rows), dtype=np.float32)
            return rows, lens
        frames = [getattr(f, 'tensor', f) for f in sample]
        lens = np.array([int(f.shape[0]) for f in frames], dtype=np.int64)
        if frames and all(torch.is_tensor(f) and f.is_cuda for f in frames):
            return frames, lens                     # device frames: copied into the packed buffer one by one
        frames = [np.ascontiguousarray(f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f), dtype=np.float32)
                  for f in frames]
        return frames, lens

    # ------------------------------------------------------------------ the call
    def _stage(self, points, tracklets, candidates, params, records, extra=()):
        """the host side of a call, shared with sst_amd.tracklet_tta: the checks, ``prepare_boxes``, the tables and ONE packed
        host-to-device copy of [points | frame offsets | sample tables | frame records | frame values | records | boxes].
        ``records``: params -> the kernels' records (one per sample here; one per (view, sample) for the test-time views);
        ``extra``: host arrays that travel in the same copy (their offsets: ``at_extra``).
        -> a namespace of what the launches need"""
        if not torch.cuda.is_available():
            raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
        batch = len(tracklets)
        if batch < 1 or len(points) != batch or (candidates is not None and len(candidates) != batch):
            raise RuntimeError(f'{WHERE}: one entry of points (and of candidates) per tracklet expected, and at least one tracklet')
        if batch >= 2 ** 31:
            raise NotImplementedError(f'{WHERE}: {batch} samples; the sample field of the sort key holds 2^31 - 1')
        if len(params) != batch:
            raise RuntimeError(f'{WHERE}: params for {len(params)} samples, {batch} given')
        full_lens = [len(t) for t in tracklets]
        given = [self._frames_of(p) for p in points]
        for i, (_, lens) in enumerate(given):
            if len(lens) != full_lens[i]:
                raise RuntimeError(f'{WHERE}: sample {i} has {len(lens)} frames of points and {full_lens[i]} boxes')
        first = given[0][0]
        first = first[0] if isinstance(first, list) else first
        cols = int(first.shape[1])
        if cols < 3 or cols > MAX_COLS:
            raise NotImplementedError(f'{WHERE}: {cols} point columns; the kernels take 3 to {MAX_COLS} (SST_AUG_MAX_COLS)')
        if isinstance(self.use_dim, int) and cols != self.use_dim:
            raise RuntimeError(f'{WHERE}: LoadTrackletPoints(use_dim={self.use_dim}) and {cols} point columns')
        deco = self.deco
        per_sample, boxes, ranges = self.prepare_boxes(tracklets, candidates, params)
        n_frames = [ps[3][1] for ps in per_sample]
        if max(n_frames) > MAX_FRAMES:
            raise NotImplementedError(f'{WHERE}: a tracklet of {max(n_frames)} frames; the kernels take {MAX_FRAMES} '
                                      f'(SST_TRK_AUG_MAX_FRAMES)')
        rec = records(params)

        # the kept frames of every sample: offsets only, nothing is copied before the packing
        spans, frame_lens = [], []
        for i, (rows, lens) in enumerate(given):
            head, n = per_sample[i][3]
            starts = np.concatenate([[0], np.cumsum(lens)])
            spans.append((int(starts[head]), int(starts[head + n])))
            frame_lens.append(lens[head:head + n])
        rows_per = np.array([b - a for a, b in spans], np.int64)
        n_total = int(rows_per.sum())
        if n_total > 2 ** 31 - 1 - _BLOCK:
            raise NotImplementedError(f'{WHERE}: {n_total} rows in a batch; the kernels index 2^31 - 257')
        frame_rows = np.concatenate([[0], np.cumsum(np.concatenate(frame_lens))]).astype(np.int32)
        sample_frames = np.concatenate([[0], np.cumsum(n_frames)]).astype(np.int32)
        blk_off = np.concatenate([[0], np.cumsum((rows_per + _BLOCK - 1) // _BLOCK)]).astype(np.int32)
        total_frames = int(sample_frames[-1])
        frames = np.zeros((total_frames, 12 + deco), np.float32)
        frames[:, :12] = torch.cat([ps[0] for ps in per_sample], 0)[:, :3, :].reshape(total_frames, 12).numpy()
        frames[:, 12:] = torch.cat([ps[1] for ps in per_sample], 0).numpy()
        frame_values = np.concatenate([ps[2] for ps in per_sample])
        box_cols = int(boxes.size(1))
        box_off = np.array([r[0][0] for r in ranges] + [int(boxes.size(0))], np.int32)

        on_device = [isinstance(rows, list) and len(rows) > 0 and torch.is_tensor(rows[0]) and rows[0].is_cuda
                     or (torch.is_tensor(rows) and rows.is_cuda) for rows, _ in given]
        all_device = all(on_device)
        dev = None
        for (rows, _), d in zip(given, on_device):
            if d:
                dev = (rows[0] if isinstance(rows, list) else rows).device
        if dev is None:
            dev = torch.device('cuda', torch.cuda.current_device())

        # one host buffer, one copy: [points of the batch | frame offsets | sample tables | frame records | frame values | records | boxes]
        parts, cursor = [], [0]

        def place(arr):
            arr = np.ascontiguousarray(arr)
            at = cursor[0]
            parts.append((at, arr))
            cursor[0] = (at + max(arr.nbytes, 1) + 255) // 256 * 256
            return at

        at_points = None
        row_off = np.concatenate([[0], np.cumsum(rows_per)])
        if not all_device:
            at_points = cursor[0]
            for i, (rows, lens) in enumerate(given):
                if on_device[i]:
                    continue
                base = at_points + int(row_off[i]) * cols * 4
                if isinstance(rows, list):
                    head, n = per_sample[i][3]
                    for f in rows[head:head + n]:
                        if f.ndim != 2 or f.shape[1] != cols:
                            raise RuntimeError(f'{WHERE}: points must be float32 [N, {cols}], got {tuple(f.shape)}')
                        parts.append((base, f))
                        base += f.nbytes
                else:
                    if rows.ndim != 2 or rows.shape[1] != cols:
                        raise RuntimeError(f'{WHERE}: points must be float32 [N, {cols}], got {tuple(rows.shape)}')
                    parts.append((base, rows[spans[i][0]:spans[i][1]]))
            cursor[0] = (at_points + max(n_total * cols * 4, 1) + 255) // 256 * 256
        at_fr, at_sf, at_blk = place(frame_rows), place(sample_frames), place(blk_off)
        at_frames, at_fv, at_rec = place(frames), place(frame_values), place(rec)
        at_boxes, at_boff = place(boxes.numpy()), place(box_off)
        at_extra = [place(e) for e in extra]
        nbytes = cursor[0]
        host = self._buffer('host', nbytes, torch.uint8, None, pin=True)
        host_np = host.numpy()
        for at, arr in parts:
            if arr.nbytes:
                host_np[at:at + arr.nbytes] = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        stage = self._buffer('stage', nbytes, torch.uint8, dev)
        stage.copy_(host, non_blocking=True)
        base = stage.data_ptr()
        at = lambda off: ctypes.c_void_p(base + off)                                     # noqa: E731

        if any(on_device):
            if all_device:
                packed = self._buffer('points_in', (n_total, cols), torch.float32, dev)
            else:
                packed = stage[at_points:at_points + n_total * cols * 4].view(torch.float32).view(n_total, cols)
            for i, (rows, lens) in enumerate(given):
                if not on_device[i]:
                    continue
                r0 = int(row_off[i])
                if isinstance(rows, list):
                    head, n = per_sample[i][3]
                    for f in rows[head:head + n]:
                        if f.dim() != 2 or f.shape[1] != cols or f.dtype != torch.float32:
                            raise RuntimeError(f'{WHERE}: points must be float32 [N, {cols}], got {tuple(f.shape)}')
                        packed[r0:r0 + f.shape[0]].copy_(f)
                        r0 += f.shape[0]
                else:
                    if rows.dim() != 2 or rows.shape[1] != cols or rows.dtype != torch.float32:
                        raise RuntimeError(f'{WHERE}: points must be float32 [N, {cols}], got {tuple(rows.shape)}')
                    packed[r0:r0 + int(rows_per[i])].copy_(rows[spans[i][0]:spans[i][1]])
            points_ptr = _lib.ptr(packed)
        else:
            points_ptr = at(at_points)

        return SimpleNamespace(batch=batch, cols=cols, deco=deco, per_sample=per_sample, boxes=boxes, ranges=ranges, rec=rec,
                               n_frames=n_frames, n_total=n_total, blk_off=blk_off, total_frames=total_frames, box_cols=box_cols,
                               dev=dev, stage=stage, at=at, points_ptr=points_ptr, at_fr=at_fr, at_sf=at_sf, at_blk=at_blk,
                               at_frames=at_frames, at_fv=at_fv, at_rec=at_rec, at_boxes=at_boxes, at_boff=at_boff, at_extra=at_extra)

    def __call__(self, points, tracklets, candidates=None, params=None):
        """points: per sample the list (or object array) of per-frame [n_f, C] float32 arrays or tensors (host or device), or
        (one concatenated [N, C] array or tensor, the frame lengths); 3 <= C <= 8.  tracklets: one frozen LiDARTracklet per sample
        with ``pose_list`` set; candidates: per sample the list of its ground-truth candidates (with their own ``pose_list``), or
        None (test pipelines).  params: a ``TrackletParams`` (default: ``draw_params(tracklets)``).

        -> dict(points: per-sample [n_kept, C + D] VIEWS of the packed output, pts_frame_inds: per-sample int32 views,
        points_packed, offsets (list, B + 1), counts (list, the one host read of the call), tracklets, candidates: the objects
        handed in, their ``boxes`` now row ranges of ONE device buffer, ``shared_pose`` set, ``rot_angle`` set on the tracklet as
        tracklet_pipelines.py:292 sets it; params, records, and per sample pcd_horizontal_flip, pcd_vertical_flip, pcd_rot_angle,
        pcd_scale_factor, pcd_trans, shared_pose)."""
        if not torch.cuda.is_available():
            raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
        if params is None and len(tracklets) >= 1 and len(points) == len(tracklets) and \
                (candidates is None or len(candidates) == len(tracklets)):       # otherwise _stage raises before anything is drawn
            params = self.draw_params(tracklets)
        st = self._stage(points, tracklets, candidates, params, self.records)
        batch, cols, deco, per_sample, boxes, ranges, rec = st.batch, st.cols, st.deco, st.per_sample, st.boxes, st.ranges, st.rec
        n_frames, n_total, blk_off, total_frames, box_cols = st.n_frames, st.n_total, st.blk_off, st.total_frames, st.box_cols
        dev, at, points_ptr = st.dev, st.at, st.points_ptr
        at_fr, at_sf, at_blk, at_frames, at_fv, at_rec = st.at_fr, st.at_sf, st.at_blk, st.at_frames, st.at_fv, st.at_rec
        at_boxes, at_boff = st.at_boxes, st.at_boff
        width = cols + deco
        counts = self._buffer('counts', 2 * batch, torch.int32, dev)
        out = self._buffer('out', (n_total, width), torch.float32, dev)
        out_frames = self._buffer('out_frames', n_total, torch.int32, dev)
        lib = _lib.load()
        ws_bytes = lib.sst_tracklet_augment_workspace_bytes(n_total, batch)
        ws = self._buffer('workspace', max(ws_bytes, 256), torch.uint8, dev)
        a = _lib.TrackletAugmentArgs()
        a.points, a.frame_rows, a.sample_frames, a.block_offsets = points_ptr, at(at_fr), at(at_sf), at(at_blk)
        a.frames, a.frame_values, a.params = at(at_frames), at(at_fv), at(at_rec)
        a.out, a.out_frame_inds, a.counts = _lib.ptr(out), _lib.ptr(out_frames), _lib.ptr(counts)
        a.workspace, a.workspace_bytes, a.n_total = _lib.ptr(ws), ws.numel(), n_total
        a.batch, a.cols, a.deco, a.n_blocks = batch, cols, deco, int(blk_off[-1])
        a.n_frames, a.max_frames = total_frames, int(max(n_frames))
        _lib.check(lib.sst_tracklet_augment_points_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_tracklet_augment_points_f32')

        n_boxes = int(boxes.size(0))
        boxes_out = self._buffer('boxes_out', (n_boxes, box_cols), torch.float32, dev)
        b = _lib.AugmentBoxArgs()
        b.params, b.batch, b.cols = at(at_rec), batch, box_cols
        b.boxes, b.labels, b.box_offsets, b.boxes_out, b.labels_out = at(at_boxes), None, at(at_boff), _lib.ptr(boxes_out), None
        b.counts = ctypes.c_void_p(counts.data_ptr() + 4 * batch)
        b.n_boxes, b.filter, b.always_rotate = n_boxes, 0, int(self.rst is not None)
        _lib.check(lib.sst_augment_boxes_f32(ctypes.byref(b), _lib.stream_ptr()), 'sst_augment_boxes_f32')

        got = counts[:batch].tolist()                                            # the one host read of the call
        offsets = [0]
        for c in got:
            offsets.append(offsets[-1] + c)
        for i, trk in enumerate(tracklets):
            members = [trk] + list(candidates[i] if candidates is not None else [])
            for m, (r0, r1) in zip(members, ranges[i]):
                m.boxes = boxes_out[r0:r1]
                m.size = r1 - r0
                m.device = boxes_out.device
                m.shared_pose = per_sample[i][4]
            if self.rst is not None:
                trk.rot_angle = float(params.angle[i])
        return dict(points=[out[offsets[i]:offsets[i + 1]] for i in range(batch)],
                    pts_frame_inds=[out_frames[offsets[i]:offsets[i + 1]] for i in range(batch)],
                    points_packed=out[:offsets[-1]], offsets=offsets, counts=got, tracklets=list(tracklets),
                    candidates=None if candidates is None else [list(c) for c in candidates], params=params, records=rec,
                    boxes_packed=boxes_out, box_ranges=ranges,
                    pcd_horizontal_flip=[bool(v) for v in params.flip_h], pcd_vertical_flip=[bool(v) for v in params.flip_v],
                    pcd_rot_angle=[float(v) if self.rst is not None else None for v in params.angle],
                    pcd_scale_factor=[float(v) for v in params.scale], pcd_trans=[params.trans[i].copy() for i in range(batch)],
                    shared_pose=[ps[4] for ps in per_sample])

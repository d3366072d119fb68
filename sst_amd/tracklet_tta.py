"""Test-time augmentation of the CTRL tracklet family on the device (csrc/tracklet_tta.hip): the ``tta_pipeline``
and the ``test_cfg.tta`` block every shipped CTRL config carries.

Reference: ``MultiScaleFlipAug3D`` (mmdet3d/datasets/pipelines/test_time_aug.py:88-109) deep-copies the sample once per view and
runs ``TrackletGlobalRotScaleTrans`` (tracklet_pipelines.py:329-355), ``TrackletRandomFlip`` (:414-439), ``PointsRangeFilter`` and
``PointShuffle`` on every copy in a data-loader worker; ``TrackletDetector.aug_test`` (detectors/tracklet_detector.py:315-332) calls
``simple_test`` once per view; ``TrackletRoIHead.inverse_aug`` (roi_heads/tracklet_roi_head.py:168-179) un-flips and un-rotates
the box lists on the host, ``LiDARTracklet.update_from_prediction`` (lidar_tracklet.py:403-445) takes them back to every frame's
own pose and ``LiDARTracklet.merge_augs`` (:548-602) merges numpy lists.  Here: one packed copy and three launches and a sort
in front of the network (``TrackletTTA.__call__``: the views of the whole batch, view-major), the network, one launch
(``tta_finish``) and one host read behind it.  The network runs once per view by default and once over the K * B samples with
``tta_single_pass``: the single pass is not bit-equal to the passes per view (the vendor GEMM behind the box head's fp32 linears
picks its tiles by the number of rows; see ``TrackletTTADetector``).

It is opt-in through new names: ``TrackletAugment.from_pipeline`` keeps refusing ``MultiScaleFlipAug3D`` and the builders keep
refusing ``test_cfg.tta``; ``attach_tracklet_tta(detector, tta_cfg, tta_pipeline)`` turns a detector built without ``tta`` into one
whose ``aug_test`` / ``forward_test`` run the path above.

Reproduced from the reference: the views in its loop order (horizontal flip, then vertical flip, then ``pts_rots``); inside a view
rotation -> scale -> translation -> flip h -> flip v (sst_amd.augment flips first: not this order); the zero-std
``np.random.normal`` draw of ``_trans_bbox_points`` still adds ``+0.0``; points rotate by ``-angle`` and boxes by ``angle``.

Deviations: ``PointShuffle`` is the stable sort by the hash of DESIGN.md 3.26 with ``seed + v * 0xD6E8FEB86659FD93`` for view v
(view 0 keeps the sample's seed); the reference also sends the OLD tracklet through the augmentation and back before it takes the
box of an invalid RoI from it - here the un-augmented old boxes are used directly (the round trip is the identity up to fp32
rounding); a tracklet comes back with ``boxes`` float64 [n, 7] on the host, as ``merge_augs`` leaves its ``box_list``.  There is no
eager fall-back: every call needs a GPU."""
import ctypes

import numpy as np
import torch

from . import _lib
from .augment import PARAMS_DTYPE
from .tracklet_augment import MAX_DECO, _DECO_WIDTH, TrackletAugment, TrackletParams
from .tracklet_detector import TrackletDetector, decode_tracklet_rows

WHERE = 'sst_amd.tracklet_tta'
MAX_VIEWS = 32
VIEW_SEED = 0xD6E8FEB86659FD93
MERGE_MODES = dict(max=0, weighted=1, iou_clamped_weighted=2)

_SKIPPED = ('TrackletFormatBundle', 'Collect3D')
_OUTER = ('TrackletPoseTransform', 'PointDecoration', 'MultiScaleFlipAug3D')
_INNER = ('TrackletGlobalRotScaleTrans', 'TrackletRandomFlip', 'PointsRangeFilter', 'PointShuffle')


def _refuse(name, why):
    raise NotImplementedError(f'{WHERE}: {name} is not supported ({why})')


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v]


class TrackletTTA(TrackletAugment):
    """A shipped CTRL ``tta_pipeline`` (see ``from_pipeline``) as one device call that makes every view of a batch."""

    def __init__(self):
        super().__init__()
        self.views = [(False, False, 0.0)]       # (pcd_horizontal_flip, pcd_vertical_flip, pcd_rot_angle), in the reference's order

    @property
    def n_views(self):
        return len(self.views)

    # ------------------------------------------------------------------ the pipeline's text
    @classmethod
    def from_pipeline(cls, pipeline):
        """``pipeline``: the list of dicts of a shipped CTRL ``tta_pipeline``.  Accepted, in this order: LoadTrackletPoints (its
        ``use_dim`` is checked against the input), TrackletPoseTransform(centering=False), PointDecoration(yaw, size, score,
        length), and ONE MultiScaleFlipAug3D whose ``transforms`` are, in this order, TrackletGlobalRotScaleTrans,
        TrackletRandomFlip, PointsRangeFilter, PointShuffle (the last two may be absent); TrackletFormatBundle and Collect3D are
        skipped, ``img_scale`` is ignored.  Everything else raises NotImplementedError with its name and the reason."""
        self = cls()
        last, seen_tta = -1, False
        for step in pipeline:
            step = dict(step)
            name = step.pop('type')
            if name == 'LoadTrackletPoints':
                if last >= 0:
                    _refuse(name, 'it comes after a step that needs the points')
                self.use_dim = step.get('use_dim', 5)
                continue
            if name in _SKIPPED:
                continue
            if name not in _OUTER:
                _refuse(name, 'a tta_pipeline is LoadTrackletPoints, TrackletPoseTransform, PointDecoration and one '
                              'MultiScaleFlipAug3D; ' + ('it belongs inside MultiScaleFlipAug3D' if name in _INNER else
                                                         'no shipped CTRL tta_pipeline has it'))
            pos = _OUTER.index(name)
            if pos <= last:
                _refuse(name, 'it comes twice, or after a step that runs later: the order is ' + ', '.join(_OUTER))
            last = pos
            if name == 'TrackletPoseTransform':
                if step.get('centering', False):
                    _refuse('TrackletPoseTransform(centering=True)', 'no shipped CTRL config centres the tracklet')
                self.pose = True
            elif name == 'PointDecoration':
                props = list(step['properties'])
                for p in props:
                    if p not in _DECO_WIDTH:
                        _refuse(f'PointDecoration({p})', 'yaw, size, score and length are restated')
                self.properties = tuple(props)
                if self.deco > MAX_DECO:
                    _refuse('PointDecoration', f'{self.deco} appended columns; the kernels take {MAX_DECO} (SST_TRK_AUG_MAX_DECO)')
            else:
                seen_tta = True
                self._parse_tta(step)
        if not self.pose:
            _refuse('a pipeline without TrackletPoseTransform', 'PointDecoration and the detector need the shared pose')
        if not seen_tta:
            _refuse('a pipeline without MultiScaleFlipAug3D', 'it has no views: use TrackletAugment for a test_pipeline')
        return self

    def _parse_tta(self, step):
        scales = [float(s) for s in _as_list(step.get('pts_scale_ratio', 1))]
        if len(scales) != 1:
            _refuse(f'MultiScaleFlipAug3D(pts_scale_ratio={scales})', 'more than one scale: inverse_aug never undoes the scale')
        if scales[0] != 1.0:
            _refuse(f'MultiScaleFlipAug3D(pts_scale_ratio={scales[0]})', 'a scale that is not 1: inverse_aug never undoes the scale')
        directions = _as_list(step.get('flip_direction', 'horizontal'))
        if len(directions) != 1:
            _refuse(f'MultiScaleFlipAug3D(flip_direction={directions})', 'the tracklet transforms never read it: more than one '
                                                                        'would only duplicate views')
        rots = [float(r) for r in _as_list(step.get('pts_rots', 0))]
        flip = bool(step.get('flip', False))
        hs = [False, True] if flip and step.get('pcd_horizontal_flip', False) else [False]
        vs = [False, True] if flip and step.get('pcd_vertical_flip', False) else [False]
        views = [(h, v, r) for h in hs for v in vs for r in rots]
        if len(views) > MAX_VIEWS:
            _refuse(f'MultiScaleFlipAug3D with {len(views)} views', f'the kernels take {MAX_VIEWS} (SST_TRK_TTA_MAX_VIEWS)')
        if len(views) == 0:
            _refuse('MultiScaleFlipAug3D(pts_rots=[])', 'no view at all')
        last, have = -1, set()
        for inner in step.get('transforms', []):
            inner = dict(inner)
            name = inner.pop('type')
            if name in _SKIPPED:
                continue
            if name not in _INNER:
                _refuse(name + ' inside MultiScaleFlipAug3D', 'its transforms are ' + ', '.join(_INNER))
            pos = _INNER.index(name)
            if pos <= last:
                _refuse(name + ' inside MultiScaleFlipAug3D', 'it comes twice, or after a step the kernels apply later: the order '
                                                              'is ' + ', '.join(_INNER))
            last = pos
            have.add(name)
            if name == 'TrackletGlobalRotScaleTrans':
                if inner.get('shift_height', False):
                    _refuse('TrackletGlobalRotScaleTrans(shift_height=True)', 'no height attribute column is scaled')
                rot = inner.get('rot_range', [-0.78539816, 0.78539816])
                rot = [-rot, rot] if not isinstance(rot, (list, tuple, np.ndarray)) else list(rot)
                scale = list(inner.get('scale_ratio_range', [0.95, 1.05]))
                if rot[0] != rot[1]:
                    _refuse(f'TrackletGlobalRotScaleTrans(rot_range={rot}) inside MultiScaleFlipAug3D',
                            'a range that is not degenerate: pcd_rot_angle overrides it in every view')
                if scale[0] != scale[1]:
                    _refuse(f'TrackletGlobalRotScaleTrans(scale_ratio_range={scale}) inside MultiScaleFlipAug3D',
                            'a range that is not degenerate: pcd_scale_factor overrides it in every view')
                std = _as_list(inner.get('translation_std', [0, 0, 0]))
                if any(float(s) != 0 for s in std):
                    _refuse(f'TrackletGlobalRotScaleTrans(translation_std={std}) inside MultiScaleFlipAug3D',
                            'inverse_aug never undoes the translation')
                self.rst = ([0.0, 0.0], [1.0, 1.0], [0.0, 0.0, 0.0])
            elif name == 'TrackletRandomFlip':
                self.flip = (0.0, 0.0)           # the ratios are never read: the view's meta keys decide
            elif name == 'PointsRangeFilter':
                self.point_range = np.array(inner['point_cloud_range'], dtype=np.float32)
            elif name == 'PointShuffle':
                self.shuffle = True
        if 'TrackletGlobalRotScaleTrans' not in have:
            _refuse('MultiScaleFlipAug3D without TrackletGlobalRotScaleTrans', 'nothing would apply pcd_rot_angle')
        if 'TrackletRandomFlip' not in have:
            _refuse('MultiScaleFlipAug3D without TrackletRandomFlip', 'nothing would apply the flips')
        self.views = views

    # ------------------------------------------------------------------ the records
    def view_records(self, seeds):
        """the kernels' records (PARAMS_DTYPE [K * B], view-major): every view rotates (TrackletGlobalRotScaleTrans always does),
        scales by 1 and adds +0.0 (the zero-std normal draw), then flips; ``cos`` / ``sin`` are ``torch.cos`` / ``torch.sin`` of
        the float32 angle on the CPU.  The seed is the sample's: the kernel folds the view in"""
        seeds = np.asarray(seeds, np.uint64).reshape(-1)
        batch = len(seeds)
        rng6 = self.point_range if self.point_range is not None else np.array([-np.inf] * 3 + [np.inf] * 3, np.float32)
        rec = np.zeros((self.n_views, batch), PARAMS_DTYPE)
        for k, (h, v, rot) in enumerate(self.views):
            angle = torch.tensor(rot, dtype=torch.float64).to(torch.float32)
            rec[k]['flip_h'], rec[k]['flip_v'], rec[k]['rotate'], rec[k]['shuffle'] = int(h), int(v), 1, int(self.shuffle)
            rec[k]['cos'], rec[k]['sin'], rec[k]['angle'] = float(torch.cos(angle)), float(torch.sin(angle)), float(angle)
            rec[k]['scale'] = 1.0
            rec[k]['range'] = np.asarray(rng6, np.float32)[None]
            rec[k]['seed'] = seeds
        return rec.reshape(-1)

    def view_meta(self):
        """per view what MultiScaleFlipAug3D writes into the sample: pcd_horizontal_flip, pcd_vertical_flip, pcd_rot_angle"""
        return [dict(pcd_horizontal_flip=h, pcd_vertical_flip=v, pcd_rot_angle=r, pcd_scale_factor=1.0) for h, v, r in self.views]

    # ------------------------------------------------------------------ the call
    def __call__(self, points, tracklets, seeds=None, rng=np.random):
        """points, tracklets: as ``TrackletAugment.__call__`` takes them (frozen tracklets with ``pose_list`` and no shared pose).
        seeds: uint64 per sample for the shuffle (default: drawn from ``rng`` as ``TrackletAugment.draw_params`` draws them).

        -> dict(points, pts_frame_inds: K * B views of the packed output, view-major (entry v * B + s is view v of sample s);
        points_packed, offsets (K * B + 1), counts (the one host read of the call), n_views, batch, views (``view_meta``),
        boxes_views [K, n_rows, 7 | 9]: the tracklets' boxes of every view; old_boxes [n_rows, 7 | 9]: the un-augmented boxes in
        the shared pose; box_ranges: per sample its rows; ego_mats [n_rows, 12]: rows 0..2 of inv(pose_i) @ shared_pose;
        row_sample, row_frame int32 [n_rows], old_scores float64 [n_rows], roi_scores float32 [n_rows], labels int32 [n_rows]: all
        device views of the ONE packed copy; tracklets: the objects handed in, ``boxes`` = their rows of old_boxes and
        ``shared_pose`` set; records, seeds, shared_pose)."""
        if not torch.cuda.is_available():
            raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
        batch = len(tracklets)
        if batch < 1:
            raise RuntimeError(f'{WHERE}: at least one tracklet expected')
        K = self.n_views
        params = TrackletParams(batch)
        if seeds is None:
            seeds = [(int(rng.randint(0, 2 ** 32)) << 32) | int(rng.randint(0, 2 ** 32)) for _ in range(batch)]
        params.seed[:] = np.asarray(seeds, np.uint64)
        # per row: the matrix that takes the shared pose back to the frame's own, in the expression shared2ego uses
        mats, lens = [], []
        for i, trk in enumerate(tracklets):
            if getattr(trk, 'pose_list', None) is None:
                raise RuntimeError(f'{WHERE}: tracklet {i} has no pose_list (set_poses)')
            n = len(trk)
            if n == 0:
                raise RuntimeError(f'{WHERE}: tracklet {i} has no frame')
            poses = torch.stack([torch.as_tensor(p) for p in trk.pose_list], 0).to(torch.float32)
            mats.append((torch.linalg.inv(poses) @ poses[n // 2])[:, :3, :].reshape(n, 12))
            lens.append(n)
        n_rows = int(sum(lens))
        ego = torch.cat(mats, 0).numpy()
        row_sample = np.repeat(np.arange(batch, dtype=np.int32), lens)
        row_frame = np.concatenate([np.arange(n, dtype=np.int32) for n in lens])
        old_scores = np.array([float(s) for t in tracklets for s in t.score_list], np.float64)
        labels = np.array([int(t.type) for t, n in zip(tracklets, lens) for _ in range(n)], np.int32)
        extra = (ego, row_sample, row_frame, old_scores, old_scores.astype(np.float32), labels)
        st = self._stage(points, tracklets, None, params, lambda p: self.view_records(p.seed), extra=extra)
        cols, deco, n_total, dev, at = st.cols, st.deco, st.n_total, st.dev, st.at
        width = cols + deco
        if K * n_total > 2 ** 31 - 1 - 256:
            raise NotImplementedError(f'{WHERE}: {K} views of {n_total} rows; the kernels index 2^31 - 257 (view, row) pairs')

        lib = _lib.load()
        counts = self._buffer('counts', K * batch, torch.int32, dev)
        out = self._buffer('out', (K * n_total, width), torch.float32, dev)
        out_frames = self._buffer('out_frames', K * n_total, torch.int32, dev)
        ws_bytes = lib.sst_tracklet_tta_views_workspace_bytes(n_total, batch, K, width)
        ws = self._buffer('workspace', max(ws_bytes, 256), torch.uint8, dev)
        a = _lib.TrackletTTAViewsArgs()
        a.points, a.frame_rows, a.sample_frames, a.block_offsets = st.points_ptr, at(st.at_fr), at(st.at_sf), at(st.at_blk)
        a.frames, a.frame_values, a.params = at(st.at_frames), at(st.at_fv), at(st.at_rec)
        a.out, a.out_frame_inds, a.counts = _lib.ptr(out), _lib.ptr(out_frames), _lib.ptr(counts)
        a.workspace, a.workspace_bytes, a.n_total = _lib.ptr(ws), ws.numel(), n_total
        a.batch, a.cols, a.deco, a.n_blocks = batch, cols, deco, int(st.blk_off[-1])
        a.n_frames, a.max_frames, a.n_views = st.total_frames, int(max(st.n_frames)), K
        _lib.check(lib.sst_tracklet_tta_views_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_tracklet_tta_views_f32')

        n_boxes, box_cols = int(st.boxes.size(0)), st.box_cols
        assert n_boxes == n_rows
        boxes_views = self._buffer('boxes_views', (K, n_boxes, box_cols), torch.float32, dev)
        b = _lib.TrackletTTABoxArgs()
        b.boxes, b.box_offsets, b.params, b.boxes_out = at(st.at_boxes), at(st.at_boff), at(st.at_rec), _lib.ptr(boxes_views)
        b.batch, b.cols, b.n_boxes, b.n_views = batch, box_cols, n_boxes, K
        _lib.check(lib.sst_tracklet_tta_boxes_f32(ctypes.byref(b), _lib.stream_ptr()), 'sst_tracklet_tta_boxes_f32')

        def staged(off, count, dtype, shape):
            nbytes = count * torch.empty((), dtype=dtype).element_size()
            return st.stage[off:off + nbytes].view(dtype).view(shape)

        old_boxes = staged(st.at_boxes, n_boxes * box_cols, torch.float32, (n_boxes, box_cols))
        e = st.at_extra
        got = counts.tolist()                                                    # the one host read of the call
        offsets = [0]
        for c in got:
            offsets.append(offsets[-1] + c)
        for i, trk in enumerate(tracklets):
            r0, r1 = st.ranges[i][0]
            trk.boxes = old_boxes[r0:r1]
            trk.size = r1 - r0
            trk.device = old_boxes.device
            trk.shared_pose = st.per_sample[i][4]
        return dict(points=[out[offsets[i]:offsets[i + 1]] for i in range(K * batch)],
                    pts_frame_inds=[out_frames[offsets[i]:offsets[i + 1]] for i in range(K * batch)],
                    points_packed=out[:offsets[-1]], frame_inds_packed=out_frames[:offsets[-1]], offsets=offsets, counts=got,
                    n_views=K, batch=batch, views=self.view_meta(), boxes_views=boxes_views, old_boxes=old_boxes,
                    box_ranges=[r[0] for r in st.ranges], ego_mats=staged(e[0], n_rows * 12, torch.float32, (n_rows, 12)),
                    row_sample=staged(e[1], n_rows, torch.int32, (n_rows,)), row_frame=staged(e[2], n_rows, torch.int32, (n_rows,)),
                    old_scores=staged(e[3], n_rows, torch.float64, (n_rows,)),
                    roi_scores=staged(e[4], n_rows, torch.float32, (n_rows,)), labels=staged(e[5], n_rows, torch.int32, (n_rows,)),
                    tracklets=list(tracklets), records=st.rec, seeds=params.seed.copy(),
                    shared_pose=[ps[4] for ps in st.per_sample])


def view_records_of(views):
    """[(flip_h, flip_v, angle)] -> a filled ``views`` array of sst_tracklet_tta_finish_args"""
    arr = (_lib.TrackletTTAView * MAX_VIEWS)()
    for k, (h, v, rot) in enumerate(views):
        angle = torch.tensor(rot, dtype=torch.float64).to(torch.float32)
        arr[k].flip_h, arr[k].flip_v, arr[k].rotate = int(bool(h)), int(bool(v)), 1
        arr[k].angle, arr[k].cos, arr[k].sin = float(angle), float(torch.cos(angle)), float(torch.sin(angle))
    return arr


@torch.no_grad()
def tta_finish(boxes, scores, valid, old_boxes, old_scores, ego_mats, views, merge='weighted', iou_merge_thresh=0.0,
               return_views=True):
    """``inverse_aug`` + ``update_from_prediction`` + ``merge_augs`` for every tracklet row of a batch in one launch
    (sst_tracklet_tta_finish).  boxes [K, n, 7], scores [K, n] float32, valid [K, n] bool / uint8: the decoded boxes of every view;
    old_boxes [n, >= 7] (un-augmented, shared pose), old_scores float64 [n], ego_mats [n, 12]; views: [(flip_h, flip_v, angle)].
    -> dict(merged [n, 8] float64 = (box, score) in ONE buffer, merged_boxes, merged_scores: its views; with ``return_views``
    view_boxes float32 [K, n, 7]: every view's boxes in the frames' own poses, view_scores float64 [K, n]: the scores the merge
    used)."""
    if merge not in MERGE_MODES:
        raise NotImplementedError(f'{WHERE}: merge mode {merge!r}; the reference has ' + ', '.join(MERGE_MODES))
    if not boxes.is_cuda:
        raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
    K, n = int(boxes.size(0)), int(boxes.size(1))
    if K != len(views) or K < 1 or K > MAX_VIEWS:
        raise RuntimeError(f'{WHERE}: {K} views of boxes and {len(views)} view records (1 to {MAX_VIEWS})')
    dev = boxes.device
    boxes = boxes[:, :, :7].to(torch.float32).contiguous()
    scores = scores.to(torch.float32).reshape(K, n).contiguous()
    valid = valid.reshape(K, n).to(torch.uint8).contiguous()
    old_boxes = old_boxes[:, :7].to(torch.float32).contiguous()
    old_scores = old_scores.to(torch.float64).contiguous()
    ego_mats = ego_mats.to(torch.float32).reshape(n, 12).contiguous()
    merged = torch.empty(n * 8, dtype=torch.float64, device=dev)
    lib = _lib.load()
    a = _lib.TrackletTTAFinishArgs()
    a.boxes, a.scores, a.valid = _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(valid)
    a.old_boxes, a.old_scores, a.mats = _lib.ptr(old_boxes), _lib.ptr(old_scores), _lib.ptr(ego_mats)
    a.merged_boxes, a.merged_scores = _lib.ptr(merged), ctypes.c_void_p(merged.data_ptr() + 8 * 7 * n)
    view_boxes = view_scores = ws = None
    if return_views:
        view_boxes = torch.empty((K, n, 7), dtype=torch.float32, device=dev)
        view_scores = torch.empty((K, n), dtype=torch.float64, device=dev)
        a.view_boxes, a.view_scores = _lib.ptr(view_boxes), _lib.ptr(view_scores)
    else:
        ws = torch.empty(max(lib.sst_tracklet_tta_finish_workspace_bytes(n, K), 16), dtype=torch.uint8, device=dev)
        a.workspace, a.workspace_bytes = _lib.ptr(ws), ws.numel()
    a.n_rows, a.n_views, a.mode, a.iou_merge_thresh = n, K, MERGE_MODES[merge], float(iou_merge_thresh)
    a.views = view_records_of(views)
    _lib.check(lib.sst_tracklet_tta_finish(ctypes.byref(a), _lib.stream_ptr()), 'sst_tracklet_tta_finish')
    return dict(merged=merged, merged_boxes=merged[:7 * n].view(n, 7), merged_scores=merged[7 * n:], view_boxes=view_boxes,
                view_scores=view_scores)


class TrackletTTADetector(TrackletDetector):
    """A ``TrackletDetector`` after ``attach_tracklet_tta``: ``aug_test`` and ``forward_test`` make the views of the batch on the
    device in one call, run the segmentor and the RoI head on them and merge in one launch.  Never built from a config: the
    builders keep refusing ``test_cfg.tta``."""

    tta = None
    tta_cfg = None
    # One pass over the K * B samples is NOT bit-equal to K passes of B samples: the fp32 linears of the box head's SIR layers are
    # ``x @ weight.t()`` (sst_amd.dense.tall_linear), a vendor GEMM whose tile and split choice follows the number of rows, so a
    # row's sum is rounded in another order when the batch grows (about 1e-6 relative per layer on the test model; every kernel of
    # this library on the path IS row- or segment-local: the segmentor's outputs are bit-equal).  The default therefore runs the
    # network once per view, as the reference does, with the views and the finish fused; True runs the single pass.
    tta_single_pass = False

    @torch.no_grad()
    def tta_network(self, v):
        """the segmentor and the RoI head on the views ``v`` of ``TrackletTTA.__call__``, once per view or, with
        ``tta_single_pass``, once over the K * B samples -> (decoded boxes [K, n, 7], scores [K, n], valid RoI mask [K, n])"""
        K, B = v['n_views'], v['batch']
        n = int(v['old_boxes'].size(0))
        head = self.roi_head
        dev = v['old_boxes'].device
        roi_frame_inds = v['row_frame'].long()
        if self.tta_single_pass:
            pts = self.fake_points_for_empty_input(v['points'])
            inds = self.fake_points_for_empty_input([f.long() for f in v['pts_frame_inds']])
            seg = self.segmentor.forward_train(points=pts, pts_frame_inds=inds, img_metas=None)
            sample = (torch.arange(K, device=dev, dtype=torch.int32)[:, None] * B + v['row_sample'][None]).to(torch.float32)
            rois = torch.cat([sample[:, :, None], v['boxes_views'][:, :, :7]], 2).reshape(K * n, 8)
            cls_preds = v['roi_scores'].repeat(K)
            # the extractor's cap on the pairs of a batch (max_all_point) is a cap per pass: K views in one pass get K times it
            ext = head.roi_extractor
            cap = ext.max_all_point
            ext.max_all_point = tuple(K * c for c in cap) if isinstance(cap, (tuple, list)) else K * cap
            try:
                res = head._bbox_forward(seg['seg_points'][:, :3], seg['seg_feats'], seg['batch_idx'], seg['pts_frame_inds'], rois,
                                         cls_preds, roi_frame_inds.repeat(K))
            finally:
                ext.max_all_point = cap
            boxes, scores = decode_tracklet_rows(rois, res['cls_score'], res['bbox_pred'], cls_preds, None, head.test_cfg)
            valid = res['valid_roi_mask'].reshape(K, n)
        else:
            sample = v['row_sample'].to(torch.float32)[:, None]
            per_view = []
            for k in range(K):
                pts = self.fake_points_for_empty_input(v['points'][k * B:(k + 1) * B])
                inds = self.fake_points_for_empty_input([f.long() for f in v['pts_frame_inds'][k * B:(k + 1) * B]])
                seg = self.segmentor.forward_train(points=pts, pts_frame_inds=inds, img_metas=None)
                rois = torch.cat([sample, v['boxes_views'][k, :, :7]], 1)
                res = head._bbox_forward(seg['seg_points'][:, :3], seg['seg_feats'], seg['batch_idx'], seg['pts_frame_inds'], rois,
                                         v['roi_scores'], roi_frame_inds)
                per_view.append(decode_tracklet_rows(rois, res['cls_score'], res['bbox_pred'], v['roi_scores'], None, head.test_cfg)
                                + (res['valid_roi_mask'],))
            boxes, scores, valid = (torch.stack([p[j] for p in per_view], 0) for j in range(3))
        return boxes.reshape(K, n, -1), scores.reshape(K, n), valid

    @torch.no_grad()
    def aug_forward(self, points, tracklet, seeds=None):
        """views -> ``tta_network`` -> finish, everything left on the device
        -> dict(views: what ``TrackletTTA.__call__`` returned, decoded_boxes [K, n, 7], decoded_scores [K, n], valid [K, n],
        and ``tta_finish``'s outputs)"""
        if not torch.cuda.is_available():
            raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
        self.from_collate_format(tracklet, None)
        v = self.tta(points, tracklet, seeds=seeds)
        boxes, scores, valid = self.tta_network(v)
        cfg = self.tta_cfg
        out = tta_finish(boxes, scores, valid, v['old_boxes'], v['old_scores'], v['ego_mats'], self.tta.views, cfg['merge'],
                         cfg.get('iou_merge_thresh', 0.0))
        out.update(views=v, decoded_boxes=boxes, decoded_scores=scores, valid=valid)
        return out

    def aug_test(self, points, img_metas=None, pts_frame_inds=None, tracklet=None, rescale=False, seeds=None):
        """points: per sample the per-frame points as ``TrackletAugment.__call__`` takes them (what LoadTrackletPoints leaves:
        the rest of the ``tta_pipeline`` runs here); tracklet: one frozen LiDARTracklet per sample with ``pose_list``.
        ``pts_frame_inds`` is not read: the frames are the structure of ``points``.  -> the tracklets as ``merge_augs`` leaves
        ``result_list[0]``: boxes float64 [n, 7] in every frame's own pose, the merged scores, ``pose_list`` None"""
        out = self.aug_forward(points, tracklet, seeds=seeds)
        merged = out['merged'].cpu()                                             # the one host read behind the network
        n = int(out['views']['old_boxes'].size(0))
        boxes, scores = merged[:7 * n].view(n, 7), merged[7 * n:]
        for trk, (r0, r1) in zip(tracklet, out['views']['box_ranges']):
            trk.boxes = boxes[r0:r1].clone()
            trk.size = r1 - r0
            trk.device = trk.boxes.device
            trk.score_list = scores[r0:r1].tolist()
            trk.type = int(trk.type)
            trk.pose_list = None
        return list(tracklet)

    def forward_test(self, points, img_metas=None, img=None, **kwargs):
        if not isinstance(points, list):
            raise TypeError('{} must be a list, but got {}'.format('points', type(points)))
        return self.aug_test(points, img_metas, **kwargs)


def attach_tracklet_tta(det, tta_cfg, pipeline):
    """Rebind a ``TrackletDetector`` that was built WITHOUT ``test_cfg.tta`` to ``TrackletTTADetector``.  tta_cfg: the config's
    ``test_cfg.tta`` block, ``dict(merge='max' | 'weighted' | 'iou_clamped_weighted'[, iou_merge_thresh=...])``; pipeline: its
    ``tta_pipeline`` (or a ``TrackletTTA``).  -> the detector.  Without this call a detector is what it was."""
    if not isinstance(det, TrackletDetector):
        raise TypeError(f'{WHERE}: attach_tracklet_tta needs a TrackletDetector, got {type(det).__name__}')
    cfg = dict(tta_cfg)
    merge = cfg.get('merge')
    if merge not in MERGE_MODES:
        raise NotImplementedError(f'{WHERE}: test_cfg.tta merge {merge!r}; the reference has ' + ', '.join(MERGE_MODES))
    if merge == 'iou_clamped_weighted' and 'iou_merge_thresh' not in cfg:
        raise KeyError(f'{WHERE}: merge=\'iou_clamped_weighted\' reads test_cfg.tta.iou_merge_thresh')
    plan = pipeline if isinstance(pipeline, TrackletTTA) else TrackletTTA.from_pipeline(pipeline)
    if type(det) is not TrackletTTADetector:
        if type(det) is not TrackletDetector:
            raise TypeError(f'{WHERE}: {type(det).__name__} is a subclass of TrackletDetector: rebinding it would drop its methods')
        det.__class__ = TrackletTTADetector
    det.tta, det.tta_cfg = plan, cfg
    return det


__all__ = ['TrackletTTA', 'TrackletTTADetector', 'attach_tracklet_tta', 'tta_finish', 'MAX_VIEWS', 'MERGE_MODES']

"""The kernels of csrc/tracklet_prep.hip on the GPU.  Rules: the affinity of a pair is bit-equal (compared as int32)
to the maximum of sst_amd.aligned_iou_3d over the pair's shared frames; candidate lists, crops, counts and keep masks equal the
reference's own results (tests/golden/tracklet_prep.npz) exactly; the crops of every frame and box are ``points[m[:, b] != 0]`` with
``m = sst_amd.points_in_boxes_batch(...)``, rows and indices exactly; two runs are bit-equal."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import tracklet_ref as T
import tracklet_prep_ref as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold():
    return load_golden('tracklet_prep.npz')


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def by_hand(trks_pd, trks_gt):
    """the reference's pair loop on the parent's ops: per pair the maximum of aligned_iou_3d over the shared frames (all pairs'
    frames in ONE aligned_iou_3d call; the maximum per pair with torch.max, where a NaN wins) -> per predicted tracklet float32 array"""
    import sst_amd
    a_rows, b_rows, spans, k = [], [], [], 0
    by_seg = {}
    for i, t in enumerate(trks_gt):
        by_seg.setdefault(t.segment_name, []).append(i)
    for pd in trks_pd:
        for g in by_seg.get(pd.segment_name, []):
            i1, i2 = P.shared(pd, trks_gt[g])
            a_rows.append(pd.boxes[i1].reshape(-1, 7))
            b_rows.append(trks_gt[g].boxes[i2].reshape(-1, 7))
            spans.append((k, k + len(i1)))
            k += len(i1)
    iou = sst_amd.aligned_iou_3d(torch.cat(a_rows).to(DEV), torch.cat(b_rows).to(DEV)).cpu() if k else torch.zeros(0)
    out, s = [], 0
    for pd in trks_pd:
        n = len(by_seg.get(pd.segment_name, []))
        vals = [iou[a:b].max() if b > a else torch.zeros(()) for a, b in spans[s:s + n]]       # tensors: a NaN keeps its bits
        out.append(torch.stack(vals).numpy() if vals else np.zeros(0, np.float32))
        s += n
    return out


def run_affinity(trks_pd, trks_gt, device=None, **kw):
    import sst_amd
    out = sst_amd.tracklet_affinity([P.lidar(t, device) for t in trks_pd], [P.lidar(t, device) for t in trks_gt], device=DEV, **kw)
    torch.cuda.synchronize()
    return out


def assert_bit_equal(got, want, what):
    for k, ((_, a), w) in enumerate(zip(got, want)):
        assert a.dtype == np.float32 and a.shape == w.shape, (what, k)
        assert np.array_equal(bits(a), bits(w)), (what, k, a, w)


# ---- affinity ---------------------------------------------------------------------------------------------------------------------

def test_affinity_of_the_golden_scene_is_bit_equal_to_the_parent_iou_and_gives_the_reference_candidates(gold):
    import sst_amd
    pd, gt = P.gold_scene(gold)
    got = run_affinity(pd, gt)
    assert_bit_equal(got, by_hand(pd, gt), 'golden')
    assert [g.tolist() for g, _ in got] == [list(range(5))] * 5 + [[]]
    err = float(np.abs(np.stack([a for _, a in got[:5]]).astype(np.float64) - gold['aff_f64']).max())
    print('affinity vs the reference float64: err', err, 'gap', float(gold['noise_aff']), 'bar', T.bar(gold['noise_aff']))
    assert err <= T.bar(gold['noise_aff'])
    lp, lg = [P.lidar(t) for t in pd], [P.lidar(t) for t in gt]
    cands = sst_amd.generate_candidates(lp, lg, float(gold['thresh']), device=DEV)
    want = [c.tolist() for c in P.split(gold['cand_flat'], gold['cand_counts'])]
    assert [[lg.index(c) for c in cl] for cl in cands] == want and cands[5] == []
    assert sst_amd.candidate_stats(lp, cands) == tuple(gold['stats'].tolist())
    # one pair through LiDARTracklet.max_iou: a Python float of the same bits; device-resident tracklets; one segment per launch
    v = lp[2].max_iou(lg[1])
    assert isinstance(v, float) and np.float32(v) == got[2][1][1] and lp[1].max_iou(lg[3]) == 0.0
    assert_bit_equal(run_affinity(pd, gt, device=DEV), [a for _, a in got], 'device tracklets')
    assert_bit_equal(run_affinity(pd, gt, row_budget=1), [a for _, a in got], 'row budget')


def edge_scene():
    rng = np.random.default_rng(7)
    path = T.track_boxes(rng, 320, 0)
    mk = lambda fr, seg, name, boxes=None, scale=0.5: P.Trk(T.jitter(rng, path[list(fr)], scale) if boxes is None else boxes,   # noqa: E731
                                                           P.frames_ts(fr), [0.5] * len(list(fr)), 1, seg, name)
    pd = [mk(range(257), 'e5', 'long'), mk([5], 'e5', 'one')]
    gt = [mk(range(129), 'e5', 'g129'), mk(range(63), 'e5', 'g63'), mk(range(64), 'e5', 'g64'), mk(range(65), 'e5', 'g65'),
          mk(range(300, 311), 'e5', 'later')]                              # shared 129, 63, 64, 65 and 0 (disjoint in time); 1 with 'one'
    for seg, n_gt in (('e1', 1), ('e3', 3), ('e4', 4)):                    # workgroup tails: ranges of 1, 3 and 4
        pd += [mk(range(10, 50), seg, f'{seg}a'), mk(range(0, 257, 2), seg, f'{seg}b', scale=1.5)]
        gt += [mk(sorted(rng.choice(120, 30 + 7 * k, replace=False).tolist()), seg, f'{seg}g{k}', scale=0.3 * k) for k in range(n_gt)]
    # geometry on both sides of bev_overlap's early out, one pair per case: tracklets of one frame each
    base = np.array([3.0, -2.0, 0.5, 2.0, 4.0, 1.5, 0.0], np.float32)

    def moved(dx=0.0, dy=0.0, **kw):
        b = base.copy()
        b[0] += dx
        b[1] += dy
        for k, v in kw.items():
            b[dict(w=3, l=4, h=5, yaw=6, x=0, z=2)[k]] = v
        return b[None]

    cases = [moved(dx=2.0 + 1e-3), moved(dx=2.0), moved(dx=2.0, dy=4.0), moved(w=1.0, l=2.0), moved(dx=0.3, yaw=0.7), moved(dx=40.0),
             moved(dx=4.4, yaw=0.3), moved(w=0.0), moved(x=float('nan')), moved(h=0.0), moved(z=float('inf')), moved(), moved(w=float('inf'))]
    #        just apart      touching face  touching corner    concentric            overlapping            far (rejected)
    #        inside the reject's reach, no overlap   zero size    NaN     zero height    infinite z   identical   infinite width
    for k, c in enumerate(cases):
        pd.append(mk([k], 'geo', f'p{k}', np.repeat(base[None], 1, 0)))
        gt.append(mk([k], 'geo', f'q{k}', c.astype(np.float32)))
    pd.append(mk(range(len(cases)), 'geo', 'all', np.repeat(base[None], len(cases), 0)))       # the maximum over every case
    return pd, gt, len(cases)


def test_affinity_at_every_edge_is_bit_equal_to_the_parent_iou():
    pd, gt, n_cases = edge_scene()
    got = run_affinity(pd, gt)
    want = by_hand(pd, gt)
    assert_bit_equal(got, want, 'edge')
    assert sorted({len(a) for _, a in got}) == [1, 3, 4, 5, n_cases]
    long, one = got[0][1], got[1][1]
    assert (long[:4] > 0.3).all() and long[4] == 0.0 and (one[:4] > 0).all() and one[4] == 0.0      # frame 5 lies in the first four
    geo = np.stack([a for _, a in got[-n_cases - 1:-1]])
    diag = np.diag(geo)
    print('geometry cases', diag.tolist(), 'all', got[-1][1].tolist())
    assert (geo[~np.eye(n_cases, dtype=bool)] == 0).all()                # different frames: nothing shared
    assert diag[0] == 0 and diag[5] == 0 and diag[6] == 0 and 0.2 < diag[3] < 0.3 and diag[4] > 0.2 and diag[11] > 0.99
    again = run_affinity(pd, gt)
    assert_bit_equal(again, [a for _, a in got], 'two runs')


def test_timestamps_are_compared_as_int64():
    """timestamps that differ only above bit 32, or only below bit 24, are different frames"""
    box = np.array([[1.0, 2.0, 0.0, 2.0, 4.0, 1.5, 0.2]], np.float32)
    t0 = T.TS0 + 123_456_789
    mk = lambda ts, name: P.Trk(np.repeat(box, len(ts), 0), ts, [0.5] * len(ts), 1, 's', name)      # noqa: E731
    pd = [mk([t0], 'p')]
    gt = [mk([t0 + (1 << 33)], 'high'), mk([t0 + 1], 'low'), mk([t0 - (1 << 32), t0 + 3], 'both'), mk([t0], 'same'),
          mk([t0 - 5, t0, t0 + (1 << 40)], 'mixed')]
    assert np.float32(t0) == np.float32(t0 + 1) and (t0 & 0xffffffff) == ((t0 + (1 << 33)) & 0xffffffff)
    got = run_affinity(pd, gt)[0][1]
    print('int64 timestamps', got.tolist())
    assert got[:3].tolist() == [0.0, 0.0, 0.0] and got[3] > 0.99 and got[4] == got[3]


# ---- crops ------------------------------------------------------------------------------------------------------------------------

def parent_crops(points_list, boxes_list):
    """rows, src, counts of every frame and box from the parent's membership: points[m[:, b] != 0]"""
    import sst_amd
    rows, src, counts = [], [], []
    for p, b in zip(points_list, boxes_list):
        if p.size(0) == 0 or b.size(0) == 0:
            counts.append(torch.zeros(b.size(0), dtype=torch.int32, device=DEV))
            continue
        m = sst_amd.points_in_boxes_batch(p[None, :, :3].contiguous(), b[None].contiguous())[0]        # [N, B]
        idx = (m.t() != 0).nonzero()                                                                     # (box, ascending point)
        src.append(idx[:, 1])
        rows.append(p[idx[:, 1]])
        counts.append((m != 0).sum(0).to(torch.int32))
    cols = points_list[0].size(1)
    return (torch.cat(rows + [torch.zeros((0, cols), device=DEV)]), torch.cat(src + [torch.zeros(0, dtype=torch.long, device=DEV)]),
            torch.cat(counts + [torch.zeros(0, dtype=torch.int32, device=DEV)]))


def check_crops(points_list, boxes_list):
    import sst_amd
    rows, src, counts, offsets = sst_amd.box_point_crops(points_list, boxes_list)
    only = sst_amd.box_point_counts(points_list, boxes_list)
    torch.cuda.synchronize()
    w_rows, w_src, w_counts = parent_crops(points_list, boxes_list)
    assert counts.dtype == torch.int32 and src.dtype == torch.long and rows.dtype == torch.float32
    assert torch.equal(counts, w_counts) and torch.equal(only, counts)
    assert torch.equal(src, w_src) and torch.equal(rows.view(torch.int32), w_rows.view(torch.int32))
    assert offsets[0] == 0 and torch.equal(offsets[1:], counts.long().cumsum(0)) and int(offsets[-1]) == rows.size(0)
    return rows, src, counts, offsets


@pytest.mark.parametrize('cols', [3, 5, 6])
def test_crops_at_every_tile_and_chunk_edge_equal_the_parent_membership(cols):
    from sst_amd import _lib
    tile, chunk = _lib.load().sst_box_crops_tile(), _lib.load().sst_box_crops_box_chunk()
    rng = np.random.default_rng(100 + cols)
    points_list, boxes_list = [], []
    for n in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1):
        for nb in (0, 1, 64, 65, chunk + 1):
            boxes = np.concatenate([T.track_boxes(rng, 1, k % 3) for k in range(nb)] + [np.zeros((0, 7), np.float32)])
            boxes[:, 3:6] *= 2.5
            pts = P.points_around(rng, boxes, (n * 2) // 3 if nb else 0, n - ((n * 2) // 3 if nb else 0), cols, margin=0)
            points_list.append(torch.as_tensor(pts).to(DEV))
            boxes_list.append(torch.as_tensor(boxes).to(DEV))
    rows, src, counts, _ = check_crops(points_list, boxes_list)
    print('cols', cols, 'frames', len(points_list), 'rows', rows.size(0), 'boxes with points', int((counts > 0).sum()), 'of', counts.numel())
    assert rows.size(0) > 5000 and int((counts > 0).sum()) > 300
    again = __import__('sst_amd').box_point_crops(points_list, boxes_list)
    assert torch.equal(again[0].view(torch.int32), rows.view(torch.int32)) and torch.equal(again[1], src)      # two runs


def test_crops_of_shared_duplicate_and_missing_points():
    rng = np.random.default_rng(3)
    box = np.array([0.0, 0.0, -1.0, 2.0, 4.0, 2.0, 0.4], np.float32)
    three = np.stack([box, box * np.array([1, 1, 1, 1.5, 1.5, 1, 1], np.float32), box * np.array([1, 1, 1, 0.5, 0.5, 1, 1], np.float32),
                      box + np.array([60, 0, 0, 0, 0, 0, 0], np.float32)])               # three concentric boxes and one far away
    pts = rng.uniform(-1, 1, (300, 6)).astype(np.float32) * np.array([3, 3, 1.5, 1, 1, 1], np.float32)
    pts[:3, :3] = 0.0                                                                     # the centre: inside all three
    pts[10:13] = pts[9]                                                                   # duplicate points
    full = torch.as_tensor(pts).to(DEV)
    empty = torch.zeros((0, 6), device=DEV)
    b = torch.as_tensor(three).to(DEV)
    rows, src, counts, offsets = check_crops([full, empty, full], [b, b, b])             # an empty frame between full ones
    c = counts.cpu().numpy().reshape(3, 4)
    assert (c[1] == 0).all() and np.array_equal(c[0], c[2]) and c[0][3] == 0 and c[0][1] >= c[0][0] >= c[0][2] >= 3
    for k in range(3):                                                                    # the centre in each of the three boxes
        assert src[offsets[k]:offsets[k] + 3].tolist() == [0, 1, 2]
    src, offsets = src.cpu().numpy(), offsets.cpu().numpy()
    for k in range(len(offsets) - 1):
        s = src[offsets[k]:offsets[k + 1]]
        assert (np.diff(s) > 0).all()                                                     # ascending inside every box
        dup = set(range(9, 13)) & set(s.tolist())
        assert dup in (set(), set(range(9, 13)))                                          # duplicate points: all of them or none


def test_crops_counts_and_keep_masks_of_the_golden_scene_equal_the_reference(gold):
    import sst_amd
    trks, frames = P.gold_crop_scene(gold)
    lt = [P.lidar(t) for t in trks]
    pcs = sst_amd.crop_tracklet_points(lt, frames, float(gold['extra_width']), device=DEV)
    flat = [p for tr in pcs for p in tr]
    assert [len(p) for p in flat] == gold['crop_num_pts'].tolist()
    assert np.array_equal(bits(np.concatenate(flat)), bits(gold['crop_rows']))
    assert [n for t in lt for n in t.num_pts_in_boxes] == gold['crop_num_pts'].tolist() and [len(tr) for tr in pcs] == gold['crop_lens'].tolist()
    small = sst_amd.crop_tracklet_points([P.lidar(t) for t in trks], frames, float(gold['extra_width']), device=DEV, byte_budget=1)
    assert all(np.array_equal(a, b) for x, y in zip(pcs, small) for a, b in zip(x, y))      # one frame per launch: the same crops
    boxes_list = [torch.as_tensor(b).to(DEV) for b in P.split(gold['re_boxes'], gold['re_box_lens'])]
    points_list = [torch.as_tensor(np.ascontiguousarray(p)).to(DEV) for p in P.split(gold['re_points'], gold['re_pt_lens'])]
    for name, cfg in sst_amd.tracklet_prep.REMOVE_EMPTY_DEFAULTS.items():
        masks, dropped = sst_amd.remove_empty_boxes(boxes_list, points_list, cfg['bottom_lift'], cfg['extra_hw'],
                                                    box_grouping=cfg['box_grouping'], group_size=cfg['group_size'])
        assert np.array_equal(np.concatenate(masks), gold[f're_mask_{name}']) and dropped == [False, True, True, False]

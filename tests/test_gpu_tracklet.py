"""The kernels of csrc/tracklet.hip on the GPU against the reference's own results (tests/golden/tracklet_train.npz) and the
restatement of tests/tracklet_ref.py.  Rules: chosen candidate, assigned_gt_inds, permutation, counts, reg_mask
and labels exactly; the IoU bit for bit equal to aligned_iou_3d built on the box ops' aligned overlap; soft labels and targets
within max(4 x the reference's own float32-vs-float64 gap, 1e-6) of the reference's float64 run (of the largest element); the rows
forward bit for bit equal to torch indexing + cat, backward bit for bit on integer data and within the same bar of a float64
restatement on real data; two runs bit-equal.  Every test prints what it achieved."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import tracklet_ref as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT = ('chosen', 'assigned_gt_inds', 'frame_inds', 'counts', 'reg_mask', 'labels')
ROW_KEYS = ('rois', 'src', 'gt_index', 'labels', 'iou', 'soft_label', 'reg_mask', 'targets', 'frame_inds', 'scores', 'pos_gt_bboxes')
FRAME_KEYS = ('matched', 'overlaps', 'assigned_gt_inds')


@pytest.fixture(scope='module')
def gold():
    return load_golden('tracklet_train.npz')


def lidar(trk, name='t', device=None):
    import sst_amd
    t = sst_amd.LiDARTracklet('seg', name, int(trk.type), True, trk.boxes.clone(), list(trk.ts_list), list(trk.score_list))
    t.freeze()
    return t.to(device) if device is not None else t


def fused(trks, cand_lists, cfg, device=None):
    import sst_amd
    out = sst_amd.tracklet_targets([lidar(t, str(i), device) for i, t in enumerate(trks)],
                                   [[lidar(c, 'c', device) for c in cs] for cs in cand_lists],
                                   dict(cfg, assigner=dict(object_centric=cfg['object_centric'], iou_thr=cfg['iou_thr'])), device=DEV)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def gold_runs(gold):
    """the fused targets of the golden batch, object_centric off and on: computed once, read by the tests below"""
    trks, cand_lists = T.gold_scene(gold)
    return {oc: fused(trks, cand_lists, dict(T.GOLD_CFG, object_centric=bool(oc))) for oc in (0, 1)}


@pytest.mark.parametrize('oc', [0, 1])
def test_targets_equal_the_reference(gold, gold_runs, oc):
    got = gold_runs[oc]
    for k in EXACT:
        assert np.array_equal(got[k].cpu().numpy().astype(np.int64), gold[f'oc{oc}_{k}'].astype(np.int64)), k
    for k in ('iou', 'soft_label', 'targets'):
        err, gap = T.rel_err(got[k].cpu().numpy(), gold[f'oc{oc}_{k}_f64']), float(gold[f'noise_oc{oc}_{k}'])
        print(k, 'err', err, 'gap', gap, 'bar', T.bar(gap))
        assert err <= T.bar(gap), (k, err)
    n_pos = got['counts'][:, 0].cpu()
    assert int(n_pos[1]) == 0 and int(n_pos[5]) == 0 and int(got['chosen'][5]) == 0      # no candidate; one that shares nothing


@pytest.mark.parametrize('oc', [0, 1])
def test_rows_equal_the_restatement_on_the_kernel_iou(gold, gold_runs, oc):
    """every output of the launch against the reference's algorithm run tracklet by tracklet on the device with the library's
    aligned IoU: integers, boxes, IoU, soft labels and targets bit for bit"""
    import sst_amd
    trks, cand_lists = T.gold_scene(gold)
    on_dev = lambda t: T.Trk(t.boxes.to(DEV), t.ts_list, t.score_list, t.type)      # noqa: E731
    stats = {}
    ref = T.targets([on_dev(t) for t in trks], [[on_dev(c) for c in cs] for cs in cand_lists], dict(T.GOLD_CFG, object_centric=bool(oc)),
                    torch.float32, iou_fn=sst_amd.aligned_iou_3d, stats=stats)
    got = gold_runs[oc]
    for k in ref:
        a, b = got[k].cpu(), ref[k]
        assert torch.equal(a, b.to(a.dtype)), k
    print('the reference-style run:', stats, '- the fused run: 1 launch, 0 host reads')


def test_iou_is_bit_equal_to_the_box_ops(gold, gold_runs):
    import sst_amd
    got = gold_runs[0]
    pos = got['gt_index'] >= 0
    ious = sst_amd.aligned_iou_3d(got['rois'][pos, 1:8].contiguous(), got['gts'][got['gt_index'][pos].long()].contiguous())
    assert int(pos.sum()) > 300 and torch.equal(ious, got['iou'][pos])
    # and in frame order, against LiDARTracklet.self_ious (the reference's own route to the same numbers)
    trks, cand_lists = T.gold_scene(gold)
    t4, c4 = lidar(trks[4], 'a', DEV), lidar(cand_lists[4][2], 'b', DEV)
    r0 = int(sum(gold['lens'][:4]))
    assert torch.equal(t4.self_ious(c4), got['overlaps'][r0:r0 + len(t4)])
    assert not pos.all() and not got['iou'][~pos].any()        # object_centric off: a negative is a row without a match, IoU 0


def test_batch_equals_the_assigner_per_tracklet(gold, gold_runs):
    import sst_amd
    trks, cand_lists = T.gold_scene(gold)
    got = gold_runs[1]
    assigner = sst_amd.TrackletAssigner(object_centric=True, iou_thr=T.GOLD_CFG['iou_thr'])
    chosen = got['chosen'].tolist()
    r0 = 0
    for t, (trk, cands) in enumerate(zip(trks, cand_lists)):
        n = len(trk.ts_list)
        pd = lidar(trk, 'p', DEV)
        gt = lidar(cands[chosen[t]], 'g', DEV) if chosen[t] >= 0 else pd.new_empty()
        res = assigner.assign(pd, gt)
        assert res.num_gts == len(gt)
        assert torch.equal(res.gt_inds, got['assigned_gt_inds'][r0:r0 + n]) and torch.equal(res.max_overlaps, got['overlaps'][r0:r0 + n])
        assert torch.equal(res.scores, torch.tensor(trk.score_list, dtype=torch.float32, device=DEV).reshape(-1))
        assert torch.equal(res.labels, torch.where(res.gt_inds > 0, int(gt.type), -1))
        for k in ('iou', 'targets', 'frame_inds', 'reg_mask'):      # the rest of the one-tracklet launch (no soft label: an assigner has no class thresholds)
            assert torch.equal(res.targets[k], got[k][r0:r0 + n]), (t, k)
        r0 += n


def test_outputs_do_not_depend_on_the_order_of_the_tracklets(gold, gold_runs):
    trks, cand_lists = T.gold_scene(gold)
    perm = [4, 0, 7, 1, 6, 2, 5, 3]
    cfg = dict(T.GOLD_CFG, object_centric=True)
    got, base = fused([trks[p] for p in perm], [cand_lists[p] for p in perm], cfg), gold_runs[1]
    again = fused([trks[p] for p in perm], [cand_lists[p] for p in perm], cfg, device=DEV)       # boxes already on the device
    starts = np.concatenate([[0], np.cumsum(gold['lens'])])
    cstarts = np.concatenate([[0], np.cumsum([sum(len(c.ts_list) for c in cs) for cs in cand_lists])])
    r0 = g0 = 0
    for slot, p in enumerate(perm):
        n = int(gold['lens'][p])
        a, b = slice(r0, r0 + n), slice(int(starts[p]), int(starts[p]) + n)
        for k in ROW_KEYS + FRAME_KEYS:
            x, y = got[k][a].clone(), base[k][b].clone()
            if k == 'rois':
                assert bool((x[:, 0] == slot).all()) and bool((y[:, 0] == p).all())
                x, y = x[:, 1:], y[:, 1:]
            if k == 'src':
                x, y = x - r0, y - int(starts[p])
            if k == 'gt_index':
                x, y = torch.where(x >= 0, x - g0, x), torch.where(y >= 0, y - int(cstarts[p]), y)
            assert torch.equal(x, y), (p, k)
        assert torch.equal(got['counts'][slot], base['counts'][p]) and int(got['chosen'][slot]) == int(base['chosen'][p])
        r0, g0 = r0 + n, g0 + sum(len(c.ts_list) for c in cand_lists[p])
    for k in ROW_KEYS + FRAME_KEYS + ('chosen', 'counts'):
        assert torch.equal(got[k], again[k]), k


def test_single_tracklet_and_empty_members(gold, gold_runs):
    trks, cand_lists = T.gold_scene(gold)
    cfg = dict(T.GOLD_CFG, object_centric=True)
    one = fused([trks[3]], [cand_lists[3]], cfg)                      # T = 1
    r0 = int(sum(gold['lens'][:3]))
    for k in ('iou', 'soft_label', 'targets', 'frame_inds', 'reg_mask', 'labels', 'assigned_gt_inds'):
        assert torch.equal(one[k], gold_runs[1][k][r0:r0 + 65]), k
    assert one['counts'].tolist() == [gold['oc1_counts'][3].tolist()] and one['chosen'].tolist() == [0]
    # a member without frames between two others, and one whose every candidate is empty
    empty = T.Trk(np.zeros((0, 7), np.float32), [], [], 1)
    got = fused([trks[6], empty, trks[7]], [cand_lists[6], [empty], [empty, empty]], cfg)
    assert got['counts'].tolist() == [gold['oc1_counts'][6].tolist(), [0, 0], [0, 17]] and got['chosen'].tolist() == [0, 0, 0]
    assert torch.equal(got['targets'][:30], gold_runs[1]['targets'][int(sum(gold['lens'][:6])):int(sum(gold['lens'][:7]))])
    tail = slice(30, 47)
    assert not got['reg_mask'][tail].any() and not got['iou'][tail].any() and bool((got['gt_index'][tail] == -1).all())
    assert torch.equal(got['frame_inds'][tail], torch.arange(17, device=DEV)) and bool((got['rois'][tail, 0] == 2).all())
    import sst_amd
    none = sst_amd.tracklet_targets([], [], cfg, device=DEV)
    assert none['rois'].shape == (0, 8) and none['counts'].shape == (0, 2)


# ---- the rows of the box head --------------------------------------------------------------------------------------------------

def rows_case(F, m, repeat, seed, integer=False):
    """n points, m output rows; point 5 appears in ``repeat`` rows (1, 2 or 200 for the combined form's every-box-of-the-tracklet
    case), rows 0 and m - 1 are the pool's fake row (-1)"""
    g = torch.Generator().manual_seed(seed)
    n, n_rois = 61, 23
    draw = (lambda *s: torch.randint(-4, 5, s, generator=g).float()) if integer else (lambda *s: torch.randn(*s, generator=g))
    feats, xyz = draw(n, F), draw(n, 3)
    pts_frame, roi_frame = torch.randint(0, 4, (n,), generator=g), torch.randint(0, 4, (n_rois,), generator=g)
    others = torch.tensor([i for i in range(n) if i != 5])
    pts_inds = others[torch.randint(0, n - 1, (m,), generator=g)]
    roi_inds = torch.randint(0, n_rois, (m,), generator=g)
    where = 1 + torch.randperm(max(m - 2, 0), generator=g)[:repeat]
    pts_inds[where] = 5
    pts_inds[0], roi_inds[0] = -1, -1
    pts_inds[m - 1] = -1
    scores = torch.rand(n_rois, generator=g)
    weight = draw(m, F + 2)
    return [x.to(DEV) for x in (feats, xyz, pts_frame, pts_inds, roi_inds, roi_frame, scores, weight)]


@pytest.mark.parametrize('F', [64, 67])
@pytest.mark.parametrize('m,repeat', [(1, 1), (63, 2), (65, 1), (5000, 200)])
def test_rows_forward_and_integer_backward_are_bit_equal(F, m, repeat):
    import sst_amd
    feats, xyz, pts_frame, pts_inds, roi_inds, roi_frame, scores, weight = rows_case(F, m, repeat, 100 + m, integer=True)
    assert int((pts_inds == 5).sum()) == min(repeat, max(m - 2, 0))
    for combined in (True, False):
        for with_scores in (True, False):
            feats.requires_grad_(True)
            out, oxyz = sst_amd.tracklet_rows(feats, xyz, pts_frame, pts_inds, roi_inds, roi_frame, scores, combined=combined,
                                              with_roi_scores=with_scores)
            ref, rxyz = T.rows(feats, xyz, pts_frame, pts_inds, roi_inds, roi_frame, scores, combined, with_scores)
            assert out.shape == (m, F + combined + with_scores) and torch.equal(out, ref) and torch.equal(oxyz, rxyz)
            assert torch.equal(out[0, :F], feats[-1].detach()) and not oxyz.requires_grad              # the fake row reads the last row
            w = weight[:, :out.size(1)]
            got, = torch.autograd.grad((out * w).sum(), feats)
            exp, = torch.autograd.grad((ref * w).sum(), feats)
            assert torch.equal(got, exp), (combined, with_scores)            # small integers: every order of the sum is exact


@pytest.mark.parametrize('F', [64, 67])
def test_rows_backward_on_real_data_in_a_fixed_order(F):
    import sst_amd
    m = 5000
    feats, xyz, pts_frame, pts_inds, roi_inds, roi_frame, scores, weight = rows_case(F, m, 200, 7)
    feats.requires_grad_(True)
    out, _ = sst_amd.tracklet_rows(feats, xyz, pts_frame, pts_inds, roi_inds, roi_frame, scores, combined=True, with_roi_scores=True)
    w = weight[:, :out.size(1)].contiguous()
    got, = torch.autograd.grad(out, feats, w, retain_graph=True)
    again, = torch.autograd.grad(out, feats, w)
    assert torch.equal(got, again)                                           # two runs are bit-equal
    ref64 = T.rows_grad(w.cpu(), pts_inds.cpu(), feats.size(0), F, torch.float64)
    ref32 = T.rows_grad(w.cpu(), pts_inds.cpu(), feats.size(0), F, torch.float32)
    gap = T.rel_err(ref32.numpy(), ref64.numpy())
    err = T.rel_err(got.cpu().numpy(), ref64.numpy())
    print('F', F, 'err', err, 'restatement float32-vs-float64 gap', gap, 'bar', T.bar(gap))
    assert err <= T.bar(gap)
    assert torch.equal(got.cpu(), ref32)                                     # the same order of the additions as the restatement
    assert int((pts_inds == 5).sum()) == 200 and float(got[5].abs().max()) > 0

"""The kernels of csrc/cluster_head.hip on the GPU against the reference's own results (tests/golden/cluster_head_train.npz) and
the restatement of tests/cluster_head_ref.py.  Rules: integers, centre deltas, velocities and weights bit for
bit; log / sin / cos / exp / atan2 / sigmoid within 2 ulp of torch's CPU functions; losses and gradients within max(4 x the
reference's own float32-vs-float64 gap, 1e-6) of float64 autograd of the restatement.  Every test prints what it achieved."""
import ast
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import cluster_head_ref as R
from test_cluster_head_host import CASES, restated_targets, scene

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gold():
    return load_golden('cluster_head_train.npz')


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def gpu_targets(sc, rows=None, tasks=None, names=None, labels=None, boxes=None):
    import sst_amd
    sel = slice(None) if rows is None else rows
    xyz = dev(sc['xyz'][sel])
    xa = dev(sc['xyz_assign'][sel])
    out = sst_amd.cluster_targets(xa, dev(sc['cluster_inds'][sel]), [dev(b) for b in (boxes or sc['boxes'])],
                                  [dev(l) for l in (labels or sc['labels'])], tasks or sc['tasks'], names or sc['names'],
                                  sc['code'], sc['width'], xyz_base=xyz)
    torch.cuda.synchronize()
    return [tuple(v.cpu() for v in task) for task in out]


def compare_targets(got, want, code, what):
    worst = 0
    for t, ((lab, assigned, tg, wt), (r_lab, r_assigned, r_tg, r_wt)) in enumerate(zip(got, want)):
        assert torch.equal(lab, r_lab), (what, t)
        assert torch.equal(assigned.long(), r_assigned), (what, t)
        plain = [0, 1, 2] + ([8, 9] if code == 10 else [])
        assert torch.equal(tg[:, plain], r_tg[:, plain]) and torch.equal(wt, r_wt), (what, t)
        if len(tg):
            worst = max(worst, int(R.ulp_distance(tg[:, 3:8].numpy(), r_tg[:, 3:8].numpy()).max()))
    print(f'{what}: integers, deltas and weights equal; log / sin / cos columns within {worst} ulp')
    assert worst <= 2


@pytest.mark.parametrize('case', list(CASES))
def test_targets_equal_the_reference_and_the_restatement(gold, case):
    sc = scene(gold, case)
    got = gpu_targets(sc)
    compare_targets(got, restated_targets(sc), sc['code'], case + ' vs restatement')
    ref = [tuple(torch.as_tensor(gold[f'{case}_t{t}_{k}']) for k in ('labels', 'assigned', 'bbox_targets', 'bbox_weights'))
           for t in range(len(sc['tasks']))]
    compare_targets(got, ref, sc['code'], case + ' vs reference')


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257])
def test_targets_at_the_workgroup_boundaries(gold, n):
    """the rows are class-major, so the samples interleave inside every workgroup"""
    sc = scene(gold, 'multi_centroid')
    rows = np.arange(600 - n, 600) if n else np.zeros(0, np.int64)
    sub = dict(sc, xyz=sc['xyz'][rows], xyz_assign=sc['xyz_assign'][rows], cluster_inds=sc['cluster_inds'][rows])
    if n > 1:
        assert len(np.unique(sub['cluster_inds'][:, 1])) == 3
    got = gpu_targets(sub)
    assert all(len(t[0]) == n for t in got)
    compare_targets(got, restated_targets(sub), 10, f'N = {n}')
    # the sample vector on its own gives the same as column 1 of cluster_inds read in place
    again = gpu_targets(dict(sub, cluster_inds=np.ascontiguousarray(sub['cluster_inds'][:, 1])))
    assert all(torch.equal(a, b) for x, y in zip(got, again) for a, b in zip(x, y))


def test_targets_without_any_box(gold):
    sc = scene(gold, 'waymo_p03')
    empty = dict(sc, boxes=[b[:0] for b in sc['boxes']], labels=[l[:0] for l in sc['labels']])
    got = gpu_targets(empty)
    for t, (lab, assigned, tg, wt) in enumerate(got):
        assert (lab == 1).all() and (assigned == -1).all() and not tg.any() and not wt.any()
    compare_targets(got, restated_targets(empty), 8, 'G = 0')


def test_targets_with_more_boxes_than_one_tile_and_eight_tasks():
    """sample 1 has box_tile + 3 boxes on a grid: rows at the centres of boxes on both sides of the tile boundary; eight
    single-class tasks"""
    import sst_amd
    tile = sst_amd.cluster_head.cluster_targets_box_tile()
    assert sst_amd.cluster_head.cluster_max_tasks() == 8
    g = tile + 3
    rng = np.random.default_rng(5)
    boxes = np.zeros((g, 7), np.float32)
    boxes[:, 0], boxes[:, 1] = (np.arange(g) % 20) * 3.0, (np.arange(g) // 20) * 3.0
    boxes[:, 2], boxes[:, 3:6], boxes[:, 6] = -1.0, np.float32([1.6, 2.4, 1.5]), rng.uniform(-3, 3, g)
    few = boxes[:5].copy()
    few[:, :2] += 100
    labels = [(np.arange(5) % 8).astype(np.int64), ((np.arange(g) * 3) % 8).astype(np.int64)]
    pick = np.array([0, 1, tile - 2, tile - 1, tile, tile + 1, tile + 2, 17, 140])
    xyz = np.concatenate([boxes[pick, :3] + np.float32([0.1, -0.1, 0.7]), few[:, :3] + np.float32([0, 0, 0.5]),
                          np.float32([[500, 500, 0]])]).astype(np.float32)
    bidx = np.array([1] * len(pick) + [0] * 5 + [1], np.int64)
    order = rng.permutation(len(xyz))
    xyz, bidx = xyz[order], bidx[order]
    names = [f'c{i}' for i in range(8)]
    tasks = [dict(class_names=[n]) for n in names]
    inds = np.stack([np.zeros_like(bidx), bidx, np.arange(len(bidx))], 1)
    sc = dict(xyz=xyz, xyz_assign=xyz, cluster_inds=inds, boxes=[few, boxes], labels=labels, tasks=tasks, names=names, code=8,
              width=None)
    got = gpu_targets(sc)
    compare_targets(got, restated_targets(sc), 8, f'{g} boxes in one sample, 8 tasks')
    hit = torch.stack([t[1] for t in got]).max(0)[0].numpy()
    want = np.concatenate([pick + 5, np.arange(5), [-1]])[order]
    assert np.array_equal(hit, want)                     # boxes beyond the first tile are found


def loss_inputs(gold, case, repeat=1, rows=None):
    sc = scene(gold, case)
    fam = case.split('_')[0]
    tg = restated_targets(sc)
    sel = np.arange(len(sc['xyz'])) if rows is None else rows
    sel = np.tile(sel, repeat)
    out = []
    for t, (lab, assigned, tgt, wt) in enumerate(tg):
        out.append(dict(logits=gold[f'{fam}_logits{t}'].astype(np.float32)[sc['rows']][sel],
                        reg=gold[f'{fam}_reg{t}'].astype(np.float32)[sc['rows']][sel], labels=lab.numpy()[sel],
                        tg=tgt.numpy()[sel], wt=wt.numpy()[sel]))
    return sc, out


def run_gpu_loss(tasks, upstream=None, **kw):
    import sst_amd
    logits = [dev(t['logits']).requires_grad_(True) for t in tasks]
    reg = [dev(t['reg']).requires_grad_(True) for t in tasks]
    losses, counts = sst_amd.cluster_loss(logits, reg, [dev(t['labels']) for t in tasks], [dev(t['tg']) for t in tasks],
                                          [dev(t['wt']) for t in tasks], gamma=R.LOSS_CFG['gamma'], alpha=R.LOSS_CFG['alpha'],
                                          loss_weights=[R.LOSS_CFG[k] for k in ('w_cls', 'w_center', 'w_size', 'w_rot', 'w_vel')],
                                          **kw)
    up = upstream or [1.0] * 5
    sum(up[k] * l for task in losses for k, l in enumerate(task)).backward()
    torch.cuda.synchronize()
    return ([[float(l) for l in task] for task in losses], counts.cpu().numpy(), [t.grad.cpu() for t in logits],
            [t.grad.cpu() for t in reg])


def check_losses(gold, case, tasks, got, code_weight, what, beta=None, upstream=None):
    losses, counts, d_logits, d_reg = got
    code = tasks[0]['reg'].shape[1]
    for t, task in enumerate(tasks):
        ref = R.losses_and_grads(task['logits'], task['reg'], task['labels'], task['tg'], task['wt'], upstream=upstream,
                                 code_weight=code_weight, beta=beta)
        assert counts[t, 0] == ref['num_pos'] and counts[t, 1] == ref['status'] == 0
        assert counts[t, 2] == len(task['labels']) and counts[t, 3] == ref['num_pos']
        pre = f'{case}_t{t}_'
        for k, name in enumerate(R.LOSS_NAMES[:code // 2]):
            tol = max(4 * float(gold[f'noise_{pre}{name}']), 1e-6)
            err = abs(losses[t][k] - ref[name]) / abs(ref[name]) if ref[name] else abs(losses[t][k])
            print(f'{what} task {t} {name}: {losses[t][k]:.9g} vs {ref[name]:.9g}, relative error {err:.2e} (allowed {tol:.1e})')
            assert err <= tol
            if ref['num_pos'] == 0 and k:
                assert losses[t][k] == 0.0
        if code == 8:
            assert losses[t][4] == 0.0
        for name, g, r in (('d_logits', d_logits[t], ref['d_logits']), ('d_reg', d_reg[t], ref['d_reg'])):
            assert bool(torch.isfinite(g).all())
            tol = max(4 * float(gold[f'noise_{pre}{name}']), 1e-6)
            scale = float(r.abs().max())
            err = float((g.double() - r).abs().max()) / scale if scale else float(g.abs().max())
            print(f'{what} task {t} {name}: max error {err:.2e} of the largest gradient (allowed {tol:.1e})')
            assert err <= tol
            assert torch.equal(g != 0, r != 0) or name == 'd_logits'      # zeros on background rows, exactly
        if ref['num_pos'] == 0:
            assert not d_reg[t].any()


@pytest.mark.parametrize('repeat', [1, 4])
@pytest.mark.parametrize('case', R.LOSS_CASES)
def test_losses_and_gradients(gold, case, repeat):
    """600 rows are one row tile of the forward, 2 400 are three; the logits reach +-60; waymo's third task has no positive"""
    import sst_amd
    sc, tasks = loss_inputs(gold, case, repeat)
    n = len(tasks[0]['labels'])
    assert -(-n // sst_amd.cluster_head.cluster_loss_tile_rows()) == (1 if repeat == 1 else 3)
    assert max(np.abs(t['logits']).max() for t in tasks) == 60
    got = run_gpu_loss(tasks, code_weight=sc['code_weight'])
    check_losses(gold, case, tasks, got, sc['code_weight'], f'{case} x{repeat}')
    again = run_gpu_loss(tasks, code_weight=sc['code_weight'])
    assert got[0] == again[0] and np.array_equal(got[1], again[1])
    assert all(torch.equal(a, b) for a, b in zip(got[2] + got[3], again[2] + again[3]))           # bit-identical runs


@pytest.mark.parametrize('repeat', [1, 40])
def test_losses_with_every_row_positive_upstream_gradients_and_smooth_l1(gold, repeat):
    sc, tasks = loss_inputs(gold, 'multi_none')
    pos = np.nonzero(tasks[0]['labels'] < 3)[0]
    sc, tasks = loss_inputs(gold, 'multi_none', repeat, rows=pos)
    tasks = tasks[:1]
    assert (tasks[0]['labels'] < 3).all() and (len(pos) * repeat > 2048) == (repeat == 40)
    up = [0.5, 2.0, 1.0, 3.0, 0.25]
    got = run_gpu_loss(tasks, upstream=up, code_weight=sc['code_weight'])
    check_losses(gold, 'multi_none', tasks, got, sc['code_weight'], f'all positive x{repeat}', upstream=up)
    beta = [0.0, 0.1, 0.5, 0.0, 1.0]
    got = run_gpu_loss(tasks, code_weight=sc['code_weight'], smooth_l1_beta=beta)
    check_losses(gold, 'multi_none', tasks, got, sc['code_weight'], f'smooth L1 x{repeat}', beta=beta)


def test_status_bits(gold):
    sc, tasks = loss_inputs(gold, 'multi_none')
    base = run_gpu_loss(tasks, code_weight=sc['code_weight'])
    assert (base[1][:, 1] == 0).all()
    bad = [dict(t) for t in tasks]
    bad[0]['labels'] = bad[0]['labels'].copy()
    bad[0]['labels'][[3, 400]] = [7, -1]                     # outside [0, 3]
    pos = np.nonzero(bad[1]['labels'] < 3)[0]
    bad[1]['wt'] = bad[1]['wt'].copy()
    bad[1]['wt'][pos[0], 9] = 0.5                            # a copy-paste flag that is neither 0 nor 1
    got = run_gpu_loss(bad, code_weight=sc['code_weight'])
    print('status per task:', got[1][:, 1])
    assert got[1][0, 1] == 1 and got[1][1, 1] == 2
    ref = R.losses_and_grads(bad[0]['logits'], bad[0]['reg'], bad[0]['labels'], bad[0]['tg'], bad[0]['wt'],
                             code_weight=sc['code_weight'])
    tol = max(4 * float(gold['noise_multi_none_t0_loss_cls']), 1e-6)
    assert ref['status'] == 1 and abs(got[0][0][0] - ref['loss_cls']) <= tol * ref['loss_cls']     # the rows add nothing
    assert not got[2][0][[3, 400]].any()


def test_decode_and_the_coder(gold):
    import sst_amd
    n = 600
    for fam, t in (('waymo', 0), ('multi', 1)):
        reg, logits = gold[f'{fam}_reg{t}'].astype(np.float32), gold[f'{fam}_logits{t}'].astype(np.float32)
        boxes, scores, bev = (v.cpu().numpy() for v in sst_amd.cluster_decode(dev(reg), dev(gold['xyz']), dev(logits)))
        r_boxes, r_scores, r_bev = (v.numpy() for v in R.decode(reg, gold['xyz'], logits))
        assert boxes.shape == (n, reg.shape[1] - 1) and scores.shape == (n, logits.shape[1] + 1)
        plain = [0, 1, 2] + ([7, 8] if reg.shape[1] == 10 else [])
        assert np.array_equal(boxes[:, plain], r_boxes[:, plain])
        u_box, u_sc = int(R.ulp_distance(boxes, r_boxes).max()), int(R.ulp_distance(scores, r_scores).max())
        print(f'{fam}: centres and velocities equal; exp / atan2 within {u_box} ulp, scores within {u_sc} ulp')
        assert u_box <= 2 and u_sc <= 2 and not scores[:, -1].any()
        # the NMS rows from the kernel's own w, l, yaw: one rounded operation each
        assert np.array_equal(bev[:, 0], boxes[:, 0] - boxes[:, 3] / 2) and np.array_equal(bev[:, 3], boxes[:, 1] + boxes[:, 4] / 2)
        assert np.array_equal(bev[:, 4], boxes[:, 6])
        coder = sst_amd.BasePointBBoxCoder(code_size=reg.shape[1])
        assert torch.equal(coder.decode(dev(reg), dev(gold['xyz'])).cpu(), torch.as_tensor(boxes))
    # encode on the assigned boxes equals the targets kernel's rows
    sc = scene(gold, 'multi_p03')
    lab, assigned, tg, wt = gpu_targets(sc)[0]
    pos = (assigned >= 0).numpy()
    allb = np.concatenate(sc['boxes'])
    enc = sst_amd.BasePointBBoxCoder(code_size=10).encode(dev(allb[assigned[pos].numpy()]), dev(sc['xyz'][pos])).cpu()
    assert torch.equal(enc, tg[pos])


BOX_CFGS = {'rpn_train': dict(nms_pre=-1, nms_thr=None, score_thr=0.1, max_num=500, use_rotate_nms=True),
            'nms': dict(nms_pre=-1, nms_thr=0.25, score_thr=0.1, max_num=500, use_rotate_nms=True),
            'nms_pre': dict(nms_pre=50, nms_thr=0.25, score_thr=0.05, max_num=500, use_rotate_nms=True),
            'max_num': dict(nms_pre=-1, nms_thr=0.25, score_thr=0.05, max_num=20, use_rotate_nms=True)}


def _small_head(kind, tasks, names, code, train_cfg, test_cfg, **kw):
    import sst_amd
    attrs = dict(center=(3, 1, 8), dim=(3, 1, 8), rot=(2, 1, 8))
    cfg = dict(type=kind, num_classes=len(names), bbox_coder=dict(type='BasePointBBoxCoder', code_size=code),
               loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
               loss_center=dict(type='L1Loss', loss_weight=0.5), loss_size=dict(type='L1Loss', loss_weight=0.5),
               loss_rot=dict(type='L1Loss', loss_weight=0.2), in_channel=16, shared_mlp_dims=[16], tasks=tasks,
               class_names=names, common_attrs=attrs, num_cls_layer=1, cls_hidden_dim=8,
               separate_head=dict(type='FSDSeparateHead', norm_cfg=dict(type='LN'), act='relu'), train_cfg=train_cfg,
               test_cfg=test_cfg, **kw)
    if code == 10:
        cfg['common_attrs'] = dict(attrs, vel=(2, 1, 8))
        cfg['loss_vel'] = dict(type='L1Loss', loss_weight=0.2)
    return sst_amd.build_head(cfg).to(DEV)


def _plausible_predictions(gold, fam, n_tasks):
    """the golden predictions with sizes and centres of real boxes, so that the NMS has overlaps to judge"""
    rng = np.random.default_rng(11)
    # + a small noise: float16-valued logits repeat, and equal scores have no defined order in topk and the NMS
    logits = [gold[f'{fam}_logits{t}'].astype(np.float32) for t in range(n_tasks)]
    logits = [(l + rng.normal(0, 1e-3, l.shape)).astype(np.float32) for l in logits]
    reg = [gold[f'{fam}_reg{t}'].astype(np.float32).copy() for t in range(n_tasks)]
    for r in reg:
        r[:, :3] *= 0.3
        r[:, 3:6] = np.log(np.float32([1.8, 4.2, 1.6])) + rng.normal(0, 0.1, (len(r), 3)).astype(np.float32)
    return logits, reg


@pytest.mark.parametrize('name', list(BOX_CFGS) + ['all_task_max_num'])
def test_get_bboxes_equals_decode_and_host_nms(gold, name):
    fsdv2 = name == 'all_task_max_num'
    cfg = dict(BOX_CFGS['nms'], all_task_max_num=30) if fsdv2 else BOX_CFGS[name]
    fam, tasks, names, code = ('multi', R.MULTI_TASKS, R.MULTI_NAMES, 10) if fsdv2 or name == 'nms_pre' else \
        ('waymo', R.WAYMO_TASKS, R.WAYMO_NAMES, 8)
    as_rpn = name == 'rpn_train'
    # the multi-class tasks list their classes in another order than the global list: only FSDV2Head accepts that
    head = _small_head('FSDV2Head' if fam == 'multi' else 'SparseClusterHeadV2', tasks, names, code,
                       dict(rpn=cfg) if as_rpn else dict(), None if as_rpn else cfg, as_rpn=as_rpn)
    head.train(as_rpn)
    logits, reg = _plausible_predictions(gold, fam, len(tasks))
    inds = gold['cluster_inds']
    got = head.get_bboxes([dev(l) for l in logits], [dev(r) for r in reg], dev(gold['xyz']), dev(inds), [dict()] * 3)
    want = R.get_bboxes(logits, reg, gold['xyz'], inds[:, 1], 3, tasks, names, cfg, cfg.get('all_task_max_num'))
    total = 0
    for s in range(3):
        boxes, scores, labels = (v.cpu().numpy() for v in got[s])
        r_boxes, r_scores, r_labels = want[s]
        assert boxes.shape == r_boxes.shape and np.array_equal(labels, r_labels), (name, s)
        assert R.ulp_distance(scores, r_scores).max() <= 2 and R.ulp_distance(boxes, r_boxes).max() <= 2
        total += len(scores)
        if name == 'max_num':
            assert len(scores) <= 20 * len(tasks)
        if fsdv2:
            assert len(scores) == 30
    n_cand = sum(int((1 / (1 + np.exp(-l.astype(np.float64))) > cfg['score_thr']).sum()) for l in logits)
    print(f'{name}: {total} boxes kept of {n_cand} candidates, equal to the restated decode + host NMS')
    assert 0 < total < n_cand or name == 'rpn_train'
    if name == 'rpn_train':
        assert total == n_cand


def _device_events(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]


def _composed_loss(head, out, xyz, aux, inds, boxes, labels):
    """the same targets, the loss written from torch ops on the device (float32)"""
    import sst_amd
    xa = aux if (head.train_cfg or {}).get('centroid_assign') else xyz
    tg = sst_amd.cluster_targets(xa, inds, boxes, labels, head.tasks, head.class_names, head.box_code_size, head.enlarge_width,
                                 xyz_base=xyz)
    w = head.loss_weights
    losses = {}
    for t, (lab, _, tgt, wt) in enumerate(tg):
        z, reg = out['cls_logits'][t], out['reg_preds'][t]
        c = z.size(1)
        onehot = torch.nn.functional.one_hot(lab, c + 1)[:, :c].float()
        p = z.sigmoid()
        bce = torch.nn.functional.binary_cross_entropy_with_logits(z, onehot, reduction='none')
        focal = bce * (head.alpha * onehot + (1 - head.alpha) * (1 - onehot)) * (onehot - p).abs().pow(head.gamma)
        losses[f'loss_cls.task{t}'] = w[0] * focal.sum() / z.size(0)
        pos = (lab < c).float()[:, None]
        n_pos = pos.sum().clamp(min=1)
        diff = (reg - tgt).abs() * wt * pos
        for k, (name, (lo, hi)) in enumerate(zip(R.LOSS_NAMES[1:], R.GROUPS)):
            if lo < reg.size(1) and (name != 'loss_vel' or head.with_vel):
                losses[f'{name}.task{t}'] = w[k + 1] * diff[:, lo:hi].sum() / (2 * n_pos if name == 'loss_vel' else n_pos)
    return losses


@pytest.mark.parametrize('name', ['fsd/fsd_waymoD1_1x', 'fsdv2/fsdv2_nusc_1x'])
def test_forward_loss_backward_of_the_shipped_heads(name):
    import sst_amd
    model = ast.literal_eval(open(os.path.join(GOLDEN, 'configs', name + '.model.py')).read())
    torch.manual_seed(3)
    head = sst_amd.build_head(dict(model['bbox_head'], train_cfg=model['train_cfg'], test_cfg=model['test_cfg'])).to(DEV)
    head.train()
    v2 = name.startswith('fsdv2')
    n, rng = 300, np.random.default_rng(9)
    cols, names = (10, model['bbox_head']['class_names']) if v2 else (7, model['bbox_head']['class_names'])
    boxes, labels = [], []
    for s in range(2):
        b = np.zeros((12, cols), np.float32)
        b[:, :2], b[:, 2] = rng.uniform(-20, 20, (12, 2)), -1.0
        b[:, 3:6], b[:, 6] = np.float32([2.0, 4.5, 1.7]) * rng.uniform(0.8, 1.2, (12, 3)), rng.uniform(-3, 3, 12)
        if v2:
            b[:, 7:9], b[:, 9] = rng.normal(0, 1, (12, 2)), np.arange(12) % 2
        boxes.append(dev(b))
        labels.append(dev(rng.integers(0, len(names), 12)))
    bidx = rng.integers(0, 2, n)
    near = np.stack([boxes[s].cpu().numpy()[rng.integers(0, 12)][:3] for s in bidx]) + np.float32([0, 0, 0.8])
    xyz = dev((near + rng.normal(0, 0.8, (n, 3)) * (rng.random((n, 1)) < 0.7)).astype(np.float32))
    aux = (xyz + 0.05 * torch.randn_like(xyz)).contiguous()
    inds = dev(np.stack([np.zeros(n, np.int64), bidx, np.arange(n)], 1))
    feats = torch.randn(n, model['bbox_head']['in_channel'], device=DEV)
    params = [p for p in head.parameters()]

    def fused_loss(out):
        return head.loss(out['cls_logits'], out['reg_preds'], xyz, inds, boxes, labels, **(dict(aux_xyz=aux) if v2 else {}))

    def step(loss_fn):
        for p in params:
            p.grad = None
        out = head(feats)
        losses = loss_fn(out)
        sum(losses.values()).backward()
        return {k: float(v) for k, v in losses.items()}, [p.grad.clone() for p in params]

    got, g_fused = step(fused_loss)
    want, g_comp = step(lambda out: _composed_loss(head, out, xyz, aux, inds, boxes, labels))
    n_tasks = len(head.tasks)
    assert set(got) == set(want) and len(got) == n_tasks * (5 if v2 else 4)
    assert (head.last_counts[:, 1] == 0).all() and (head.last_counts[:, 0] > 0).any()
    for k in sorted(got):
        err = abs(got[k] - want[k]) / max(abs(want[k]), 1e-12)
        print(f'{name} {k}: fused {got[k]:.7g}, composed in float32 {want[k]:.7g}, relative gap {err:.1e}')
        assert err <= 2e-5           # the composed float32 sum over 300 x C elements: a few 1e-6 of rounding of its own
    worst = max(float((a - b).abs().max() / b.abs().max().clamp(min=1e-20)) for a, b in zip(g_fused, g_comp))
    print(f'{name}: parameter gradients, largest gap {worst:.1e} of a parameter\'s largest gradient')
    # the same network backward fed with upstream gradients that differ by float32 rounding (1e-6): 1e-4 is two decades above
    assert worst <= 1e-4
    # launches of the loss alone: one targets kernel and two loss kernels forward, one backward; nothing comes back to the host
    out = head(feats)
    fwd = _device_events(lambda: fused_loss(out))
    losses = fused_loss(out)
    total = sum(losses.values())
    leaves = out['cls_logits'] + out['reg_preds']
    bwd = _device_events(lambda: torch.autograd.grad(total, leaves, retain_graph=True))
    ours_f, ours_b = [e for e in fwd if 'cluster_' in e], [e for e in bwd if 'cluster_' in e]
    print(f'{name}: loss forward {len(fwd)} device events ({len(ours_f)} of cluster_head.hip), backward {len(bwd)} ({len(ours_b)})')
    assert fwd and bwd, 'the profiler recorded no device event'
    kernel = re.compile(r'cluster_\w+_k')
    assert sorted(kernel.search(e).group(0) for e in ours_f) == ['cluster_loss_final_k', 'cluster_loss_partial_k',
                                                                'cluster_targets_k']
    assert [kernel.search(e).group(0) for e in ours_b] == ['cluster_loss_bwd_k']
    # what a read-back looks like to this profiler: the copy events of a deliberate one
    readback = {e for e in _device_events(lambda: float(torch.zeros(2, device=DEV).sum())) if 'memcpy' in e.lower()}
    print(f'{name}: a host read shows up as {sorted(readback)}; copies of the loss: {sorted(set(e for e in fwd + bwd if "memcpy" in e.lower()))}')
    assert readback, 'the profiler does not show the copy of a host read'
    assert not [e for e in fwd + bwd if e in readback or 'dtoh' in e.lower()]
    # torch's glue: the two concatenations of the lists of boxes and labels and the offset upload forward; the stacking of the
    # upstream gradients backward
    assert len(fwd) - len(ours_f) <= 6 and len(bwd) - len(ours_b) <= 4

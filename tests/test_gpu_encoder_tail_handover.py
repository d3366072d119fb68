"""GPU: the hand-over mode of the one-kernel encoder tails (csrc/layer_tail_x6.hip, SST_TAIL_HANDOVER) against the row-major
mode of the same kernels on the same inputs.  In hand-over mode s1, s2 and the feed-forward tensor travel from the forward to the
backward kernel in a tile-blocked layout, and the feed-forward tensor holds act'(pre) instead of pre.  Everything anybody else
reads - y1, h, y2, y2p, the statistics, ds2, dpre, ds1, d_o, the LayerNorm parameter gradients and their per-workgroup partials -
must keep its BITS: the same function of the same input, and a permutation.

Shapes: m on both sides of a 16-row tile (15, 16, 17), of a 64-row workgroup (63, 64, 65), one row, and 130 (three workgroups,
a 2-row last tile).  Every buffer a kernel writes is NaN before the call, so an element that is not written, or a padded element
that is read into a result, shows.

pre is steered through eight feed-forward columns whose W1 rows are zero, so that pre = b1 there: 0, a negative zero bias (the
sum starts from a +0 accumulator, so the kernel's pre is +0 there too: -0 cannot occur in this chain), +-1e-30, +-1e-39
(subnormal), +-20; the other 248 columns are Gaussian on both sides of 0.

act' against float64: 1e-6 absolute.  erf_as is within 1.5e-7 of erf (csrc/gelu.h), so Phi = (1 + erf) / 2 is within 0.75e-7;
x phi(x) is at most 0.242 in magnitude and carries the few-ulp relative error of the hardware exponential (< 1e-7 absolute);
three fp32 roundings of values <= 1.13 add < 2e-7: 1e-6 leaves a factor of two."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 1e-5
MS = (1, 15, 16, 17, 63, 64, 65, 130)
STEERED = (0.0, -0.0, 1e-30, -1e-30, 1e-39, -1e-39, 20.0, -20.0)
_cache = {}


def _params():
    if 'p' not in _cache:
        from sst_amd import dense as D
        g = torch.Generator().manual_seed(1234)

        def r(*shape, s=1.0):
            return torch.randn(*shape, generator=g) * s
        w1, b1 = r(256, 128, s=0.09), r(256, s=0.1)
        w1[:len(STEERED)] = 0.0
        b1[:len(STEERED)] = torch.tensor(STEERED)
        p = dict(w_out=r(128, 128, s=0.09), b_out=r(128, s=0.1), w1=w1, b1=b1, w2=r(128, 256, s=0.06), b2=r(128, s=0.1),
                 n1w=1 + r(128, s=0.2), n1b=r(128, s=0.1), n2w=1 + r(128, s=0.2), n2b=r(128, s=0.1))
        p = {k: v.to(DEV) for k, v in p.items()}
        with D.matmul_mode_scope('f32x6'):
            p['packed'] = D.encoder_tail_pack(p['w_out'], p['w1'], p['w2'])
        p['pos'] = (r(144, 128).to(DEV), torch.randint(0, 144, (MS[-1],), generator=g, dtype=torch.int32).to(DEV))
        _cache['p'] = p
    return _cache['p']


def _inputs(m):
    g = torch.Generator().manual_seed(100 + m)
    return [torch.randn(m, 128, generator=g).to(DEV) for _ in range(4)]     # o, x, dy2, dy2p


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


def _forward(m, act, with_pos, handover, o, x):
    from sst_amd import dense as D
    p = _params()
    rows = D.handover_rows(m) if handover else m
    out = dict(s1=_nan(rows, 128), st1=_nan(m, 2), y1=_nan(m, 128), pre=_nan(rows, 256), h=_nan(m, 256), s2=_nan(rows, 128),
               st2=_nan(m, 2), y2=_nan(m, 128))
    pos = None
    if with_pos:
        out['y2p'] = _nan(m, 128)
        pos = (p['pos'][0], p['pos'][1][:m].contiguous())
    with D.matmul_mode_scope('f32x6'):
        return D.encoder_tail_fwd(o, x, p['packed'], p['b_out'], p['b1'], p['b2'], p['n1w'], p['n1b'], p['n2w'], p['n2b'], EPS, act,
                                  save=True, pos=pos, out=out, handover=handover)


def _backward(m, act, handover, dy2, dy2p, fwd):
    """-> [ds2, dpre, ds1, d_o, dn, the LayerNorm partials of the workspace]"""
    from sst_amd import _lib, dense as D
    p = _params()
    nbytes = int(_lib.load().sst_encoder_tail_bwd_workspace_bytes(m))
    ws = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device=DEV)
    out = dict(ds2=_nan(m, 128), dpre=_nan(m, 256), ds1=_nan(m, 128), d_o=_nan(m, 128), dn=_nan(4, 128), ws=ws)
    with D.matmul_mode_scope('f32x6'):
        res = D.encoder_tail_bwd(dy2, dy2p, fwd['s2'], fwd['st2'], fwd['pre'], fwd['s1'], fwd['st1'], p['packed'], p['n1w'],
                                 p['n2w'], act, out=out, handover=handover)
    wgs = (m + 63) // 64
    return list(res) + [ws[:2 * wgs * 256]]       # norm2's [workgroups][256] partials, then norm1's


def _rows_to_handover(t):
    """the inverse of sst_amd.dense.handover_to_rows for a [rows, cols] tensor (rows a multiple of 16)"""
    rows, cols = t.shape
    v = t.reshape(rows // 16, 16, cols // 32, 4, 2, 4)       # tile, c, block, g, half, e
    return v.permute(0, 2, 4, 3, 1, 5).reshape(rows, cols).contiguous()


def _act_grad64(pre, act):
    x = pre.double()
    if act == 'relu':
        return (x > 0).double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize('with_pos', [False, True])
@pytest.mark.parametrize('with_dy2p', [False, True])
@pytest.mark.parametrize('act', ['gelu', 'relu'])
@pytest.mark.parametrize('m', MS)
def test_handover_keeps_every_bit(m, act, with_dy2p, with_pos):
    from sst_amd import dense as D
    o, x, dy2, dy2p = _inputs(m)
    dy2p = dy2p if with_dy2p else None
    ref = _forward(m, act, with_pos, False, o, x)
    new = _forward(m, act, with_pos, True, o, x)

    pre = ref['pre']
    assert bool((pre[:, 0] == 0).all()) and bool((pre[:, 1] == 0).all())
    assert bool((pre[:, 2] == 1e-30).all()) and bool((pre[:, 3] == -1e-30).all())
    assert bool((pre[:, 4:6].abs() < 1e-38).all())      # subnormal (or flushed): the float64 reference below is taken of THIS pre
    assert bool((pre[:, 6] == 20).all()) and bool((pre[:, 7] == -20).all())
    assert bool((pre[:, 8:] > 0).any()) and bool((pre[:, 8:] < 0).any())

    # forward: what others read is bit-equal
    for k in ('y1', 'h', 'y2', 'st1', 'st2') + (('y2p',) if with_pos else ()):
        assert torch.equal(new[k], ref[k]), k
    # layout: the de-blocked hand-over tensors
    rows = D.handover_rows(m)
    assert rows % 64 == 0 and 0 <= rows - m < 64
    for k, cols in (('s1', 128), ('s2', 128), ('pre', 256)):
        assert new[k].shape == (rows, cols)
        assert bool(torch.isfinite(new[k]).all()), k     # the padded rows are written too (the clamped last row's values)
    assert torch.equal(D.handover_to_rows(new['s1'], m), ref['s1'])
    assert torch.equal(D.handover_to_rows(new['s2'], m), ref['s2'])
    dact = D.handover_to_rows(new['pre'], m)
    want = _act_grad64(pre, act)
    err = float((dact.double() - want).abs().max())
    print(f'm={m} act={act}: max |act\' - float64| = {err:.3e}')
    if act == 'relu':
        assert torch.equal(dact.double(), want)
    else:
        assert err <= 1e-6, err

    # backward: every result is bit-equal
    names = ('ds2', 'dpre', 'ds1', 'd_o', 'dn', 'partials')
    bref = _backward(m, act, False, dy2, dy2p, ref)
    bnew = _backward(m, act, True, dy2, dy2p, new)
    for k, a, b in zip(names, bnew, bref):
        assert torch.equal(a, b), k

    # ... whatever the padded rows hold: NaN in every row past m
    if rows > m:
        poisoned = dict(new)
        for k in ('s1', 's2', 'pre'):
            t = D.handover_to_rows(new[k], rows).clone()
            t[m:] = float('nan')
            poisoned[k] = _rows_to_handover(t)
            assert torch.equal(D.handover_to_rows(poisoned[k], m), D.handover_to_rows(new[k], m))
        bpoi = _backward(m, act, True, dy2, dy2p, poisoned)
        for k, a, b in zip(names, bpoi, bref):
            assert torch.equal(a, b), 'padded rows leak into ' + k


@pytest.mark.parametrize('act', ['gelu', 'relu'])
def test_handover_is_repeatable(act):
    m = 130
    o, x, dy2, dy2p = _inputs(m)
    runs = []
    for _ in range(2):
        f = _forward(m, act, True, True, o, x)
        b = _backward(m, act, True, dy2, dy2p, f)
        runs.append([f[k].clone() for k in ('s1', 'st1', 'y1', 'pre', 'h', 's2', 'st2', 'y2', 'y2p')] + [t.clone() for t in b])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_handover_arguments():
    import ctypes
    from sst_amd import _lib
    lib = _lib.load()
    args = _lib.EncoderTailFwdArgs()
    args.m, args.act, args.flags = 16, 1, 2          # an unknown flag bit
    assert lib.sst_encoder_tail_fwd_f32x6(ctypes.byref(args), _lib.stream_ptr()) == _lib.SST_ERR_ARG
    b = _lib.EncoderTailBwdArgs()
    b.m, b.act, b.flags = 16, 1, 2
    assert lib.sst_encoder_tail_bwd_f32x6(ctypes.byref(b), _lib.stream_ptr()) == _lib.SST_ERR_ARG

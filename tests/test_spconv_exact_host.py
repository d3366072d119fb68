"""Host side of the exact sparse-convolution tests (no GPU): the float64 reference of tests/spconv_exact_ref.py against the
oracle, the CPU emulation of the kernels' accumulation schemes under each recipe's caps, the bf16 parts the recipes really
exercise, and the launch-plan queries of the library (sst_spconv_conv_os_plan, sst_spconv_wgrad_os_plan)."""
import numpy as np
import torch

import spconv_exact_ref as R


def test_reference_equals_the_oracle_on_a_real_rulebook():
    """conv_ref on out2in = indice_conv, conv_ref on in2out with the transposed weights = the data gradient, wgrad_ref on the
    pair lists = the filter gradient of oracle/spconv_oracle.py, on a small submanifold and a small strided rulebook; recipe B
    operands, whose float64 sums are exact in any order, so the comparison is `==`"""
    from oracle import spconv_oracle as O
    rng = np.random.default_rng(5)
    batch, shape, n, cin, cout = 2, [5, 9, 8], 150, 8, 12
    lin = rng.choice(batch * int(np.prod(shape)), n, replace=False)
    b, r = lin // int(np.prod(shape)), lin % int(np.prod(shape))
    ind = np.stack([b, r // (shape[1] * shape[2]), (r // shape[2]) % shape[1], r % shape[2]], 1).astype(np.int32)
    gen = torch.Generator().manual_seed(5)
    for subm, st in ((True, 1), (False, 2)):
        outids, pairs, num, _ = O.indice_pairs(ind, batch, shape, [3] * 3, [st] * 3, [1] * 3, [1] * 3, (0, 0, 0), subm, False)
        m = len(outids)
        in2out, out2in = O.maps_from_pairs(pairs, num, n, m)
        x, w, _ = R.conv_operands('B', 'x', n, 27, cin, cout, gen)
        gy = R.values('B', False, (m, cout), gen)
        w5 = w.numpy().reshape(3, 3, 3, cin, cout)
        y = R.conv_ref(x, torch.from_numpy(out2in), w)
        assert np.array_equal(y.numpy(), O.indice_conv(x.numpy(), w5, pairs, num, m))
        dx_want, dw_want = O.indice_conv_backward(x.numpy(), w5, gy.numpy(), pairs, num)
        dx = R.conv_ref(gy, torch.from_numpy(in2out), w.transpose(1, 2))
        assert np.array_equal(dx.numpy(), dx_want)
        dw = R.wgrad_ref(x, gy, torch.from_numpy(pairs), [int(v) for v in num], 0)
        assert np.array_equal(dw.numpy().reshape(w5.shape), dw_want)
        swapped = torch.from_numpy(np.ascontiguousarray(pairs[:, ::-1]))
        assert torch.equal(R.wgrad_ref(x, gy, swapped, [int(v) for v in num], 1), dw)
        assert num.sum() > 0 and float(y.abs().max()) > 0


def _worst(recipe, terms, n, fine_first, gen):
    """[terms, n] operands of the recipe with the worst case planted in the first columns: every term at the largest magnitude,
    all of one sign"""
    fine = R.values(recipe, True, (terms, n), gen)
    unit = R.values(recipe, False, (terms, n), gen)
    top = {'A': 4.0, 'B': 2047 / 1024.0, 'D': (2 ** 20 - 1) / 2.0 ** 20}[recipe]
    fine[:, :4], unit[:, :4] = top, (4.0 if recipe == 'A' else 1.0)
    fine[:, 4:8], unit[:, 4:8] = -top, (4.0 if recipe == 'A' else 1.0)
    return (fine, unit) if fine_first else (unit, fine)


def test_emulated_accumulations_are_exact_under_the_caps():
    """the fp32 chain, the two-way split (x3) and the three-way split with its leading product and its corrections in separate
    chains (x6), each in random order, reproduce the float64 sum bit for bit at the caps the condition leaves: A 27 x 256
    terms, B 4096 terms, D 4 terms (+ a bias of the fine kind) - both ways round.  The two-way split is NOT exact under D: the
    x3 kernel does not get that recipe."""
    gen = torch.Generator().manual_seed(11)
    x3_inexact = 0
    for recipe, terms, modes in (('A', 27 * 256, ('f32', 'x3', 'x6')), ('B', 4096, ('f32', 'x3', 'x6')), ('D', 4, ('f32', 'x6'))):
        for fine_first in (True, False):
            a, b = _worst(recipe, terms, 256 if terms > 4 else 4096, fine_first, gen)
            want = (a.double() * b.double()).sum(0)
            R.assert_exact(recipe, (a.double().abs() * b.double().abs()).sum(0))
            for mode in modes:
                got = R.emulate(mode, a, b, gen)
                assert torch.equal(got.double(), want), (recipe, terms, mode, fine_first)
            if recipe == 'D':
                bias = R.values('D', True, (a.size(1),), gen)
                R.assert_exact('D', (a.double().abs() * b.double().abs()).sum(0) + bias.double().abs())
                assert torch.equal((R.emulate('x6', a, b, gen) + bias).double(), want + bias.double())
                x3_inexact += int(not torch.equal(R.emulate('x3', a, b, gen).double(), want))
    assert x3_inexact == 2


def test_recipes_exercise_the_bf16_parts():
    """B has a second part in at least half of its fine entries (measured 0.81), D a third part in at least a quarter (measured
    0.50); A and the unit operands have one part.  And the finding that made D necessary: k / 2^17 NEVER has a third part -
    under round-to-nearest each part gains nine bits (eight and the sign of the remainder), so 17 bits fit in two."""
    gen = torch.Generator().manual_seed(3)
    share = lambda t: float((t != 0).float().mean())     # noqa: E731
    pb = R.bf16_parts(R.values('B', True, (200000,), gen))
    assert share(pb[1]) >= 0.5 and share(pb[2]) == 0.0, (share(pb[1]), share(pb[2]))
    pd = R.bf16_parts(R.values('D', True, (200000,), gen))
    assert share(pd[1]) >= 0.5 and share(pd[2]) >= 0.25, (share(pd[1]), share(pd[2]))
    for t in (R.values('A', True, (10000,), gen), R.values('B', False, (10000,), gen), R.one_hot_rows(500, 20, gen)):
        p = R.bf16_parts(t)
        assert share(p[1]) == 0.0 and share(p[2]) == 0.0
    k = torch.arange(-(2 ** 17 - 1), 2 ** 17).float()            # all 262 143 values of the 17-bit recipe
    assert k.numel() == 262143 and share(R.bf16_parts(k / 2.0 ** 17)[2]) == 0.0
    # the D placements: one non-zero per row / per (k, n)
    assert bool(((R.one_hot_rows(300, 12, gen) != 0).sum(1) == 1).all())
    assert bool(((R.one_hot_weights(27, 12, 20, gen) != 0).sum(1) == 1).all())


def test_map_and_pair_families_keep_their_promises():
    """every index in range, the shapes the families are named for, at most 4 partners per row / 4 terms per element for D"""
    rng = np.random.default_rng(2)
    for kvol in (1, 8, 27, 32):
        for m in (1, 64, 65, 191):
            for fam in R.MAP_FAMILIES + ('empty',):
                mp = R.make_map(fam, kvol, m, 50, rng, lo=1)
                R.check_map(mp, 50)
                assert mp.shape == (kvol, m) and (mp != 0).all()
            s4 = R.make_map('sparse4', kvol, m, 50, rng) >= 0
            assert (s4.sum(0) == min(4, kvol)).all()
            if m >= 16 and kvol <= 32:
                assert s4[:, :m // 16 * 16].reshape(kvol, -1, 16).any(-1).all()
            so = R.make_map('single_offset', kvol, m, 50, rng) >= 0
            assert not so[:-1].any()
    et = R.make_map('empty_tile', 27, 191, 50, rng) >= 0
    assert not et[:, :64].any() and not et[:, 80:96].any() and et[:, 64:80].any() and et[:, 96:].any()
    lr = R.make_map('last_row', 27, 191, 50, rng) >= 0
    assert lr[:, 128:].sum() == 1 and lr[13, 190] and lr[:, :128].any()
    ob = R.make_map('one_block', 27, 191, 50, rng) >= 0
    assert (np.pad(ob, ((0, 0), (0, 1))).reshape(27, 3, 4, 16).any(-1).sum(-1) == 1).all()
    gen = torch.Generator().manual_seed(2)
    hot = R.one_hot_rows(90, 8, gen)
    channel = hot.abs().argmax(1).numpy()
    num = [0, 1, 5, 32, 17]
    for side in (0, 1):
        pairs = R.make_pairs(num, 40, 90 if side == 0 else 70, 70 if side == 0 else 90, rng, hot=(side, channel, 4))
        for k, n in enumerate(num):
            assert (pairs[k, :, n:] == -1).all() and (pairs[k, :, :n] >= 0).all()
            assert n == 0 or np.bincount(channel[pairs[k, side, :n]]).max() <= 4
    plain = R.make_pairs(num, 40, 90, 70, rng)
    assert plain[:, 0].max() == 89 and plain[:, 1].max() == 69 and (plain[3, :, :32] == 0).any()


# ------------------------------------------------------------------------------------------------------------------------------
# the launch plan, asked of the library
# ------------------------------------------------------------------------------------------------------------------------------
F32, F32X3, F32X6, ROWS_F32X6 = R.F32, R.F32X3, R.F32X6, R.ROWS_F32X6
conv_plan, wgrad_plan = R.conv_plan, R.wgrad_plan


def test_plan_queries():
    from sst_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(9)
    seen_cols, seen_split = set(), set()
    for _ in range(400):
        m = int(rng.choice([1, 63, 64, 65, 200, 2000, 6000, 40000, 70000, 140000, 299999]))
        kvol = int(rng.choice([1, 3, 8, 16, 27, 32]))
        cin = 4 * int(rng.integers(1, 65))
        cout = int(rng.integers(1, 300))
        pack = lib.sst_spconv_conv_os_f32x6_workspace_bytes(kvol, cin, cout)
        full = lib.sst_spconv_conv_os_f32x6_workspace_bytes_rows(kvol, cin, cout, m)
        assert full >= pack > 0
        for entry, cfg, nbytes in ((F32, 0, 0), (F32, 41, 0), (F32, 42, 0), (F32, 81, 0), (F32, 82, 0), (F32X3, 0, 0),
                                   (F32X6, 0, 0), (ROWS_F32X6, 0, pack), (ROWS_F32X6, 0, full), (ROWS_F32X6, 0, (pack + full) // 2)):
            rc, rows, cols, split, wgs = conv_plan(entry, m, kvol, cin, cout, cfg, nbytes)
            assert rc == 0, (entry, m, kvol, cin, cout, cfg, rc)
            assert rows in (64, 128) and cols in (64, 128)
            assert split in (1, 2, 4, 8) and (split == 1 or split <= kvol)
            if cfg:
                assert (cols, rows) == (16 * (cfg // 10), 64 * (cfg % 10))
            if entry == F32:
                assert rows == lib.sst_spconv_conv_os_tile_rows(m, cout, cfg)
            else:
                assert rows == 64
            if entry != ROWS_F32X6 or nbytes == pack:
                assert split == 1                      # only the packed weights offered: nowhere to put partial tiles
            live = -(-m // rows) * -(-cout // cols) * split
            assert live <= wgs < live + 32 and wgs % 8 == 0
            seen_cols.add(cols)
            seen_split.add(split)
    assert seen_cols == {64, 128} and seen_split == {1, 2, 4, 8}
    # the same refusals as the entries
    assert conv_plan(F32, 100, 27, 6, 16)[0] == _lib.SST_ERR_UNSUPPORTED
    assert conv_plan(F32X6, 100, 33, 8, 16)[0] == _lib.SST_ERR_UNSUPPORTED
    assert conv_plan(F32X3, 100, 27, 8, 16, tile_cfg=41)[0] == _lib.SST_ERR_ARG
    assert conv_plan(F32, 100, 27, 8, 16, tile_cfg=43)[0] == _lib.SST_ERR_ARG
    assert conv_plan(ROWS_F32X6, 100, 27, 8, 16, workspace_bytes=1000)[0] == _lib.SST_ERR_ARG
    assert conv_plan(7, 100, 27, 8, 16)[0] == _lib.SST_ERR_ARG
    # filter gradient: chunk sizes of 64-pair stages in 512 .. 2048, and room for every chunk of any consistent count vector
    sizes = set()
    for _ in range(400):
        kvol = int(rng.choice([1, 8, 27, 32]))
        pair_ld = int(rng.choice([1, 100, 3000, 40000]))
        cin, cout = 4 * int(rng.integers(1, 65)), 4 * int(rng.integers(1, 65))
        num = rng.integers(0, pair_ld + 1, kvol) * (rng.random(kvol) < 0.7)
        if rng.random() < 0.3:
            num[:] = pair_ld
        for total in (int(num.sum()), -1):
            rc, chunk, slots = wgrad_plan(kvol, pair_ld, total, cin, cout)
            assert rc == 0 and 512 <= chunk <= 2048 and chunk % 64 == 0
            assert slots >= sum(-(-int(v) // chunk) for v in num), (kvol, pair_ld, total, chunk, slots)
            assert lib.sst_spconv_wgrad_os_workspace_bytes(kvol, pair_ld, total, cin, cout) == slots * cin * cout * 4 + 256
            sizes.add(chunk)
    assert {512, 2048} <= sizes and len(sizes) > 2
    assert wgrad_plan(27, 0, 0, 8, 8)[0] == _lib.SST_ERR_ARG

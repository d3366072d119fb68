"""The 'bf16' operand mode of the sparse convolutions (csrc/spconv_os_bf16.hip): what the tests of it share
(tests/test_spconv_bf16_host.py without a GPU, tests/test_gpu_spconv_bf16.py on one).

The mode rounds every operand of the contraction to bf16 once (round to nearest even), multiplies bf16 x bf16 and accumulates in
fp32.  With operands that ARE bf16 numbers and sums that stay fp32 numbers, a correct kernel returns the float64 result of
tests/spconv_exact_ref.py bit for bit.  Recipes of such operands:
  A  (of spconv_exact_ref) integers in [-4, 4] on both sides
  E  fine side k / 128 with |k| <= 255 - every one of the 8 significand bits of bf16 is used -, unit side in {-1, 0, 1}
With kvol <= 32 and cin <= 256 a sum of E products has at most 32 * 256 terms of at most 255 granules of 2^-7: below 2^21
granules, and `assert_exact` (2^23 granules) is asserted from the operands before anything is launched."""
import torch

import spconv_exact_ref as R

GRANULE_E = 2.0 ** -7
R.GRANULE.setdefault('E', GRANULE_E)       # assert_exact / assert_conv_exact / assert_wgrad_exact of the shared helper take 'E'
ROWS_BF16 = 4                              # SST_SPCONV_OS_ENTRY_ROWS_BF16


def round_bf16(t):
    """fp32 -> nearest bf16 value, ties to even, as fp32"""
    return t.to(torch.bfloat16).to(torch.float32)


def values(recipe, fine, shape, gen):
    """fp32 CPU tensor of recipe A or E; `fine`: the many-valued operand of E"""
    if recipe == 'A':
        return R.values('A', fine, shape, gen)
    assert recipe == 'E'
    lo, hi = (-255, 255) if fine else (-1, 1)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()
    return t / 128.0 if fine else t


def is_bf16(t):
    return torch.equal(round_bf16(t), t)


def conv_operands(recipe, fine, n_x, kvol, cin, cout, gen):
    """x [n_x, cin], w [kvol, cin, cout], bias [cout]; fine: 'x' | 'w'.  The bias is added in fp32 behind the contraction: it is
    of the fine kind (a multiple of the granule)"""
    x = values(recipe, fine == 'x', (n_x, cin), gen)
    w = values(recipe, fine == 'w', (kvol, cin, cout), gen)
    assert is_bf16(x) and is_bf16(w)
    return x, w, values(recipe, True, (cout,), gen)


def wgrad_operands(recipe, fine, rows_x, rows_dy, cin, cout, gen):
    """x [rows_x, cin], dy [rows_dy, cout]; fine: 'x' | 'dy'"""
    x = values(recipe, fine == 'x', (rows_x, cin), gen)
    dy = values(recipe, fine == 'dy', (rows_dy, cout), gen)
    assert is_bf16(x) and is_bf16(dy)
    return x, dy


def worst_case_granules(kvol, cin):
    """the most granules a sum of E products can reach: every term at 255 / 128, all of one sign"""
    return kvol * cin * 255


# the shapes tests/test_gpu_spconv_bf16.py runs recipe E on: (kvol, cin) of the contraction ((kvol, cout) with the weights
# transposed) and (pairs of an offset, 1) of the filter gradient, whose sums run over pairs
GPU_CONV_SHAPES = [(27, 12), (27, 20), (27, 64), (1, 16), (8, 16), (32, 16), (32, 32), (27, 4), (27, 16), (27, 7), (27, 66),
                   (27, 68), (27, 132), (27, 128), (27, 160), (27, 256)]
GPU_WGRAD_MAX_PAIRS = 1100      # pair_ld of the chunk-edge case: no offset has more pairs in any test

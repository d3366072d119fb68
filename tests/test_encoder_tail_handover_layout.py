"""No GPU: sst_amd.dense.handover_to_rows (the de-blocking of the encoder tails' hand-over buffers, csrc/layer_tail_x6.hip)
against the index formula of that layout written out element by element, and the size helper the buffers are allocated with."""
import numpy as np
import pytest
import torch


def _rows(m):
    return (m + 63) // 64 * 64


@pytest.mark.parametrize('cols', [128, 256])
@pytest.mark.parametrize('m', [1, 17, 64, 65])
def test_deblocking_matches_the_index_formula(m, cols):
    from sst_amd import dense as D
    rows = _rows(m)
    buf = np.arange(rows * cols, dtype=np.float32)          # every element knows its position in the buffer
    want = np.empty((m, cols), dtype=np.float32)
    ncb = cols // 32
    for r in range(m):
        tile, c = divmod(r, 16)
        for col in range(cols):
            cb, k = divmod(col, 32)
            g, k8 = divmod(k, 8)
            half, e = divmod(k8, 4)
            lane = 16 * g + c
            want[r, col] = buf[(((tile * ncb + cb) * 2 + half) * 64 + lane) * 4 + e]
    got = D.handover_to_rows(torch.from_numpy(buf).reshape(rows, cols), m)
    assert got.shape == (m, cols)
    np.testing.assert_array_equal(got.numpy(), want)


def test_handover_rows_is_the_workgroup_multiple():
    from sst_amd import _lib, dense as D
    lib = _lib.load()
    for m in (0, 1, 17, 64, 65, 90107):
        assert D.handover_rows(m) == _rows(m)
    assert lib.sst_encoder_tail_handover_rows(-1) == _lib.SST_ERR_ARG

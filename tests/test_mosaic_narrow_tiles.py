"""qb3x_decode_mosaic with NARROW tiles (under 4 pixels wide or high): such a tile is decoded through a stand-in shape and copied into
place, and that copy must write the tile's own rows only -- in a mosaic the bytes between them are the neighbouring tiles' columns.
(It used to be one block of stride * rows bytes, which wrote zeros over the neighbours.)"""
import numpy as np
import pytest

from qb3_mosaic_windows import Mosaic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    return torch


@pytest.mark.parametrize("case", [(10, 40, 3, 16), (40, 10, 16, 3)], ids=["3-wide", "3-high"])
def test_narrow_tiles_decode_into_place(qb3, oracle, torch_, case):
    W, H, tw, th = case
    raster = oracle.generate(W, H, 3, 0, "NOISY3", 31)
    m = Mosaic(qb3, torch_, raster, tw, th, 0, 8, index_chunk=0)
    back, ok = m.whole()
    assert all(ok)
    assert np.array_equal(back, raster)

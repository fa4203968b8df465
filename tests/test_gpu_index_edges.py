"""The device index of a mask (``DeviceIndex.from_mask``: flags -> exclusive scan -> compaction -> int64 copy) at the sizes where
its shared pieces change behaviour: 64 (a wave), 256 (a block of the compaction and of the widening kernel) and 2048 (the scan
tile, ``SCAN_TILE`` in csrc/xr_scan.hip), one below, at and one above each, the empty mask and a size of three tiles."""
import numpy as np
import pytest

from xugrid_amd import engine

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)


def masks(n):
    last = np.zeros(n, dtype=bool)
    last[n - 1 :] = True  # (n = 0: nothing to set)
    return {
        "none": np.zeros(n, dtype=bool),
        "all": np.ones(n, dtype=bool),
        "alternating": np.arange(n) % 2 == 0,
        "last": last,
        "random": np.random.default_rng(1000 + n).random(n) < 0.5,
    }


@pytest.mark.parametrize("n", SIZES)
def test_index_from_mask_at_wave_block_and_tile_edges(hip, n):
    for name, mask in masks(n).items():
        expected = np.nonzero(mask)[0].astype(np.int64)
        dev = engine.DeviceArray.from_host(mask.view(np.uint8))
        index = engine.DeviceIndex.from_mask(dev.ptr, n)
        assert index.n == expected.size, name  # (DeviceIndex reads its length through xr_index_info)
        got = index.to_dev().download()
        assert got.dtype == np.int64, name
        assert np.array_equal(got, expected), name

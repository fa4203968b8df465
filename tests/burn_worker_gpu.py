"""Worker of test_device_grid_and_device_geometry: burning on a grid made from device arrays with torch coordinate, offset
and value tensors.  torch first (its HIP runtime has to be up before the engine binds the device), then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import xugrid_amd as xa  # noqa: E402
from burn_cases import at_size_polygons, ragged  # noqa: E402
from xugrid_amd import burn, meshgen  # noqa: E402

XY, FACES = meshgen.triangle_mesh(20_000, 0)
HOST = xa.Ugrid2d(XY[:, 0], XY[:, 1], -1, FACES)


def tensors(parts):
    return tuple(torch.tensor(part, device="cuda:0") for part in parts)


def device_grid():
    """The result is a float64 tensor on the GPU equal to the host-array call, before and after ``drop_device_caches()``;
    the host copy of the grid is never made; the inputs are unchanged."""
    grid = xa.Ugrid2d.from_device_arrays(torch.tensor(XY, device="cuda:0"), torch.tensor(FACES, device="cuda:0"))

    def fail():
        raise AssertionError("the host copy of a device grid was made")

    grid._materialise = fail
    polygons = ragged(at_size_polygons())
    polygons += (3.0 + 1.5 * np.arange(polygons[2].size - 1),)
    rng = np.random.default_rng(9)
    lines = (rng.uniform(0.0, 1.0, (30, 2)), np.array([0, 10, 30]), np.array([-1.0, -2.0]))
    points = (rng.uniform(-0.1, 1.1, (20, 2)), -10.0 - np.arange(20.0))
    for all_touched in (False, True):
        expected = xa.burn_vector_geometry(HOST, polygons=polygons, lines=lines, points=points, all_touched=all_touched)
        assert isinstance(expected, np.ndarray) and (expected < 0).any() and np.isnan(expected).any() and (expected > 0).any()
        d_polygons, d_lines, d_points = tensors(polygons), tensors(lines), tensors(points)
        before = [t.clone() for t in d_polygons + d_lines + d_points]
        for dropped in (False, True):
            if dropped:
                grid.drop_device_caches()
            got = xa.burn_vector_geometry(grid, polygons=d_polygons, lines=d_lines, points=d_points, all_touched=all_touched)
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
            assert np.array_equal(got.cpu().numpy(), expected, equal_nan=True)
        assert all(torch.equal(a, b) for a, b in zip(d_polygons + d_lines + d_points, before))
        # host geometry on the device grid: numpy out; one device coordinate array among host ones: a tensor out
        got = xa.burn_vector_geometry(grid, polygons=polygons, lines=lines, points=points, all_touched=all_touched)
        assert isinstance(got, np.ndarray) and np.array_equal(got, expected, equal_nan=True)
        got = xa.burn_vector_geometry(grid, polygons=polygons, lines=lines, points=d_points, all_touched=all_touched)
        assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy(), expected, equal_nan=True)
    winner = burn.polygon_winner(grid, *d_polygons[:3])
    assert isinstance(winner, torch.Tensor) and winner.is_cuda and winner.dtype == torch.int32
    assert np.array_equal(winner.cpu().numpy(), burn.polygon_winner(HOST, *polygons[:3]))
    # offsets are checked on the device before anything is read through them
    bad = d_polygons[1].clone()
    bad[-1] += 5
    try:
        xa.burn_vector_geometry(grid, polygons=(d_polygons[0], bad, d_polygons[2]))
    except ValueError as e:
        assert "ring_offsets" in str(e)
    else:
        raise AssertionError("offsets past the coordinates were accepted")
    assert grid._host is None


if __name__ == "__main__":
    device_grid()
    print("TORCH_BURN_OK")

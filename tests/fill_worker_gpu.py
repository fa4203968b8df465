"""Worker of test_torch_route_and_regrid_then_fill: the fills on torch tensors that live on the GPU.  torch first (its HIP
runtime has to be up before the engine binds the device), then the package."""
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
from fill_cases import brute_nearest, scaled_residual  # noqa: E402
from xugrid_amd import fill, meshgen  # noqa: E402


def torch_route():
    """A tensor in gives a float64 tensor out on the same device, the input unchanged, equal to the numpy route."""
    xy, faces = meshgen.triangle_mesh(2000, 0)
    grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    c = grid.centroids
    rng = np.random.default_rng(0)
    data = np.stack([np.sin(3 * c[:, 0]) + c[:, 1]] * 2)
    data[0, rng.random(grid.n_face) < 0.2] = np.nan
    data[1, np.hypot(c[:, 0] - 0.5, c[:, 1] - 0.5) < 0.2] = np.nan
    t = torch.tensor(data, device="cuda:0")
    before = t.clone()
    for method in (grid.laplace_interpolate, grid.interpolate_na):
        out = method(t)
        assert isinstance(out, torch.Tensor) and out.device == t.device and out.dtype == torch.float64
        assert torch.equal(torch.nan_to_num(t, nan=-7.0), torch.nan_to_num(before, nan=-7.0))
        assert np.array_equal(out.cpu().numpy(), method(data), equal_nan=True)
        assert not torch.isnan(out).any()
    f32 = grid.laplace_interpolate(t.float())
    assert f32.dtype == torch.float64


def regrid_then_fill():
    """A device grid regridded onto a larger target (NaN outside the source), then both fills: no NaN left, the nearest
    fill equal to a brute-force search on the regridded values, the Laplace fill within the CG's stopping rule."""
    sxy, sf = meshgen.triangle_mesh(2000, 0)
    txy, tf = meshgen.triangle_mesh(3000, 1, 0.0, 1.4)
    source = xa.Ugrid2d.from_device_arrays(torch.tensor(sxy, device="cuda:0"), torch.tensor(sf, device="cuda:0"))
    target = xa.Ugrid2d(txy[:, 0] - 0.2, txy[:, 1] - 0.2, -1, tf)
    data = torch.tensor(meshgen.smooth_field(source.centroids, 0), device="cuda:0")
    out = xa.OverlapRegridder(source, target, method="mean").regrid(data)
    assert isinstance(out, torch.Tensor) and torch.isnan(out).any()
    for filled in (target.interpolate_na(out), target.laplace_interpolate(out)):
        assert isinstance(filled, torch.Tensor) and not torch.isnan(filled).any()
    regridded = out.cpu().numpy()
    near = target.interpolate_na(out).cpu().numpy()
    assert np.array_equal(near, regridded[brute_nearest(target.centroids, regridded)])
    lap = target.laplace_interpolate(out).cpu().numpy()
    conn = target.get_connectivity_matrix("face", xy_weights=True)
    assert scaled_residual(lap, regridded, conn, True) < 1e-4


def more_slices_than_one_launch_grid():
    """tests/test_gpu_fill_edges.py::test_more_slices_than_one_launch_grid on a tensor: K = 70 000 slices, tiled."""
    from test_gpu_fill_edges import K_BIG, SAMPLE, big_stack

    grid, data = big_stack()
    t = torch.tensor(data, device="cuda:0")
    near = grid.interpolate_na(t)
    lap = grid.laplace_interpolate(t)
    iters = fill.last_iterations
    assert tuple(near.shape) == tuple(lap.shape) == data.shape and iters.shape == (K_BIG,)
    near, lap = near.cpu().numpy(), lap.cpu().numpy()
    for k in SAMPLE:
        assert np.array_equal(near[k].view(np.int64), grid.interpolate_na(data[k]).view(np.int64)), k
        assert np.array_equal(lap[k].view(np.int64), grid.laplace_interpolate(data[k]).view(np.int64)), k
        assert iters[k] == fill.last_iterations[0], k


if __name__ == "__main__":
    torch_route()
    regrid_then_fill()
    more_slices_than_one_launch_grid()
    print("TORCH_FILL_OK")

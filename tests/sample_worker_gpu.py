"""Worker of test_torch_route_and_device_grid: point and line sampling on torch tensors that live on the GPU, and on a grid
made from device arrays.  torch first (its HIP runtime has to be up before the engine binds the device), then the package."""
import os
import sys
import warnings

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import xugrid_amd as xa  # noqa: E402
from xugrid_amd import meshgen  # noqa: E402

XY, FACES = meshgen.triangle_mesh(100_000, 0)
HOST = xa.Ugrid2d(XY[:, 0], XY[:, 1], -1, FACES)


def torch_route():
    """A tensor in gives a float64 tensor out on the same device, equal to the numpy route bit for bit; the input unchanged."""
    rng = np.random.default_rng(21)
    pts = rng.uniform(-0.05, 1.05, (5000, 2))
    for dtype in (np.float64, np.float32):
        data = rng.normal(size=(3, 2, HOST.n_face)).astype(dtype)
        t = torch.tensor(data, device="cuda:0")
        before = t.clone()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host = HOST.sel_points(data, pts[:, 0], pts[:, 1])
            got = HOST.sel_points(t, pts[:, 0], pts[:, 1])
        assert isinstance(got.values, torch.Tensor) and got.values.device == t.device and got.values.dtype == torch.float64
        assert tuple(got.values.shape) == (3, 2, 5000) and np.isnan(host.values).any()
        assert np.array_equal(got.values.cpu().numpy().view(np.int64), host.values.view(np.int64))
        assert torch.equal(t, before) and np.array_equal(got.index, host.index)


def device_grid():
    """``Ugrid2d.from_device_arrays``: sel_points on face and node data and intersect_line never make the host copy."""
    grid = xa.Ugrid2d.from_device_arrays(torch.tensor(XY, device="cuda:0"), torch.tensor(FACES, device="cuda:0"))

    def fail():
        raise AssertionError("the host copy of a device grid was made")

    grid._materialise = fail
    rng = np.random.default_rng(41)
    pts = rng.uniform(-0.05, 1.05, (4000, 2))
    face_data, node_data = rng.normal(size=(3, HOST.n_face)), rng.normal(size=(2, HOST.n_node))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for data, dim, method in ((face_data, None, None), (node_data, "node", None), (face_data, None, "nearest")):
            got = grid.sel_points(torch.tensor(data, device="cuda:0"), pts[:, 0], pts[:, 1], dim=dim, method=method)
            expected = HOST.sel_points(data, pts[:, 0], pts[:, 1], dim=dim, method=method)
            assert isinstance(got.values, torch.Tensor) and got.values.is_cuda
            assert np.isnan(expected.values).any() and not np.isnan(expected.values).all()
            assert np.array_equal(got.values.cpu().numpy(), expected.values, equal_nan=True)
    got = grid.intersect_line(torch.tensor(face_data, device="cuda:0"), (-0.2, -0.1), (1.2, 1.1))
    expected = HOST.intersect_line(face_data, (-0.2, -0.1), (1.2, 1.1))
    assert len(expected.s) > 500
    for a, b in zip(got, expected):
        assert isinstance(a, torch.Tensor) and a.is_cuda
        assert np.array_equal(a.cpu().numpy(), b)
    assert bool(torch.all(got.s[1:] >= got.s[:-1]))
    # device points in, device indices out
    idx = grid.locate_nearest_face(torch.tensor(pts, device="cuda:0"))
    assert isinstance(idx, torch.Tensor) and idx.dtype == torch.int64
    assert np.array_equal(idx.cpu().numpy(), HOST.locate_nearest_face(pts))
    assert np.array_equal(grid.locate_nearest_node(torch.tensor(pts, device="cuda:0")).cpu().numpy(), HOST.locate_nearest_node(pts))
    assert grid._host is None


if __name__ == "__main__":
    torch_route()
    device_grid()
    print("TORCH_SAMPLE_OK")

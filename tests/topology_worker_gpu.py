"""Worker of test_gpu_topology.py::test_no_host_detour_on_a_device_grid: a grid made from torch tensors on the GPU fills,
labels and dilates without ever downloading its mesh.  torch first (its HIP runtime has to be up before the engine binds the
device), then the package."""
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
from fill_cases import scaled_residual  # noqa: E402
from graph_cases import binary_iterate  # noqa: E402
from scipy.sparse import csgraph  # noqa: E402
from xugrid_amd import meshgen  # noqa: E402


def no_host_detour():
    xy, faces = meshgen.triangle_mesh(3000, 0)
    grid = xa.Ugrid2d.from_device_arrays(torch.tensor(xy, device="cuda:0"), torch.tensor(faces, device="cuda:0"))
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    c = host.centroids
    data = np.sin(3 * c[:, 0]) + c[:, 1]
    data[np.hypot(c[:, 0] - 0.5, c[:, 1] - 0.5) < 0.2] = np.nan
    data[np.random.default_rng(0).random(data.size) < 0.1] = np.nan
    t = torch.tensor(data, device="cuda:0")
    lap = grid.laplace_interpolate(t)
    assert isinstance(lap, torch.Tensor) and not torch.isnan(lap).any()
    e = host.edge_coordinates
    edge_data = np.cos(4 * e[:, 0]) - e[:, 1]
    edge_data[np.random.default_rng(1).random(edge_data.size) < 0.3] = np.nan
    near = grid.interpolate_na(torch.tensor(edge_data, device="cuda:0"), dim="edge")
    assert isinstance(near, torch.Tensor) and not torch.isnan(near).any()
    comp = grid.connected_components()
    index = grid.locate_nearest_edge(torch.tensor(e[:50], device="cuda:0"))
    assert grid._host is None, "the device grid downloaded its mesh"
    # ... and the answers are right
    assert np.array_equal(near.cpu().numpy(), host.interpolate_na(edge_data, dim="edge"))
    assert np.array_equal(comp, csgraph.connected_components(host.face_face_connectivity, directed=False)[1])
    assert np.array_equal(index.cpu().numpy(), np.arange(50))
    conn = host.get_connectivity_matrix("face", xy_weights=True)
    assert scaled_residual(lap.cpu().numpy(), data, conn, True) < 1e-4


def tensor_in_tensor_out():
    xy, faces = meshgen.triangle_mesh(3000, 0)
    grid = xa.Ugrid2d.from_device_arrays(torch.tensor(xy, device="cuda:0"), torch.tensor(faces, device="cuda:0"))
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    rng = np.random.default_rng(4)
    field = rng.random((2, grid.n_face)) < 0.3
    mask = rng.random(grid.n_face) < 0.1
    for dtype in (torch.bool, torch.uint8):
        t = torch.tensor(field, device="cuda:0").to(dtype)
        before = t.clone()
        out = grid.binary_dilation(t, 2, mask=torch.tensor(mask, device="cuda:0"), border_value=True)
        assert isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == t.device and tuple(out.shape) == field.shape
        assert torch.equal(t, before)
        for k in range(2):
            exp = binary_iterate(host.face_face_connectivity, field[k], True, 2, mask, host.exterior_faces, True)
            assert np.array_equal(out[k].cpu().numpy().astype(bool), exp)
    assert grid._host is None


if __name__ == "__main__":
    no_host_detour()
    tensor_in_tensor_out()
    print("TORCH_TOPOLOGY_OK")

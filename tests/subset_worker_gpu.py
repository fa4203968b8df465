"""Worker of test_torch_in_torch_out (tests/test_gpu_subset.py): sub-meshes with torch tensors as indexers and as data, on a
host grid and on a grid made from tensors.  torch first (its HIP runtime has to be up before the engine binds the device),
then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import subset_cases as sc  # noqa: E402
import xugrid_amd as xa  # noqa: E402
from subset_cases import assert_grid, assert_indexes, to_numpy  # noqa: E402
from xugrid_amd import meshgen  # noqa: E402


def grids(xy, faces):
    yield xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    yield xa.Ugrid2d.from_device_arrays(torch.tensor(xy, device="cuda:0"), torch.tensor(faces, device="cuda:0"))


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def torch_indexes():
    """A torch index gives torch indexes; a bool tensor is a mask; an int32 tensor is widened; refusals are worded alike."""
    xy, faces = sc.mesh("mixed36")
    index = sc.selections("mixed36")["permuted_subset"]
    mask = sc.selections("mixed36")["mask"]
    xy_sub, faces_sub, node_index, ids = sc.topology_subset(xy, faces, index)
    m_xy, m_faces, m_nodes, m_ids = sc.topology_subset(xy, faces, mask)
    for grid in grids(xy, faces):
        for tensor in (cuda(index), cuda(index.astype(np.int32))):
            before = tensor.clone()
            sub, indexes = grid.topology_subset(tensor, return_index=True)
            assert type(sub) is type(grid)
            assert_grid(sub, xy_sub, faces_sub)
            assert_indexes(grid, indexes, node_index, sc.edge_index(faces, ids), ids, torch.Tensor)
            assert all(v.is_cuda for v in indexes.values()) and torch.equal(tensor, before)
        sub, indexes = grid.isel({grid.face_dimension: cuda(index)}, return_index=True)
        assert_indexes(grid, indexes, node_index, sc.edge_index(faces, ids), ids, torch.Tensor)
        sub, indexes = grid.topology_subset(cuda(mask), return_index=True)
        assert_grid(sub, m_xy, m_faces)
        assert_indexes(grid, indexes, m_nodes, sc.edge_index(faces, m_ids), m_ids, torch.Tensor)
        assert grid.topology_subset(torch.ones(grid.n_face, dtype=torch.bool, device="cuda:0")) is grid
        assert grid.topology_subset(torch.arange(grid.n_face, device="cuda:0")) is grid
        n = grid.n_face
        for bad, error in (([3, 5, 3], ValueError), ([0, n], IndexError), ([2, -1], IndexError)):
            for call in (lambda t: grid.topology_subset(t), lambda t: grid.isel({grid.node_dimension: t})):
                try:
                    call(cuda(np.array(bad)))
                except error:
                    pass
                else:
                    raise AssertionError(f"{bad} was not refused")
        try:
            grid.topology_subset(torch.ones(n - 1, dtype=torch.bool, device="cuda:0"))
        except ValueError:
            pass
        else:
            raise AssertionError("a short mask was not refused")
        assert_grid(grid.topology_subset(cuda(index)), xy_sub, faces_sub)  # usable afterwards


def torch_data_through_isel():
    """isel by face, node and edge with f32 and f64 tensors on every facet: tensors out, float64, equal to numpy's take."""
    xy, faces = sc.mesh("disconnected")
    face_ids = np.arange(len(meshgen.triangle_mesh(30, 1)[1]), len(faces) - 1)  # the second patch
    xy_sub, faces_sub, node_index, edge_index, ids = sc.isel(xy, faces, face=face_ids)
    by = {"face": ids, "node": node_index, "edge": edge_index}
    rng = np.random.default_rng(3)
    for grid in grids(xy, faces):
        dims = {"face": grid.face_dimension, "node": grid.node_dimension, "edge": grid.edge_dimension}
        for dtype in (np.float32, np.float64):
            for selector in ("face", "node", "edge"):
                for facet in by:
                    data = rng.random((2, getattr(grid, f"n_{facet}"))).astype(dtype)
                    for indexer in (by[selector], cuda(by[selector])):
                        sub, indexes, values = grid.isel({dims[selector]: indexer}, return_index=True, data=cuda(data))
                        assert_grid(sub, xy_sub, faces_sub)
                        assert_indexes(grid, indexes, node_index, edge_index, ids)
                        assert isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64
                        assert np.array_equal(to_numpy(values), data[:, by[facet]].astype(np.float64))


if __name__ == "__main__":
    torch_indexes()
    torch_data_through_isel()
    print("TORCH_SUBSET_OK")

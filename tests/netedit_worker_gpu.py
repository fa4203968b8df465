"""Worker of test_torch_in_torch_out (tests/test_gpu_netedit.py): the network edits with torch tensors as indexers, as data and as
vertices.  torch first (its HIP runtime has to be up before the engine binds the device), then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import netedit_cases as nc  # noqa: E402
import xugrid_amd as xa  # noqa: E402


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def grid_of(xy, edges):
    return xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, edges)


def same_network(grid, xy, edges):
    return np.array_equal(grid.node_coordinates.view(np.uint64), np.ascontiguousarray(xy).view(np.uint64)) and np.array_equal(
        grid.edge_node_connectivity, edges)


def is_index(t, want):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), want)


def subset_with_tensors():
    xy, edges = nc.random_network(2000)
    grid = grid_of(xy, edges)
    index = np.random.default_rng(70).permutation(len(edges))[:1000]
    e_xy, e_edges, e_nodes = nc.subset_ref(xy, edges, index)
    for tensor in (cuda(index), cuda(index.astype(np.int32))):
        before = tensor.clone()
        sub, indexes = grid.topology_subset(tensor, return_index=True)
        assert same_network(sub, e_xy, e_edges) and torch.equal(tensor, before)
        assert is_index(indexes[grid.node_dimension], e_nodes) and is_index(indexes[grid.edge_dimension], index)
    mask = np.zeros(len(edges), dtype=bool)
    mask[index] = True
    sub, indexes = grid.isel({grid.edge_dimension: cuda(mask)}, return_index=True)
    assert same_network(sub, *nc.subset_ref(xy, edges, np.flatnonzero(mask))[:2])
    assert is_index(indexes[grid.edge_dimension], np.flatnonzero(mask))
    data = np.random.default_rng(71).random((2, len(edges))).astype(np.float32)
    sub, values = grid.isel({grid.edge_dimension: cuda(index)}, data=cuda(data))
    assert isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64
    assert np.array_equal(values.cpu().numpy(), data[:, index].astype(np.float64))
    try:
        grid.topology_subset(cuda(np.array([4, 9, 4])))
        raise AssertionError("a repeated id was accepted")
    except ValueError as e:
        assert "repeated" in str(e)
    print("subset_with_tensors ok")


def merge_with_tensor_data():
    parts = nc.MERGE_CASES["overlapping"]()
    e = nc.merge_ref(parts)
    grids = [grid_of(xy, edges) for xy, edges in parts]
    rng = np.random.default_rng(72)
    for facet, key in (("node", "node_index"), ("edge", "edge_index")):
        data = [rng.random((3, getattr(g, f"n_{facet}"))) for g in grids]
        merged, indexes, values = xa.merge_partitions(grids, return_index=True, data=[cuda(d) for d in data],
                                                      dim=getattr(grids[0], f"{facet}_dimension"))
        assert same_network(merged, e["xy"], e["edges"])
        assert all(is_index(t, want) for t, want in zip(indexes[getattr(merged, f"{facet}_dimension")], e[key]))
        assert isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64
        assert np.array_equal(values.cpu().numpy(), np.concatenate([d[:, i] for d, i in zip(data, e[key])], axis=1))
    print("merge_with_tensor_data ok")


def refine_with_tensors():
    xy, edges, vertices, tolerance, _ = nc.REFINE_CASES["long_row"]()
    e = nc.refine_ref(xy, edges, vertices, tolerance)
    grid = grid_of(xy, edges)
    tensor = cuda(vertices)
    before = tensor.clone()
    data = np.array([[1.5, -2.0], [3.0, 4.0]])
    refined, node_index, values = grid.refine_by_vertices(tensor, return_index=True, tolerance=tolerance, data=cuda(data))
    assert same_network(refined, e["xy"], e["edges"]) and torch.equal(tensor, before)
    assert is_index(node_index, e["node_index"])
    assert isinstance(values, torch.Tensor) and values.is_cuda and np.array_equal(values.cpu().numpy(), data[:, e["parent_edge"]])
    try:
        grid.refine_by_vertices(cuda(np.array([[5.0, 0.0], [5.0, 1.0]])), tolerance=0.5)
        raise AssertionError("a vertex off every edge was accepted")
    except ValueError as err:
        assert str(err) == f"The following vertices are not located on any edge:\n{np.array([[5.0, 1.0]])}"
    print("refine_with_tensors ok")


if __name__ == "__main__":
    subset_with_tensors()
    merge_with_tensor_data()
    refine_with_tensors()
    print("TORCH_NETEDIT_OK")

"""Worker of tests/test_gpu_netfill.py::test_torch_route: the network fill and network_distance on torch tensors that live on
the GPU.  torch first (its HIP runtime has to be up before the engine binds the device), then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import netfill_cases as nc  # noqa: E402
import xugrid_amd as xa  # noqa: E402


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def fill_kinds(xy, edges, grid):
    """A float64 tensor in gives a float64 tensor out on the same device, the input unchanged; a float32 tensor comes back as
    float64; both equal to the reference on the same values."""
    n = len(edges)
    graph = nc.reference_graph(xy, edges, "edge")
    data = nc.slice_data(n).reshape(3, 1, n)
    expected = np.stack([nc.reference_fill(row, graph, nc.SLICE_LIMIT) for row in data[:, 0]]).reshape(3, 1, n)
    t64 = torch.tensor(data, device="cuda:0")
    out = grid.interpolate_na(t64, max_distance=nc.SLICE_LIMIT, metric="network")
    assert isinstance(out, torch.Tensor) and out.device == t64.device and out.dtype == torch.float64 and tuple(out.shape) == (3, 1, n)
    assert same(out.cpu().numpy(), expected)
    assert same(t64.cpu().numpy(), data)
    assert same(grid.interpolate_na(data, max_distance=nc.SLICE_LIMIT, metric="network"), expected)  # (numpy in, numpy out)
    out = grid.interpolate_na(t64.float(), max_distance=nc.SLICE_LIMIT, metric="network")
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float64
    data32 = data.astype(np.float32).astype(np.float64)
    assert same(out.cpu().numpy(), np.stack([nc.reference_fill(row, graph, nc.SLICE_LIMIT) for row in data32[:, 0]]).reshape(3, 1, n))


def distance_kinds(xy, edges, grid):
    for facet in ("node", "edge"):
        for max_distance in (None, 0.6):
            mask, ids, d_ref, s_ref = nc.distance_case(xy, edges, facet, max_distance)
            for sources in (torch.tensor(mask, device="cuda:0"), torch.tensor(ids, device="cuda:0")):
                distance, source = grid.network_distance(sources, dim=facet, max_distance=max_distance)
                assert isinstance(distance, torch.Tensor) and distance.is_cuda and distance.dtype == torch.float64
                assert isinstance(source, torch.Tensor) and source.is_cuda and source.dtype == torch.int64
                assert np.array_equal(distance.cpu().numpy(), d_ref) and np.array_equal(source.cpu().numpy(), s_ref)
    try:
        grid.network_distance(torch.tensor([1, 1], device="cuda:0"), dim="node")
    except ValueError as e:
        assert "unique" in str(e)
    else:
        raise AssertionError("repeated ids were accepted")


if __name__ == "__main__":
    xy, edges = nc.random_network()
    grid = xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, edges)
    fill_kinds(xy, edges, grid)
    distance_kinds(xy, edges, grid)
    print("TORCH_NETFILL_OK")

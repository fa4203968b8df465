"""Worker of test_torch_in_torch_out (tests/test_gpu_partition.py): merging and matching with torch tensors as labels, as data
and as coordinates, on host grids and on grids made from tensors.  torch first (its HIP runtime has to be up before the engine
binds the device), then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import partition_cases as pc  # noqa: E402
import subset_cases as sc  # noqa: E402
import xugrid_amd as xa  # noqa: E402
from partition_cases import assert_index_lists, assert_merged, to_numpy  # noqa: E402


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def host_grid(xy, faces):
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)


def tensor_grid(xy, faces):
    return xa.Ugrid2d.from_device_arrays(cuda(xy), cuda(faces))


def merge_with_tensor_data():
    """Tensor data gives a tensor result and tensor indexes, whatever the kind of the grids."""
    name = "mixed36_halo3"
    e = pc.expected(name)
    rng = np.random.default_rng(31)
    for make in (host_grid, tensor_grid):
        grids = [make(xy, faces) for xy, faces in pc.partitions(name)]
        for facet, sizes in (("node", [g.n_node for g in grids]), ("face", [g.n_face for g in grids]), ("edge", [g.n_edge for g in grids])):
            data = [rng.random((3, n)).astype(np.float32 if facet == "face" else np.float64) for n in sizes]
            dim = getattr(grids[0], f"{facet}_dimension")
            merged, indexes, values = xa.merge_partitions(grids, return_index=True, data=[cuda(d) for d in data], dim=dim)
            assert_merged(merged, e)
            assert_index_lists(merged, indexes, e, torch.Tensor)
            assert isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64
            assert np.array_equal(values.cpu().numpy(), pc.merge_data(e, data, facet)), facet
    print("merge_with_tensor_data ok")


def tensor_labels():
    xy, faces = sc.mesh("mixed36")
    labels = np.random.default_rng(37).integers(0, 4, size=len(faces))
    want = pc.labels_to_indices(labels)
    for tensor in (cuda(labels), cuda(labels.astype(np.int32))):
        before = tensor.clone()
        got = xa.labels_to_indices(tensor)
        assert len(got) == len(want) and all(isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.int64 for g in got)
        assert all(np.array_equal(to_numpy(g), w) for g, w in zip(got, want)) and torch.equal(tensor, before)
    try:
        xa.labels_to_indices(cuda(labels.astype(np.float64)))
    except TypeError as err:
        assert "labels must have integer dtype" in str(err)
    else:
        raise AssertionError("float labels were accepted")
    for make in (host_grid, tensor_grid):
        grid = make(xy, faces)
        data = np.arange(grid.n_face, dtype=np.float64)
        pieces = grid.partition_by_label(cuda(labels), data=cuda(data))
        assert len(pieces) == len(want)
        for (sub, indexes, values), ids in zip(pieces, want):
            assert type(sub) is type(grid) and sub.n_face == len(ids)
            assert isinstance(indexes[grid.face_dimension], torch.Tensor) and np.array_equal(to_numpy(indexes[grid.face_dimension]), ids)
            assert isinstance(values, torch.Tensor) and np.array_equal(values.cpu().numpy(), data[ids])
        merged, merged_data = xa.merge_partitions([p[0] for p in pieces], data=[p[2] for p in pieces])
        back = merged.reindex_like(grid, merged_data)
        assert isinstance(back, torch.Tensor) and np.array_equal(back.cpu().numpy(), data)
    print("tensor_labels ok")


def tensor_coordinates():
    for name, (a, b, tolerance) in pc.like_cases().items():
        got = xa.connectivity.index_like_device(cuda(a), cuda(b), tolerance=tolerance)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), pc.index_like(a, b, tolerance)), name
    try:
        xa.connectivity.index_like_device(cuda(np.zeros((3, 2))), cuda(np.zeros((3, 2))))
    except ValueError as err:
        assert "not identical after sorting" in str(err)
    else:
        raise AssertionError("repeated keys were accepted")
    print("tensor_coordinates ok")


if __name__ == "__main__":
    merge_with_tensor_data()
    tensor_labels()
    tensor_coordinates()
    print("TORCH_PARTITION_OK")

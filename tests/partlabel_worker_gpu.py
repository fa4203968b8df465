"""Worker of test_torch_in_torch_out (tests/test_gpu_partlabel.py): ``label_partitions`` / ``partition`` with torch tensors as
weights, on a host grid and on a grid made from tensors.  torch first (its HIP runtime has to be up before the engine binds the
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

import partlabel_cases as pc  # noqa: E402
import rcm_cases as rc  # noqa: E402
import xugrid_amd as xa  # noqa: E402


def main():
    xy, faces = rc.delaunay(300, 0)
    A = rc.face_graph(faces)
    w = pc.half_weights(len(faces))
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    device = xa.Ugrid2d.from_device_arrays(torch.tensor(xy, device="cuda:0"), torch.tensor(faces, device="cuda:0"))
    expected = pc.label(A, host.centroids, 4, w)[0]
    for grid in (host, device):
        for dtype in (torch.int64, torch.int32):
            tensor = torch.as_tensor(w).to("cuda:0").to(dtype)
            before = tensor.clone()
            labels = grid.label_partitions(4, weights=tensor)
            assert isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int64
            assert np.array_equal(labels.cpu().numpy(), expected)
            assert torch.equal(tensor, before)
        try:
            grid.label_partitions(4, weights=torch.as_tensor(w).to("cuda:0").double())
            raise AssertionError("float weights were accepted")
        except TypeError as e:
            assert "Wrong type on weights." in str(e)
        try:
            grid.label_partitions(4, weights=-torch.as_tensor(w).to("cuda:0"))
            raise AssertionError("negative weights were accepted")
        except ValueError as e:
            assert "Wrong values on weights." in str(e)
        entries = grid.partition(4, weights=torch.as_tensor(w).to("cuda:0"), return_index=True)
        assert len(entries) == 4
        for label, (part, indexes) in enumerate(entries):
            index = indexes[grid.face_dimension]
            assert type(part) is type(grid) and isinstance(index, torch.Tensor) and index.is_cuda
            assert np.array_equal(index.cpu().numpy(), np.nonzero(expected == label)[0])
        plain = grid.label_partitions(4)  # no torch in: numpy for the host grid, a DeviceArray for the device grid
        assert isinstance(plain, np.ndarray if grid is host else xa.engine.DeviceArray)


if __name__ == "__main__":
    main()
    print("TORCH_PARTLABEL_OK")

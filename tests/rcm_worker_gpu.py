"""Worker of test_torch_in_torch_out (tests/test_gpu_rcm.py): ``reverse_cuthill_mckee`` with torch tensors as data, on a host
grid and on a grid made from tensors.  torch first (its HIP runtime has to be up before the engine binds the device), then the
package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import rcm_cases as rc  # noqa: E402
import xugrid_amd as xa  # noqa: E402


def main():
    xy, faces = rc.with_ear(*rc.delaunay(300, 0))
    expected = rc.sequential(rc.face_graph(faces))
    data = np.random.default_rng(3).random((3, len(faces)))
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    device = xa.Ugrid2d.from_device_arrays(torch.tensor(xy, device="cuda:0"), torch.tensor(faces, device="cuda:0"))
    for grid in (host, device):
        for dtype in (np.float32, np.float64):
            tensor = torch.as_tensor(data.astype(dtype)).to("cuda:0")
            before = tensor.clone()
            reordered, index, moved = grid.reverse_cuthill_mckee(data=tensor, return_device=True)
            assert type(reordered) is type(grid)
            assert np.array_equal(reordered.face_node_connectivity, faces[expected])
            assert np.array_equal(reordered.node_coordinates, xy)
            assert isinstance(moved, torch.Tensor) and moved.is_cuda and moved.dtype == torch.float64
            assert np.array_equal(moved.cpu().numpy(), data.astype(dtype)[:, expected].astype(np.float64))
            assert torch.equal(tensor, before)
            if grid is device:  # the index is of the data's kind and never leaves the device
                assert isinstance(index, torch.Tensor) and index.is_cuda and index.dtype == torch.int64
                assert np.array_equal(index.cpu().numpy(), expected)
            else:
                assert isinstance(index, np.ndarray) and np.array_equal(index, expected)
        _, index = grid.reverse_cuthill_mckee()
        assert isinstance(index, np.ndarray) and np.array_equal(index, expected)


if __name__ == "__main__":
    main()
    print("TORCH_RCM_OK")

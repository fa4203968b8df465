"""Worker of test_torch_in_torch_out (tests/test_gpu_periodic.py): both conversions with torch tensors as data, on host grids and
on grids made from tensors.  torch first (its HIP runtime has to be up before the engine binds the device), then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import periodic_cases as pc  # noqa: E402
import xugrid_amd as xa  # noqa: E402
from periodic_cases import assert_grid, assert_indexes  # noqa: E402


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def host_grid(xy, faces):
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)


def tensor_grid(xy, faces):
    return xa.Ugrid2d.from_device_arrays(cuda(xy), cuda(faces))


def tensor_data():
    """Tensor data gives a tensor result and tensor indexes, whatever the kind of the grid."""
    rng = np.random.default_rng(59)
    for name in ("shuffled", "mixed"):
        xy, faces, xmax = pc.mesh(name)
        wrapped_e, unwrapped_e = pc.expected(name)
        for make in (host_grid, tensor_grid):
            grid = make(xy, faces)
            wrapped = grid.to_periodic()
            for source, e, convert in ((grid, wrapped_e, lambda **kw: grid.to_periodic(**kw)),
                                       (wrapped, unwrapped_e, lambda **kw: wrapped.to_nonperiodic(xmax, **kw))):
                for facet in ("node", "edge", "face"):
                    data = rng.random((3, getattr(source, f"n_{facet}"))).astype(np.float32 if facet == "face" else np.float64)
                    tensor = cuda(data)
                    before = tensor.clone()
                    new, indexes, values = convert(data=tensor, dim=getattr(source, f"{facet}_dimension"), return_index=True)
                    assert type(new) is type(grid)
                    assert_grid(new, e)
                    assert_indexes(source, indexes, e, torch.Tensor)
                    assert all(i.is_cuda and i.dtype == torch.int64 for i in indexes.values())
                    assert isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64
                    assert np.array_equal(values.cpu().numpy(), data[..., e[f"{facet}_index"]].astype(np.float64)), facet
                    assert torch.equal(tensor, before)
    print("tensor_data ok")


def refusal_leaves_tensors_usable():
    xy, faces, _ = pc.mesh("quads32")
    moved = xy.copy()
    moved[7, 1] += 0.25
    try:
        tensor_grid(moved, faces).to_periodic(data=cuda(np.zeros(len(faces))))
    except ValueError as err:
        assert "y-coordinates of the left and right boundaries do not match" in str(err)
    else:
        raise AssertionError("mismatching boundaries were accepted")
    assert_grid(tensor_grid(xy, faces).to_periodic(), pc.expected("quads32")[0])
    print("refusal_leaves_tensors_usable ok")


if __name__ == "__main__":
    tensor_data()
    refusal_leaves_tensors_usable()
    print("TORCH_PERIODIC_OK")

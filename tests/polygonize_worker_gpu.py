"""Worker of test_torch_in_torch_out: polygonize on a grid made from device arrays with a torch tensor of face data.  torch
first (its HIP runtime has to be up before the engine binds the device), then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import polygonize_cases as pc  # noqa: E402
import xugrid_amd as xa  # noqa: E402

KEYS = ("coords", "ring_offsets", "polygon_offsets", "values", "face_polygon")


def torch_in_torch_out():
    """Tensors in give tensors out, equal to the yardstick; the round trip through burn_vector_geometry stays on the device;
    the input is unchanged and the host copy of the grid is never made."""
    xy, faces, data = pc.case("nested")
    e = pc.expected("nested")
    grid = xa.Ugrid2d.from_device_arrays(torch.tensor(xy, device="cuda:0"), torch.tensor(faces, device="cuda:0"))
    for dtype in (torch.float64, torch.float32):
        tensor = torch.from_numpy(data).to("cuda:0").to(dtype)
        before = tensor.clone()
        out = grid.polygonize(tensor, return_index=True)
        assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in out)
        assert [a.dtype for a in out] == [torch.float64, torch.int64, torch.int64, torch.float64, torch.int64]
        for key, got in zip(KEYS, out):
            got = got.cpu().numpy()
            assert got.shape == e[key].shape and np.array_equal(got, e[key], equal_nan=True), key
        assert torch.equal(torch.nan_to_num(tensor, nan=-7.0), torch.nan_to_num(before, nan=-7.0))
        back = xa.burn_vector_geometry(grid, polygons=out[:4])
        assert isinstance(back, torch.Tensor) and back.is_cuda and np.array_equal(back.cpu().numpy(), data, equal_nan=True)
        assert len(xa.polygonize(grid, tensor)) == 4
    labels = torch.tensor(np.nan_to_num(data, nan=7.0).astype(np.int32), device="cuda:0")  # int32: no NaN, the gap is a class
    out = grid.polygonize(labels, return_index=True)
    want = pc.polygonize_numpy(xy, faces, np.nan_to_num(data, nan=7.0))
    for key, got in zip(KEYS, out):
        assert np.array_equal(got.cpu().numpy(), want[key]), key
    assert grid._host is None


if __name__ == "__main__":
    torch_in_torch_out()
    print("TORCH_POLYGONIZE_OK")

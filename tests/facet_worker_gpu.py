"""Worker of test_torch_tensor_in_gives_tensor_out: facet mapping on torch tensors that live on the GPU, on a host-built grid
and on a grid made from device tensors.  torch first (its HIP runtime has to be up before the engine binds the device), then
the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import facet_cases as fc  # noqa: E402
import graph_cases as gc  # noqa: E402
import xugrid_amd as xa  # noqa: E402


def main():
    xy, faces = gc.disconnected()
    tables = fc.host_tables(faces, len(xy))
    n = fc.sizes(tables)
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    device = xa.Ugrid2d.from_device_arrays(torch.tensor(xy, device="cuda:0"), torch.tensor(faces, device="cuda:0"))

    def fail():
        raise AssertionError("the host copy of a device grid was made")

    device._materialise = fail
    for grid in (host, device):
        for dtype in (np.float64, np.float32):
            for target, source in fc.DIRECTIONS:
                data = fc.field(n[source], K=4, seed=13, dtype=dtype).reshape(2, 2, -1)
                t = torch.tensor(data, device="cuda:0")
                before = t.clone()
                for form in (None,) + fc.REDUCERS:
                    got = getattr(grid, f"to_{target}")(t, dim=source, reduce=form)
                    assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == torch.float64
                    wide = data.astype(np.float64)
                    table = tables[(target, source)]
                    exp = fc.raw(table, wide) if form is None else fc.reduce_sequential(table, wide, form)
                    assert tuple(got.shape) == exp.shape, (target, source, form)
                    assert np.array_equal(got.cpu().numpy(), exp, equal_nan=True), (target, source, form)
                    assert torch.equal(t.view(torch.int64 if dtype == np.float64 else torch.int32),
                                       before.view(torch.int64 if dtype == np.float64 else torch.int32))
        try:
            grid.to_node(torch.zeros(n["face"], dtype=torch.int64, device="cuda:0"), dim="face")
        except TypeError:
            pass
        else:
            raise AssertionError("integer data was not refused")
    assert device._host is None
    print("TORCH_FACET_OK")


if __name__ == "__main__":
    main()

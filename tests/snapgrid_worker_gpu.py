"""Worker of test_torch_in_torch_out (tests/test_gpu_snapgrid.py): ``create_snap_to_grid_dataframe`` and ``snap_to_grid`` with
torch tensors as lines, on a host grid and on a grid made from tensors.  torch first (its HIP runtime has to be up before the
engine binds the device), then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import snapgrid_cases as sg  # noqa: E402
import xugrid_amd as xa  # noqa: E402
from oracle import oracle  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, dtype):
    got = got.cpu().numpy()
    want = np.asarray(want, dtype=dtype)
    return got.dtype == dtype and got.shape == want.shape and (
        np.array_equal(bits(got), bits(want)) if dtype == np.float64 else np.array_equal(got, want))


def main():
    oracle.build()
    node_xy, faces, coords, offsets, d = sg.CASES["random_mixed"]()
    values = np.arange(len(offsets) - 1, dtype=np.float64)
    host = xa.Ugrid2d(node_xy[:, 0].copy(), node_xy[:, 1].copy(), -1, faces)
    device = xa.Ugrid2d.from_device_arrays(torch.tensor(node_xy, device="cuda:0"), torch.tensor(faces, device="cuda:0"))
    frame = sg.frame_ref(oracle, node_xy, faces, host.centroids, host.face_edge_connectivity, host.edge_face_connectivity, coords,
                         offsets, d)
    winners = sg.winners_ref(frame, host.n_edge)
    for grid in (host, device):
        t_coords, t_offsets, t_values = (torch.as_tensor(a).to("cuda:0") for a in (coords, offsets, values))
        before = [t.clone() for t in (t_coords, t_offsets, t_values)]
        got = xa.create_snap_to_grid_dataframe((t_coords, t_offsets), grid, d)
        assert tuple(got) == sg.COLUMNS
        for column in sg.COLUMNS:
            assert isinstance(got[column], torch.Tensor) and got[column].device == t_coords.device
            assert same(got[column], frame[column], sg.FRAME_DTYPES[column]), column
        result = grid.snap_to_grid((t_coords, t_offsets, t_values), d)
        assert len(result) == 4 and all(isinstance(v, torch.Tensor) and v.device == t_coords.device for v in result)
        for v, w, dtype in zip(result, winners, (np.float64, np.int64, np.int64)):
            assert same(v, w, dtype)
        assert same(result[3], sg.gather_values(values, winners[0]), np.float64)
        assert all(torch.equal(t, b) for t, b in zip((t_coords, t_offsets, t_values), before))


if __name__ == "__main__":
    main()
    print("TORCH_SNAPGRID_OK")

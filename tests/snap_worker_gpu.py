"""Worker of test_torch_in_torch_out (tests/test_gpu_snap.py): snapping with torch tensors as coordinates.  torch first (its HIP
runtime has to be up before the engine binds the device), then the package."""
import os
import sys

import numpy as np
import torch

assert torch.cuda.is_available()
torch.zeros(1, device="cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import snap_cases as sc  # noqa: E402
import xugrid_amd as xa  # noqa: E402


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def same(t, want):
    want = np.asarray(want)
    got = t.cpu().numpy()
    view = np.uint64 if want.dtype.kind == "f" else np.int64
    return isinstance(t, torch.Tensor) and t.is_cuda and got.dtype == want.dtype and np.array_equal(got.view(view), want.view(view))


def nodes_with_tensors():
    x, y, d = sc.NODES_CASES["lattice257_0.5"]()
    e_inverse, _, e_x, e_y = sc.snap_nodes_ref(x, y, d)
    tx, ty = cuda(x), cuda(y)
    before = tx.clone()
    inverse, xs, ys = xa.snap_nodes(tx, ty, d)
    assert same(inverse, e_inverse.astype(np.int64)) and same(xs, e_x) and same(ys, e_y) and torch.equal(tx, before)
    x, y = sc.scattered(257)  # (nothing within the distance: None and copies)
    tx, ty = cuda(x), cuda(y)
    inverse, xs, ys = xa.snap_nodes(tx, ty, 1e-6)
    assert inverse is None and same(xs, x) and same(ys, y) and xs.data_ptr() != tx.data_ptr() and ys.data_ptr() != ty.data_ptr()
    print("nodes_with_tensors ok")


def to_nodes_with_tensors():
    x, y, to_x, to_y, d = sc.TO_CASES["random65x63_several"]()
    e_x, e_y, e_index, _ = sc.snap_to_nodes_ref(x, y, to_x, to_y, d)
    xs, ys, index = xa.snap_to_nodes(cuda(x), cuda(y), cuda(to_x), cuda(to_y), d, tiebreaker="nearest", return_index=True)
    assert same(xs, e_x) and same(ys, e_y) and same(index, e_index)
    try:
        xa.snap_to_nodes(cuda(x), cuda(y), cuda(to_x), cuda(to_y), d)
        raise AssertionError("ties were accepted")
    except ValueError as e:
        assert str(e) == sc.TIES
    print("to_nodes_with_tensors ok")


if __name__ == "__main__":
    nodes_with_tensors()
    to_nodes_with_tensors()
    print("TORCH_SNAP_OK")

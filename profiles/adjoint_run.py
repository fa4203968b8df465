"""The adjoint apply on the benchmark's matrix: what the transposition costs once, and what a call costs beside two
forward applies of code that existed before it.

On the 1M -> 1M Delaunay pair of bench.py (meshgen.triangle_mesh(500 000, 0) -> (500 000, 1, 30 deg, 0.7)), OverlapRegridder
weights built on the device, reducer `mean`, K = 1 and K = 256 float64 variables that stay in HBM (device pointers in, device
pointers out; wall clock around calls that end synchronised; 3 warm-ups, median of 15):
  * the one-off transposition: the first adjoint call of the process, and `transpose()` on a fresh cache -- which also allocates
    and fills the independent S x T handle it returns, so `transpose_ms` is an upper bound of the build (its kernels are listed);
  * the adjoint per call, with its kernels under the engine's per-kernel hipEvent table (in a run of its own);
  * the forward `mean` apply of the same K on the same matrix;
  * the forward `first_order_conservative` apply of the scipy-transposed matrix uploaded as an ordinary DeviceCSR: the same
    sums over the same columns by the forward kernels -- the yardstick for the column pass.
`python profiles/adjoint_run.py [out.json] [points]`"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse
import xugrid_amd as xa
from xugrid_amd import meshgen
from xugrid_amd import engine as E

out_path = sys.argv[1] if len(sys.argv) > 1 else "adjoint_run.json"
points = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
WARM, REPS = 3, 15
MEAN, FOC = E.METHOD_IDS["mean"], E.METHOD_IDS["first_order_conservative"]


def wall_ms(fn):
    E.dev_sync(); t0 = time.perf_counter(); fn(); E.dev_sync()
    return 1e3 * (time.perf_counter() - t0)


def median_ms(fn):
    for _ in range(WARM):
        fn()
    times = [wall_ms(fn) for _ in range(REPS)]
    return float(np.median(times)), times


def kernels(fn):
    with E.KernelTimer() as timer:
        fn()
    return {k: [int(v[0]), float(v[1])] for k, v in sorted(timer.records.items())}


E.init(0)
sxy, sf = meshgen.triangle_mesh(points, 0)
txy, tf = meshgen.triangle_mesh(points, 1, 30.0, 0.7)
rg = xa.OverlapRegridder(xa.Ugrid2d(sxy[:, 0], sxy[:, 1], -1, sf), xa.Ugrid2d(txy[:, 0], txy[:, 1], -1, tf), method="mean")
W = rg._ensure_device_weights()
data, indices, indptr = W.download()
T, S = W.n, W.m
WT_host = scipy.sparse.csr_matrix((data, indices, indptr), shape=(T, S)).T.tocsr()
WT = E.DeviceCSR.from_arrays(WT_host.data, WT_host.indices, WT_host.indptr, S, T)
col_len = np.diff(WT_host.indptr)
result = {"points": points, "T": int(T), "S": int(S), "nnz": int(W.nnz), "warm_ups": WARM, "repeats": REPS,
          "longest_row": int(np.diff(indptr).max()), "longest_column": int(col_len.max()),
          "columns_over_32": int((col_len > 32).sum()), "runs": []}
rng = np.random.default_rng(0)
first = True
for K in (1, 256):
    v = E.DeviceArray.from_host(rng.normal(size=(K, S)))
    g = E.DeviceArray.from_host(rng.normal(size=(K, T)))
    a = E.DeviceArray((K, S))
    y = E.DeviceArray((K, T))
    adjoint = lambda: W.adjoint_dev(v.ptr, E.XR_F64, g.ptr, K, a.ptr, MEAN)
    forward = lambda: W.apply_dev(v.ptr, E.XR_F64, K, y.ptr, MEAN)
    yardstick = lambda: WT.apply_dev(g.ptr, E.XR_F64, K, a.ptr, FOC)
    row = {"K": K}
    if first:  # the one-off transposition: inside the first adjoint call, and on its own
        row["first_adjoint_call_ms"] = wall_ms(adjoint)
        W.drop_transpose()
        row["transpose_ms"] = wall_ms(lambda: W.transpose())
        W.drop_transpose()
        row["transpose_kernels"] = kernels(lambda: W.transpose())
        first = False
    row["adjoint_ms_median"], row["adjoint_ms_all"] = median_ms(adjoint)
    row["forward_mean_ms_median"], row["forward_mean_ms_all"] = median_ms(forward)
    row["forward_foc_of_transposed_ms_median"], row["forward_foc_of_transposed_ms_all"] = median_ms(yardstick)
    row["adjoint_kernels"] = kernels(adjoint)
    row["forward_mean_kernels"] = kernels(forward)
    row["forward_foc_of_transposed_kernels"] = kernels(yardstick)
    # the same sums by both routes (the yardstick leaves NaN in the columns the adjoint sets to +0.0)
    yardstick(); E.dev_sync(); ref = a.download()
    W.adjoint_dev(0, E.XR_F64, g.ptr, K, a.ptr, FOC); E.dev_sync()
    row["max_abs_difference_adjoint_foc_vs_yardstick"] = float(np.nanmax(np.abs(a.download() - ref)))
    print(json.dumps({k: x for k, x in row.items() if not k.endswith("_all") and not k.endswith("kernels")}), flush=True)
    result["runs"].append(row)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)

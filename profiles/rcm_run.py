"""Ugrid2d.reverse_cuthill_mckee on the device: what the renumbering costs and what it buys downstream.

Cost, on the 1M-face benchmark source mesh (meshgen.triangle_mesh(500 000, 0), qhull numbering) and on a 1000 x 1000 quad
raster, both as grids whose mesh lives in HBM: the first call (face topology + graph build included), a call with the graph
cached (wall clock around the call, which ends synchronised; median of 5), its levels and kernel launches (the engine's
per-kernel hipEvent table, in a run of its own), and scipy.sparse.csgraph.reverse_cuthill_mckee on the same adjacency in this
process (median of 3).  The bandwidth max |i - j| of the adjacency before and after is computed on the host.

Downstream, on the benchmark pair three ways -- both meshes as given, both renumbered, and as given with the source columns of the
weights keyed by Morton (xr_csr_set_col_keys; the apply then gathers the caller's source block into the stored order first,
`expect_permuted` says the caller did): the K = 256 apply of cached weights (2 warm-ups, 10 back-to-back applies between device
synchronisations) and the step of bench.py (both meshes invalidated, weights + mean apply of one variable through
xr_overlap_apply_dev under xr_set_async; 5 warm-ups, 30 steps).  The variants alternate over ROUNDS rounds; every round is kept.
`python profiles/rcm_run.py [out.json] [points per mesh]`"""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import reverse_cuthill_mckee as scipy_rcm
import xugrid_amd as xa
from xugrid_amd import _lib, graph, meshgen
from xugrid_amd import engine as E

out_path = sys.argv[1] if len(sys.argv) > 1 else "rcm_run.json"
points = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
K, ROUNDS = 256, 2
E.init(0)
lib = _lib.load()


def wall_ms(fn):
    E.dev_sync(); t0 = time.perf_counter(); out = fn(); E.dev_sync()
    return 1e3 * (time.perf_counter() - t0), out


def device_grid(xy, faces):
    keep = E.DeviceArray.from_host(np.ascontiguousarray(xy)), E.DeviceArray.from_host(np.ascontiguousarray(faces))
    grid = xa.Ugrid2d.from_device_arrays(*keep)
    grid._keep = keep
    return grid


def bandwidth(indptr, indices, order=None):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    if order is not None:
        new = np.empty(len(order), dtype=np.int64)
        new[order] = np.arange(len(order))
        rows, indices = new[rows], new[indices]
    return int(np.abs(rows - indices).max()) if len(indices) else 0


def renumbering_cost(name, grid):
    first_ms, (_, order) = wall_ms(lambda: grid.reverse_cuthill_mckee(return_device=True))
    cached = [wall_ms(lambda: grid.reverse_cuthill_mckee(return_device=True))[0] for _ in range(5)]
    order_only = [wall_ms(lambda: graph.rcm_dev(grid._graph("face")))[0] for _ in range(5)]
    with E.KernelTimer() as timer:
        graph.rcm_dev(grid._graph("face"))
    rcm_kernels = {k: v for k, v in timer.records.items() if k.startswith("rcm_") or k.startswith("scan_") or k == "fill_i32"}
    indptr, indices, _ = grid._graph("face").download()
    A = csr_matrix((np.ones(len(indices)), indices, indptr), shape=(grid.n_face, grid.n_face))
    scipy_ms, scipy_order = [], None
    for _ in range(3):
        t0 = time.perf_counter(); scipy_order = scipy_rcm(A, symmetric_mode=True); scipy_ms.append(1e3 * (time.perf_counter() - t0))
    order = order.download()
    assert np.array_equal(np.sort(order), np.arange(grid.n_face))
    row = {
        "mesh": name, "n_face": int(grid.n_face), "nnz": int(len(indices)),
        "first_call_ms_with_topology_and_graph": first_ms,
        "cached_graph_call_ms_median": float(np.median(cached)), "cached_graph_call_ms_all": cached,
        "order_only_ms_median": float(np.median(order_only)),
        "levels": int(graph.last_levels), "launches": int(sum(v[0] for v in rcm_kernels.values())),
        "kernel_ms_sum_under_timer": float(sum(v[1] for v in rcm_kernels.values())),
        "kernels_under_timer": {k: [int(v[0]), float(v[1])] for k, v in rcm_kernels.items()},
        "scipy_ms_median": float(np.median(scipy_ms)), "scipy_ms_all": scipy_ms,
        "scipy_over_device_order_only": float(np.median(scipy_ms) / np.median(order_only)),
        "equals_scipy_on_this_machine": bool(np.array_equal(order, scipy_order)),
        "bandwidth_as_given": bandwidth(indptr, indices), "bandwidth_renumbered": bandwidth(indptr, indices, order),
        "bandwidth_scipy": bandwidth(indptr, indices, scipy_order),
    }
    print(json.dumps(row), flush=True)
    return row


def apply_ms(csr, d_src, d_out, reps=10):
    for _ in range(2):
        csr.apply_dev(d_src, E.XR_F64, K, d_out, 0)
    E.dev_sync(); t0 = time.perf_counter()
    for _ in range(reps):
        csr.apply_dev(d_src, E.XR_F64, K, d_out, 0)
    E.dev_sync()
    return 1e3 * (time.perf_counter() - t0) / reps


def step_ms(ms, mt, d_src, d_out, steps=30, warm=5):
    def step():
        ms.invalidate(); mt.invalidate()
        return ms.overlap_apply_dev(mt, d_src, E.XR_F64, 1, d_out, 0)
    E.set_async(True)
    for _ in range(warm):
        step()
    E.dev_sync(); t0 = time.perf_counter()
    for _ in range(steps):
        step()
    E.dev_sync()
    E.set_async(False)
    return 1e3 * (time.perf_counter() - t0) / steps


# Measured once with the variant built, on the same two meshes, and not kept: one 1024-thread block running up to
# 64 consecutive levels per launch while the level has at most 4096 vertices, the four kernels of one level behind every such launch.
ONE_BLOCK_VARIANT_NOT_KEPT = [
    {
        "mesh": "benchmark source, 1M Delaunay faces",
        "levels": 770,
        "launches": 91,
        "order_only_ms_median": 19.36509198276326,
        "cached_graph_call_ms_median": 19.448116014245898,
        "scipy_ms_median": 41.77796799922362
    },
    {
        "mesh": "1000 x 1000 quad raster",
        "levels": 1999,
        "launches": 175,
        "order_only_ms_median": 32.03680401202291,
        "cached_graph_call_ms_median": 32.143678050488234,
        "scipy_ms_median": 26.614193979185075
    }
]
result = {"points_per_mesh": points, "K": K, "rounds": ROUNDS, "one_block_variant_measured_and_not_kept": ONE_BLOCK_VARIANT_NOT_KEPT}
sxy, sf = meshgen.triangle_mesh(points, 0)
txy, tf = meshgen.triangle_mesh(points, 1, 30.0, 0.7)
source, target = device_grid(sxy, sf), device_grid(txy, tf)
raster = device_grid(*meshgen.quad_mesh(np.arange(1001, dtype=np.float64), np.arange(1001, dtype=np.float64)))
result["renumbering"] = [renumbering_cost("benchmark source, 1M Delaunay faces", source),
                         renumbering_cost("1000 x 1000 quad raster", raster)]

S, T = sf.shape[0], tf.shape[0]
d_src, d_out = E.DeviceArray((K, S)), E.DeviceArray((K, T))
block = np.random.default_rng(5).standard_normal((32, S))
for k0 in range(0, K, 32):
    _lib.check(lib.xr_dev_upload(ctypes.c_void_p(d_src.ptr + 8 * k0 * S), block.ctypes.data_as(ctypes.c_void_p), 8 * min(32, K - k0) * S))
pairs = {
    "as given": (source.device_mesh, target.device_mesh),
    "both renumbered": (source.reverse_cuthill_mckee()[0].device_mesh, target.reverse_cuthill_mckee()[0].device_mesh),
}
weights = {name: ms.overlap(mt) for name, (ms, mt) in pairs.items()}
keyed = pairs["as given"][0].overlap(pairs["as given"][1])
keyed.set_col_keys(*E.morton_row_keys(pairs["as given"][0].centroids(), faces_per_tile=8))
weights["as given, Morton column keys"] = keyed
nnz = {name: int(w.nnz) for name, w in weights.items()}
assert len(set(nnz.values())) == 1, nnz  # the same pairs whatever the numbering
table = {name: {"apply_k256_ms": [], "step_ms": []} for name in weights}
table["as given, Morton column keys, source already in stored order"] = {"apply_k256_ms": [], "step_ms": "as 'as given': the keys touch the apply only"}
table["as given, Morton column keys"]["step_ms"] = "as 'as given': the keys touch the apply only"
for _ in range(ROUNDS):
    for name, w in weights.items():
        table[name]["apply_k256_ms"].append(apply_ms(w, d_src.ptr, d_out.ptr))
    keyed.expect_permuted(True)
    table["as given, Morton column keys, source already in stored order"]["apply_k256_ms"].append(apply_ms(keyed, d_src.ptr, d_out.ptr))
    keyed.expect_permuted(False)
    for name, (ms, mt) in pairs.items():
        table[name]["step_ms"].append(step_ms(ms, mt, d_src.ptr, d_out.ptr))
algorithmic_bytes = 12 * nnz["as given"] + 4 * (T + 1) + 8 * K * (S + T)
for name, row in table.items():
    best = min(row["apply_k256_ms"])
    row["apply_k256_frac_of_8TBps_best"] = algorithmic_bytes / (best * 1e-3) / 8e12
result["downstream"] = {"S": S, "T": T, "nnz": nnz["as given"], "algorithmic_bytes_k256": algorithmic_bytes, "table": table}
print(json.dumps(result["downstream"]), flush=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)

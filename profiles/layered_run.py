"""The layered (3-D) weight build on the benchmark's pair: what each pass costs beside the 2-D build it starts from, and how
far each pass is from the bytes it must move.

On the 1M -> 1M Delaunay pair of bench.py (meshgen.triangle_mesh(500 000, 0) -> (500 000, 1, 30 deg, 0.7)) the 2-D overlap
weights are built once on the device; `DeviceCSR.layered` then builds the 3-D matrix from them and from top / bottom arrays
that already live in HBM (device pointers in, a device matrix out; wall clock around calls that end synchronised; 3 warm-ups,
median of 12), for 16 source x 12 target layers on columns that share the extent [0, 1] (every column its own random cuts)
and for 1 x 1.  Per run: the call, its kernels under the engine's per-kernel hipEvent table (in a call of their own), and per
pass the bytes it must move -- the counts, the offsets, the entries written, W and the bounds read once -- over the measured
kernel time, as a share of the 4.85 TB/s the copy kernel of DESIGN section 5 reaches.  The 2-D build of the same process is
timed the same way as the yardstick.
`python profiles/layered_run.py [out.json] [points]`"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import xugrid_amd as xa
from xugrid_amd import meshgen
from xugrid_amd import engine as E

out_path = sys.argv[1] if len(sys.argv) > 1 else "layered_run.json"
points = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
WARM, REPS = 3, 12
COPY_BYTES_PER_MS = 4.85e9  # copy bandwidth (1 GiB read + write)


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


def shared_columns(rng, n_layer, n_col):
    """(top, bottom) float64 (n_layer, n_col), bottom-up, every column cut at its own random heights of [0, 1]"""
    edges = np.concatenate([np.zeros((1, n_col)), np.sort(rng.random((n_layer - 1, n_col)), axis=0), np.ones((1, n_col))])
    return np.ascontiguousarray(edges[1:]), np.ascontiguousarray(edges[:-1])


E.init(0)
sxy, sf = meshgen.triangle_mesh(points, 0)
txy, tf = meshgen.triangle_mesh(points, 1, 30.0, 0.7)
source, target = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
build_2d = lambda: source.overlap(target)
W = build_2d()
T, S, nnz2d = W.n, W.m, W.nnz
result = {"points": points, "T": int(T), "S": int(S), "nnz_2d": int(nnz2d), "warm_ups": WARM, "repeats": REPS,
          "copy_bytes_per_ms": COPY_BYTES_PER_MS, "runs": []}
result["build_2d_ms_median"], result["build_2d_ms_all"] = median_ms(build_2d)
result["build_2d_kernels"] = kernels(build_2d)
print(json.dumps({"build_2d_ms_median": result["build_2d_ms_median"], "nnz_2d": nnz2d}), flush=True)
rng = np.random.default_rng(0)
for n_layer_s, n_layer_t in ((16, 12), (1, 1)):
    bounds = [E.DeviceArray.from_host(a) for a in shared_columns(rng, n_layer_s, S) + shared_columns(rng, n_layer_t, T)]
    build = lambda: W.layered(*bounds)
    W3 = build()
    items, nnz = n_layer_t * nnz2d, W3.nnz
    row = {"n_layer_s": n_layer_s, "n_layer_t": n_layer_t, "items": int(items), "nnz": int(nnz), "rows": int(W3.n),
           "rows_over_32": int(W3.long_rows().size)}
    del W3
    row["layered_ms_median"], row["layered_ms_all"] = median_ms(build)
    row["kernels"] = k = kernels(build)
    bounds_bytes = 16 * (n_layer_s * S + n_layer_t * T)
    must_move = {  # bytes a pass cannot avoid
        "layered_count": 4 * items + 8 * nnz2d + bounds_bytes,          # counts out; ids of W (column, row) and the bounds in
        "scan": 12 * items,                                             # xr_scan.hip: every count read twice, every offset written
        "layered_fill": 4 * items + 16 * nnz2d + bounds_bytes + 12 * nnz,  # offsets, W and the bounds in; the entries out
        "layered_indptr": 8 * (n_layer_t * T) + 4 * T,                  # two offsets per row gathered, the row pointer out
    }
    measured = {"layered_count": k["layered_count"][1], "layered_fill": k["layered_fill"][1],
                "layered_indptr": k["layered_indptr"][1],
                "scan": sum(v[1] for name, v in k.items() if name.startswith("scan_"))}
    row["passes"] = {name: {"ms": measured[name], "must_move_bytes": int(must_move[name]),
                            "floor_ms": must_move[name] / COPY_BYTES_PER_MS,
                            "share_of_copy": must_move[name] / COPY_BYTES_PER_MS / measured[name]} for name in must_move}
    print(json.dumps({x: y for x, y in row.items() if not x.endswith("_all") and x != "kernels"}), flush=True)
    result["runs"].append(row)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)

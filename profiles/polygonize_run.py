"""polygonize at the size of bench.py's mesh: meshgen.triangle_mesh(500 000, 0) (about 1M Delaunay faces), once in qhull's
numbering and once with the faces randomly permuted; the grid and the float64 data live in HBM.  Three inputs:
  a  five classes of a smooth field (few long rings)
  b  three random classes per face (boundary-heavy: most edges are boundaries)
  c  every face its own value (rings = faces: the largest ring table the host step can see)
After one warm-up call per input: REPS calls timed on the wall (each ending in a device synchronise, results copied into
fresh device arrays), then REPS calls under xr_prof for the kernel times per launch name (launches, total ms).  Median of REPS,
every sample kept; label_rounds, the read-backs the call waited for, and the rounds the minimum-label propagation of the face
graph takes on the same grid.  There is no earlier implementation to compare a time against.
`python profiles/polygonize_run.py [points] [out.json]`"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import xugrid_amd as xa
from xugrid_amd import engine, meshgen
from xugrid_amd.polygonize import polygonize_device

n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 500_000
out_path = sys.argv[2] if len(sys.argv) > 2 else "polygonize_run.json"
REPS = 5


def say(*a):
    print(*a, flush=True)


def inputs(xy, faces):
    c = xy[faces].mean(axis=1)
    smooth = meshgen.smooth_field(c, 0)
    edges = np.quantile(smooth, [0.2, 0.4, 0.6, 0.8])
    return {"a_five_smooth_classes": np.digitize(smooth, edges).astype(np.float64),
            "b_three_random_classes": np.random.default_rng(1).integers(0, 3, len(faces)).astype(np.float64),
            "c_every_face_its_own": np.arange(len(faces), dtype=np.float64)}


def measure(label, xy, faces, res, reps=REPS):
    xy_dev, faces_dev = engine.DeviceArray.from_host(xy), engine.DeviceArray.from_host(faces)
    grid = xa.Ugrid2d.from_device_arrays(xy_dev, faces_dev)
    grid.device_topology()  # (built once per grid, outside the timing)
    r = {"n_face": int(len(faces)), "label_propagation_rounds_face_graph": int(grid._graph("face").label_rounds())}
    for name, data in inputs(xy, faces).items():
        data_dev = engine.DeviceArray.from_host(data)
        info, _ = polygonize_device(grid, data_dev)  # warm-up, and the counts
        row = {"n_polygon": info.n_polygon, "n_ring": info.n_ring, "n_halfedge": info.n_halfedge,
               "label_rounds": info.label_rounds, "readbacks": info.readbacks, "wall_ms_samples": [], "kernels_ms_samples": []}
        del info
        for _ in range(reps):
            engine.dev_sync(); t0 = time.perf_counter()
            out = grid.polygonize(data_dev, return_index=True); engine.dev_sync()
            row["wall_ms_samples"].append(1e3 * (time.perf_counter() - t0)); del out
        for _ in range(reps):
            engine.prof_enable(True); engine.prof_reset(); engine.dev_sync()
            out = grid.polygonize(data_dev, return_index=True); engine.dev_sync()
            row["kernels_ms_samples"].append({k: [n, ms] for k, (n, ms) in engine.kernel_times().items()}); engine.prof_enable(False)
            del out
        names = sorted(set().union(*row["kernels_ms_samples"]))
        row["wall_ms_median"] = float(np.median(row["wall_ms_samples"]))
        row["kernels_ms_median"] = {k: float(np.median([s.get(k, [0, 0.0])[1] for s in row["kernels_ms_samples"]])) for k in names}
        row["kernel_launches"] = {k: int(row["kernels_ms_samples"][0].get(k, [0, 0.0])[0]) for k in names}
        row["kernel_ms_total_median"] = float(sum(row["kernels_ms_median"].values()))
        row["largest_kernel"] = max(row["kernels_ms_median"], key=row["kernels_ms_median"].get)
        r[name] = row
        say(label, name, {k: row[k] for k in ("n_polygon", "n_ring", "n_halfedge", "label_rounds", "readbacks", "wall_ms_median",
                                              "kernel_ms_total_median", "largest_kernel")})
    assert grid._host is None, "the device route downloaded the mesh"
    res[label] = r


xy0, f0 = meshgen.triangle_mesh(2000, 0)
measure("warm_up", xy0, f0, {}, reps=1)  # untimed: code objects, pools
xy, faces = meshgen.triangle_mesh(n_points, 0)
res = {"status": "measured", "mesh": f"meshgen.triangle_mesh({n_points}, 0)", "reps": REPS}
for label, f in (("qhull_numbering", faces), ("permuted", faces[np.random.default_rng(5).permutation(len(faces))])):
    measure(label, xy, f, res)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)

"""Meshes from cell geometry on the device, on a 1000 x 1000 rotated, sheared lattice:

* `from_structured_bounds` on its (1000, 1000, 4) corner arrays resident in HBM -> a device grid, beside a vectorised numpy
  restatement of the reference's algorithm (np.lexsort, np.argsort, np.unique(axis=0)) on the same box's CPUs;
* `from_structured` on the lattice's 2-D centres resident in HBM;
* `from_polygons` on the `to_polygons()` of that grid.

After a warm-up on a small lattice every call is timed REPS times with a host clock, each sample between two device
synchronisations, the calls alternating; median, smallest and largest are kept.  Kernel times come from the library's event
table in one run of their own per call (untimed by the host clock) and are summed into the parts of the pipeline: cell pass,
key table, sort (with the passes run and skipped), scans, compaction; fills of status words and of the table are "other".
`python profiles/geometry_run.py [out.json] [--no-host]`; the default output is profiles/geometry_run.json."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

REPS, HOST_REPS = 9, 2
PARTS = {
    "cell_pass": ("bounds_test", "bounds_orient", "bounds_faces", "ring_check", "ring_rows", "ring_faces", "interval_breaks", "lattice",
                  "face_ring_len", "face_ring_coords", "count_up"),
    "key_table": ("merge_insert", "merge_rep"),
    "sort": ("sort_count", "sort_scatter", "unique_key_stats", "unique_key_fold"),
    "scan": ("scan_reduce", "scan_apply", "scan_partials"),
    "compaction": ("unique_compact", "unique_emit", "merge_inverse", "widen_i32"),
}


def say(*a):
    print(*a, flush=True)


def numpy_bounds(xb, yb):
    """The reference's algorithm for (N, M, 4) bounds, vectorised: what a user runs on the host today."""
    import numpy as np

    x, y = xb.reshape(-1, 4), yb.reshape(-1, 4)
    by_xy = np.lexsort((y, x))
    corners = np.stack([np.take_along_axis(x, by_xy, 1), np.take_along_axis(y, by_xy, 1)], axis=-1)
    n_unique = (corners != np.roll(corners, 1, axis=1)).any(axis=-1).sum(axis=1)
    rel = corners - corners[:, :1]
    fan = rel[:, :-1, 0] * rel[:, 1:, 1] - rel[:, :-1, 1] * rel[:, 1:, 0]
    keep = (n_unique >= 3) & (0.5 * np.abs(fan).sum(axis=1) > 0) & np.isfinite(corners.reshape(-1, 8)).all(axis=1)
    corners = corners[keep]
    rel = corners - corners.mean(axis=1)[:, None]
    angle = np.arctan2(rel[..., 1], rel[..., 0])
    angle[:, 1:][angle[:, 1:] == angle[:, :-1]] = np.inf
    corners = np.take_along_axis(corners, np.argsort(angle, axis=1)[..., None], axis=1)
    xy, inverse = np.unique(corners.reshape(-1, 2), return_inverse=True, axis=0)
    faces = np.asarray(inverse).reshape(-1, 4)
    faces[n_unique[keep] == 3, -1] = -1
    return xy, faces, keep


def main():
    import geometry_cases as gc
    import numpy as np
    import xugrid_amd as xa
    from xugrid_amd import engine, geometry

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(HERE, "geometry_run.json")
    with_host = "--no-host" not in sys.argv

    def wall(fn):
        engine.dev_sync(); t0 = time.perf_counter(); fn(); engine.dev_sync()
        return 1e3 * (time.perf_counter() - t0)

    def stats(samples):
        q1, q3 = np.percentile(samples, [25, 75])
        return {"median_ms": float(np.median(samples)), "min_ms": float(min(samples)), "max_ms": float(max(samples)),
                "iqr_ms": float(q3 - q1), "samples_ms": samples}

    def kernels(fn):
        with engine.KernelTimer() as timer:
            fn()
        per_kernel = {k: [int(n), float(ms)] for k, (n, ms) in timer.records.items()}
        parts = {part: float(sum(ms for k, (_, ms) in per_kernel.items() if k in names)) for part, names in PARTS.items()}
        parts["other"] = float(sum(ms for k, (_, ms) in per_kernel.items() if not any(k in names for names in PARTS.values())))
        return int(sum(n for n, _ in per_kernel.values())), per_kernel, parts

    def measure(label, n, res, reps, host_reps):
        xb, yb = gc.lattice_bounds(n, n, seed=11)
        cx, cy = gc.centres(n, n)
        d_xb, d_yb, d_cx, d_cy = (engine.DeviceArray.from_host(a) for a in (xb, yb, cx, cy))
        grid = xa.Ugrid2d.from_structured_bounds(d_xb, d_yb)
        polygons = grid.to_polygons()
        counts = geometry.bounds_mesh(d_xb, d_yb)[2]
        routes = {
            "from_structured_bounds_3d": lambda: xa.Ugrid2d.from_structured_bounds(d_xb, d_yb),
            "from_structured_2d_centres": lambda: xa.Ugrid2d.from_structured(d_cx, d_cy),
            "to_polygons": lambda: grid.to_polygons(),
            "from_polygons": lambda: xa.Ugrid2d.from_polygons(polygons),
        }
        for fn in routes.values():
            fn()
        samples = {name: [] for name in routes}
        for _ in range(reps):  # (the calls alternate: drift of the box hits all of them alike)
            for name, fn in routes.items():
                samples[name].append(wall(fn))
        r = {"cells": int(n * n), "n_face": int(grid.n_face), "n_node": int(grid.n_node), "corner_rows": int(4 * grid.n_face),
             "sort_digit_bits": 8, "sort_passes_run": counts[2], "sort_passes_skipped": counts[3], "calls": {}}
        for name, fn in routes.items():
            row = stats(samples[name])
            n_launch, per_kernel, parts = kernels(fn)
            row.update(launches=n_launch, kernel_ms=per_kernel, kernel_ms_by_part=parts, kernel_ms_total=float(sum(parts.values())))
            r["calls"][name] = row
            say(label, name, "device", row["median_ms"], "ms wall;", row["kernel_ms_total"], "ms in", n_launch, "kernels;", parts)
        if host_reps:
            r["calls"]["from_structured_bounds_3d"]["host_numpy"] = stats([wall(lambda: numpy_bounds(xb, yb)) for _ in range(host_reps)])
            say(label, "numpy restatement of the bounds rule", r["calls"]["from_structured_bounds_3d"]["host_numpy"]["median_ms"], "ms")
            xy, faces, keep = numpy_bounds(xb, yb)
            got_xy, got_faces = grid.device_mesh.download()
            r["equals_numpy"] = bool(np.array_equal(got_xy, xy) and np.array_equal(got_faces, faces) and keep.all())
            say(label, "device grid equals the numpy restatement:", r["equals_numpy"])
        res[label] = r

    res = {"reps": REPS, "host_reps": HOST_REPS if with_host else 0}
    measure("warm_up", 40, {}, 2, 0)  # untimed: code objects, pools
    measure("lattice_1000x1000", 1000, res, REPS, HOST_REPS if with_host else 0)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()

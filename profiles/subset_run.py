"""Sub-meshes cut on the device: `topology_subset`, `clip_box` and `topology_subset(return_index=True)` on the
bench's 1M-face Delaunay mesh (meshgen.triangle_mesh(500 000, 0)), the grid resident in HBM and the index a device array.
Selections: a box of about a quarter of the faces (as an index), every other face, one Morton block of an eighth (in Morton
order: an unsorted index), the full random permutation, `clip_box` of the quarter box, and the quarter with `return_index=True`
-- the grid's topology cache is dropped before every sample of that one, so it includes the topology build.

After a warm-up every call is timed REPS times with a host clock, each sample between two device synchronisations; median,
smallest and largest are kept.  Beside them the numpy restatement on the host (tests/subset_cases.py; HOST_REPS samples).  Per
call also: the kernel launches (the library's own count, one untimed call under its kernel timer), the synchronising
read-backs (counted from the code: one per cut, one per index made from flags, four per topology build) and the bytes the
call MUST move, computed from the shapes -- the index, the selected rows of the face table in and out, the kept coordinates in
and out, the node index out -- over the measured time, as a share of the HBM peak of 8.0 TB/s.  These calls are bound by their
launches and read-backs, not by that traffic; the share says how far.
`python profiles/subset_run.py [out.json] [--no-host]`; the default output is profiles/subset_run.json."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

REPS, HOST_REPS = 15, 2
HBM_PEAK = 8.0e12  # bytes / s, MI355X specification


def say(*a):
    print(*a, flush=True)


def morton_order(c):
    """Order of the points ``c`` along the Z curve of a 1024 x 1024 grid over their bounds."""
    import numpy as np

    lo, hi = c.min(axis=0), c.max(axis=0)
    q = np.minimum(((c - lo) / (hi - lo) * 1024).astype(np.int64), 1023)
    key = np.zeros(len(c), dtype=np.int64)
    for b in range(10):
        key |= ((q[:, 0] >> b) & 1) << (2 * b) | ((q[:, 1] >> b) & 1) << (2 * b + 1)
    return np.argsort(key, kind="stable")


def main():
    import numpy as np
    import subset_cases as sc
    import xugrid_amd as xa
    from xugrid_amd import engine

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(HERE, "subset_run.json")
    with_host = "--no-host" not in sys.argv

    def wall(fn):
        engine.dev_sync(); t0 = time.perf_counter(); fn(); engine.dev_sync()
        return 1e3 * (time.perf_counter() - t0)

    def stats(samples):
        q1, q3 = np.percentile(samples, [25, 75])
        return {"median_ms": float(np.median(samples)), "min_ms": float(min(samples)), "max_ms": float(max(samples)),
                "iqr_ms": float(q3 - q1), "samples_ms": samples}

    def launches(fn):
        with engine.KernelTimer() as timer:
            fn()
        return int(sum(n for n, _ in timer.records.values()))

    def measure(label, xy, faces, res, reps, host_reps):
        xy_dev, faces_dev = engine.DeviceArray.from_host(xy), engine.DeviceArray.from_host(faces)
        grid = xa.Ugrid2d.from_device_arrays(xy_dev, faces_dev)
        c = grid.centroids
        F, m = faces.shape
        (x0, x1), (y0, y1) = np.percentile(c[:, 0], [25, 75]), np.percentile(c[:, 1], [25, 75])
        box = (float(x0), float(y0), float(x1), float(y1))
        quarter = sc.box_faces(c, *box)
        rng = np.random.default_rng(0)
        index = {"box_quarter": quarter, "every_other_face": np.arange(0, F, 2), "morton_eighth": morton_order(c)[: F // 8],
                 "full_permutation": rng.permutation(F)}
        index_dev = {k: engine.DeviceArray.from_host(v.astype(np.int64)) for k, v in index.items()}

        def with_index():
            grid.__dict__.pop("_topology_cache", None)  # (the topology build is part of this one)
            return grid.topology_subset(index_dev["box_quarter"], return_index=True)

        routes = {k: (lambda k=k: grid.topology_subset(index_dev[k])) for k in index}
        routes["clip_box_quarter"] = lambda: grid.clip_box(*box)
        routes["box_quarter_return_index"] = with_index
        selected = dict(index, clip_box_quarter=quarter, box_quarter_return_index=quarter)
        # one cut: the status words; clip_box: + the length of the box index; return_index: + four of the topology build, + the
        # length of the edge index
        readbacks = {k: 1 for k in index}
        readbacks.update(clip_box_quarter=2, box_quarter_return_index=6)
        for fn in routes.values():
            fn()
        samples = {name: [] for name in routes}
        for _ in range(reps):  # (the calls alternate: drift of the box hits all of them alike)
            for name, fn in routes.items():
                samples[name].append(wall(fn))
        r = {"n_face": int(F), "n_node": int(len(xy)), "calls": {}}
        for name, fn in routes.items():
            ids = selected[name]
            n_kept = int(np.unique(faces[ids]).size)
            need = 8 * len(ids) + 2 * 4 * len(ids) * m + 2 * 16 * n_kept + 4 * n_kept
            row = stats(samples[name])
            row.update(n_selected=int(len(ids)), n_node_kept=n_kept, launches=launches(fn), readbacks=readbacks[name],
                       necessary_bytes=int(need))
            row["necessary_bytes_over_time_as_share_of_hbm_peak_8.0TBps"] = need / (row["median_ms"] * 1e-3) / HBM_PEAK
            r["calls"][name] = row
        if host_reps:
            host = {k: (lambda k=k: sc.topology_subset(xy, faces, index[k])) for k in index}
            host["clip_box_quarter"] = lambda: sc.topology_subset(xy, faces, sc.box_faces(c, *box))
            host["box_quarter_return_index"] = lambda: (sc.topology_subset(xy, faces, quarter), sc.edge_index(faces, quarter))
            for name, fn in host.items():
                r["calls"][name]["host_numpy"] = stats([wall(fn) for _ in range(host_reps)])
        for name, row in r["calls"].items():
            say(label, name, "device", row["median_ms"], "ms, launches", row["launches"], "read-backs", row["readbacks"], "host",
                row.get("host_numpy", {}).get("median_ms"))
        res[label] = r

    res = {"reps": REPS, "host_reps": HOST_REPS if with_host else 0}
    xy0, f0 = xa.meshgen.triangle_mesh(2000, 0)
    measure("warm_up", xy0, f0, {}, 2, 0)  # untimed: code objects, pools
    xy, faces = xa.meshgen.triangle_mesh(500_000, 0)
    measure("delaunay_1m", xy, faces, res, REPS, HOST_REPS if with_host else 0)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()

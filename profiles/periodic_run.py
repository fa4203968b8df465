"""Periodic meshes converted on the device: `to_periodic` and `to_nonperiodic`, each with and without
`return_index`, on a 1000 x 1000 quad mesh (meshgen.quad_mesh: 1 002 001 nodes, 1 000 000 faces; the bench's Delaunay mesh has
no matching boundaries) resident in HBM.  `to_nonperiodic` runs on the periodic grid `to_periodic` made.

After a warm-up every call is timed REPS times with a host clock, each sample between two device synchronisations, the calls
alternating; median, smallest and largest are kept.  Beside them the numpy restatement on the host (tests/periodic_cases.py;
HOST_REPS samples; without the edge arithmetic for the calls without `return_index`).  Per call also: the kernel launches (the
library's own count, one untimed call under its kernel timer), the synchronising read-backs (counted from the code) and the
bytes the call MUST move, computed from the shapes, over the measured time as a share of the HBM peak of 8.0 TB/s.  The kernel
timer's per-kernel milliseconds of one call are kept too: they say which kernel the time belongs to.
`python profiles/periodic_run.py [out.json] [--no-host]`; the default output is profiles/periodic_run.json."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

REPS, HOST_REPS = 15, 1
HBM_PEAK = 8.0e12  # bytes / s, MI355X specification


def say(*a):
    print(*a, flush=True)


def main():
    import numpy as np
    import periodic_cases as pc
    import xugrid_amd as xa
    from xugrid_amd import engine

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(HERE, "periodic_run.json")
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
        return int(sum(n for n, _ in timer.records.values())), {k: [int(n), float(ms)] for k, (n, ms) in timer.records.items()}

    def measure(label, n, res, reps, host_reps):
        xy, faces = xa.meshgen.quad_mesh(np.arange(n + 1.0), np.arange(n + 1.0))
        xmax = float(n)
        grid = xa.Ugrid2d.from_device_arrays(engine.DeviceArray.from_host(xy), engine.DeviceArray.from_host(faces))
        grid.device_topology()  # (the grid keeps its topology: a caller who works on its edges has it)
        periodic = grid.to_periodic()
        periodic.device_topology()
        routes = {
            "to_periodic": lambda: grid.to_periodic(),
            "to_periodic_return_index": lambda: grid.to_periodic(return_index=True),
            "to_nonperiodic": lambda: periodic.to_nonperiodic(xmax),
            "to_nonperiodic_return_index": lambda: periodic.to_nonperiodic(xmax, return_index=True),
        }
        # to_periodic: the bounds, the boundary counts, the boundary y, the kept count; to_nonperiodic: the bounds, the new-node
        # count; return_index: + the edge misses + four of the new grid's topology build
        readbacks = {"to_periodic": 4, "to_periodic_return_index": 9, "to_nonperiodic": 2, "to_nonperiodic_return_index": 7}
        N, F, m, E = grid.n_node, grid.n_face, faces.shape[1], grid.n_edge
        Np, Ep = periodic.n_node, periodic.n_edge
        # coordinates read and written once, the face table read and written once; return_index: + the three int64 indexes and
        # both edge tables read once
        need = {"to_periodic": 16 * N + 16 * Np + 2 * 4 * m * F, "to_nonperiodic": 16 * Np + 16 * N + 2 * 4 * m * F}
        need["to_periodic_return_index"] = need["to_periodic"] + 8 * (Np + F + Ep) + 8 * (E + Ep)
        need["to_nonperiodic_return_index"] = need["to_nonperiodic"] + 8 * (N + F + E) + 8 * (E + Ep)
        for fn in routes.values():
            fn()
        samples = {name: [] for name in routes}
        for _ in range(reps):  # (the calls alternate: drift of the box hits all of them alike)
            for name, fn in routes.items():
                samples[name].append(wall(fn))
        r = {"n_face": int(F), "n_node": int(N), "n_edge": int(E), "periodic_nodes": int(Np), "periodic_edges": int(Ep), "calls": {}}
        for name, fn in routes.items():
            row = stats(samples[name])
            n_launch, per_kernel = kernels(fn)
            row.update(launches=n_launch, readbacks=readbacks[name], necessary_bytes=int(need[name]), kernel_ms=per_kernel)
            row["necessary_bytes_over_time_as_share_of_hbm_peak_8.0TBps"] = need[name] / (row["median_ms"] * 1e-3) / HBM_PEAK
            r["calls"][name] = row
        if host_reps:
            p_xy, p_faces = np.asarray(periodic.node_coordinates), np.asarray(periodic.face_node_connectivity)
            host = {"to_periodic": lambda: pc.to_periodic(xy, faces, edges=False),
                    "to_periodic_return_index": lambda: pc.to_periodic(xy, faces),
                    "to_nonperiodic": lambda: pc.to_nonperiodic(p_xy, p_faces, xmax, edges=False),
                    "to_nonperiodic_return_index": lambda: pc.to_nonperiodic(p_xy, p_faces, xmax)}
            for name, fn in host.items():
                r["calls"][name]["host_numpy"] = stats([wall(fn) for _ in range(host_reps)])
        for name, row in r["calls"].items():
            say(label, name, "device", row["median_ms"], "ms, launches", row["launches"], "read-backs", row["readbacks"], "host",
                row.get("host_numpy", {}).get("median_ms"))
        res[label] = r

    res = {"reps": REPS, "host_reps": HOST_REPS if with_host else 0}
    measure("warm_up", 40, {}, 2, 0)  # untimed: code objects, pools
    measure("quads_1000x1000", 1000, res, REPS, HOST_REPS if with_host else 0)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()

"""Meshes joined and matched on the device: `merge_partitions` with and without `return_index`,
`labels_to_indices` and `reindex_like` on faces, on the bench's 1M-face Delaunay mesh (meshgen.triangle_mesh(500 000, 0)) cut
into eight Morton blocks with a one-face halo (the faces touching a node of the block), each cut by `topology_subset` on the
device; grids, labels, coordinates and data resident in HBM.

After a warm-up every call is timed REPS times with a host clock, each sample between two device synchronisations, the calls
alternating; median, smallest and largest are kept.  Beside them the numpy restatement on the host (tests/partition_cases.py;
HOST_REPS samples).  Per call also: the kernel launches (the library's own count, one untimed call under its kernel timer), the
synchronising read-backs (counted from the code) and the bytes the call MUST move, computed from the shapes, over the measured
time as a share of the HBM peak of 8.0 TB/s.  The kernel timer's per-kernel milliseconds of one merge are kept too: they say
which kernel the time belongs to.
`python profiles/merge_run.py [out.json] [--no-host]`; the default output is profiles/merge_run.json."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

REPS, HOST_REPS, N_BLOCK = 15, 1, 8
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
    import partition_cases as pc
    import xugrid_amd as xa
    from xugrid_amd import engine, sample

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(HERE, "merge_run.json")
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

    def measure(label, xy, faces, res, reps, host_reps):
        grid = xa.Ugrid2d.from_device_arrays(engine.DeviceArray.from_host(xy), engine.DeviceArray.from_host(faces))
        c = grid.centroids
        F, m = faces.shape
        order = morton_order(c)
        labels = np.empty(F, dtype=np.int64)
        labels[order] = np.minimum(np.arange(F) * N_BLOCK // F, N_BLOCK - 1)
        blocks = []
        for l in range(N_BLOCK):  # the block and the faces that touch one of its nodes
            flag = np.zeros(len(xy), dtype=bool)
            flag[faces[labels == l].ravel()] = True
            blocks.append(np.nonzero(flag[faces].any(axis=1))[0])
        parts = [grid.topology_subset(engine.DeviceArray.from_host(ids.astype(np.int64))) for ids in blocks]
        host_parts = [(np.asarray(p.node_coordinates), np.asarray(p.face_node_connectivity)) for p in parts] if host_reps else None
        for p in parts:
            p.device_topology()  # (the partitions keep their topologies: a caller who works on the parts has them)
        labels_dev = engine.DeviceArray.from_host(labels)
        merged = xa.merge_partitions(parts)
        data_dev = engine.DeviceArray.from_host(np.arange(merged.n_face, dtype=np.float64))
        c_merged, c_whole = engine.DeviceArray.from_host(merged.centroids), engine.DeviceArray.from_host(c)

        def like_resident():
            index = xa.connectivity.index_like_device(c_merged, c_whole)
            return sample.gather_points(data_dev, merged.n_face, index)

        routes = {
            "merge_partitions": lambda: xa.merge_partitions(parts),
            "merge_partitions_return_index": lambda: xa.merge_partitions(parts, return_index=True),
            "labels_to_indices": lambda: xa.labels_to_indices(labels_dev),
            "reindex_like_faces_coordinates_resident": like_resident,
            "reindex_like_faces_as_called": lambda: merged.reindex_like(grid, data_dev),
        }
        # merge: the boundary words; return_index: + the edge boundaries + four of the merged grid's topology build; labels: the
        # range, the boundaries; index_like: the two problem counts
        readbacks = {"merge_partitions": 1, "merge_partitions_return_index": 6, "labels_to_indices": 2,
                     "reindex_like_faces_coordinates_resident": 1, "reindex_like_faces_as_called": 1}
        N, Fc = sum(p.n_node for p in parts), sum(p.n_face for p in parts)
        Nn, Fn, En = merged.n_node, merged.n_face, merged.n_edge
        grid_bytes = 16 * N + 16 * Nn + 4 * m * Fc + 4 * m * Fn
        need = {"merge_partitions": grid_bytes, "merge_partitions_return_index": grid_bytes + 8 * (Nn + Fn + 2 * En) + 8 * sum(p.n_edge for p in parts),
                "labels_to_indices": 16 * F, "reindex_like_faces_coordinates_resident": 2 * 16 * Fn + 3 * 8 * Fn,
                "reindex_like_faces_as_called": 2 * 16 * Fn + 3 * 8 * Fn}
        for fn in routes.values():
            fn()
        samples = {name: [] for name in routes}
        for _ in range(reps):  # (the calls alternate: drift of the box hits all of them alike)
            for name, fn in routes.items():
                samples[name].append(wall(fn))
        r = {"n_face": int(F), "n_node": int(len(xy)), "n_block": N_BLOCK, "concatenated_nodes": int(N), "concatenated_faces": int(Fc),
             "merged_nodes": int(Nn), "merged_faces": int(Fn), "merged_edges": int(En), "calls": {}}
        for name, fn in routes.items():
            row = stats(samples[name])
            n_launch, per_kernel = kernels(fn)
            row.update(launches=n_launch, readbacks=readbacks[name], necessary_bytes=int(need[name]), kernel_ms=per_kernel)
            row["necessary_bytes_over_time_as_share_of_hbm_peak_8.0TBps"] = need[name] / (row["median_ms"] * 1e-3) / HBM_PEAK
            r["calls"][name] = row
        if host_reps:
            def host_grid():
                _, _, inverse = pc.merge_nodes(host_parts)
                return pc.merge_rows(pc.widened_faces(host_parts, inverse), np.cumsum([0] + [len(f) for _, f in host_parts]))

            c_m = merged.centroids
            host = {"merge_partitions": host_grid, "merge_partitions_return_index": lambda: pc.merge(host_parts),
                    "labels_to_indices": lambda: pc.labels_to_indices(labels),
                    "reindex_like_faces_coordinates_resident": lambda: pc.index_like(c_m, c, 0.0)}
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

"""Meshes derived on the device: `triangulate`, the default centroidal and circumcenter tessellations and
`centroid_triangulation` on the bench's 1M-face Delaunay mesh (meshgen.triangle_mesh(500 000, 0)) and on a 1M-face mixed mesh
(meshgen.mixed_mesh(660 000, 0)), grids resident in HBM.  After a warm-up every call is timed REPS times, each sample ending in
a device synchronise; median, smallest and largest are kept.  Beside them the host numpy route to the same results on the same
box (the restatements of tests/derive_cases.py and voronoi.voronoi_topology on the downloaded arrays; HOST_REPS samples).

Two comparisons say that nothing existing got slower:
  * `voronoi_topology_device(grid)` with its defaults (True, True, True) on the Delaunay mesh, this tree against a checkout
    of the parent commit built in PARENT (`--parent PARENT`): two child processes, one per tree, each with the mesh in HBM,
    take turns sample by sample at this process's word, AB_REPS samples each.  The margin is the run-to-run spread of that
    call: the larger of the two versions' interquartile ranges.
  * the default-flag tessellation (True, True, False) against that (True, True, True) call, alternating in this process: it
    does strictly less host work.
`python profiles/derive_run.py [out.json] [--parent PARENT] [--no-host]`; the default output is profiles/derive_run.json."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = "--child" in sys.argv
TREE = sys.argv[sys.argv.index("--child") + 1] if CHILD else os.path.dirname(HERE)
sys.path.insert(0, TREE)  # (a child measures the tree it is given, with this file's code)
sys.path.insert(0, os.path.join(TREE, "tests"))

REPS, HOST_REPS, AB_REPS = 9, 2, 15


def say(*a):
    print(*a, flush=True)


def child():
    """One version of voronoi_topology_device (True, True, True) on the Delaunay mesh: a sample per line of stdin."""
    import xugrid_amd as xa
    from xugrid_amd import engine, voronoi

    xy, faces = xa.meshgen.triangle_mesh(500_000, 0)
    xy_dev, faces_dev = engine.DeviceArray.from_host(xy), engine.DeviceArray.from_host(faces)
    grid = xa.Ugrid2d.from_device_arrays(xy_dev, faces_dev)
    for _ in range(3):
        voronoi.voronoi_topology_device(grid)
    say("ready")
    for line in sys.stdin:
        if line.strip() != "go":
            break
        engine.dev_sync(); t0 = time.perf_counter(); voronoi.voronoi_topology_device(grid); engine.dev_sync()
        say(1e3 * (time.perf_counter() - t0))


def alternate(parent_tree):
    """-> samples of the two versions, taken in turns."""
    import numpy as np

    procs = {}
    for name, tree in (("this_tree", os.path.dirname(HERE)), ("parent", os.path.abspath(parent_tree))):
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", tree], stdin=subprocess.PIPE,
                                       stdout=subprocess.PIPE, text=True, bufsize=1)
    samples = {name: [] for name in procs}
    try:
        for name, p in procs.items():
            line = p.stdout.readline().strip()
            if line != "ready":
                raise RuntimeError(f"{name}: child said {line!r}")
        for _ in range(AB_REPS):
            for name, p in procs.items():
                p.stdin.write("go\n"); p.stdin.flush()
                samples[name].append(float(p.stdout.readline()))
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=60)
    r = {}
    for name, v in samples.items():
        q1, q3 = np.percentile(v, [25, 75])
        r[name] = {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "iqr_ms": float(q3 - q1), "samples_ms": v}
    r["difference_ms"] = r["this_tree"]["median_ms"] - r["parent"]["median_ms"]
    r["margin_ms"] = max(r["this_tree"]["iqr_ms"], r["parent"]["iqr_ms"])
    r["slower_than_parent"] = bool(r["difference_ms"] > r["margin_ms"])
    return r


def main():
    import numpy as np
    import xugrid_amd as xa
    from xugrid_amd import engine, voronoi
    import derive_cases as dc

    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--parent"]
    out_path = args[0] if args else os.path.join(HERE, "derive_run.json")
    with_host = "--no-host" not in sys.argv
    parent_tree = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None

    def wall(fn):
        engine.dev_sync(); t0 = time.perf_counter(); fn(); engine.dev_sync()
        return 1e3 * (time.perf_counter() - t0)

    def stats(samples):
        q1, q3 = np.percentile(samples, [25, 75])
        return {"median_ms": float(np.median(samples)), "min_ms": float(min(samples)), "max_ms": float(max(samples)),
                "iqr_ms": float(q3 - q1), "samples_ms": samples}

    def measure(label, xy, faces, res, reps, host_reps):
        xy_dev, faces_dev = engine.DeviceArray.from_host(xy), engine.DeviceArray.from_host(faces)
        grid = xa.Ugrid2d.from_device_arrays(xy_dev, faces_dev)
        triangles_only = faces.shape[1] == 3

        def centroid_triangulation():
            # (the property is cached on the grid; only ITS cache is dropped -- drop_device_caches() would also throw away the
            # mesh's prepared arrays, which are not part of what is timed here)
            grid.__dict__.pop("_derive_cache", None)
            return grid.centroid_triangulation

        routes = {"voronoi_topology_device_TTT": lambda: voronoi.voronoi_topology_device(grid),
                  "tessellation_centroidal_TTF": lambda: grid.tesselate_centroidal_voronoi(),
                  "triangulate": lambda: grid.triangulate(return_index=True)}
        if triangles_only:
            routes["tessellation_circumcenter_TTF"] = lambda: grid.tesselate_circumcenter_voronoi()
        routes["centroid_triangulation"] = centroid_triangulation
        for fn in routes.values():
            fn()
        samples = {name: [] for name in routes}
        for _ in range(reps):  # (the versions alternate: drift of the box hits all of them alike)
            for name, fn in routes.items():
                samples[name].append(wall(fn))
        r = {"n_face": int(len(faces)), "n_node": int(len(xy)), "device": {k: stats(v) for k, v in samples.items()}}
        if host_reps:
            centroids = grid.centroids
            x, y = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
            host = {"triangulate": lambda: dc.triangulate_dense(faces),
                    "tessellation_centroidal_TTF": lambda: dc.host_tessellation(xy, faces, centroids, (True, True, False))}
            if triangles_only:
                host["tessellation_circumcenter_TTF"] = lambda: dc.host_tessellation(xy, faces, dc.circumcenters(faces, x, y),
                                                                                     (True, True, False))
            host["centroid_triangulation"] = lambda: dc.triangulate_dense(dc.host_tessellation(xy, faces, centroids, (True, False, False))[1])
            r["host_numpy"] = {name: stats([wall(fn) for _ in range(host_reps)]) for name, fn in host.items()}
        a, b = r["device"]["voronoi_topology_device_TTT"], r["device"]["tessellation_centroidal_TTF"]
        r["default_flags_against_TTT"] = {"difference_ms": b["median_ms"] - a["median_ms"], "margin_ms": max(a["iqr_ms"], b["iqr_ms"]),
                                          "slower": bool(b["median_ms"] - a["median_ms"] > max(a["iqr_ms"], b["iqr_ms"]))}
        for name in routes:
            say(label, name, "device", r["device"][name]["median_ms"], "host", r.get("host_numpy", {}).get(name, {}).get("median_ms"))
        res[label] = r

    res = {"reps": REPS, "host_reps": HOST_REPS if with_host else 0, "ab_reps": AB_REPS}
    if parent_tree:  # (first: this process has not opened the device yet, the two children have it to themselves)
        res["TTT_against_parent_delaunay_1m"] = alternate(parent_tree)
        say("against parent", {k: v for k, v in res["TTT_against_parent_delaunay_1m"].items() if not isinstance(v, dict)},
            res["TTT_against_parent_delaunay_1m"]["this_tree"]["median_ms"], res["TTT_against_parent_delaunay_1m"]["parent"]["median_ms"])
    xy0, f0 = xa.meshgen.triangle_mesh(2000, 0)
    measure("warm_up", xy0, f0, {}, 2, 0)  # untimed: code objects, pools
    for label, (xy, faces) in (("delaunay_1m", xa.meshgen.triangle_mesh(500_000, 0)), ("mixed_1m", xa.meshgen.mixed_mesh(660_000, 0))):
        measure(label, xy, faces, res, REPS, HOST_REPS if with_host else 0)
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        json.dump(res, open(out_path, "w"), indent=1)
    say("default flags against (T,T,T):", res["delaunay_1m"]["default_flags_against_TTT"])


if __name__ == "__main__":
    child() if CHILD else main()

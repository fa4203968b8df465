"""The device topology at the benchmark's size (1M Delaunay triangles, once in qhull's numbering and once with the faces
randomly permuted): per-kernel times of xr_topology_create and xr_graph_from_topology (xr_prof: hipEvents per launch, one
warm-up build, median of 5), and the wall time of the FIRST laplace_interpolate, interpolate_na(dim="edge") and
connected_components on a fresh DeviceUgrid2d -- against the same three calls through the host route (the route every device
grid took before the topology existed and a non-manifold grid still takes: download the mesh, numpy / scipy, upload), forced
here by withholding the topology; the parent commit itself is not run).  First calls cannot be repeated on one grid: each
is taken on 3 fresh grids, the two routes alternating, after one untimed pass on a small mesh that loads the code objects;
median, with every sample kept.  Wall times end in a device synchronise.
`python profiles/topology_run.py [points] [out.json]`"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch initialises its HIP runtime before the engine binds the device
import xugrid_amd as xa
from xugrid_amd import engine
from xugrid_amd.topology import DeviceTopology
from xugrid_amd.ugrid2d import DeviceUgrid2d

n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 500_000
out_path = sys.argv[2] if len(sys.argv) > 2 else "topology_run.json"
REPS = 3


def say(*a):
    print(*a, flush=True)


class HostRouteGrid(DeviceUgrid2d):
    def _fill_topology(self):
        return None


def kernel_table(fn, reps=5):
    """-> ({kernel: median ms over the builds, 0 where a build did not launch it}, median wall ms of fn)."""
    fn()
    rows, wall = [], []
    for _ in range(reps):
        engine.prof_enable(True); engine.prof_reset(); engine.dev_sync()
        t0 = time.perf_counter(); fn(); engine.dev_sync(); wall.append(1e3 * (time.perf_counter() - t0))
        rows.append({k: ms for k, (_, ms) in engine.kernel_times().items()}); engine.prof_enable(False)
    names = sorted(set().union(*rows))
    table = {k: float(np.median([r.get(k, 0.0) for r in rows])) for k in names}
    table["total_ms"] = float(sum(table.values()))
    return table, float(np.median(wall))


CALLS = (("laplace_interpolate", lambda g, t_face, t_edge: g.laplace_interpolate(t_face)),
         ("interpolate_na_edge", lambda g, t_face, t_edge: g.interpolate_na(t_edge, dim="edge")),
         ("connected_components", lambda g, t_face, t_edge: g.connected_components()))


def first_calls(xy, f, c, e, reps=REPS):
    """-> {route: {call: [ms per fresh grid]}}, label rounds of the face graph."""
    data = np.sin(3 * c[:, 0]) + c[:, 1]
    data[np.hypot(c[:, 0] - 0.5, c[:, 1] - 0.5) < 0.126] = np.nan
    edge = np.cos(4 * e[:, 0]) - e[:, 1]
    edge[np.random.default_rng(1).random(edge.size) < 0.05] = np.nan
    t_face, t_edge = torch.tensor(data, device="cuda"), torch.tensor(edge, device="cuda")
    xy_t, f_t = torch.tensor(xy, device="cuda"), torch.tensor(f, device="cuda")
    out = {route: {name: [] for name, _ in CALLS} for route in ("device", "host")}
    rounds = None
    for _ in range(reps):
        for name, call in CALLS:
            for route, cls in (("device", DeviceUgrid2d), ("host", HostRouteGrid)):
                grid = cls(xy_t, f_t)
                torch.cuda.synchronize(); engine.dev_sync()
                t0 = time.perf_counter(); call(grid, t_face, t_edge); torch.cuda.synchronize(); engine.dev_sync()
                out[route][name].append(1e3 * (time.perf_counter() - t0))
                if route == "device":
                    assert grid._host is None, "the device route downloaded the mesh"
                    if name == "connected_components":
                        rounds = int(grid._graph("face").label_rounds())
    return out, rounds


def small_host(points):
    xy, f = xa.meshgen.triangle_mesh(points, 0)
    g = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, f)
    return xy, f, g.centroids, g.edge_coordinates


first_calls(*small_host(2000), reps=1)  # untimed: code objects, pools, torch
say("warm-up pass done")
xy, faces = xa.meshgen.triangle_mesh(n_points, 0)
res = {"n_face": int(len(faces)), "n_node": int(len(xy)), "first_call_samples_per_route": REPS,
       "host_route_is": "this commit with the topology withheld (DeviceUgrid2d._fill_topology -> None): the download / numpy / "
                        "scipy / upload route of the parent commit, not a run of the parent commit itself"}
for label, f in (("qhull_numbering", faces), ("permuted", faces[np.random.default_rng(5).permutation(len(faces))])):
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, f)
    c, e = host.centroids, host.edge_coordinates
    mesh = host.device_mesh
    holder = {}
    r = {}
    r["topology_create_kernels_ms"], r["topology_create_wall_ms"] = kernel_table(lambda: holder.__setitem__("t", DeviceTopology(mesh)))
    topology = holder["t"]
    r["graph_from_topology_face_kernels_ms"], r["graph_from_topology_face_wall_ms"] = kernel_table(lambda: topology.graph("face"))
    r["n_edge"], r["n_long_nodes"] = int(topology.n_edge), int(topology.n_long_nodes)
    say(label, "kernel tables done")
    samples, rounds = first_calls(xy, f, c, e)
    med = {route: {k: float(np.median(v)) for k, v in samples[route].items()} for route in samples}
    r["first_call_wall_ms_device_route"] = med["device"]
    r["first_call_wall_ms_host_route"] = med["host"]
    r["first_call_wall_ms_samples"] = samples
    r["host_over_device"] = {k: med["host"][k] / med["device"][k] for k in med["device"]}
    r["label_rounds_face_graph"] = rounds
    res[label] = r
    say(label, "first calls done")
    del holder, topology, host, mesh
say(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)

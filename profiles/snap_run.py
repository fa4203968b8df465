"""Snapping on the device on the bench's 1M-face Delaunay mesh (meshgen.triangle_mesh(500 000, 0)):
`snap_nodes` on the mesh's nodes, each repeated at a jitter of a hundredth of the mean edge length, with a distance of a
twentieth of the mean edge length ("narrow": the pairs of twins) and of one mean edge length ("wide": many pairs, long chains of
decisions; rounds and pairs are recorded beside the time), and `snap_to_nodes` of 1M jittered points onto the mesh's nodes through
the grid's cached node index.  Each as the whole public call from device arrays to device arrays, wall clock around the call (it
ends with the host holding the scalars, so nothing is in flight), 2 warm-ups, median of 20; beside it the scipy restatement of
tests/snap_cases.py on the same input, once, on the host (scipy's KD-tree and numpy, one thread).
`python profiles/snap_run.py [out.json] [points]`"""
import datetime, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch initialises its HIP runtime before the engine binds the device
import snap_cases as sc
import xugrid_amd as xa
from xugrid_amd import engine

out_path = sys.argv[1] if len(sys.argv) > 1 else "snap_run.json"
n_point = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000


def timed(fn, reps=20, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def host_ms(fn):
    t0 = time.perf_counter(); out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def dev(a):
    return engine.DeviceArray.from_host(np.ascontiguousarray(a))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


xy, faces = xa.meshgen.triangle_mesh(n_point, 0)
sides = np.concatenate([xy[faces[:, k]] - xy[faces[:, (k + 1) % 3]] for k in range(3)])
mean_edge = float(np.sqrt((sides * sides).sum(axis=1)).mean())
rng = np.random.default_rng(0)
res = {"machine": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})", "date": datetime.date.today().isoformat(),
       "n_node": len(xy), "n_face": len(faces), "mean_edge_length": mean_edge, "repeats": 20}

# snap_nodes: every node and its twin
both = np.concatenate([xy, xy + rng.uniform(-0.01, 0.01, xy.shape) * mean_edge])
dx, dy = dev(both[:, 0]), dev(both[:, 1])
for name, d in (("narrow", mean_edge / 20.0), ("wide", mean_edge)):
    r = {"n": len(both), "max_snap_distance": d}
    merged = engine.DeviceSnap(dx.ptr, dy.ptr, 1, len(both), d)
    r["n_kept"], r["n_pair"], r["rounds"] = merged.n_kept, merged.n_pair, merged.rounds
    del merged
    r["device_ms"] = timed(lambda: xa.snap_nodes(dx, dy, d))
    r["host_restatement_ms"], want = host_ms(lambda: sc.snap_nodes_ref(both[:, 0], both[:, 1], d))
    inverse, xs, ys = xa.snap_nodes(dx, dy, d)
    r["equal"] = bool(np.array_equal(inverse.download(), want[0]) and np.array_equal(bits(xs.download()), bits(want[2]))
                      and np.array_equal(bits(ys.download()), bits(want[3])))
    r["host_over_device"] = r["host_restatement_ms"] / r["device_ms"]
    res[f"snap_nodes_{name}"] = r
    print(name, json.dumps(r), flush=True)

# snap_to_nodes: 1M points near nodes, onto the mesh's nodes
grid = xa.Ugrid2d.from_device_arrays(dev(xy), dev(faces.astype(np.int64)))
near = xy[rng.integers(0, len(xy), 1_000_000)] + rng.uniform(-0.1, 0.1, (1_000_000, 2)) * mean_edge
px, py = dev(near[:, 0]), dev(near[:, 1])
d = 0.2 * mean_edge
r = {"n": len(near), "n_to": len(xy), "max_distance": d}
r["index_build_ms"] = host_ms(lambda: grid._nearest_index("node"))[0]
r["device_ms"] = timed(lambda: grid.snap_to_nodes(px, py, d, tiebreaker="nearest", return_index=True))
r["host_restatement_ms"], want = host_ms(lambda: sc.snap_to_nodes_ref(near[:, 0], near[:, 1], xy[:, 0], xy[:, 1], d))
xs, ys, index = grid.snap_to_nodes(px, py, d, tiebreaker="nearest", return_index=True)
r["snapped"], r["tied"] = int((want[2] >= 0).sum()), int((want[3] > 1).sum())
r["equal"] = bool(np.array_equal(index.download(), want[2]) and np.array_equal(bits(xs.download()), bits(want[0]))
                  and np.array_equal(bits(ys.download()), bits(want[1])))
r["host_over_device"] = r["host_restatement_ms"] / r["device_ms"]
res["snap_to_nodes"] = r
print("snap_to_nodes", json.dumps(r), flush=True)

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)

"""burn_vector_geometry at the benchmark's size (1M Delaunay faces of `bench.py`'s mesh): (a) one star polygon of 100 000
vertices, (b) 1 000 polygons of about 100 vertices each, (c) the star with all_touched=True.  Mesh and geometry live on
the device (torch tensors); the whole call is timed with hipEvents (torch.cuda.Event), 3 warm-ups, 10 repeats, and the
library's per-kernel timer gives the split of one call.  `python profiles/burn_run.py [points] [out.json]`"""
import json, os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch initialises its HIP runtime before the engine binds the device
import xugrid_amd as xa
from xugrid_amd import engine

n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 500_000
out_path = sys.argv[2] if len(sys.argv) > 2 else "burn_run.json"
xy, faces = xa.meshgen.triangle_mesh(n_points, 0)
dev = torch.device("cuda")
grid = xa.Ugrid2d.from_device_arrays(torch.as_tensor(xy, device=dev), torch.as_tensor(faces, device=dev))
res = {"n_face": grid.n_face}


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def star(centre, r_outer, r_inner, n):
    angle = 2.0 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, r_outer, r_inner)
    return np.column_stack((centre[0] + r * np.cos(angle), centre[1] + r * np.sin(angle)))


def on_device(rings_per_polygon):
    rings = [ring for polygon in rings_per_polygon for ring in polygon]
    ring_offsets = np.concatenate(([0], np.cumsum([len(r) for r in rings]))).astype(np.int64)
    polygon_offsets = np.concatenate(([0], np.cumsum([len(p) for p in rings_per_polygon]))).astype(np.int64)
    return tuple(torch.as_tensor(a, device=dev) for a in (np.concatenate(rings), ring_offsets, polygon_offsets))


def kernels(fn):
    engine.prof_enable(True); engine.prof_reset(); fn(); times = engine.kernel_times(); engine.prof_enable(False)
    return times


rng = np.random.default_rng(0)
big = on_device([[star((0.5, 0.5), 0.45, 0.40, 100_000)]])
many = on_device([[star(rng.uniform(0.05, 0.95, 2), 0.03, 0.02, 100)] for _ in range(1000)])
cases = {"a_star_100k_vertices": lambda: xa.burn_vector_geometry(grid, polygons=big),
         "b_1000_polygons_of_100_vertices": lambda: xa.burn_vector_geometry(grid, polygons=many),
         "c_star_100k_vertices_all_touched": lambda: xa.burn_vector_geometry(grid, polygons=big, all_touched=True)}
for name, fn in cases.items():
    burned = int((~torch.isnan(fn())).sum())
    med, best = timed(fn)
    res[name] = {"median_ms": med, "min_ms": best, "faces_burned": burned, "kernels_of_one_call": kernels(fn)}
print(json.dumps(res, indent=1, default=str))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1, default=str)

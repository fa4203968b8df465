"""snap_to_grid on the benchmark's 1M-triangle mesh with 10 000 polylines of 100 vertices (random walks with steps of about two
mesh spacings, started anywhere in the mesh's box; a fifth of the vertices lie within the snap distance of a node).  Measured as
the whole public call from host arrays (uploads and downloads included) and as the device part alone (lines already in HBM,
the C entry point), split per stage from the in-library kernel timers, beside the numpy restatement of tests/snapgrid_cases.py on
the same input (this process's CPUs; its pieces come from the oracle's C clipper).  hipEvent timing (torch.cuda.Event), 2 warm-ups,
5 repeats, median.
`python profiles/snapgrid_run.py [out.json] [mesh points] [lines] [vertices per line]`"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch initialises its HIP runtime before the engine binds the device
import snapgrid_cases as sg
import xugrid_amd as xa
from oracle import oracle
from xugrid_amd import engine

out_path = sys.argv[1] if len(sys.argv) > 1 else "snapgrid_run.json"
n_points = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
n_line = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000
n_per_line = int(sys.argv[4]) if len(sys.argv) > 4 else 100

STAGES = {  # kernel name prefix -> stage
    "snap_": "snap", "snapgrid_check_offsets": "snap", "snapgrid_segments": "snap",
    "edges_": "clip", "edge_rows_": "clip",
    "snapgrid_rows_": "rows",
    "snapgrid_order": "order", "snapgrid_gather": "order",
    "snapgrid_longest": "reduce", "snapgrid_first": "reduce", "snapgrid_winner": "reduce", "subset_compact": "reduce",
    "snapgrid_line_index": "reduce", "snapgrid_edge_lines": "reduce", "widen_i32": "reduce",
}


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


xy, faces = xa.meshgen.triangle_mesh(n_points, 0)
grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
lo, hi = xy.min(axis=0), xy.max(axis=0)
spacing = float(np.sqrt((hi - lo).prod() / len(xy)))
rng = np.random.default_rng(11)
steps = rng.normal(0.0, 2.0 * spacing, (n_line, n_per_line, 2))
steps[:, 0] = rng.uniform(lo, hi, (n_line, 2))
coords = np.ascontiguousarray(np.cumsum(steps, axis=1).reshape(-1, 2))
offsets = np.arange(n_line + 1, dtype=np.int64) * n_per_line
d = 0.25 * spacing
lines = (coords, offsets)
d_lines = (engine.DeviceArray.from_host(coords), engine.DeviceArray.from_host(offsets))

res = {"n_face": grid.n_face, "n_line": n_line, "n_vertex": len(coords), "max_snap_distance": d}
line_index, edges, edge_lines = grid.snap_to_grid(lines, d)  # (first use: the topology, the node index, the clipper's index)
topology, node_index = grid.device_topology(), grid._nearest_index("node")
res["n_edge"], res["n_snapped_edges"] = grid.n_edge, len(edges)


def device_part():
    return engine.DeviceSnapGrid(grid.device_mesh, topology, node_index, d_lines[0].ptr, len(coords), d_lines[1].ptr, n_line, d, 1e-12, True)


made = device_part()
res["n_piece"], res["n_row"] = made.n_piece, made.n_row
res["call_host_arrays_ms"] = timed(lambda: grid.snap_to_grid(lines, d))
res["call_device_arrays_ms"] = timed(lambda: grid.snap_to_grid(d_lines, d))
res["frame_host_arrays_ms"] = timed(lambda: xa.create_snap_to_grid_dataframe(lines, grid, d))
res["device_part_ms"] = timed(device_part)

# per stage: the kernel timers of one device-array call (the timers serialise the launches, so the sum exceeds the call above)
engine.prof_enable(True); engine.prof_reset()
grid.snap_to_grid(d_lines, d)
engine.dev_sync()
times = engine.kernel_times()
engine.prof_enable(False)
stages, kernels = {}, {}
for name, (launches, ms) in times.items():
    stage = next((s for prefix, s in STAGES.items() if name.startswith(prefix)), "other")
    stages[stage] = stages.get(stage, 0.0) + ms
    kernels[name] = {"launches": launches, "ms": ms, "stage": stage}
res["stage_ms"], res["kernel_ms"] = stages, kernels

# the numpy restatement on the same input, with the grid's own tables
centroids, face_edge, edge_face = grid.centroids, grid.face_edge_connectivity, grid.edge_face_connectivity
t0 = time.perf_counter()
frame = sg.frame_ref(oracle, xy, faces, centroids, face_edge, edge_face, coords, offsets, d)
want = sg.winners_ref(frame, grid.n_edge)
res["numpy_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
res["equal"] = bool(np.array_equal(edges, want[1]) and np.array_equal(edge_lines, want[2])
                    and np.array_equal(np.isnan(line_index), np.isnan(want[0])))
got = xa.create_snap_to_grid_dataframe(lines, grid, d)
res["frame_equal"] = bool(all(np.array_equal(got[c], frame[c]) for c in sg.COLUMNS))
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)

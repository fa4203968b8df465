"""Ugrid2d.label_partitions on the device: what the labelling costs and what cut it reaches.

On the 1M-face benchmark source mesh (meshgen.triangle_mesh(500 000, 0), qhull numbering) as a grid whose mesh lives in HBM, for
n_part in {2, 8, 64}: the first call (face topology, graph and centroids included), a call with those cached (wall clock around
the call, which ends synchronised; 2 warm-ups, median of 9), the rounds run, the moves accepted, the edge cut of the seed and of
the result, the part sizes against the bounds [Lmin, L], and the launches and summed kernel time under the engine's per-kernel
hipEvent table (in a run of its own).  Beside them the edge cut of the Morton-cell ownership that
distributed.partition_faces(centroids, n_part, mode="morton") gives for the same faces -- the partition the project offers
today -- counted on the host over the same adjacency.
`python profiles/partlabel_run.py [out.json] [points]`"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import xugrid_amd as xa
from xugrid_amd import distributed, meshgen, partition
from xugrid_amd import engine as E

out_path = sys.argv[1] if len(sys.argv) > 1 else "partlabel_run.json"
points = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
PARTS, WARM, REPS = (2, 8, 64), 2, 9


def wall_ms(fn):
    E.dev_sync(); t0 = time.perf_counter(); out = fn(); E.dev_sync()
    return 1e3 * (time.perf_counter() - t0), out


def host_cut(rows, cols, labels):
    return int((labels[rows] != labels[cols]).sum()) // 2


xy, faces = meshgen.triangle_mesh(points, 0)
centroids_host = xy[faces].mean(axis=1)
morton = {P: distributed.partition_faces(centroids_host, P, mode="morton").astype(np.int64) for P in PARTS}  # (torch on the CPU, before the engine binds the device)
E.init(0)
keep = E.DeviceArray.from_host(np.ascontiguousarray(xy)), E.DeviceArray.from_host(np.ascontiguousarray(faces))
grid = xa.Ugrid2d.from_device_arrays(*keep)
first_ms, _ = wall_ms(lambda: grid.label_partitions(PARTS[0]))
indptr, indices, _ = grid._graph("face").download()
rows = np.repeat(np.arange(grid.n_face), np.diff(indptr))
result = {"points": points, "n_face": int(grid.n_face), "nnz": int(len(indices)), "warm_ups": WARM, "repeats": REPS,
          "first_call_ms_with_topology_graph_and_centroids": first_ms, "parts": []}
for P in PARTS:
    for _ in range(WARM):
        grid.label_partitions(P)
    times = [wall_ms(lambda: grid.label_partitions(P))[0] for _ in range(REPS)]
    labels = grid.label_partitions(P).download()
    info = dict(partition.last_info)
    with E.KernelTimer() as timer:
        grid.label_partitions(P)
    sizes = np.bincount(labels, minlength=P)
    T = int(grid.n_face)
    L = max(-(-T // P), T * 103 // (100 * P))
    Lmin = min(T // P, -(-(T * 97) // (100 * P)))
    assert host_cut(rows, indices, labels) == info["cut"] <= info["cut_seed"] and Lmin <= sizes.min() and sizes.max() <= L
    row = {
        "n_part": P, "call_ms_median": float(np.median(times)), "call_ms_all": times,
        "rounds": info["rounds"], "moves": info["moves"], "cut_seed": info["cut_seed"], "cut": info["cut"],
        "cut_morton_cells": host_cut(rows, indices, morton[P]),
        "morton_part_sizes_min_max": [int(np.bincount(morton[P], minlength=P).min()), int(np.bincount(morton[P], minlength=P).max())],
        "part_sizes_min_max": [int(sizes.min()), int(sizes.max())], "Lmin_L": [int(Lmin), int(L)],
        "launches": int(sum(v[0] for v in timer.records.values())),
        "kernel_ms_sum_under_timer": float(sum(v[1] for v in timer.records.values())),
        "kernels_under_timer": {k: [int(v[0]), float(v[1])] for k, v in sorted(timer.records.items())},
    }
    print(json.dumps({k: v for k, v in row.items() if k != "kernels_under_timer"}), flush=True)
    result["parts"].append(row)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)

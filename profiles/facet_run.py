"""Facet mapping (to_node / to_edge / to_face) at the size of profiles/topology_run.py: meshgen.triangle_mesh(500 000, 0), once
in qhull's numbering and once with the faces randomly permuted; K = 1 and K = 64 float64 slices resident in HBM; face -> node
mean, node -> face mean, face -> edge mean, node -> edge raw.  After a warm-up of every shape three routes alternate in one
process, each ending in a device synchronise:
  a  this feature on the grid in HBM (the tables of its device topology are read where they are)
  b  torch.where(table >= 0, data[:, table.clamp_min(0)], nan).nanmean(-1) on the dense tables, downloaded and uploaded once
     outside the timing: what a tensor user writes today
  c  the host route: download the data, tests/facet_cases.py in numpy, upload the result
Median of REPS samples, every sample kept.  For (a) the kernel time (xr_prof) with eight slices per lane and with one (option
facet_tile), and the share of the HBM peak for the bytes the algorithm has to move: the table once per TILE of slices, K x
source read once, K x output written (a lower bound: a gather that misses the caches moves whole lines).
`python profiles/facet_run.py [points] [out.json]`"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch initialises its HIP runtime before the engine binds the device
import xugrid_amd as xa
from xugrid_amd import engine
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import facet_cases as fc  # noqa: E402

n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 500_000
out_path = sys.argv[2] if len(sys.argv) > 2 else "facet_run.json"
REPS = 5
HBM_PEAK = 8.0e12      # bytes / s, MI355X specification
HBM_MEASURED = 6.29e12  # float4 copy
TILE = 8               # FACET_TILE of csrc/xr_facet.hip
DIRECTIONS = (("node", "face", "mean"), ("face", "node", "mean"), ("edge", "face", "mean"), ("edge", "node", None))


def say(*a):
    print(*a, flush=True)


def sync():
    torch.cuda.synchronize(); engine.dev_sync()


def wall(fn):
    sync(); t0 = time.perf_counter(); fn(); sync()
    return 1e3 * (time.perf_counter() - t0)


def kernel_ms(fn, reps=REPS):
    """-> median over reps of {kernel name: ms}"""
    rows = []
    for _ in range(reps):
        engine.prof_enable(True); engine.prof_reset(); engine.dev_sync()
        fn(); engine.dev_sync()
        rows.append({k: ms for k, (_, ms) in engine.kernel_times().items()}); engine.prof_enable(False)
    return {k: float(np.median([r.get(k, 0.0) for r in rows])) for k in sorted(set().union(*rows))}


def torch_route(table_t, data, form):
    gathered = torch.where(table_t >= 0, data[:, table_t.clamp_min(0)], torch.nan)
    return gathered if form is None else gathered.nanmean(-1)


def host_route(table, data, form):
    host = data.cpu().numpy()
    out = fc.raw(table, host) if form is None else fc.reduce_sequential(table, host, form)
    return torch.tensor(out, device="cuda")


def measure(label, xy, faces, res):
    grid = xa.Ugrid2d.from_device_arrays(torch.tensor(xy, device="cuda"), torch.tensor(faces, device="cuda"))
    tables = fc.host_tables(faces, len(xy))
    n = fc.sizes(tables)
    rng = np.random.default_rng(3)
    r = {"n": n}
    for target, source, form in DIRECTIONS:
        table = tables[(target, source)]
        table_t = torch.tensor(table, device="cuda")
        width = table.shape[1]
        entries = int((table >= 0).sum())
        csr = target == "node"
        for K in (1, 64):
            data = torch.tensor(rng.standard_normal((K, n[source])), device="cuda")
            routes = {"a_feature": lambda: getattr(grid, f"to_{target}")(data, dim=source, reduce=form),
                      "b_torch": lambda: torch_route(table_t, data, form),
                      "c_host": lambda: host_route(table, data, form)}
            got = routes["a_feature"]()
            exp = routes["c_host"]()
            assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(exp, nan=-7.0)), (target, source, form, K)
            routes["b_torch"]()
            del got, exp
            samples = {name: [] for name in routes}
            for _ in range(REPS):
                for name, fn in routes.items():
                    samples[name].append(wall(fn))
            row = {"wall_ms_median": {k: float(np.median(v)) for k, v in samples.items()}, "wall_ms_samples": samples}
            engine.set_option("facet_tile", 0)
            row["kernels_ms_tile_8"] = kernel_ms(routes["a_feature"])
            engine.set_option("facet_tile", 1)
            row["kernels_ms_tile_1"] = kernel_ms(routes["a_feature"])
            engine.set_option("facet_tile", 0)
            kernel = "facet_raw" if form is None else "facet_reduce"
            out_per_slice = n[target] * (width if form is None else 1)
            table_bytes = 4 * (entries + (n[target] + 1 if csr else table.size - entries))
            tiles = -(-K // TILE)
            need = tiles * table_bytes + 8 * K * n[source] + 8 * K * out_per_slice
            row["bytes_needed"] = int(need)
            row["bytes_rule"] = "table (int32) once per tile of 8 slices + K x source once + K x output once"
            t = row["kernels_ms_tile_8"][kernel] * 1e-3
            row["share_of_hbm_peak_8.0TBps"] = need / t / HBM_PEAK
            row["share_of_hbm_measured_6.29TBps"] = need / t / HBM_MEASURED
            r[f"{source}_to_{target}_{form or 'raw'}_K{K}"] = row
            say(label, target, source, form, K, row["wall_ms_median"], row["kernels_ms_tile_8"].get(kernel),
                row["kernels_ms_tile_1"].get(kernel))
            del data
        del table_t
    assert grid._host is None, "the device route downloaded the mesh"
    res[label] = r


xy0, f0 = xa.meshgen.triangle_mesh(2000, 0)
measure("warm_up", xy0, f0, {})  # untimed: code objects, pools, torch
xy, faces = xa.meshgen.triangle_mesh(n_points, 0)
res = {"n_face": int(len(faces)), "n_node": int(len(xy)), "reps": REPS, "tile": TILE}
for label, f in (("qhull_numbering", faces), ("permuted", faces[np.random.default_rng(5).permutation(len(faces))])):
    measure(label, xy, f, res)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
say(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}, indent=1))

"""The device fills at the benchmark's size (1M Delaunay faces, a ~5 % hole): ms per CG iteration for K = 1 and K = 16
against the bytes-per-iteration floor at the measured copy bandwidth, CG iterations to atol 1e-4, the nearest fill, and
scipy's unpreconditioned `cg` per iteration on the host for comparison.  hipEvent timing (torch.cuda.Event), 3 warm-ups,
10 repeats.  `python profiles/fill_run.py [points] [out.json]`"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch initialises its HIP runtime before the engine binds the device
from scipy.sparse.linalg import cg
import xugrid_amd as xa
from xugrid_amd import fill

n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 500_000
out_path = sys.argv[2] if len(sys.argv) > 2 else "fill_run.json"
xy, faces = xa.meshgen.triangle_mesh(n_points, 0)
grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
c = grid.centroids
base = xa.meshgen.smooth_field(c, 0)
base[np.hypot(c[:, 0] - 0.5, c[:, 1] - 0.5) < 0.126] = np.nan
n = grid.n_face
res = {"n_face": n, "nan_fraction": float(np.isnan(base).mean())}


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


# copy bandwidth (read + write of a 1 GiB buffer)
a = torch.empty(1 << 27, dtype=torch.float64, device="cuda"); b = torch.empty_like(a)
ms, _ = timed(lambda: b.copy_(a))
bw = 2 * a.numel() * 8 / (ms * 1e-3)
res["copy_GBps"] = bw / 1e9
del a, b

t1 = torch.tensor(base, device="cuda")
grid.laplace_interpolate(t1)
res["iterations_atol_1e-4"] = int(fill.last_iterations[0])
res["laplace_ms_K1_atol_1e-4"] = timed(lambda: grid.laplace_interpolate(t1))[0]
ITER = 200
for K in (1, 16):
    tk = t1.expand(K, n).contiguous()
    fixed = lambda: grid.laplace_interpolate(tk, atol=0.0, maxiter=ITER)  # noqa: E731  (never converges: ITER iterations)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        med, best = timed(fixed)
        zero = timed(lambda: grid.laplace_interpolate(tk, atol=0.0, maxiter=1))[0]
    per_it = (med - zero) / (ITER - 1)
    # bytes per row and iteration that must move (gathers assumed cached): CSR row (4 + 3 x 4 + 3 x 8 weights), unknown flag,
    # scale, r, p_old read and p_new, q written (spmv); unknown, p, q read and x, r read + written (update)
    bytes_row = (4 + 12 + 24 + 1 + 8 + 16 + 16) + (1 + 16 + 32)
    res[f"K{K}"] = {"ms_per_iteration": per_it, "ms_per_iteration_per_slice": per_it / K,
                    "floor_ms_per_iteration": K * n * bytes_row / bw * 1e3, "bytes_per_row": bytes_row}

res["nearest_ms_K1"] = timed(lambda: grid.interpolate_na(t1))[0]
t16 = t1.expand(16, n).contiguous()
res["nearest_ms_K16_shared_mask"] = timed(lambda: grid.interpolate_na(t16))[0]

# host: scipy's cg without preconditioner on the same scaled system, per iteration, on this process's CPUs
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from fill_cases import scaled_system  # noqa: E402
from scipy.sparse import csgraph  # noqa: E402
conn = grid.get_connectivity_matrix("face", xy_weights=True)
A, rhs, scale, unknown = scaled_system(base, conn, csgraph.connected_components(conn)[1], True)
t0 = time.perf_counter(); cg(A, rhs, atol=0.0, rtol=0.0, maxiter=ITER); t = time.perf_counter() - t0
res["host_scipy_cg_ms_per_iteration"] = 1e3 * t / ITER
res["host_scipy_cg_unknowns"] = int(unknown.sum())
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)

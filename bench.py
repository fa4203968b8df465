#!/usr/bin/env python
"""
Benchmark of the regridding hot path on MI355X.

    python bench.py --gpus 1 --steps K --warmup W [--full] [--dump-outputs DIR]
    python bench.py --gpus N --steps K --warmup W          (launches itself under torch.distributed.run, one rank per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --project-shards 8 [--strong]          (ONE GPU: per-shard table + projected 8-GPU step)

Metric (BASELINE.json): target cells regridded / s for an OverlapRegridder, area-weighted mean.
Workload at N = 1: BASELINE config 2 -- a ~1M-triangle Delaunay source mesh (500k jittered-lattice
points, seed 0) regridded to a ~1M-triangle target (seed 1, rotated 30 degrees, scaled 0.7).

One "step" is one full pass of the hot path over the batch, starting from raw mesh arrays that are
already resident in HBM (node coordinates f64, connectivity i32, source data f64):
    per-face preparation of both meshes (fill, CCW, bbox, area)  ->  spatial index over the source
    ->  candidate search  ->  polygon clip  ->  CSR assembly  ->  apply (mean) of one variable.
Nothing is cached between steps (xr_mesh_invalidate); the scalar read-backs the path needs (number
of candidate pairs, nnz) are inside the timed region.  value = T / time per step.

N > 1 (weak scaling): the meshes grow with N (N x 500k points each); source faces are sharded
over the ranks (Morton blocks), the target is replicated; each step additionally does the one
exchange step of the path: a reduce-scatter (RCCL) of the per-target partial sums.  value = total
target cells / max-over-ranks time.

Prints ONE JSON line on rank 0 (contract in the task statement) with two extra objects:
"roofline" for the dominant kernel (algorithmic bytes / hipEvent-timed duration)
and, at N = 1, "cpu_baseline" (the CPU oracle -- a port of the reference path -- timed on the host).
At N = 1 both are measured with --full only (null otherwise), as are the other figures of "config"
and "other_configs": a plain run sets up, warms up, times the K steps and prints the headline.

--dump-outputs DIR (N = 1): after the timed steps, the outputs of the last one -- the regridded field
(regridded, float64[T]) and the weight matrix (weights float64[nnz], weights_indices, weights_indptr;
CSR over the target rows) -- are written as DIR/<name>.npy, at most 64 MB in all (dump_outputs).  The
inputs are generated from fixed seeds, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md
CPU_RUNS = 5  # timed runs of the CPU baseline (median), after one warm-up
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: at most this much in all


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def make_meshes(points_per_mesh, delaunay=True):
    from xugrid_amd import meshgen

    t0 = time.perf_counter()
    sxy, sf = meshgen.triangle_mesh(points_per_mesh, 0, delaunay=delaunay)
    txy, tf = meshgen.triangle_mesh(points_per_mesh, 1, 30.0, 0.7, delaunay=delaunay)
    log(f"[bench] meshes: S={sf.shape[0]} T={tf.shape[0]} ({time.perf_counter() - t0:.1f}s)")
    return sxy, sf, txy, tf


def algorithmic_bytes(S, T, Ns, Nt, P, K=1, Ms=3, Mt=3):
    """SURVEY.md section 8(d), the contract for `roofline.achieved` (int32 structure, f64 geometry and weights):
    weights build  B_build = 4 (sum Ms + sum Mt) + 16 (Ns + Nt) + 12 P + 4 (T + 1)   (both meshes once, the CSR once)
    apply          B_apply = 12 P + 4 (T + 1) + 8 K (S + T)                            (weights once, data once)"""
    build = 4 * (Ms * S + Mt * T) + 16 * (Ns + Nt) + 12 * P + 4 * (T + 1)
    apply_ = 12 * P + 4 * (T + 1) + 8 * K * (S + T)
    return {"build": build, "apply": apply_, "step": build + apply_}


def kernel_model_bytes(S, T, Ns, Nt, C, P, Ms=3, Mt=3):
    """The engine's OWN per-kernel byte model (every array a kernel has to read or write once, intermediate
    arrays included: face-major vertex blocks, f32 record boxes, the pair queue).  Not the roofline contract --
    kept under `roofline.kernel_model` to show where the bytes beyond section 8(d) come from."""
    vs, vt = 16 * Ms, 16 * Mt
    return {
        "prepare_stats": 4 * Ms * S + 16 * Ns,                      # tree side: statistics only
        "prepare_faces": 4 * Mt * T + 16 * Nt + (vt + 1 + 32) * T,   # query side: vertex blocks, length, bbox
        "index_count": 4 * Ms * S + 16 * Ns + 4 * S,
        "index_scatter": 4 * S + 4 * Ms * S + 16 * Ns + (4 + vs + 1 + 16) * S,
        "search": 32 * T + 16 * S + 8 * T + 8 * C,
        "clip_tri": 8 * C + vt * T + vs * S + 4 * S + 12 * C,
        "assemble": 16 * C + 8 * T + 8 * T + 12 * P + 4 * T,
        "apply_stream": 12 * P + 4 * (T + 1) + 4 * T + 8 * (S + T),
        "apply_rows1": 12 * P + 4 * (T + 1) + 4 * T + 8 * (S + T),   # (the one-launch K = 1 apply: same bytes)
        "sample_stats": (4 * Ms * S + 16 * Ns) // 8 + 16 * Ns,        # tree side: every 8th block of faces + all nodes
    }


def source_sha():
    """sha1 over the kernel sources (as profiles/pmc_summary.py): PMC numbers of other kernels are refused."""
    import glob
    import hashlib

    h = hashlib.sha1()
    for f in sorted(glob.glob(os.path.join(ROOT, "xugrid_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "xugrid_amd", "csrc", "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def usable_cores(n_threads):
    """Threads worth starting: the scheduler affinity and the cgroup CPU quota of this container bound what OpenMP's
    default (one thread per visible processor) can actually use -- 256 threads on a 16-CPU quota run SLOWER than 16."""
    n = min(n_threads, len(os.sched_getaffinity(0)))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_baseline(sxy, sf, txy, tf, data):
    """The CPU oracle (oracle/xr_oracle.c: cell tree + SAT + Sutherland-Hodgman + CSR + mean apply) timed on this
    box's host cores, SURVEY.md section 8(d):
      faithful   the reference's parallel structure: tree build serial, search parallel over target faces, clip
                 parallel over candidate pairs, apply parallel over K only (numba prange, regridder.py:50) -- all cores,
                 the whole workload once; this is `value`
      favourable the same with the apply parallel over target rows as well
      one thread the tree build and the apply on the whole workload, search + clip on a sample of the target faces,
                 extrapolated linearly (bounded to a few seconds)"""
    from oracle import oracle as O

    O.build()
    cores = usable_cores(O.num_threads())
    O.set_num_threads(cores)
    T = tf.shape[0]

    def once():
        t0 = time.perf_counter()
        tree = O.CellTree2d(sxy, sf)
        t_tree = time.perf_counter() - t0
        t0 = time.perf_counter()
        q, s, a = tree.intersect_faces(txy, tf)
        indptr = O.to_csr_indptr(q, T)
        t_pairs = time.perf_counter() - t0
        t0 = time.perf_counter()
        out = O.regrid_csr("mean", data[None, :], a, s, indptr, T, parallel_rows=False)
        t_apply = time.perf_counter() - t0
        t0 = time.perf_counter()
        O.regrid_csr("mean", data[None, :], a, s, indptr, T, parallel_rows=True)
        t_apply_rows = time.perf_counter() - t0
        return (t_tree, t_pairs, t_apply, t_apply_rows), (a, s, indptr, out)

    # median after a warm-up (the first run pays page faults of ~0.5 GB of fresh arrays and the OpenMP
    # team start): one untimed run, then the median of CPU_RUNS runs, component by component
    once()
    runs = [once() for _ in range(CPU_RUNS)]
    t_tree, t_pairs, t_apply, t_apply_rows = (float(np.median([r[0][i] for r in runs])) for i in range(4))
    a, s, indptr, out = runs[-1][1]
    # one thread: bounded sample of the target faces
    n_sample = min(T, 40_000)
    sample = np.sort(np.random.default_rng(0).choice(T, n_sample, replace=False))
    O.set_num_threads(1)
    t0 = time.perf_counter()
    tree1 = O.CellTree2d(sxy, sf)
    t_tree1 = time.perf_counter() - t0
    t0 = time.perf_counter()
    tree1.intersect_faces(txy, tf[sample])
    t_pairs1 = (time.perf_counter() - t0) * (T / n_sample)
    t0 = time.perf_counter()
    O.regrid_csr("mean", data[None, :], a, s, indptr, T, parallel_rows=False)
    t_apply1 = time.perf_counter() - t0
    O.set_num_threads(cores)
    faithful = t_tree + t_pairs + t_apply
    log(f"[bench] cpu oracle, {cores} threads: tree {t_tree:.2f}s pairs {t_pairs:.2f}s apply {t_apply:.3f}s "
        f"(rows-parallel {t_apply_rows:.3f}s); 1 thread: tree {t_tree1:.2f}s pairs ~{t_pairs1:.1f}s apply {t_apply1:.3f}s; nnz {a.size}")
    return {
        "value": T / faithful,
        "unit": "target cells/s",
        "cores": cores,
        "kind": "port",
        "sample": f"full workload, median of {CPU_RUNS} runs after one warm-up: S={sf.shape[0]} T={T} K=1 "
                  f"(tree {t_tree:.2f}s + search/clip {t_pairs:.2f}s + apply {t_apply:.3f}s)",
        "runs": CPU_RUNS,
        "seconds_each": [round(sum(r[0][:3]), 4) for r in runs],
        "variants": {
            "faithful_all_cores": {"cells_per_s": T / faithful, "cores": cores, "seconds": faithful},
            "favourable_all_cores": {"cells_per_s": T / (t_tree + t_pairs + t_apply_rows), "cores": cores,
                                     "seconds": t_tree + t_pairs + t_apply_rows,
                                     "note": "apply parallel over target rows as well (the reference's is over K only)"},
            "one_thread": {"cells_per_s": T / (t_tree1 + t_pairs1 + t_apply1), "cores": 1,
                           "seconds_extrapolated": t_tree1 + t_pairs1 + t_apply1,
                           "sample": f"tree build and apply on the whole workload, search + clip on {n_sample} of {T} target "
                                     "faces (random, seed 0), scaled linearly"},
        },
    }, out[0]


def dump_outputs(path, arrays, limit=DUMP_LIMIT_BYTES):
    """Write ``arrays`` (name -> 1-D array) as ``path/<name>.npy``: float arrays as float64, integer arrays as float32 when
    every value is exact in it (|v| < 2**24), else float64.  If the whole exceeds ``limit`` bytes, each array keeps the same
    fraction of its entries, at the positions ``np.sort(np.random.default_rng(0).choice(size, n, replace=False))`` -- a fixed
    sample, so two runs on the same inputs write the same positions."""
    os.makedirs(path, exist_ok=True)
    out = {}
    for name, a in arrays.items():
        a = np.asarray(a).ravel()
        exact32 = a.dtype.kind in "iu" and (a.size == 0 or int(np.abs(a).max()) < 2 ** 24)
        out[name] = a.astype(np.float32 if exact32 else np.float64)
    total = sum(a.nbytes for a in out.values())
    room = limit - 1024 * len(out)  # (an .npy header is 128 bytes)
    if total > room:
        for name, a in out.items():
            n = int(a.size * room / total)
            out[name] = a[np.sort(np.random.default_rng(0).choice(a.size, n, replace=False))]
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)
    log(f"[bench] outputs: {', '.join(f'{k} {v.shape[0]}' for k, v in out.items())} -> {path}")


def make_step(E, ms, mt, d_src, d_out, state):
    """One step of the headline: nothing cached (both meshes lose their derived state), then the whole weight build and the
    mean apply of one variable, from HBM-resident raw arrays to an HBM-resident result."""
    two_calls = os.environ.get("XR_BENCH_TWO_CALLS", "") not in ("", "0")  # A/B: weights and apply as two entry points

    def step():
        ms.invalidate()
        mt.invalidate()
        if two_calls:
            csr = ms.overlap(mt)  # prepare x2 + index + search + clip + CSR
            csr.apply_dev(d_src, E.XR_F64, 1, d_out, 0)
        else:
            # the same through ONE entry point of the C ABI (xr_overlap_apply_dev under xr_set_async: the RAW library step --
            # the apply is enqueued before the host has read the matrix' sizes back).  The reference-shaped classes build
            # the weights in their constructor and apply in regrid(): that figure is `config.api_ms`, and the two-call form
            # of this step is XR_BENCH_TWO_CALLS=1
            csr = ms.overlap_apply_dev(mt, d_src, E.XR_F64, 1, d_out, 0)
        state["csr"] = csr

    return step


def run_single(args):
    import ctypes

    import xugrid_amd as xa
    from xugrid_amd import _lib, engine as E

    E.init(0)
    lib = _lib.load()
    sxy, sf, txy, tf = make_meshes(args.points, delaunay=not args.no_delaunay)
    S, T, Ns, Nt = sf.shape[0], tf.shape[0], sxy.shape[0], txy.shape[0]
    ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
    data = xa.meshgen.smooth_field(ms.centroids(), 0)
    # source data and output resident in HBM
    d_src, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.xr_dev_alloc(8 * S, ctypes.byref(d_src)))
    _lib.check(lib.xr_dev_alloc(8 * T, ctypes.byref(d_out)))
    _lib.check(lib.xr_dev_upload(d_src, data.ctypes.data_as(ctypes.c_void_p), 8 * S))

    state = {}
    step = make_step(E, ms, mt, d_src.value, d_out.value, state)

    # The K steps are issued back to back on the engine's stream (xr_set_async: no host synchronisation inside a step
    # beyond the one read-back of the matrix' sizes every weight build needs); the timed region is bracketed by device
    # synchronisations on both sides.  XR_BENCH_SYNC=1: every call synchronous, as until round 3 (A/B).
    sync_steps = os.environ.get("XR_BENCH_SYNC", "") not in ("", "0")
    E.set_async(not sync_steps)
    for _ in range(args.warmup):
        step()
    E.dev_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    E.dev_sync()
    elapsed = time.perf_counter() - t0
    E.set_async(False)
    ms_per_step = 1e3 * elapsed / args.steps
    csr = state["csr"]
    C, P = ms.last_candidates(), csr.nnz
    if args.dump_outputs:
        # what the caller of the timed entry point holds after the last timed step: the weight matrix and the regridded field
        out_step = np.empty(T)
        _lib.check(lib.xr_dev_download(out_step.ctypes.data_as(ctypes.c_void_p), d_out, 8 * T))
        w_data, w_indices, w_indptr = csr.download()
        dump_outputs(args.dump_outputs, {"regridded": out_step, "weights": w_data, "weights_indices": w_indices,
                                         "weights_indptr": w_indptr})
        del out_step, w_data, w_indices, w_indptr
    result = {
        "metric": "target cells regridded/s (OverlapRegridder 1M->1M tri, weights + mean apply)",
        "value": T / (elapsed / args.steps),
        "unit": "target cells/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": "BASELINE config 2: ~1M-triangle jittered-lattice Delaunay source -> ~1M-triangle target "
            "(seed 1, rotated 30 deg, scaled 0.7), OverlapRegridder area-weighted mean, K=1",
            "source_faces": S,
            "target_faces": T,
            "candidate_pairs": C,
            "nnz": P,
            "parallelism": "1 GPU",
            "step_entry_point": "xr_overlap_apply_dev under xr_set_async: the raw C-ABI step on HBM-resident arrays (weights + "
            "apply enqueued as one call); the reference-shaped classes (weights in the constructor, apply in regrid(), host "
            "arrays in and out) are `api_ms`",
        },
        "roofline": None,
        "cpu_baseline": None,
    }
    if not args.full:  # the headline only; the measurements below (and their extra runs of the step) are --full
        print(json.dumps(result), flush=True)
        return

    # weights-only and apply-only rates (reported in config, not the headline).  Apply only: every call synchronous (the
    # reference's contract: regrid() returns the result), after a few untimed calls -- the first synchronous apply of a
    # process creates the calling thread's stream (xr_engine.hip: lanes), ~10 ms that round 4's first bench lines spread over
    # the 100 timed calls (0.116 ms instead of 0.037) -- and back to back on the engine's stream (xr_set_async).
    for _ in range(5):
        csr.apply_dev(d_src.value, E.XR_F64, 1, d_out.value, 0)
    E.dev_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        csr.apply_dev(d_src.value, E.XR_F64, 1, d_out.value, 0)
    E.dev_sync()
    apply_ms = 1e3 * (time.perf_counter() - t0) / args.steps
    E.set_async(True)
    for _ in range(5):
        csr.apply_dev(d_src.value, E.XR_F64, 1, d_out.value, 0)
    E.dev_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        csr.apply_dev(d_src.value, E.XR_F64, 1, d_out.value, 0)
    E.dev_sync()
    apply_async_ms = 1e3 * (time.perf_counter() - t0) / args.steps
    E.set_async(False)

    # weights only (no apply), and the whole thing from HOST arrays (mesh uploads + step + result download over PCIe);
    # both informative, neither is `value`
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ms.invalidate()
        mt.invalidate()
        ms.overlap(mt)
    E.dev_sync()
    build_ms = 1e3 * (time.perf_counter() - t0) / args.steps
    host_times = []
    hs = ht = h_out = None
    # (--step-only: the passes from host arrays are skipped -- their freshly uploaded meshes meet cold caches, and a profiler's
    # per-kernel AVERAGE over the whole process would mix those launches with the timed step's: profiles/collect.sh)
    for _ in range(0 if args.step_only else 6):
        del hs, ht, h_out  # (the previous iteration's handles are released OUTSIDE the timed region)
        E.dev_sync()
        t0 = time.perf_counter()
        hs, ht = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
        h_out = hs.overlap(ht).apply(data[None, :], 0)
        host_times.append(time.perf_counter() - t0)
    del hs, ht, h_out
    host_to_host_ms = 1e3 * float(np.median(host_times[1:])) if host_times else None  # (the first pass warms the pinned staging path)
    # ... and through the PUBLIC API, as a user of the reference would write it (regridder.py:505-512, :212-262):
    # OverlapRegridder(Ugrid2d(...), Ugrid2d(...), "mean").regrid(data) from host arrays to a host result -- everything the
    # Python layer adds (constructor checks, grid wrappers, result allocation) is inside.  Median of 5 after one warm-up,
    # with a phase split taken on further passes.
    def api_once(split=None):
        t = [time.perf_counter()]
        src_g = xa.Ugrid2d(sxy[:, 0], sxy[:, 1], -1, sf)
        tgt_g = xa.Ugrid2d(txy[:, 0], txy[:, 1], -1, tf)
        t.append(time.perf_counter())
        if split is not None:
            src_g.device_mesh, tgt_g.device_mesh  # (uploads on their own; otherwise they happen inside the constructor below)
            E.dev_sync()
            t.append(time.perf_counter())
        rg = xa.OverlapRegridder(src_g, tgt_g, method="mean")
        if split is not None:
            E.dev_sync()
        t.append(time.perf_counter())
        res = rg.regrid(data)
        t.append(time.perf_counter())
        if split is not None:
            for k, v in zip(("grid_wrappers", "uploads", "constructor_weights", "regrid_apply_download"), np.diff(t)):
                split.setdefault(k, []).append(1e3 * v)
        return t[-1] - t[0], (src_g, tgt_g, rg, res)

    # ... and the same classes on arrays that already live in HBM (round 6): Ugrid2d.from_device_arrays x 2 + OverlapRegridder +
    # regrid(device array) -> device array.  Nothing crosses PCIe; the regridder's weights are built by its first regrid in one
    # engine call with the apply (xr_overlap_apply_dev, the entry point of the timed step); mesh validation + int64 -> int32
    # narrowing of both connectivities and the result's allocation are inside.
    def api_device_once(dev_arrays, split=None):
        d_sxy, d_sf, d_txy, d_tf, d_data = dev_arrays
        t = [time.perf_counter()]
        src_g = xa.Ugrid2d.from_device_arrays(d_sxy, d_sf)
        tgt_g = xa.Ugrid2d.from_device_arrays(d_txy, d_tf)
        t.append(time.perf_counter())
        rg = xa.OverlapRegridder(src_g, tgt_g, method="mean")
        t.append(time.perf_counter())
        res = rg.regrid(d_data)  # (returns with the result complete)
        t.append(time.perf_counter())
        if split is not None:
            for k, v in zip(("device_grids", "constructor", "regrid_weights_and_apply"), np.diff(t)):
                split.setdefault(k, []).append(1e3 * v)
        return t[-1] - t[0], (src_g, tgt_g, rg, res)

    api_times, keep = [], None
    for _ in range(0 if args.step_only else 6):
        del keep
        E.dev_sync()
        dt, keep = api_once()
        api_times.append(dt)
    api_ms = 1e3 * float(np.median(api_times[1:])) if api_times else None
    api_device_ms, api_device_phases, api_device_equal = None, {}, None
    if not args.step_only:
        dev_arrays = tuple(E.DeviceArray.from_host(a) for a in (sxy, sf, txy, tf, data))
        times, split, keep_d = [], {}, None
        for i in range(9):
            del keep_d
            E.dev_sync()
            dt, keep_d = api_device_once(dev_arrays, split if i >= 6 else None)
            if i < 6:
                times.append(dt)
        api_device_ms = 1e3 * float(np.median(times[1:]))
        api_device_phases = {k: round(float(np.median(v)), 4) for k, v in split.items()}
        api_device_result = keep_d[3].download()
        del keep_d, dev_arrays

    api_split = {}
    for _ in range(0 if args.step_only else 3):
        del keep
        E.dev_sync()
        _, keep = api_once(api_split)
    if keep is not None and api_device_ms is not None:
        api_device_equal = bool(np.array_equal(api_device_result, keep[3], equal_nan=True))
        del api_device_result
    del keep
    api_phases = {k: round(float(np.median(v)), 4) for k, v in api_split.items()}

    # per-kernel durations: the same K steps with hipEvents around every launch (engine stream); the W warm-up steps again
    # first (the host-array passes above ran other kernels and released their buffers)
    E.set_async(not sync_steps)
    for _ in range(args.warmup):
        step()
    E.dev_sync()
    with E.KernelTimer() as kt:
        for _ in range(args.steps):
            step()
    E.set_async(False)
    kernels = {k: (n, t / n) for k, (n, t) in kt.records.items()}  # name -> (launches, avg ms)
    per_step = {k: n * avg / args.steps for k, (n, avg) in kernels.items()}
    # the dominant kernel of the MAIN stream chain (the big faces' kernels run beside it on the side stream)
    side = {"search_big", "clip_big", "big_rank", "big_scan", "row_fill_long"}
    dominant = max((k for k in per_step if k not in side), key=per_step.get)
    ab = algorithmic_bytes(S, T, Ns, Nt, P)
    dom_ms = kernels[dominant][1]
    build_names = [k for k in per_step if not k.startswith("apply")]
    build_kernel_ms = sum(per_step[k] for k in build_names)
    apply_ms_kernels = sum(v for k, v in per_step.items() if k.startswith("apply"))
    gbps = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9  # noqa: E731
    # HBM-side traffic from the committed PMC passes -- only if they were taken on THESE kernel sources
    traffic, traffic_ratio, pmc_note = None, None, None
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    pmc = None
    if os.path.exists(tpath):
        try:
            pmc = json.load(open(tpath))
            if pmc.get("_meta", {}).get("source_sha") != source_sha():
                pmc_note = "profiles/pmc_traffic.json belongs to other kernel sources: traffic not reported (re-run profiles/collect.sh)"
                pmc = None
        except Exception as e:  # noqa: BLE001
            pmc_note, pmc = repr(e), None
    else:
        pmc_note = "profiles/pmc_traffic.json missing"
    pmc_names = {"prepare_faces": "k_prepare_faces", "reduce_stats": "k_reduce_stats", "index_count": "k_spatial_count",
                 "index_scatter": "k_spatial_scatter", "search": "k_search", "search_big": "k_search_big",
                 "clip_tri": "k_clip_tri_queue", "clip_big": "k_clip_tri_queue", "assemble": "k_assemble",
                 "big_rank": "k_big_rank", "big_scan": "k_big_scan", "row_fill_long": "k_row_fill_long",
                 "place_big": "k_place_big", "publish": "k_publish_all", "scan_reduce": "k_scan_reduce",
                 "scan_apply": "k_scan_apply_fused", "apply_stream": "k_apply_stream", "apply_wave": "k_apply_wave",
                 "apply_long": "k_apply_long", "apply_rows1": "k_apply_rows1", "sample_stats": "k_sample_stats",
                 "prepare_stats": "k_prepare_faces"}
    if pmc:
        def per_step_bytes(name):
            e = pmc.get("k_clip_tri_queue@65536" if name == "clip_big" else pmc_names.get(name, name))
            return e["hbm_bytes_corrected"] * kernels[name][0] / args.steps if e else 0.0

        e = pmc.get(pmc_names.get(dominant, dominant))
        traffic = e["hbm_bytes_corrected"] if e else None
        build_traffic = sum(per_step_bytes(k) for k in build_names)
        traffic_ratio = build_traffic / ab["build"]
    # The clip is FP64 issue work: next to the HBM fraction the contract asks for, how close it runs to the VALU issue
    # limit (SQ_INSTS_VALU of the committed PMC pass; ~4 SIMD cycles per wave64 instruction, measured
    # SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU).
    valu = None
    ppath = os.path.join(ROOT, "profiles", "pmc_per_launch.json")
    if pmc and os.path.exists(ppath):
        try:
            ctr = json.load(open(ppath))["k_clip_tri_queue"]
            insts = ctr["SQ_INSTS_VALU"]
            floor_ms = insts * 4 / (256 * 4) / 2.4e9 * 1e3
            clip_ms = kernels["clip_tri"][1] if "clip_tri" in kernels else None
            valu = {"kernel": "clip_tri", "wave_instructions_per_launch": insts, "issue_floor_ms": floor_ms,
                    "frac_of_issue_limit": floor_ms / clip_ms if clip_ms else None, "source": "profiles/pmc_per_launch.json"}
            if all(k in ctr for k in ("SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_WAVES")) and ctr["SQ_WAVES"] > 0:
                # The persistent clip's waves live for the whole launch: SQ_WAVE_CYCLES (quad-cycles) / waves = the launch in
                # shader cycles, i.e. the clock the chip really ran this FP64-dense kernel at; the VALU pipes' busy cycles
                # per SIMD against that lifetime = how VALU-bound the kernel is, whatever the clock.
                life_cycles = 4.0 * ctr["SQ_WAVE_CYCLES"] / ctr["SQ_WAVES"]
                busy_cycles = 4.0 * ctr["SQ_ACTIVE_INST_VALU"] / (256 * 4)
                valu["valu_busy_frac"] = busy_cycles / life_cycles
                valu["wave_lifetime_cycles"] = life_cycles
                valu["effective_clock_ghz_under_pmc"] = life_cycles / (clip_ms * 1e-3) / 1e9 if clip_ms else None
                valu["note"] = ("frac_of_issue_limit prices the instructions at 2.4 GHz; valu_busy_frac = VALU-active cycles per SIMD / "
                                "wave lifetime is clock-independent: the kernel is VALU-bound (DESIGN section 5)")
        except Exception:
            valu = None
    km = kernel_model_bytes(S, T, Ns, Nt, C, P)
    roofline = {
        "bound": "hbm",
        "kernel": dominant,
        # algorithmic bytes of the whole weight build (93 B per target cell x the T cells one launch processes)
        # / the dominant kernel's average launch duration
        "achieved": gbps(ab["build"], dom_ms),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": gbps(ab["build"], dom_ms) / HBM_PEAK_GBS,
        "traffic": traffic,
        "traffic_ratio_build": traffic_ratio,
        "traffic_note": pmc_note,
        "algorithmic_bytes_per_launch": ab["build"],
        "avg_launch_ms": dom_ms,
        "figures": {
            "dominant_kernel": {"kernel": dominant, "bytes": ab["build"], "ms": dom_ms, "frac": gbps(ab["build"], dom_ms) / HBM_PEAK_GBS},
            "build": {"bytes": ab["build"], "kernel_ms_sum": build_kernel_ms, "wall_ms": build_ms,
                      "frac_of_kernel_sum": gbps(ab["build"], build_kernel_ms) / HBM_PEAK_GBS,
                      "frac_of_wall": gbps(ab["build"], build_ms) / HBM_PEAK_GBS,
                      "note": "kernel_ms_sum counts the side-stream kernels of the big faces although they overlap the main chain"},
            "apply_K1": {"bytes": ab["apply"], "kernel_ms_sum": apply_ms_kernels, "wall_ms": apply_ms,
                         "frac_of_wall": gbps(ab["apply"], apply_ms) / HBM_PEAK_GBS,
                         "back_to_back_ms": apply_async_ms, "frac_back_to_back": gbps(ab["apply"], apply_async_ms) / HBM_PEAK_GBS},
            "step": {"bytes": ab["step"], "ms": ms_per_step, "frac": gbps(ab["step"], ms_per_step) / HBM_PEAK_GBS},
        },
        "valu_issue": valu,
        "kernel_ms_per_step": {k: round(v, 4) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])},
        "kernel_model": {k: {"bytes": km[k], "frac": gbps(km[k], kernels[k][1]) / HBM_PEAK_GBS}
                         for k in km if k in kernels},
    }

    out_gpu = np.empty(T)
    _lib.check(lib.xr_dev_download(out_gpu.ctypes.data_as(ctypes.c_void_p), d_out, 8 * T))
    cpu = None
    if not args.no_cpu:
        cpu, out_cpu = cpu_baseline(sxy, sf, txy, tf, data)
        both = ~(np.isnan(out_gpu) & np.isnan(out_cpu))
        n_diff = int((out_gpu[both] != out_cpu[both]).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            max_rel = float(np.nanmax(np.abs(out_gpu[both] - out_cpu[both]) / np.abs(out_cpu[both]))) if both.any() else 0.0
        log(f"[bench] GPU vs CPU oracle: {n_diff} of {T} values differ, max rel {max_rel:.3g} "
            "(rows > 32 entries are reduced cooperatively in a fixed tree order; all others bit-identical)")
        cpu["gpu_values_differing"] = n_diff
        cpu["gpu_max_rel_diff"] = max_rel
    result["config"].update({
            "apply_only_ms": apply_ms,
            "apply_only_cells_per_s": T / (apply_ms * 1e-3),
            "apply_only_back_to_back_ms": apply_async_ms,
            "weights_only_ms": build_ms,
            "weights_only_cells_per_s": T / (build_ms * 1e-3),
            "host_to_host_ms": host_to_host_ms,
            "host_to_host_note": "mesh uploads (pageable host arrays; the int64 connectivity is narrowed to int32 while it is "
            "copied into the pinned staging buffers) + weights + apply + download of the result vector over PCIe, median of 5; "
            "not part of `value`",
            "api_ms": api_ms,
            "api_device_ms": api_device_ms,
            "api_device_phases_ms": api_device_phases,
            "api_device_note": "the same classes on HBM-resident arrays: Ugrid2d.from_device_arrays x 2 + OverlapRegridder + regrid(device "
                               "array) -> device array; weights + apply in one engine call; equal to the host-array result: "
                               + str(api_device_equal),
            "api_phases_ms": api_phases,
            "api_note": "xa.OverlapRegridder(xa.Ugrid2d(x, y, -1, faces), xa.Ugrid2d(...), method='mean').regrid(data): host arrays "
            "in, host result out, through the reference-shaped Python classes; median of 5 after a warm-up.  api_phases_ms "
            "(further passes with a synchronisation between the phases): grid wrappers / uploads / constructor = weights / "
            "regrid = apply + download.  (3.0-3.7 ms by run: the passes allocate ~150 MB of fresh numpy arrays "
            "whose first-touch page faults depend on the state of the process heap; a mallopt() that keeps released memory did not "
            "settle it)",
    })
    result["roofline"] = roofline
    result["cpu_baseline"] = cpu
    if not args.no_extras:
        result["other_configs"] = other_configs(E, lib, _lib, csr, S, T, ms, sxy, sf, delaunay=not args.no_delaunay,
                                                 target_centroids=mt.centroids())
    print(json.dumps(result), flush=True)


def other_configs(E, lib, _lib, csr, S, T, mesh, mesh_xy, src_faces=None, delaunay=True, target_centroids=None):
    """BASELINE configs 5 and 3, a structured pair and a network, measured beside the headline (rank 0, N = 1): informative
    extras of the JSON line, never part of `value`.  Bounded to a few seconds each."""
    import ctypes

    import numpy as np

    import xugrid_amd as xa
    from xugrid_amd.regrid.structured import Raster, StructuredGrid2d

    out = {}
    try:  # config 5: cached weights, K = 256 stacked variables
        K = 256
        # the C2 field with a phase shift per variable, v_k = sin(6 pi x + 2 pi k / K) cos(4 pi y) +
        # 0.1 N(0, 1) at the source centroids -- K DIFFERENT rows (no tiled block the caches could share)
        cen = mesh.centroids()
        rng5 = np.random.default_rng(5)
        src = np.empty((K, S))
        cy = np.cos(4 * np.pi * cen[:, 1])
        for k in range(K):
            src[k] = np.sin(6 * np.pi * cen[:, 0] + 2 * np.pi * k / K) * cy
            src[k] += 0.1 * rng5.standard_normal(S)
        del cy
        d_src, d_out = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(lib.xr_dev_alloc(8 * K * S, ctypes.byref(d_src)))
        _lib.check(lib.xr_dev_alloc(8 * K * T, ctypes.byref(d_out)))
        _lib.check(lib.xr_dev_upload(d_src, src.ctypes.data_as(ctypes.c_void_p), 8 * K * S))
        del src
        for _ in range(2):
            csr.apply_dev(d_src.value, E.XR_F64, K, d_out.value, 0)
        E.dev_sync()
        t0 = time.perf_counter()
        n = 5
        for _ in range(n):
            csr.apply_dev(d_src.value, E.XR_F64, K, d_out.value, 0)
        E.dev_sync()
        dt = (time.perf_counter() - t0) / n
        nbytes = 12 * csr.nnz + 4 * (T + 1) + 8 * K * (S + T)
        out["config5_apply_K256"] = {
            "weights": "the benchmark's own matrix (qhull-numbered Delaunay meshes: a compact block of target rows is many short "
            "runs of row ids, so gathers and output stores are less local than on a lattice-numbered pair, which runs at "
            "0.99 ms = 4.2 TB/s)",
            "ms": 1e3 * dt, "cell_variables_per_s": K * T / dt, "algorithmic_GBps": nbytes / dt / 1e9,
            "frac_of_hbm_peak": nbytes / dt / 1e9 / HBM_PEAK_GBS,
            "frac_of_achievable_6p3TBps": nbytes / dt / 1e9 / 6300.0,
        }
        # ... and with option apply_contract (fused multiply-adds + one reciprocal per row: NOT bit-identical, within (n + 2) ulp;
        # off by default -- DESIGN section 4)
        E.set_option("apply_contract", 1)
        for _ in range(2):
            csr.apply_dev(d_src.value, E.XR_F64, K, d_out.value, 0)
        E.dev_sync()
        t0 = time.perf_counter()
        for _ in range(n):
            csr.apply_dev(d_src.value, E.XR_F64, K, d_out.value, 0)
        E.dev_sync()
        dtc = (time.perf_counter() - t0) / n
        E.set_option("apply_contract", 0)
        out["config5_apply_K256"]["contracted_opt_in"] = {"ms": 1e3 * dtc, "frac_of_hbm_peak": nbytes / dtc / 1e9 / HBM_PEAK_GBS}
        # the same with the source cells renumbered along a Morton curve (xr_csr_set_col_keys): once with the caller's
        # block (a gather pass per apply puts it in the stored order), once with a block that already is in that order
        keys, key_range = E.morton_row_keys(mesh.centroids(), faces_per_tile=8)  # (fine keys: 1.70 -> 1.58 ms against tiles of 64)
        csr.set_col_keys(keys, key_range)
        for tag, permuted in (("caller_order_source", False), ("stored_order_source", True)):
            csr.expect_permuted(permuted)
            for _ in range(2):
                csr.apply_dev(d_src.value, E.XR_F64, K, d_out.value, 0)
            E.dev_sync()
            t0 = time.perf_counter()
            for _ in range(n):
                csr.apply_dev(d_src.value, E.XR_F64, K, d_out.value, 0)
            E.dev_sync()
            dt2 = (time.perf_counter() - t0) / n
            out["config5_apply_K256"]["morton_columns_" + tag] = {
                "ms": 1e3 * dt2, "algorithmic_GBps": nbytes / dt2 / 1e9, "frac_of_hbm_peak": nbytes / dt2 / 1e9 / HBM_PEAK_GBS}
        # ... and with BOTH sides in the engine's order: rows regrouped at the finest granularity (every row to its own Morton
        # tile: the output is delivered in stored order, so it no longer needs runs of consecutive caller ids), source
        # block in stored column order.  For data that lives on the device across many applies.
        rkeys, rrange = E.morton_row_keys(target_centroids, faces_per_tile=4)
        csr.set_row_keys(rkeys, rrange)
        csr.expect_permuted(True)
        csr.output_stored_order(True)
        for _ in range(2):
            csr.apply_dev(d_src.value, E.XR_F64, K, d_out.value, 0)
        E.dev_sync()
        t0 = time.perf_counter()
        for _ in range(n):
            csr.apply_dev(d_src.value, E.XR_F64, K, d_out.value, 0)
        E.dev_sync()
        dt3 = (time.perf_counter() - t0) / n
        out["config5_apply_K256"]["engine_order_in_and_out"] = {
            "ms": 1e3 * dt3, "algorithmic_GBps": nbytes / dt3 / 1e9, "frac_of_hbm_peak": nbytes / dt3 / 1e9 / HBM_PEAK_GBS,
            "note": "source block in the stored (Morton) column order, result in the stored (Morton-tiled) row order: "
                    "DeviceCSR.engine_order / xr_csr_set_row_keys + xr_csr_set_col_keys + xr_csr_expect_permuted + "
                    "xr_csr_output_stored_order"}
        csr.output_stored_order(False)
        csr.expect_permuted(False)
        lib.xr_dev_free(d_src)
        lib.xr_dev_free(d_out)
    except Exception as e:  # noqa: BLE001
        out["config5_apply_K256"] = {"error": repr(e)}
    try:  # config 3 as SURVEY 8(d) states it: source as C2 (the Delaunay mesh, seed 0), 4M query points = the face
        #       centroids of a 4M-face target of the same generator (2M points, seed 2, rotated 30 deg, scaled 0.7)
        if src_faces is None:
            sxy, sf = xa.meshgen.triangle_mesh(500_000, 0, delaunay=delaunay)
        else:
            sxy, sf = mesh_xy, src_faces
        t_gen = time.perf_counter()
        txy, tf = xa.meshgen.triangle_mesh(2_000_000, 2, 30.0, 0.7, delaunay=delaunay)
        t_gen = time.perf_counter() - t_gen
        src_g = xa.Ugrid2d(sxy[:, 0], sxy[:, 1], -1, sf)
        tgt_g = xa.Ugrid2d(txy[:, 0], txy[:, 1], -1, tf)
        src_g.device_mesh, tgt_g.device_mesh  # uploads are not part of the construction
        xa.BarycentricInterpolator(src_g, tgt_g)  # untimed: first-use allocations of this process

        def construct(fresh_source):
            if fresh_source:
                src_g._voronoi_device_cache = None  # first interpolator on this source: Voronoi pre-step included
            E.dev_sync()
            t0 = time.perf_counter()
            rg = xa.BarycentricInterpolator(src_g, tgt_g)
            E.dev_sync()
            return time.perf_counter() - t0, rg

        first = [construct(True)[0] for _ in range(5)]
        cached = [construct(False) for _ in range(5)]
        rg = cached[-1][1]
        cached = [c[0] for c in cached]
        with E.KernelTimer() as kt:
            construct(True)
        k3 = {k: t for k, (n, t) in kt.records.items()}  # ms per construction, per kernel name
        dominant3 = max(k3, key=k3.get)
        dom3_ms = k3[dominant3] / max(1, kt.records[dominant3][0])  # average launch duration of the dominant kernel
        nnz_b, n_pts, S3, Ns3 = rg._device_weights.nnz, tgt_g.n_face, src_g.n_face, sxy.shape[0]
        # B_bary = 16 n + 4 sum(M_v) + 16 N_vv + 4 sum(M_s) + 16 Ns + 16 nnz_b  with sum(M_v) ~ 3 S, N_vv ~ S
        b_bary = 16 * n_pts + 12 * S3 + 16 * S3 + 12 * S3 + 16 * Ns3 + 16 * nnz_b
        med_first, med_cached = float(np.median(first)), float(np.median(cached))
        # the centroid locator on the same pair: locate the 4M target centroids in the source + CSR of (row, face, 1.0)
        loc_ms = []
        for _ in range(5):
            E.dev_sync()
            t0 = time.perf_counter()
            loc = xa.CentroidLocatorRegridder(src_g, tgt_g)
            E.dev_sync()
            loc_ms.append(1e3 * (time.perf_counter() - t0))
        loc_nnz = loc._device_weights.nnz
        del loc
        out["config3_barycentric_1M_to_4M"] = {
            "workload": f"BASELINE config 3: {'Delaunay' if delaunay else 'lattice-split'} source S={S3} (seed 0) -> "
                        f"{n_pts} query points = centroids of a {'Delaunay' if delaunay else 'lattice-split'} target (2M points, "
                        "seed 2, rotated 30 deg, scaled 0.7), BarycentricInterpolator construction",
            "construct_ms": 1e3 * med_first, "construct_ms_min": 1e3 * min(first), "construct_ms_max": 1e3 * max(first),
            "construct_ms_voronoi_cached": 1e3 * med_cached,
            "target_points_per_s": n_pts / med_first, "nnz": nnz_b,
            "centroid_locator_construct_ms": float(np.median(loc_ms)), "centroid_locator_points_per_s": n_pts / (1e-3 * float(np.median(loc_ms))),
            "centroid_locator_nnz": loc_nnz,
            "roofline": {
                "bound": "hbm", "kernel": dominant3, "algorithmic_bytes": b_bary,
                "avg_launch_ms": dom3_ms, "launches": kt.records[dominant3][0],
                "achieved": b_bary / (dom3_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": b_bary / (dom3_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "frac_of_wall": b_bary / med_first / 1e9 / HBM_PEAK_GBS,
                "frac_of_wall_voronoi_cached": b_bary / med_cached / 1e9 / HBM_PEAK_GBS,
                "kernel_ms": {k: round(v, 4) for k, v in sorted(k3.items(), key=lambda kv: -kv[1])[:12]},
                "note": "B_bary of SURVEY 8(d) / the dominant kernel's duration (hipEvents, one construction); point location "
                        "is instruction- and latency-bound, the HBM fraction is reported because the contract asks for it",
            },
            "target_mesh_generation_s": t_gen,
            "note": "source and target meshes resident; construct_ms = median of 5 constructions on a source whose Voronoi "
            "tessellation is not cached (device pre-step + native O(boundary) part + xr_barycentric_csr); "
            "construct_ms_voronoi_cached = a further interpolator on the same source (the tessellation, its prepared "
            "arrays and its index are kept on the Ugrid2d, like its celltree).  In both figures the target's face centroids come "
            "from its mesh, where the untimed first construction left them (round 6; the reference caches Ugrid2d.centroids on the "
            "grid the same way): a target that has never been one pays 0.08 ms more",
        }
        del rg, src_g, tgt_g
    except Exception as e:  # noqa: BLE001
        out["config3_barycentric_1M_to_4M"] = {"error": repr(e)}
    try:  # structured pair: 4000^2 -> 4000^2 raster cells
        ns = nt = 4000
        src_r = Raster(x=np.arange(0.5, ns), y=np.arange(ns - 0.5, 0.0, -1.0))
        tgt_r = Raster(x=0.37 + 0.98 * (np.arange(nt) + 0.5), y=(0.21 + 0.98 * (np.arange(nt) + 0.5))[::-1].copy())
        s2, t2 = StructuredGrid2d(src_r), StructuredGrid2d(tgt_r)
        s2.overlap_device(t2, False)
        E.dev_sync()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            w = s2.overlap_device(t2, False)
            E.dev_sync()
            times.append(time.perf_counter() - t0)
        dt = min(times)
        d_src, d_out = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(lib.xr_dev_alloc(8 * s2.size, ctypes.byref(d_src)))
        _lib.check(lib.xr_dev_alloc(8 * t2.size, ctypes.byref(d_out)))
        field = np.random.default_rng(0).normal(size=s2.size)
        _lib.check(lib.xr_dev_upload(d_src, field.ctypes.data_as(ctypes.c_void_p), 8 * s2.size))
        for _ in range(3):
            w.apply_dev(d_src.value, 0, 1, d_out.value)
        E.dev_sync()
        t0 = time.perf_counter()
        for _ in range(10):
            w.apply_dev(d_src.value, 0, 1, d_out.value)
        E.dev_sync()
        t_apply = (time.perf_counter() - t0) / 10
        _lib.check(lib.xr_dev_free(d_src))
        _lib.check(lib.xr_dev_free(d_out))
        out["structured_4000x4000"] = {
            "weights_ms": 1e3 * dt, "apply_mean_ms": 1e3 * t_apply, "target_cells_per_s": t2.size / (dt + t_apply),
            "apply_GBps_of_data": 8.0 * (s2.size + t2.size) / t_apply / 1e9, "nnz": w.nnz,
            "note": "weights kept as their two per-axis factors (xr_outer); the apply forms the 64M products on the fly",
        }
    except Exception as e:  # noqa: BLE001
        out["structured_4000x4000"] = {"error": repr(e)}
    try:  # NetworkGridder weights: 1M network edges over the benchmark's source mesh
        rng = np.random.default_rng(7)
        n_edge = 1_000_000
        xy_lo, xy_hi = float(mesh_xy.min()), float(mesh_xy.max())
        a = rng.uniform(xy_lo, xy_hi, (n_edge, 2))
        ang = rng.uniform(0, 2 * np.pi, n_edge)
        length = rng.exponential(0.002 * (xy_hi - xy_lo), n_edge)
        edges = np.stack([a, a + length[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])], axis=1)
        E.edge_length_csr(mesh, edges)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            w = E.edge_length_csr(mesh, edges)
            E.dev_sync()
            times.append(time.perf_counter() - t0)
        # ... and the DEVICE part on its own (round 6): the end points already in HBM (xr_edge_length_csr_dev) -- no PCIe
        d_edges = E.DeviceArray.from_host(edges)
        E.edge_length_csr(mesh, d_edges)
        dev_times = []
        for _ in range(5):
            E.dev_sync()
            t0 = time.perf_counter()
            w_dev = E.edge_length_csr(mesh, d_edges)
            E.dev_sync()
            dev_times.append(time.perf_counter() - t0)
        assert w_dev.nnz == w.nnz
        del d_edges, w_dev
        # algorithmic bytes of the edge path, in the style of SURVEY 8(d): the edge coordinates once (32 B per edge), the mesh once
        # (int32 connectivity + f64 nodes), the CSR once (12 B per entry + row offsets over the faces)
        b_edges = 32 * n_edge + 4 * 3 * S + 16 * int(mesh_xy.shape[0]) + 12 * int(w.nnz) + 4 * (S + 1)
        t_dev = float(np.median(dev_times))
        out["network_gridder_1M_edges"] = {
            "weights_ms": 1e3 * min(times), "edges_per_s": n_edge / min(times), "nnz": w.nnz,
            "device_ms": 1e3 * t_dev, "device_edges_per_s": n_edge / t_dev,
            "roofline": {"bound": "hbm", "algorithmic_bytes": b_edges, "achieved_GBps": b_edges / t_dev / 1e9,
                         "frac_of_hbm_peak": b_edges / t_dev / 1e9 / HBM_PEAK_GBS,
                         "whole_call_GBps": b_edges / min(times) / 1e9,
                         "note": "achieved / frac: the DEVICE part (end points in HBM, xr_edge_length_csr_dev: index of the mesh "
                                 "cached; tile sort of the edges, walk -> flat candidate queue, one thread per candidate clips, "
                                 "scan, fill, row sort; one host read-back of the queue cursors and nnz); whole_call: incl. the "
                                 "32 MB host -> device copy of the edge coordinates (PCIe).  The device part gathers by position "
                                 "(8.5M candidates) and counts rows with device-scope atomics: not bandwidth-bound (round 5: "
                                 "1.57 ms)"},
            "note": "1M random segments (exponential lengths, mean ~2 cell sizes) over the ~1M-triangle source mesh; "
            "weights_ms includes the 32 MB upload of the edge coordinates, device_ms does not",
        }
    except Exception as e:  # noqa: BLE001
        out["network_gridder_1M_edges"] = {"error": repr(e)}
    # non-triangle pairs through the one-round-trip pipeline (round 5): BASELINE config 1's SHAPE at scale -- the 1M-triangle
    # benchmark source onto a 1000 x 1000 raster -- and a ~1M-face mixed triangle / quadrilateral mesh onto a rotated one
    for tag, make in (("tri_1M_to_raster_1000x1000", "raster"), ("mixed_1M_to_mixed_1M", "mixed")):
        try:
            if make == "raster":
                sxy2, sf2 = (mesh_xy, src_faces) if src_faces is not None else xa.meshgen.triangle_mesh(500_000, 0, delaunay=delaunay)
                lo, hi = float(mesh_xy.min()) + 0.02, float(mesh_xy.max()) - 0.02
                txy2, tf2 = xa.meshgen.quad_mesh(np.linspace(lo, hi, 1001), np.linspace(lo, hi, 1001))
            else:
                sxy2, sf2 = xa.meshgen.mixed_mesh(660_000, 0)
                txy2, tf2 = xa.meshgen.mixed_mesh(660_000, 1, 30.0, 0.7)
            ms2, mt2 = E.DeviceMesh(sxy2, sf2, -1), E.DeviceMesh(txy2, tf2, -1)
            w2 = ms2.overlap(mt2)
            E.dev_sync()
            times = []
            for _ in range(10):
                ms2.invalidate()
                mt2.invalidate()
                t0 = time.perf_counter()
                w2 = ms2.overlap(mt2)
                E.dev_sync()
                times.append(time.perf_counter() - t0)
            dt = float(np.median(times))
            C2, P2, S2, T2 = int(ms2.last_candidates()), int(w2.nnz), int(sf2.shape[0]), int(tf2.shape[0])
            nodes_s = int((np.asarray(sf2) >= 0).sum()) if sf2.shape[1] > 3 else 3 * S2
            nodes_t = int((np.asarray(tf2) >= 0).sum()) if tf2.shape[1] > 3 else 3 * T2
            b_build = 4 * (nodes_s + nodes_t) + 16 * (sxy2.shape[0] + txy2.shape[0]) + 12 * P2 + 4 * (T2 + 1)
            out[tag] = {
                "source_faces": S2, "target_faces": T2, "candidate_pairs": C2, "nnz": P2, "weights_ms": 1e3 * dt,
                "target_cells_per_s": T2 / dt, "ns_per_candidate_pair": 1e9 * dt / max(C2, 1) if C2 else None,
                "roofline": {"bound": "hbm", "algorithmic_bytes": b_build, "achieved_GBps_whole_build": b_build / dt / 1e9,
                             "frac_of_hbm_peak_whole_build": b_build / dt / 1e9 / HBM_PEAK_GBS,
                             "note": "B_build of SURVEY 8(d) over the WHOLE weight build (prepare x2, index, search, clip, assembly), "
                                     "not over its dominant kernel"},
                "note": "weights only, rebuilt from HBM-resident raw meshes (median of 10); the triangle pair of the headline "
                        "takes config.weights_only_ms for config.candidate_pairs pairs",
            }
            del ms2, mt2, w2
        except Exception as e:  # noqa: BLE001
            out[tag] = {"error": repr(e)}
    try:  # BASELINE config 1 as SURVEY 8(d) words it, through the public API (tests/test_gpu_regridder_api.py checks the values)
        g = np.load(os.path.join(ROOT, "tests", "golden", "g8_elevation_nl.npz"))
        node_x, node_y, faces1, elev = g["node_x"], g["node_y"], g["face_nodes"].astype(np.int64), g["elevation"]
        n1 = 200
        dx1, dy1 = (node_x.max() - node_x.min()) / n1, (node_y.max() - node_y.min()) / n1
        raster = Raster(x=node_x.min() + (np.arange(n1) + 0.5) * dx1, y=node_y.max() - (np.arange(n1) + 0.5) * dy1, dx=dx1, dy=-dy1)
        grid1 = xa.Ugrid2d(node_x, node_y, -1, faces1)
        t_con, t_reg = [], []
        for i in range(6):
            t0 = time.perf_counter()
            rg = xa.OverlapRegridder(xa.Ugrid2d(node_x, node_y, -1, faces1) if i else grid1, raster, method="mean")
            t1 = time.perf_counter()
            res = rg.regrid(elev)
            t2 = time.perf_counter()
            if i:  # (first pass = warm-up)
                t_con.append(t1 - t0)
                t_reg.append(t2 - t1)
        w1 = rg._ensure_host_weights()
        out["config1_elevation_nl_to_200x200"] = {
            "workload": "BASELINE config 1: elevation_nl Ugrid2d (5248 triangles, float32 elevation) -> 200 x 200 raster, x ascending, "
                        "y descending, OverlapRegridder mean, host arrays in and out through the public API (a fresh Ugrid2d per pass)",
            "construct_ms": 1e3 * float(np.median(t_con)), "regrid_ms": 1e3 * float(np.median(t_reg)),
            "target_cells_per_s": n1 * n1 / float(np.median(t_con) + np.median(t_reg)), "nnz": int(w1.nnz),
            "weight_sum_over_mesh_area": float(w1.data.sum() / 4.2169478944e10),
            "value_range": [float(np.nanmin(res)), float(np.nanmax(res))], "nan_cells": int(np.isnan(res).sum()),
            "note": "40,000 quadrilateral targets on 5,248 triangles: a problem this small is launch / host-latency bound; kept as "
                    "the plumbing check it is in BASELINE.json",
        }
    except Exception as e:  # noqa: BLE001
        out["config1_elevation_nl_to_200x200"] = {"error": repr(e)}
    return out


def free_port():
    import socket

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N` outside torch.distributed.run (no WORLD_SIZE in the environment): re-exec this very
    command line under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N` on a free local port, one rank per
    GPU.  Rank 0's JSON line passes through on stdout; the exit code is non-zero if any rank failed."""
    import subprocess

    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (the host driver only supports dmabuf IPC: RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={max(1, args.gpus)}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    log("[bench] launching", " ".join(cmd))
    return subprocess.call(cmd, env=env)


def make_backend(args, local_rank):
    """HipBackend (the product).  --compute-backend module:attr is a TEST hook: tests/test_distributed_cpu.py runs this
    file end to end on CPU (gloo, world size 2) with the oracle-backed stand-in that lives under tests/."""
    if args.compute_backend:
        import importlib

        mod, attr = args.compute_backend.split(":")
        return getattr(importlib.import_module(mod), attr)()
    from xugrid_amd.distributed import HipBackend

    return HipBackend(local_rank)


def run_multi(args):
    """One rank per GPU (RCCL).  Three workloads, all reported as whole-job throughput over max-over-ranks time:
      default    WEAK scaling of the headline: N tiles of BASELINE config 2 (N x 1M source and target triangles); a step
                 = weight build of the rank's shard + mean apply + the one exchange step
      --strong   STRONG scaling on BASELINE config 4: the fixed 10M -> 10M pair (--strong-points per mesh) sharded over
                 the N ranks, so that N = 8 IS config 4
      --k 256    BASELINE config 5 at N GPUs: cached sharded weights, K stacked variables; a step = the apply of the K
                 variables (partial states in tiles + the tile-pipelined exchange), no weight build
    The default invocation at N > 1 carries the other two as `other_configs` of the same JSON line (fewer steps), so that
    ONE run per N yields the three multi-GPU numbers of the north star.
    """
    import torch
    import torch.distributed as dist

    from xugrid_amd.distributed import init_process_group_from_env

    # RCCL prints a version banner to the C-level stdout when its first communicator comes up: everything but the ONE JSON line
    # goes to stderr (file descriptor 1 points at stderr for the whole run; the line is written to the saved descriptor)
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    dist_backend = args.dist_backend or ("nccl" if torch.cuda.is_available() else "gloo")
    init_process_group_from_env(dist_backend)
    rank, world = dist.get_rank(), dist.get_world_size()
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    backend = make_backend(args, local_rank)
    K = max(1, int(args.k))
    result = multi_workload(args, backend, strong=args.strong, K=K, steps=args.steps, warmup=args.warmup,
                            both_exchanges=True, setup_leg=True)
    if K == 1 and not args.strong and not args.no_extras and (world > 1 or args.multi_extras):
        few, few_w = max(1, min(args.steps, 10)), max(1, min(args.warmup, 3))
        others = {}
        for name, kw in (("config4_strong_10M", dict(strong=True, K=1)),
                         ("config5_apply_K%d" % args.extras_k, dict(strong=False, K=max(2, args.extras_k)))):
            try:
                others[name] = multi_workload(args, backend, steps=few, warmup=few_w, both_exchanges=False,
                                              setup_leg=False, **kw)
            except Exception as e:  # noqa: BLE001 -- (the headline line must survive a failing extra; all ranks see the same error)
                others[name] = {"error": repr(e)}
        if rank == 0:
            result["other_configs"] = others
    if rank == 0:
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(result) + "\n").encode())
    dist.barrier()
    dist.destroy_process_group()


def multi_workload(args, backend, strong, K, steps, warmup, both_exchanges, setup_leg):
    """One of the three multi-GPU workloads on the initialised process group -> the JSON object (rank 0; None elsewhere)."""
    import torch
    import torch.distributed as dist

    from xugrid_amd import meshgen
    from xugrid_amd.distributed import HipBackend, ShardedOverlapRegridder, TargetPartitionedRegridder

    rank, world = dist.get_rank(), dist.get_world_size()
    dev = getattr(backend, "device", None)
    on_gpu = dev is not None and dev.type == "cuda"
    dsync = torch.cuda.synchronize if on_gpu else (lambda: None)
    # Weak scaling: N tiles of the single-GPU benchmark pair (the same Delaunay meshes, hull slivers included, side by
    # side), N x 1M faces per mesh.  One qhull run serves any N; with --points > 600k (config 4's 10M faces on one box)
    # or --no-delaunay the lattice-split triangulation is used so that set-up stays within seconds.
    t_gen = time.perf_counter()
    if strong:
        sxy, sf, txy, tf = make_meshes(args.strong_points, delaunay=False)
        mesh_kind = "BASELINE config 4, fixed size (lattice-split triangulation)"
    elif args.no_delaunay or args.points > 600_000:
        sxy, sf, txy, tf = make_meshes(args.points * world, delaunay=False)
        mesh_kind = "lattice-split triangulation"
    else:
        sxy, sf, txy, tf = make_meshes(args.points, delaunay=True)
        sxy, sf = meshgen.tiled_mesh(sxy, sf, world)
        txy, tf = meshgen.tiled_mesh(txy, tf, world)
        mesh_kind = f"{world} tile(s) of the Delaunay benchmark pair"
    S, T = sf.shape[0], tf.shape[0]
    data = meshgen.smooth_field(sxy[sf].mean(axis=1), 0) if K == 1 else None
    t_gen = time.perf_counter() - t_gen

    def local_block(rg):
        """(K, S_local) source block of this rank on its device.  K > 1: SURVEY 8(d) config 5's field with a phase
        shift per variable, evaluated on the device at the centroids of the rank's own source faces (the global
        (K, S) block -- 2 GB per 1M faces -- is never built)."""
        if K == 1:
            return rg.local_source(data)
        cen = torch.as_tensor(sxy[sf[rg.local_faces]].mean(axis=1), device=dev)
        phase = 2.0 * np.pi * torch.arange(K, device=dev, dtype=torch.float64)[:, None] / K
        return (torch.sin(6.0 * np.pi * cen[None, :, 0] + phase) * torch.cos(4.0 * np.pi * cen[None, :, 1])).contiguous()

    # K > 1 (cached weights, many variables): by default the TARGETS are partitioned -- every rank owns a slice of the rows
    # with all their entries, applies with the single-GPU many-variable kernels and needs NO data-path collective (SURVEY
    # 8e "not shardable over sources": the same layout serves any reducer).  Sharding the SOURCES for an apply-only job
    # moves C x K x T partial states through the exchange, more bytes than the apply itself reads (--k-mode source keeps
    # that path measurable: one rank, K = 256: 19.7 ms per step against 1.8 ms).
    target_partitioned = K > 1 and args.k_mode == "target"

    def timed(fn, n):
        """n calls of fn bracketed by barrier + device synchronisation on both sides -> (max-over-ranks seconds, own seconds)"""
        dsync()
        dist.barrier()
        dsync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        dsync()
        mine = time.perf_counter() - t0  # this rank's own time to finish (before the closing barrier)
        dist.barrier()
        dsync()
        elapsed = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
        return float(elapsed.item()), mine

    def measure(exchange):
        dsync()
        t0 = time.perf_counter()
        if target_partitioned:
            rg = TargetPartitionedRegridder(sxy, sf, txy, tf, backend, method="mean")
        else:
            rg = ShardedOverlapRegridder(sxy, sf, txy, tf, backend, partition=args.partition, exchange=exchange,
                                         k_tile=args.k_tile, ownership=(args.ownership if exchange == "sparse" else None))
        dsync()
        setup_s = time.perf_counter() - t0
        local = local_block(rg)

        def step():
            if K == 1:
                return rg.rebuild_regrid_local(local)  # (weights + partial states: one engine call)
            return rg.regrid_local(local)

        for _ in range(warmup):
            step()
        elapsed, mine = timed(step, steps)
        # the exchange step by itself: the same steps again with device events around every collective (untimed leg)
        if target_partitioned or not on_gpu:
            exch_ms, n_coll = 0.0, 0
            eb = {"sent_off_gpu": 0} if target_partitioned else rg.exchange_bytes(K)
        else:
            rg.start_timing()
            for _ in range(steps):
                step()
            exch_ms, n_coll = rg.stop_timing()
            eb = rg.exchange_bytes(K)
        per_rank = torch.tensor([mine / steps * 1e3, exch_ms / steps, float(eb["sent_off_gpu"]),
                                 float(rg.local_faces.size), float(rg.local_targets.size), float(rg.weights.nnz)],
                                dtype=torch.float64, device=dev)
        gathered = [torch.empty_like(per_rank) for _ in range(world)]
        dist.all_gather(gathered, per_rank)
        table = torch.stack(gathered).cpu().numpy()
        stats = {
            "step_ms_per_rank": {"min": float(table[:, 0].min()), "max": float(table[:, 0].max()),
                                 "all": [round(float(v), 4) for v in table[:, 0]]},
            "exchange_ms": float(table[:, 1].max()),
            "exchange_ms_per_rank": {"min": float(table[:, 1].min()), "max": float(table[:, 1].max())},
            "collectives_per_step": n_coll / max(1, steps),
            "exchange_bytes_sent_per_rank": {"min": int(table[:, 2].min()), "max": int(table[:, 2].max()),
                                             "total": int(table[:, 2].sum())},
            "source_faces_per_rank": {"min": int(table[:, 3].min()), "max": int(table[:, 3].max())},
            "target_faces_per_rank": {"min": int(table[:, 4].min()), "max": int(table[:, 4].max())},
            "nnz": int(table[:, 5].sum()),
        }
        return rg, step, local, elapsed, stats, setup_s

    rg, step, local, elapsed, stats, setup_s = measure(args.exchange)
    other = "dense" if args.exchange == "sparse" else "sparse"
    if target_partitioned or not both_exchanges:
        elapsed_other, stats_other = None, None
    else:
        _, _, _, elapsed_other, stats_other, _ = measure(other)
    # Like for like with N = 1, whose step starts from the raw arrays of the whole mesh: here the raw arrays of the SHARD
    # have to be cut out of the replicated mesh first -- partition of the source faces, near-shard filter of the targets,
    # the shard's two mesh handles (device to device), the exchange lists -- all of it device code from HBM-resident
    # tensors (ShardedOverlapRegridder.setup).  A "step including set-up" = setup() [which builds the weights] + the apply
    # + the exchange; reported beside the headline, which keeps the partition across steps as a real job would.
    including = None
    if setup_leg and K == 1 and not target_partitioned:
        def full_step():
            rg.setup()
            return rg.regrid_local(local)

        full_step()
        n_full = max(1, min(steps, 10))
        el_full, _ = timed(full_step, n_full)
        ms_full = 1e3 * el_full / n_full
        including = {"ms_per_step_including_setup": ms_full,
                     "setup_ms_per_rebuild": ms_full - 1e3 * elapsed / steps,
                     "value_including_setup": T * K / (el_full / n_full), "steps": n_full,
                     "what": "partition of the source faces + near-shard target filter + the shard's mesh handles (device to "
                             "device) + exchange lists, redone every step from the HBM-resident replicated meshes, then "
                             "weight build + apply + exchange: what N = 1 counts from its raw arrays"}
    # rank 0's kernels of a few more steps (hipEvents around every launch): roofline of its dominant kernel
    roofline = None
    if on_gpu and isinstance(backend, HipBackend):
        from xugrid_amd import engine as E

        with E.KernelTimer() as kt:
            for _ in range(3):
                step()
        dist.barrier()
        if rank == 0:
            try:
                kernels = {k: (n, t / n) for k, (n, t) in kt.records.items()}
                per_step = {k: n * avg / 3 for k, (n, avg) in kernels.items()}
                side = {"search_big", "clip_big", "big_rank", "big_scan", "row_fill_long"}
                dominant = max((k for k in per_step if k not in side), key=per_step.get)
                s_loc, t_loc = rg.local_faces.size, rg.local_targets.size
                ab = algorithmic_bytes(s_loc, t_loc, sxy.shape[0] // world, txy.shape[0] // world, rg.weights.nnz, K=K)
                # K = 1: SURVEY 8(d) B_build of the rank's shard / its dominant kernel; K > 1 (cached weights): B_apply of the shard
                dom_bytes, dom_ms = (ab["build"] if K == 1 else ab["apply"]), kernels[dominant][1]
                launches = kernels[dominant][0] / 3
                achieved = dom_bytes / (dom_ms * launches * 1e-3) / 1e9 if dom_bytes else None
                roofline = {
                    "bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS if achieved else None, "traffic": None,
                    "algorithmic_bytes_per_step": dom_bytes, "avg_launch_ms": dom_ms, "launches_per_step": launches, "rank": 0,
                    "local_source_faces": int(s_loc), "local_target_faces": int(t_loc),
                    "kernel_ms_per_step": {k: round(v, 4) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])},
                }
            except Exception as e:  # noqa: BLE001
                roofline = {"error": repr(e)}
    del rg, step, local
    if rank != 0:
        return None
    exchange_name = {"sparse": "RCCL sparse all-to-all (the reduce-scatter restricted to the touched targets) of per-target partial sums",
                     "dense": "RCCL reduce-scatter of per-target partial sums"}
    units = T * K
    if K > 1:
        metric = f"target cell-variables regridded/s (cached OverlapRegridder weights, K={K} stacked variables, mean apply)"
        workload = (f"BASELINE config 5 at {world} GPU(s) ({mesh_kind}): {S} source -> {T} target triangles, cached weights, "
                    + (f"K={K} variables; target rows partitioned over the ranks (complete rows on their owner: no collective)"
                       if target_partitioned else f"source-sharded, K={K} variables exchanged in tiles of {args.k_tile}"))
        unit = "target cell-variables/s"
    elif strong:
        metric = "target cells regridded/s (OverlapRegridder 10M->10M tri, source faces sharded, weights + mean apply)"
        workload = (f"{mesh_kind}: {S} source -> {T} target triangles sharded over {world} GPU(s), "
                    "OverlapRegridder mean, K=1")
        unit = "target cells/s"
    else:
        metric = "target cells regridded/s (OverlapRegridder 1M->1M tri per GPU, weights + mean apply)"
        workload = (f"{world} x BASELINE config 2 ({mesh_kind}): {S} source -> {T} target triangles, "
                    "OverlapRegridder mean, K=1")
        unit = "target cells/s"
    config = {
        "workload": workload,
        "source_faces": S,
        "target_faces": T,
        "variables": K,
        "nnz": stats["nnz"],
        "parallelism": (f"target rows partitioned over {world} GPUs (contiguous slices + the source faces near them), "
                        "no data-path collective" if target_partitioned else
                        f"source faces sharded over {world} GPUs ({args.partition} blocks), target replicated, "
                        + exchange_name[args.exchange]),
        "rccl_ranks": world,
        "collective_backend": dist.get_backend(),
        "exchange": "none" if target_partitioned else args.exchange,
        "exchange_ms": stats["exchange_ms"],
        "exchange_ms_note": "device events around every collective of a step (behind the partial-state kernel that feeds "
        "it / behind the wait for it), max over ranks; measured on a further, untimed set of steps",
        "per_rank": stats,
        "setup_s_untimed": {"mesh_generation": t_gen, "partition_filter_first_build": setup_s,
                            "note": "first construction (host meshes uploaded once, first-use allocations, first weight "
                            "build, exchange lists); what it costs per rebuild from resident meshes is "
                            "`including_setup.setup_ms_per_rebuild`"},
    }
    if elapsed_other is not None:
        config["other_exchange"] = {"exchange": other, "ms_per_step": 1e3 * elapsed_other / steps,
                                    "value": units / (elapsed_other / steps), "what": exchange_name[other],
                                    "exchange_ms": stats_other["exchange_ms"],
                                    "exchange_bytes_sent_per_rank": stats_other["exchange_bytes_sent_per_rank"]}
    elif target_partitioned:
        config["other_exchange"] = {"exchange": "none", "exchange_ms": 0.0}
    if including is not None:
        config["including_setup"] = including
    return {
        "metric": metric,
        "value": units / (elapsed / steps),
        "unit": unit,
        "n_gpus": world,
        "steps": steps,
        "warmup": warmup,
        "ms_per_step": 1e3 * elapsed / steps,
        "higher_is_better": True,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": config,
        "roofline": roofline,
        "cpu_baseline": None,
    }


XGMI_LINK_GBS = 153.0   # per direct xGMI link and direction (7 links x ~153 GB/s per GPU)
EXCHANGE_LATENCY_MS = 0.03  # launch + hand-shake of one small all-to-all (assumption of the projection)


class ProjectionDist:
    """Stand-in for the few torch.distributed calls of ShardedOverlapRegridder, for ONE "rank" at a time on ONE GPU
    (`bench.py --project-shards W`): the exchange LISTS are the real ones (computed from all W shards beforehand), the
    data path of a collective is a device copy of the right shape -- its time is measured and taken out of the
    projection, which prices the exchange from the bytes and the xGMI link rate instead.  The set-up collectives are
    answered in the order ShardedOverlapRegridder issues them (`tables["setup"]`: one precomputed answer per call)."""

    class _Done:
        def wait(self):
            return True

    class ReduceOp:
        SUM, MAX = "sum", "max"

    def __init__(self, rank, world, tables):
        self.rank, self.world = rank, world
        self._answers = list(tables["setup"][rank])
        self._cycle = {}

    def get_rank(self, group=None):
        return self.rank

    def get_world_size(self, group=None):
        return self.world

    def get_backend(self, group=None):
        return "nccl"

    def barrier(self, group=None):
        pass

    def _next(self, kind):
        got_kind, value = self._answers.pop(0)
        assert got_kind == kind, f"projection stand-in: expected a {got_kind} call, ShardedOverlapRegridder issued {kind}"
        return value

    def all_to_all_single(self, output, input, output_split_sizes=None, input_split_sizes=None, group=None, async_op=False):
        import torch

        if input.dtype == torch.int64:                                     # set-up: counts, claims, owners, row ids
            output.copy_(self._next("a2a").to(output.device))
        else:                                                              # a step: rows of partial states (values: my own, cycled)
            n_out, n_in = output.shape[0], input.shape[0]
            if n_out and n_in:
                key = (n_out, n_in)
                if key not in self._cycle:
                    self._cycle[key] = torch.arange(n_out, device=output.device) % n_in
                torch.index_select(input, 0, self._cycle[key], out=output)
            elif n_out:
                output.zero_()
        return self._Done() if async_op else None

    def reduce_scatter_tensor(self, output, input, op="sum", group=None, async_op=False):
        output.copy_(input[self.rank])
        return self._Done() if async_op else None

    def all_gather(self, tensor_list, tensor, group=None):
        import torch

        if tensor.dtype == torch.int64 and self._answers:                  # set-up: every rank's owned rows
            for dst, src in zip(tensor_list, self._next("gather")):
                dst.copy_(src.to(dst.device))
            return
        for dst in tensor_list:
            dst.copy_(tensor)


def run_projection(args):
    """ONE GPU, W shards one after another: the real ShardedOverlapRegridder + HipBackend per shard (its own partition,
    near-shard filter, weight build, partial states, multi-sender combination with the real receive lists), collectives
    looped back.  Prints the per-shard table, the max / mean imbalance and a PROJECTED W-GPU step: max over shards of the
    measured compute time + an exchange time modelled from the bytes a rank sends to one peer over one xGMI link.
    Projected, not measured -- the multi-GPU curve itself is the driver's (bench.py --gpus N)."""
    import torch

    from xugrid_amd import engine as E, meshgen
    from xugrid_amd.distributed import HipBackend, ShardedOverlapRegridder, _t, shard_lists

    W = int(args.project_shards)
    backend = HipBackend(0)
    dev = backend.device
    t_gen = time.perf_counter()
    if args.strong:
        sxy, sf, txy, tf = make_meshes(args.strong_points, delaunay=False)
        mesh_kind = f"BASELINE config 4: fixed {sf.shape[0]} -> {tf.shape[0]} lattice-split triangles over {W} shards (strong)"
    elif args.no_delaunay or args.points > 600_000:
        sxy, sf, txy, tf = make_meshes(args.points * W, delaunay=False)
        mesh_kind = f"{W} x config-2 size, lattice-split triangulation (weak)"
    else:
        sxy, sf, txy, tf = make_meshes(args.points, delaunay=True)
        sxy, sf = meshgen.tiled_mesh(sxy, sf, W)
        txy, tf = meshgen.tiled_mesh(txy, tf, W)
        mesh_kind = f"{W} tiles of the Delaunay benchmark pair (weak)"
    t_gen = time.perf_counter() - t_gen
    S, T = sf.shape[0], tf.shape[0]
    data = meshgen.smooth_field(sxy[sf].mean(axis=1), 0)
    steps, warmup = max(1, min(args.steps, 20)), max(1, min(args.warmup, 5))

    def shard_tables(world, ownership):
        """The real exchange lists of all `world` shards, as the set-up collectives of ShardedOverlapRegridder would deliver
        them: per rank the answers in call order, and counts[s, o] = rows of sender s for owner o."""
        full = (_t(sxy, dev), _t(sf.astype(np.int64), dev), _t(txy, dev), _t(tf.astype(np.int64), dev))
        t_chunk = -(-T // world)
        lts = [shard_lists(full, world, r, args.partition, backend)[1] for r in range(world)]
        del full
        auth = [torch.div(lt, t_chunk, rounding_mode="floor") for lt in lts]
        claim_counts = torch.stack([torch.bincount(a, minlength=world) for a in auth]).cpu()  # [sender, authority]
        setup = [[] for _ in range(world)]
        if ownership == "partition":
            lowest = torch.full((T,), world, dtype=torch.int64, device=dev)
            for r in reversed(range(world)):
                lowest[lts[r]] = r
            claims_to = [list(torch.split(lt - a * t_chunk, [int(c) for c in claim_counts[r]])) for r, (lt, a) in enumerate(zip(lts, auth))]
            rows, owners = [], []
            for r in range(world):
                own = lowest[lts[r]]
                order = torch.argsort(own, stable=True)
                rows.append(lts[r][order])
                owners.append(own[order])
            owned = [rows[r][owners[r] == r] for r in range(world)]
            counts = torch.stack([torch.bincount(o, minlength=world) for o in owners]).cpu()    # [sender, owner]
            rows_to = [list(torch.split(rows[r], [int(c) for c in counts[r]])) for r in range(world)]
            pad = max(max(int(o.numel()) for o in owned), 1)
            padded = []
            for o in owned:
                p = torch.full((pad,), -1, dtype=torch.int64, device=dev)
                p[: o.numel()] = o
                padded.append(p)
            for r in range(world):
                setup[r] = [("a2a", claim_counts[:, r].clone()), ("a2a", torch.cat([claims_to[s][r] for s in range(world)])),
                            ("a2a", lowest[lts[r]]), ("a2a", counts[:, r].clone()),
                            ("a2a", torch.cat([rows_to[s][r] for s in range(world)])),
                            ("gather", [torch.tensor([int(o.numel())]) for o in owned]), ("gather", padded)]
            counts = counts.numpy()
        else:
            counts = claim_counts.numpy()
            ids_to = [list(torch.split(lt - a * t_chunk, [int(c) for c in claim_counts[r]])) for r, (lt, a) in enumerate(zip(lts, auth))]
            for r in range(world):
                setup[r] = [("a2a", claim_counts[:, r].clone()), ("a2a", torch.cat([ids_to[s][r] for s in range(world)]))]
        return counts, {"setup": setup}

    def run_shards(world):
        ownership = args.ownership or ("partition" if args.exchange == "sparse" and args.partition != "hash" else "chunk")
        counts, tables = shard_tables(world, ownership)
        rows = []
        for r in range(world):
            pd = ProjectionDist(r, world, tables)
            rg = ShardedOverlapRegridder(sxy, sf, txy, tf, backend, partition=args.partition, exchange=args.exchange,
                                         k_tile=args.k_tile, dist=pd, ownership=ownership)
            local = rg.local_source(data)

            def step():
                return rg.rebuild_regrid_local(local)

            for _ in range(warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            step_ms = 1e3 * (time.perf_counter() - t0) / steps
            rg.start_timing()
            for _ in range(steps):
                step()
            loop_ms, _ = rg.stop_timing()
            loop_ms /= steps
            with E.KernelTimer() as kt:
                for _ in range(3):
                    step()
            kms = {k: round(t / 3, 4) for k, (n, t) in kt.records.items()}
            C = backend.n_components(rg.method.method_id)
            sent = counts[r].copy()
            sent[r] = 0
            rows.append({
                "shard": r, "source_faces": int(rg.local_faces.size), "target_faces": int(rg.local_targets.size),
                "nnz": int(rg.weights.nnz), "step_ms": step_ms, "loopback_copy_ms": loop_ms, "compute_ms": step_ms - loop_ms,
                "rows_sent_off_gpu": int(sent.sum()), "bytes_sent_off_gpu": int(8 * C * sent.sum()),
                "bytes_to_busiest_peer": int(8 * C * sent.max()),
                "rows_received": int(counts[:, r].sum()),
                "side_chain_ms": round(sum(kms.get(k, 0.0) for k in ("search_big", "clip_big", "row_fill_long")), 4),
                "kernel_ms": dict(sorted(kms.items(), key=lambda kv: -kv[1])[:8]),
            })
            del rg, local, step
            log(f"[project] W={world} shard {r}: step {step_ms:.3f} ms (loop-back copy {loop_ms:.3f}), "
                f"S_loc {rows[-1]['source_faces']} T_loc {rows[-1]['target_faces']} nnz {rows[-1]['nnz']}")
        comp = np.array([x["compute_ms"] for x in rows])
        exch_ms = max(x["bytes_to_busiest_peer"] for x in rows) / (XGMI_LINK_GBS * 1e9) * 1e3 + (EXCHANGE_LATENCY_MS if world > 1 else 0.0)
        return rows, comp, exch_ms

    rows, comp, exch_ms = run_shards(W)
    projected_ms = float(comp.max() + exch_ms)
    # the 1-GPU point of the same curve through the same code (one shard = the whole problem of ONE GPU's share)
    if args.strong:
        base_rows, base_comp, _ = run_shards(1)
        base_ms, base_cells = float(base_comp.max()), T
    else:  # weak: one tile on one GPU
        keep = (sxy, sf, txy, tf, data, S, T)
        if args.no_delaunay or args.points > 600_000:
            sxy, sf, txy, tf = make_meshes(args.points, delaunay=False)
        else:
            sxy, sf, txy, tf = make_meshes(args.points, delaunay=True)
        S, T = sf.shape[0], tf.shape[0]
        data = meshgen.smooth_field(sxy[sf].mean(axis=1), 0)
        base_rows, base_comp, _ = run_shards(1)
        base_ms, base_cells = float(base_comp.max()), T
        sxy, sf, txy, tf, data, S, T = keep
    value_1 = base_cells / (base_ms * 1e-3)
    value_w = T / (projected_ms * 1e-3)
    out = {
        "what": "PROJECTED, NOT MEASURED: W shards of the multi-GPU workload run one after another on ONE MI355X (real "
                "ShardedOverlapRegridder + HipBackend per shard, collectives looped back); projected step = max over shards of "
                "the measured compute time + modelled exchange",
        "workload": mesh_kind, "shards": W, "partition": args.partition, "exchange": args.exchange,
        "ownership": args.ownership or ("partition" if args.exchange == "sparse" and args.partition != "hash" else "chunk"),
        "source_faces": S, "target_faces": T, "steps": steps, "warmup": warmup,
        "per_shard": rows,
        "imbalance_max_over_mean": float(comp.max() / comp.mean()),
        "compute_ms": {"max": float(comp.max()), "mean": float(comp.mean()), "min": float(comp.min())},
        "modelled_exchange_ms": exch_ms,
        "exchange_model": f"bytes a rank sends to its busiest peer / {XGMI_LINK_GBS} GB/s (one direct xGMI link per peer, all "
                          f"links in parallel) + {EXCHANGE_LATENCY_MS} ms latency; no overlap with compute assumed",
        "projected_step_ms": projected_ms, "projected_value_cells_per_s": value_w,
        "one_gpu_step_ms_same_code": base_ms, "one_gpu_value_cells_per_s": value_1,
        "projected_speedup_1_to_W": value_w / value_1,
        "projected_efficiency_1_to_W": value_w / value_1 / W,
        "scaling": "strong" if args.strong else "weak",
        "mesh_generation_s": t_gen,
    }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--points", type=int, default=500_000, help="lattice points per mesh and per GPU (faces ~ 2x)")
    ap.add_argument("--no-delaunay", action="store_true", help="lattice-split triangulation instead of qhull")
    ap.add_argument("--full", action="store_true",
                    help="N = 1: after the headline also measure everything else the line reports (apply-only, weights-only, "
                    "host-array and public-API passes, per-kernel roofline, the CPU oracle baseline and its comparison, "
                    "other_configs); without it the run times the step and prints the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="N = 1: write what the last timed step computed (regridded field, weight matrix) as DIR/<name>.npy")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--no-extras", action="store_true", help="skip the informative extras (--full at N = 1: configs 3 and 5, "
                    "structured pair; N > 1: the config-4 and config-5 workloads)")
    ap.add_argument("--step-only", action="store_true", help="--full: skip the passes from host arrays (host_to_host_ms, api_ms): "
                    "every launch of the process then belongs to the step's loops (profiler runs)")
    ap.add_argument("--partition", default="balanced", choices=["balanced", "morton", "hash"],
                    help="source shards: Morton blocks of equal estimated work (default) / equal face counts, or id mod N")
    ap.add_argument("--exchange", default="sparse", choices=["sparse", "dense"],
                    help="sparse all-to-all of the touched targets (default) or dense reduce-scatter")
    ap.add_argument("--ownership", default=None, choices=["partition", "chunk"],
                    help="sparse exchange: who finalises a target row -- the lowest rank whose shard touches it (default for the "
                    "spatial partitions: only the boundary layer leaves a GPU) or its id chunk")
    ap.add_argument("--force-dist", action="store_true", help="run the multi-GPU code path even with one rank")
    ap.add_argument("--strong", action="store_true",
                    help="multi-GPU: strong scaling on BASELINE config 4 (a fixed 10M -> 10M pair sharded over the ranks)")
    ap.add_argument("--strong-points", type=int, default=5_000_000, help="lattice points per mesh of the --strong pair")
    ap.add_argument("--k", type=int, default=1,
                    help="multi-GPU: K > 1 = BASELINE config 5 at N GPUs (cached sharded weights, K stacked variables per step)")
    ap.add_argument("--k-tile", type=int, default=32, help="variables per collective of the K-tiled exchange")
    ap.add_argument("--k-mode", default="target", choices=["target", "source"],
                    help="K > 1: partition the target rows (no collective; default) or shard the source faces (exchange of partial states)")
    ap.add_argument("--multi-extras", action="store_true",
                    help="multi-GPU path with ONE rank: also run the config-4 strong and config-5 K=256 workloads as "
                    "`other_configs` (done by default when N > 1)")
    ap.add_argument("--extras-k", type=int, default=256, help="stacked variables of the config-5 extra of the multi-GPU line")
    ap.add_argument("--project-shards", type=int, default=0,
                    help="ONE GPU: run each of W shards of the multi-GPU workload one after another (real sharded regridder, "
                    "looped-back collectives) and print the per-shard table + a projected W-GPU step -- projected, not measured")
    ap.add_argument("--dist-backend", default=None, choices=["nccl", "gloo"], help=argparse.SUPPRESS)
    ap.add_argument("--compute-backend", default=None, help=argparse.SUPPRESS)  # test hook: module:attr of a backend class
    args = ap.parse_args()
    in_group = "WORLD_SIZE" in os.environ and "RANK" in os.environ
    if args.dump_outputs and (args.project_shards > 1 or args.gpus > 1 or args.force_dist
                              or (in_group and int(os.environ["WORLD_SIZE"]) > 1)):
        ap.error("--dump-outputs writes the outputs of the one-GPU step only")
    if args.project_shards > 1:
        run_projection(args)
    elif (args.gpus > 1 or args.force_dist) and not in_group:
        sys.exit(self_launch(args))
    elif in_group and (args.gpus > 1 or args.force_dist or int(os.environ["WORLD_SIZE"]) > 1):
        run_multi(args)
    else:
        run_single(args)


if __name__ == "__main__":
    main()

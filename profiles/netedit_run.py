"""The network edits (Ugrid1d.topology_subset, merge_partitions, refine_by_vertices) on two networks of 1M edges -- a lattice-like
net and a set of long chains: topology_subset of half the edges, a merge of 8 overlapping partitions, refine_by_vertices with
1M vertices.  Each as the whole public call (host grids in, a host grid out: uploads, downloads and the Ugrid1d constructor
included) and as the device part alone (arrays already in HBM, the C entry point), beside the numpy restatement of
tests/netedit_cases.py on the same input (this process's CPUs).  The restatement of the refinement is given the located edges:
its own search is all pairs.  hipEvent timing (torch.cuda.Event), 2 warm-ups, 5 repeats, median.
`python profiles/netedit_run.py [out.json] [edges]`"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch initialises its HIP runtime before the engine binds the device
import netedit_cases as nc
import xugrid_amd as xa
from xugrid_amd import engine, netedit

out_path = sys.argv[1] if len(sys.argv) > 1 else "netedit_run.json"
n_edge_wanted = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
N_PART, OVERLAP = 8, 1000


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def host_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), out


def merge_numpy(parts):
    """partitioning.py:81-116, :137-148 with np.unique, as the reference does it (no NaN here)."""
    node_off = np.cumsum([0] + [len(xy) for xy, _ in parts])
    all_xy = np.concatenate([xy for xy, _ in parts])
    _, index, inverse = np.unique(all_xy, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(index), dtype=np.int64)
    rank[np.argsort(index)] = np.arange(len(index))
    inverse = rank[inverse.ravel()]
    index.sort()
    gathered = np.concatenate([inverse[e + off] for (_, e), off in zip(parts, node_off)])
    _, first = np.unique(np.sort(gathered, axis=1), axis=0, return_index=True)
    first.sort()
    return all_xy[index], gathered[first]


def lattice(n_edge):
    """The lattice of profiles/netfill_run.py: a square lattice of streets, nodes jittered; horizontal edges row by row, then the
    vertical ones."""
    m = int(round((1 + np.sqrt(1 + 2 * n_edge)) / 2))
    rng = np.random.default_rng(0)
    y, x = np.divmod(np.arange(m * m), m)
    xy = np.column_stack([x, y]) + rng.uniform(-0.2, 0.2, (m * m, 2))
    ids = np.arange(m * m).reshape(m, m)
    edges = np.concatenate([np.column_stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()]),
                            np.column_stack([ids[:-1].ravel(), ids[1:].ravel()])])
    return xy, edges.astype(np.int64)


def chains(n_edge, length=10_000):
    """The chains of profiles/netfill_run.py: `length` edges each, nodes numbered along the chains, irregular spacing."""
    n_chain = max(n_edge // length, 1)
    rng = np.random.default_rng(1)
    x = np.cumsum(rng.uniform(0.5, 1.5, (n_chain, length + 1)), axis=1)
    xy = np.column_stack([x.ravel(), np.repeat(np.arange(n_chain) * 10.0, length + 1)])
    ids = np.arange(n_chain * (length + 1)).reshape(n_chain, length + 1)
    return xy, np.column_stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()]).astype(np.int64)


def same(grid, xy, edges):
    return bool(np.array_equal(grid.node_coordinates.view(np.uint64), np.ascontiguousarray(xy).view(np.uint64))
                and np.array_equal(grid.edge_node_connectivity, edges))


res = {"n_part": N_PART, "overlap_edges": OVERLAP}
for name, make in (("lattice", lattice), ("chains", chains)):
    xy, edges = make(n_edge_wanted)
    grid = xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, edges)
    n = grid.n_edge
    rng = np.random.default_rng(5)
    r = {"n_node": grid.n_node, "n_edge": n}
    args = netedit._network_args(grid)  # (uploads the grid's arrays once)

    # topology_subset of half the edges, in random order
    index = rng.permutation(n)[: n // 2].astype(np.int64)
    d_index = engine.DeviceArray.from_host(index)
    r["subset_call_ms"] = timed(lambda: grid.topology_subset(index))
    r["subset_device_ms"] = timed(lambda: engine.DeviceNetEdit.subset(*args, d_index.ptr, index.size))
    r["subset_numpy_ms"], want = host_ms(lambda: nc.subset_ref(xy, edges, index))
    r["subset_equal"] = same(grid.topology_subset(index), want[0], want[1])

    # merge of N_PART overlapping partitions (consecutive blocks of edges, OVERLAP edges shared with the block before)
    cuts = np.linspace(0, n, N_PART + 1).astype(np.int64)
    parts = [nc.subset_ref(xy, edges, np.arange(max(cuts[p] - (OVERLAP if p else 0), 0), cuts[p + 1]))[:2] for p in range(N_PART)]
    grids = [xa.Ugrid1d(p_xy[:, 0], p_xy[:, 1], -1, p_edges) for p_xy, p_edges in parts]
    p_args = [netedit._network_args(g) for g in grids]
    cols = [[a[k] for a in p_args] for k in range(4)]
    r["merge_call_ms"] = timed(lambda: xa.merge_partitions(grids))
    r["merge_device_ms"] = timed(lambda: engine.DeviceNetEdit.merge(*cols))
    r["merge_numpy_ms"], want = host_ms(lambda: merge_numpy(parts))
    r["merge_equal"] = same(xa.merge_partitions(grids), want[0], want[1])
    del grids, p_args, cols

    # refine_by_vertices: 1M vertices, each on a random edge between a quarter and three quarters of its length
    on = rng.integers(0, n, n_edge_wanted)
    t = rng.uniform(0.25, 0.75, n_edge_wanted)[:, None]
    a, b = xy[edges[on, 0]], xy[edges[on, 1]]
    vertices = np.ascontiguousarray(a + t * (b - a))
    d_vertices = engine.DeviceArray.from_host(vertices)
    tolerance = netedit.default_tolerance(grid)
    r["refine_vertices"], r["refine_tolerance"] = len(vertices), tolerance
    r["refine_call_ms"] = timed(lambda: grid.refine_by_vertices(vertices))
    r["refine_device_ms"] = timed(lambda: engine.DeviceNetEdit.refine(*args, d_vertices.ptr, len(vertices), tolerance))
    r["refine_numpy_without_search_ms"], want = host_ms(lambda: nc.refine_ref(xy, edges, vertices, tolerance, edge_index=on))
    refined, node_index = grid.refine_by_vertices(vertices, return_index=True)
    r["refine_equal"] = same(refined, want["xy"], want["edges"]) and bool(np.array_equal(node_index, want["node_index"]))
    r["refine_longest_row"] = int(np.bincount(on).max())
    res[name] = r
    print(name, json.dumps(r), flush=True)
    grid.drop_device_caches()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)

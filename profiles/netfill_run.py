"""The network fill (Ugrid1d.interpolate_na(metric="network")) on two networks of 1M edges -- a lattice-like net and a set of
long chains -- with 10 % of the edge values missing in runs of consecutive edges: the device graph build, the fill at K = 1
and K = 16, the round count, beside the host reference on the same input (scipy's graph build plus its multi-source
dijkstra, one slice, this process's CPUs).  hipEvent timing (torch.cuda.Event), 2 warm-ups, 5 repeats.
`python profiles/netfill_run.py [out.json] [edges]`"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch initialises its HIP runtime before the engine binds the device
from scipy import sparse
from scipy.sparse.csgraph import dijkstra
import xugrid_amd as xa
from xugrid_amd import fill

out_path = sys.argv[1] if len(sys.argv) > 1 else "netfill_run.json"
n_edge_wanted = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
RUN = 200  # consecutive edges per gap


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def lattice(n_edge):
    """A square lattice of streets, nodes jittered (no two path lengths tie): horizontal edges row by row, then the vertical ones."""
    m = int(round((1 + np.sqrt(1 + 2 * n_edge)) / 2))
    rng = np.random.default_rng(0)
    y, x = np.divmod(np.arange(m * m), m)
    xy = np.column_stack([x, y]) + rng.uniform(-0.2, 0.2, (m * m, 2))
    ids = np.arange(m * m).reshape(m, m)
    edges = np.concatenate([np.column_stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()]),
                            np.column_stack([ids[:-1].ravel(), ids[1:].ravel()])])
    return xy, edges.astype(np.int64)


def chains(n_edge, length=10_000):
    """Chains of `length` edges each, nodes numbered along the chains, irregular spacing."""
    n_chain = max(n_edge // length, 1)
    rng = np.random.default_rng(1)
    x = np.cumsum(rng.uniform(0.5, 1.5, (n_chain, length + 1)), axis=1)
    xy = np.column_stack([x.ravel(), np.repeat(np.arange(n_chain) * 10.0, length + 1)])
    ids = np.arange(n_chain * (length + 1)).reshape(n_chain, length + 1)
    return xy, np.column_stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()]).astype(np.int64)


def with_gaps(n, seed):
    """Values on the edges, 10 % missing: one run of RUN consecutive edges out of every 10 RUN, at a random offset."""
    rng = np.random.default_rng(seed)
    data = 1000.0 + np.arange(n, dtype=np.float64)
    for start in range(0, n - 10 * RUN, 10 * RUN):
        at = start + int(rng.integers(0, 9 * RUN))
        data[at:at + RUN] = np.nan
    return data


res = {"run_length": RUN}
for name, make in (("lattice", lattice), ("chains", chains)):
    xy, edges = make(n_edge_wanted)
    grid = xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, edges)
    n = grid.n_edge
    data = with_gaps(n, 2)
    r = {"n_node": grid.n_node, "n_edge": n, "nan_fraction": float(np.isnan(data).mean())}

    # device: the graph (upload of the node and edge tables included), then the fill on tensors
    r["device_graph_build_ms"] = timed(lambda: fill.DeviceGraph.network(xy, edges, "edge"))
    graph = fill.network_graph(grid, "edge")
    r["graph_nnz"] = graph.nnz
    t1 = torch.tensor(data, device="cuda")
    out = grid.interpolate_na(t1, metric="network")
    r["rounds"] = int(fill.last_rounds)
    r["device_fill_ms_K1"] = timed(lambda: grid.interpolate_na(t1, metric="network"))
    t16 = torch.stack([torch.tensor(with_gaps(n, 2 + k), device="cuda") for k in range(16)])
    grid.interpolate_na(t16, metric="network")
    r["rounds_K16"] = int(fill.last_rounds)
    r["device_fill_ms_K16"] = timed(lambda: grid.interpolate_na(t16, metric="network"))
    r["device_fill_ms_K1_host_arrays"] = timed(lambda: grid.interpolate_na(data, metric="network"))

    # host: the reference's steps with scipy on the same input
    t0 = time.perf_counter()
    coo = grid.edge_edge_connectivity.tocoo()
    length = grid.edge_length
    host_graph = sparse.csr_matrix((0.5 * (length[coo.row] + length[coo.col]), (coo.row, coo.col)), shape=(n, n))
    r["host_graph_build_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    isnull = np.isnan(data)
    _, _, index = dijkstra(csgraph=host_graph, indices=np.flatnonzero(~isnull), return_predecessors=True, limit=np.inf, min_only=True)
    expected = data.copy()
    expected[index != -9999] = data[index[index != -9999]]
    r["host_dijkstra_fill_ms_K1"] = 1e3 * (time.perf_counter() - t0)
    r["equal_to_host"] = bool(np.array_equal(out.cpu().numpy(), expected, equal_nan=True))
    res[name] = r
    print(name, json.dumps(r), flush=True)
    grid.drop_device_caches()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)

"""
GPU (-m gpu): the int32 exclusive scan behind every row pointer of the library (csrc/xr_scan.hip: exclusive_scan_i32), at its
tile edges and on both of its paths -- reduce + fused apply up to ``scan_fused_tiles`` tiles of 2048 elements (8192 by default:
n <= 16 777 216), reduce + single-block scan of the tile sums + apply above.

The scan is driven through ``DeviceCSR.from_triplet``, which scans ``bincount(row)`` over the n rows into ``indptr`` and hands
all n + 1 values back verbatim; the yardstick is numpy's int64 cumulative sum and every comparison is ``np.array_equal``.
Each case also asserts WHICH path ran, from the launch counts of the library's kernel timer: ``scan_partials`` has one launch
on the three-kernel path and none on the fused one.
"""
import numpy as np
import pytest

import graph_cases as gc
from sample_cases import brute_nearest
from xugrid_amd import engine, meshgen, sample

pytestmark = pytest.mark.gpu

TILE = 2048          # SCAN_TILE: 256 threads x 8 elements
FUSED_TILES = 8192   # SCAN_FUSED_TILES: the built-in limit of the fused pair
HEAVY = 3001         # entries of the one heavy row
N_COL = 7

FUSED, THREE, NONE = "fused", "three kernels", "no scan kernel"
_LAUNCHES = {
    FUSED: {"scan_reduce": 1, "scan_apply": 1},
    THREE: {"scan_reduce": 1, "scan_partials": 1, "scan_apply": 1},
    NONE: {},  # n = 0: out[0] by fill_i32
}


def count_patterns(n, seed):
    """name -> int64 counts per row: every pattern the length allows (nnz stays below 2.5 n + HEAVY)."""
    rng = np.random.default_rng(seed)
    out = {"nnz0": np.zeros(n, dtype=np.int64)}
    if n == 0:
        return out
    out["ones"] = np.ones(n, dtype=np.int64)
    counts = rng.integers(0, 6, n)
    counts[rng.permutation(n)[: (n + 1) // 2]] = 0  # at least half the rows are empty
    out["random"] = counts
    for r in sorted({0, TILE - 1, TILE, n - 1}):
        if r < n:
            counts = rng.integers(0, 2, n)
            counts[r] = HEAVY
            out[f"heavy{r}"] = counts
    out["last_only"] = np.zeros(n, dtype=np.int64)
    out["last_only"][-1] = 777
    return out


def scan_through_csr(counts):
    """counts -> (indptr as downloaded, scan launches by kernel name); the entries' columns and values must come back as
    they went in and nnz must be the scan's total."""
    n = len(counts)
    row = np.repeat(np.arange(n, dtype=np.int64), counts)
    col = np.arange(row.size, dtype=np.int64) % N_COL
    data = np.arange(row.size, dtype=np.float64) + 0.5
    with engine.KernelTimer() as timer:
        csr = engine.DeviceCSR.from_triplet(row, col, data, n, N_COL)
    launches = {k: v[0] for k, v in timer.records.items() if k.startswith("scan_")}
    got_data, got_indices, indptr = csr.download()
    expected = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n), dtype=np.int64)])
    assert indptr.shape == (n + 1,)
    bad = np.nonzero(indptr != expected)[0]
    assert np.array_equal(indptr, expected), (
        f"n = {n}: {bad.size} of {n + 1} values differ, first at {bad[:3]}: got {indptr[bad[:3]]}, expected {expected[bad[:3]]}")
    assert csr.nnz == indptr[-1] == row.size
    assert np.array_equal(got_indices, col) and np.array_equal(got_data.view(np.int64), data.view(np.int64))
    return indptr, launches


def check_length(n, path, seed=0):
    for name, counts in count_patterns(n, seed + n).items():
        indptr, launches = scan_through_csr(counts)
        assert launches == _LAUNCHES[path], f"n = {n}, {name}: expected {path}, the timer saw {launches}"
        if name == "ones":
            assert np.array_equal(indptr, np.arange(n + 1))


# ---- the fused pair, default option -------------------------------------------------------------------------------------------
FUSED_LENGTHS = (
    [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257]                                   # below one block's 2048
    + [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 5]  # around tile ends
    + [256 * TILE - 1, 256 * TILE, 256 * TILE + 1, 257 * TILE + 1]              # the offset loop's second trip begins
    + [600 * TILE + 777]                                                         # ragged, third trip
)


@pytest.mark.parametrize("n", FUSED_LENGTHS)
def test_fused_path_lengths(hip, n):
    assert engine.get_option("scan_fused_tiles") == 0
    check_length(n, NONE if n == 0 else FUSED)


# ---- the three-kernel path, forced with scan_fused_tiles = 1 -------------------------------------------------------------------
THREE_TILES = [2, 3, 255, 256, 257, 512, 513]  # 257 and 513: the carry of k_scan_partials crosses an iteration of 256 partials
# last tile full, of one element, and of 2041 .. 2047 elements (one n per residue mod 8)
THREE_LENGTHS = [(nb - 1) * TILE + last for nb in THREE_TILES for last in [TILE, 1] + list(range(2041, 2048))]


@pytest.mark.parametrize("n", THREE_LENGTHS)
def test_three_kernel_path_lengths(hip, xr_option, n):
    xr_option("scan_fused_tiles", 1)
    check_length(n, THREE)


def test_one_tile_stays_fused_under_the_smallest_limit(hip, xr_option):
    xr_option("scan_fused_tiles", 1)
    for n in (1, TILE - 1, TILE):
        check_length(n, FUSED)
    check_length(0, NONE)


# ---- the switch itself --------------------------------------------------------------------------------------------------------
def test_switch_follows_the_option(hip, xr_option):
    xr_option("scan_fused_tiles", 4)
    check_length(4 * TILE, FUSED)
    check_length(4 * TILE + 1, THREE)
    check_length(5 * TILE, THREE)
    xr_option("scan_fused_tiles", None)
    check_length(5 * TILE, FUSED)


@pytest.mark.parametrize("n, path", [(FUSED_TILES * TILE, FUSED), (FUSED_TILES * TILE + 1, THREE)])
def test_switch_at_the_built_in_limit(hip, n, path):
    """The one true-size case: 8192 tiles are fused, one element more takes three kernels (default option).  About 2M random
    entries plus forced ones in row 0, in the last row of tile 8192 and in row n - 1; 134 MB of indptr come back."""
    assert engine.get_option("scan_fused_tiles") == 0
    rng = np.random.default_rng(n)
    counts = np.bincount(rng.integers(0, n, 2_000_000), minlength=n)
    counts[0] += 3
    counts[FUSED_TILES * TILE - 1] += 5
    counts[n - 1] += 7
    _, launches = scan_through_csr(counts)
    assert launches == _LAUNCHES[path], f"n = {n}: expected {path}, the timer saw {launches}"


# ---- no consumer's result depends on the option ---------------------------------------------------------------------------------
def with_and_without_fused(xr_option, build):
    """build() once with scan_fused_tiles = 1 and once with the default -> the two results; the first run must have gone
    through k_scan_partials, the second must not."""
    results = []
    for tiles in (1, None):
        xr_option("scan_fused_tiles", tiles)
        with engine.KernelTimer() as timer:
            results.append(build())
        partials = timer.records.get("scan_partials", (0, 0.0))[0]
        assert (partials >= 1) if tiles == 1 else (partials == 0), (tiles, timer.records)
    return results


def test_overlap_general_chain_does_not_depend_on_the_option(hip, xr_option):
    """xr_overlap through the general chain: the scan of the rows' survivor counts sends nnz and the clip-overflow word to the
    host in one mailbox round trip -- on the three-kernel path from k_scan_partials."""
    xr_option("overlap_fused", 0)
    sxy, sf = meshgen.triangle_mesh(3000, 11)
    txy, tf = meshgen.triangle_mesh(3600, 12, 25.0, 0.8)
    assert tf.shape[0] > 3 * TILE

    def build():
        csr = engine.DeviceMesh(sxy, sf, -1).overlap(engine.DeviceMesh(txy, tf, -1), False)
        data, indices, indptr = csr.download()
        assert csr.n == tf.shape[0] and csr.nnz == indptr[-1] == indices.size > csr.n
        return indptr, indices, data.view(np.int64), np.int64(csr.nnz)

    forced, default = with_and_without_fused(xr_option, build)
    for a, b in zip(forced, default):
        assert np.array_equal(a, b)


def topology_arrays(topology):
    ff, nn = topology.face_face_connectivity, topology.node_node_connectivity
    return [np.int64(topology.n_edge), topology.edge_node_connectivity, topology.face_edge_connectivity,
            topology.edge_face_connectivity, ff.indptr, ff.indices, ff.data, nn.indptr, nn.indices, nn.data,
            np.int64(topology.n_exterior_edge), topology.exterior_edges, topology.exterior_faces]


def test_topology_does_not_depend_on_the_option(hip, xr_option):
    """node -> face table, node_node and face_face rows and the lexicographic edge ids (xr_topology.hip): four scans over the
    ~20k nodes and ~40k faces of a randomly numbered mesh."""
    xy, faces = gc.topology_mesh("permuted40k")
    assert len(xy) > 3 * TILE
    forced, default = with_and_without_fused(xr_option, lambda: topology_arrays(gc.device_grid(xy, faces).device_topology()))
    for a, b in zip(forced, default):
        assert np.array_equal(a, b)
    host = gc.host_topology(faces, len(xy))
    assert np.array_equal(default[1], host["edge_node"]) and np.array_equal(default[4], host["face_face"].indptr)


def test_nearest_index_does_not_depend_on_the_option(hip, xr_option):
    """The cell starts of an xr_nn index over ~10 000 cells and the cell starts of its sorted queries."""
    rng = np.random.default_rng(12)
    points = rng.random((20_000, 2))
    queries = rng.uniform(-0.1, 1.1, (30_000, 2))
    queries[::97] = np.nan
    xr_option("nn_query_sort", 1)

    def build():
        index = sample.NearestIndex.from_points(points)
        assert index.n_cell > TILE
        return index.query(queries), index.query(queries, 0.01)

    forced, default = with_and_without_fused(xr_option, build)
    for a, b in zip(forced, default):
        assert np.array_equal(a, b)
    head = slice(0, 300)  # (the yardstick is a host loop: kept short)
    assert np.array_equal(default[0][head], brute_nearest(points, queries[head]))
    assert np.array_equal(default[1][head], brute_nearest(points, queries[head], 0.01))

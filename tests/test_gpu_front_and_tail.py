"""
GPU (-m gpu): the front of a fused weight build in one launch, behind the run-time option ``front_fused`` so that both forms
run in one process: the tree's sampled statistics (k_sample_stats, from 131072 faces on) lead the query's k_prepare_faces
grid (mesh_prepare_pair); every pair that does not qualify takes the two launches.

Every comparison is byte for byte: the CSR (indptr, indices, data, row_order) with the option at 1 against the option at 0,
and against the CPU oracle's pairs and areas.  Which form ran is read from the kernel timer's launch names.

(The second half of the file's name: the mailbox leaving through place_big's last block was built with this, passed the same
kind of tests, lost its A/B and is not in the library -- DESIGN 5.3, profiles/r08_experiments/.)
"""
import ctypes

import numpy as np
import pytest

from conftest import same_or_nan
from xugrid_amd import meshgen

pytestmark = pytest.mark.gpu

SAMPLE_MIN_FACES = 131072  # xr_mesh_front.hip: smaller trees take the full statistics pass
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def front_source():
    """~140k Delaunay triangles; trees are its first F faces (all nodes kept)."""
    return cached("front_source", lambda: meshgen.triangle_mesh(70_000, 0))


def front_query():
    """~140k triangles, rotated and shrunk into the source's interior; queries are its first T faces."""
    return cached("front_query", lambda: meshgen.triangle_mesh(70_000, 1, 30.0, 0.6))


def lattice_query():
    """~80k lattice-split triangles inside the source (rows of a few entries): a coherent numbering, which the engine keeps (no `order_scatter`), so
    that the stored row order is specified"""
    return cached("lattice_query", lambda: meshgen.triangle_mesh(40_000, 4, 30.0, 0.6, delaunay=False))


def oracle_tree(oracle, key, xy, faces):
    return cached(("tree", key), lambda: oracle.CellTree2d(xy, faces, -1))


def oracle_pairs(oracle, key, sxy, sf, txy, tf):
    """(target, source, area) of the oracle, computed once per pair of meshes and never modified."""

    def make():
        out = oracle_tree(oracle, key[0], sxy, sf).intersect_faces(txy, tf, -1)
        for a in out:
            a.setflags(write=False)
        return out

    return cached(("pairs",) + tuple(key), make)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def build(hip, sxy, sf, txy, tf, same_handle=False):
    """-> ((indptr, indices, data, row_order), launches by kernel name) of one weight build on fresh handles."""
    E = hip.engine
    ms = E.DeviceMesh(sxy, sf)
    mt = ms if same_handle else E.DeviceMesh(txy, tf)
    with E.KernelTimer() as timer:
        csr = ms.overlap(mt)
    data, indices, indptr = csr.download()
    launches = {k: v[0] for k, v in timer.records.items() if v[0]}
    return (indptr, indices, data, csr.row_order()), launches


def assert_same_csr(a, b, tag, query_sorted):
    """a == b, byte for byte.  `query_sorted`: the build launched `order_scatter`, i.e. the engine sorted the query itself (a
    numbering that is not spatially coherent, such as the first faces of a Delaunay mesh).  Inside a cell of that sort the
    order follows the atomics (xr_mesh_order.hip: "unspecified"), so the stored row order differs from build to build of ONE
    form; what is left to ask of it then is that it is a permutation of the rows -- the matrix in the caller's numbering is
    compared all the same."""
    for name, x, y in zip(("indptr", "indices", "data"), a, b):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (tag, name)
    if query_sorted:
        for csr in (a, b):
            assert np.array_equal(np.sort(csr[3]), np.arange(csr[3].size)), (tag, "row_order is no permutation")
    else:
        assert np.array_equal(a[3], b[3]), (tag, "row_order")


def assert_oracle(csr, pairs, tag):
    indptr, indices, data, _ = csr
    oq, os_, oa = pairs
    assert np.array_equal(np.repeat(np.arange(indptr.size - 1), np.diff(indptr)), oq), (tag, "target indices differ")
    assert np.array_equal(indices, os_), (tag, "source indices differ")
    assert np.array_equal(bits(data), bits(oa)), (tag, "areas not bit-exact")


def both_forms(hip, xr_option, option, sxy, sf, txy, tf, **kw):
    """the same build with `option` at 1 and at 0 -> {1: (csr, launches), 0: (csr, launches)}; equal CSRs asserted"""
    out = {}
    for value in (1, 0):
        xr_option(option, value)
        out[value] = build(hip, sxy, sf, txy, tf, **kw)
    xr_option(option, None)
    assert ("order_scatter" in out[1][1]) == ("order_scatter" in out[0][1])
    assert_same_csr(out[1][0], out[0][0], option, "order_scatter" in out[1][1])
    return out


class DeviceBlocks:
    """a (K, S) source block on the device and room for (K, T) results, through the C ABI's raw allocations"""

    def __init__(self, v, T):
        from xugrid_amd import _lib

        self._lib, self.lib = _lib, _lib.load()
        self.v, self.K, self.T = np.ascontiguousarray(v), v.shape[0], T

    def __enter__(self):
        src, out = ctypes.c_void_p(), ctypes.c_void_p()
        self._lib.check(self.lib.xr_dev_alloc(self.v.nbytes, ctypes.byref(src)))
        self._lib.check(self.lib.xr_dev_alloc(8 * self.K * self.T, ctypes.byref(out)))
        self._lib.check(self.lib.xr_dev_upload(src, self.v.ctypes.data_as(ctypes.c_void_p), self.v.nbytes))
        self._src, self._out = src, out
        self.src, self.out = src.value, out.value
        return self

    def fetch(self):
        out = np.empty((self.K, self.T))
        self._lib.check(self.lib.xr_dev_download(out.ctypes.data_as(ctypes.c_void_p), self._out, out.nbytes))
        return out

    def __exit__(self, *exc):
        self.lib.xr_dev_free(self._src)
        self.lib.xr_dev_free(self._out)


def front_launches(launches):
    return {k: launches.get(k, 0) for k in ("sample_stats", "prepare_stats", "prepare_faces")}


ONE_LAUNCH = {"sample_stats": 0, "prepare_stats": 0, "prepare_faces": 1}
TWO_SAMPLED = {"sample_stats": 1, "prepare_stats": 0, "prepare_faces": 1}
TWO_FULL = {"sample_stats": 0, "prepare_stats": 1, "prepare_faces": 1}


# ---- front ------------------------------------------------------------------------------------------------------------------
# F = 131072: 512 blocks of faces, 64 of them sampled -- the smallest tree that samples.  F + 1: a 65th sampled block that holds
# one face.  Queries of 1 .. 257 faces: one and two prepare_faces blocks behind the sampling blocks, full and partial; the whole
# query mesh: more prepare_faces blocks (~547) than sampling blocks.
@pytest.mark.parametrize("n_tree", [SAMPLE_MIN_FACES, SAMPLE_MIN_FACES + 1])
@pytest.mark.parametrize("n_query", [1, 255, 256, 257, None])
def test_front_one_launch_equals_two(hip, oracle, xr_option, n_tree, n_query):
    sxy, sf_all = front_source()
    txy, tf_all = front_query()
    assert sf_all.shape[0] > SAMPLE_MIN_FACES + 1 and tf_all.shape[0] > 8 * 256 * 64
    sf, tf = sf_all[:n_tree], tf_all[:n_query]
    got = both_forms(hip, xr_option, "front_fused", sxy, sf, txy, tf)
    assert front_launches(got[1][1]) == ONE_LAUNCH, got[1][1]
    assert front_launches(got[0][1]) == TWO_SAMPLED, got[0][1]
    assert_oracle(got[1][0], oracle_pairs(oracle, (n_tree, n_query), sxy, sf, txy, tf), (n_tree, n_query))


def test_front_tree_below_the_sampling_limit_takes_two_launches(hip, oracle, xr_option):
    sxy, sf_all = front_source()
    txy, tf_all = front_query()
    sf, tf = sf_all[: SAMPLE_MIN_FACES - 1], tf_all[:257]
    got = both_forms(hip, xr_option, "front_fused", sxy, sf, txy, tf)
    assert front_launches(got[1][1]) == TWO_FULL and front_launches(got[0][1]) == TWO_FULL, got[1][1]
    assert_oracle(got[1][0], oracle_pairs(oracle, (SAMPLE_MIN_FACES - 1, 257), sxy, sf, txy, tf), "below the limit")


def test_front_same_handle_as_tree_and_query_falls_back(hip, oracle, xr_option):
    sxy, sf_all = front_source()
    sf = sf_all[:SAMPLE_MIN_FACES]
    got = both_forms(hip, xr_option, "front_fused", sxy, sf, sxy, sf, same_handle=True)
    assert front_launches(got[1][1]) == TWO_SAMPLED, got[1][1]
    assert_oracle(got[1][0], oracle_pairs(oracle, (SAMPLE_MIN_FACES, "self"), sxy, sf, sxy, sf), "same handle")


@pytest.mark.parametrize("prepared", ["tree", "query"])
def test_front_one_side_already_prepared_falls_back(hip, oracle, xr_option, prepared):
    """One of the two meshes keeps its preparation from an earlier build: the other one is prepared alone."""
    E = hip.engine
    sxy, sf_all = front_source()
    txy, tf = lattice_query()
    sf = sf_all[:SAMPLE_MIN_FACES]
    oxy, of = meshgen.triangle_mesh(300, 7)  # the partner of the earlier build
    results = []
    for value in (1, 0):
        xr_option("front_fused", value)
        ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
        if prepared == "tree":
            ms.overlap(E.DeviceMesh(oxy, of))
        else:
            E.DeviceMesh(oxy, of).overlap(mt)
        with E.KernelTimer() as timer:
            csr = ms.overlap(mt)
        launches = front_launches({k: v[0] for k, v in timer.records.items()})
        expected = {"sample_stats": 0 if prepared == "tree" else 1, "prepare_stats": 0, "prepare_faces": 1 if prepared == "tree" else 0}
        assert launches == expected, (prepared, value, launches)
        assert timer.records.get("order_scatter", (0, 0.0))[0] == 0
        data, indices, indptr = csr.download()
        results.append((indptr, indices, data, csr.row_order()))
    xr_option("front_fused", None)
    assert_same_csr(results[0], results[1], prepared, query_sorted=False)
    assert_oracle(results[0], oracle_pairs(oracle, (SAMPLE_MIN_FACES, "lattice"), sxy, sf, txy, tf), prepared)


def test_front_three_builds_in_a_row_without_synchronisation(hip, oracle, xr_option):
    """The benchmark's pattern: both meshes invalidated and the weights rebuilt, asynchronously, three times with no
    synchronisation in between -- the tail's sequence word and arrival counters must be right on every pass."""
    E = hip.engine
    sxy, sf_all = front_source()
    txy, tf = lattice_query()
    sf = sf_all[: SAMPLE_MIN_FACES + 1]
    S, T = sf.shape[0], tf.shape[0]
    v = np.random.default_rng(3).normal(size=(1, S))
    pairs = oracle_pairs(oracle, (SAMPLE_MIN_FACES + 1, "lattice"), sxy, sf, txy, tf)
    with DeviceBlocks(v, T) as dev:
        results = []
        for value in (1, 0):
            xr_option("front_fused", value)
            ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
            kept = []
            E.set_async(True)
            try:
                with E.KernelTimer() as timer:
                    for _ in range(3):
                        ms.invalidate()
                        mt.invalidate()
                        kept.append(ms.overlap_apply_dev(mt, dev.src, E.XR_F64, 1, dev.out, 0))
                    E.dev_sync()
            finally:
                E.set_async(False)
            launches = front_launches({k: v_[0] for k, v_ in timer.records.items()})
            assert launches == ({"sample_stats": 0, "prepare_stats": 0, "prepare_faces": 3} if value else
                                {"sample_stats": 3, "prepare_stats": 0, "prepare_faces": 3}), launches
            assert timer.records.get("order_scatter", (0, 0.0))[0] == 0
            out = dev.fetch()
            csrs = []
            for csr in kept:
                data, indices, indptr = csr.download()
                csrs.append((indptr, indices, data, csr.row_order()))
                assert_oracle(csrs[-1], pairs, ("pass", len(csrs), value))
            assert same_or_nan(out, kept[-1].apply(v, 0)).all()
            results.append((csrs[-1], out))
        xr_option("front_fused", None)
    assert_same_csr(results[0][0], results[1][0], "async", query_sorted=False)
    assert np.array_equal(bits(results[0][1]), bits(results[1][1]))


def test_front_quadrilateral_query_on_triangle_tree(hip, oracle, xr_option):
    sxy, sf_all = front_source()
    sf = sf_all[:SAMPLE_MIN_FACES]
    txy, tf = meshgen.quad_mesh(np.linspace(0.11, 0.87, 58), np.linspace(0.13, 0.9, 41))
    got = both_forms(hip, xr_option, "front_fused", sxy, sf, txy, tf)
    assert front_launches(got[1][1]) == ONE_LAUNCH, got[1][1]
    assert_oracle(got[1][0], oracle_pairs(oracle, (SAMPLE_MIN_FACES, "quads"), sxy, sf, txy, tf), "quads")

"""
GPU (-m gpu): the per-run survivor count of the clip kernels (xr_prims.h: wave_run_add) at the edges of a wave.

Every clip kernel ends by adding, per run of pairs with the same target face, the pairs with a positive area to the face's
row count (per block of 256 target faces in the persistent clip of the one-round-trip chain).  A run may start at lane 0,
end at lane 63 or continue in the next wave; a wave may be full, partly filled or hold a single run.  A query mesh that grows
face by face against a small tree walks the number of candidate pairs from a few to several hundred -- across one wave (64)
and two (128) -- through both chains and every clip kernel a dense pair can take; a hexagon query takes the generic clip.
Each matrix is compared with the oracle's as test_gpu_parity.test_overlap_triangles_delaunay does: target and source indices
and the areas bit for bit, rows ascending by source index.
"""
import numpy as np
import pytest

from xugrid_amd import meshgen

pytestmark = pytest.mark.gpu

SWEEP = range(1, 41)  # faces of the query mesh


def first_faces(xy, faces, k):
    """The first k faces of a mesh as a mesh of their own (nodes renumbered, none unused)."""
    f = np.asarray(faces)[:k]
    used, inverse = np.unique(f, return_inverse=True)
    return np.ascontiguousarray(xy[used]), np.ascontiguousarray(inverse.reshape(f.shape).astype(np.int64))


def hexagon_mesh(nx, ny, x0, y0, r):
    """nx x ny regular hexagons of circumradius r, counter-clockwise, every one with six nodes of its own."""
    corner = np.deg2rad(60.0 * np.arange(6))
    xy = []
    for j in range(ny):
        for i in range(nx):
            cx, cy = x0 + 1.5 * r * i, y0 + np.sqrt(3.0) * r * (j + 0.5 * (i % 2))
            xy.append(np.column_stack([cx + r * np.cos(corner), cy + r * np.sin(corner)]))
    xy = np.concatenate(xy)
    return np.ascontiguousarray(xy), np.arange(xy.shape[0], dtype=np.int64).reshape(-1, 6)


@pytest.fixture(scope="module")
def tree(hip, oracle):
    """A Delaunay tree of about 200 faces: (coordinates, faces, the oracle's tree, the device mesh)."""
    sxy, sf = meshgen.triangle_mesh(121, 0)
    assert 180 <= sf.shape[0] <= 260
    return sxy, sf, oracle.CellTree2d(sxy, sf, -1), hip.engine.DeviceMesh(sxy, sf, -1)


def assert_parity(hip, tree, txy, tf):
    """The device matrix of (tree, query) against the oracle's; -> the candidate pairs the device clipped."""
    sxy, sf, otree, dev_tree = tree
    oq, os_, oa = otree.intersect_faces(txy, tf, -1)
    csr = dev_tree.overlap(hip.engine.DeviceMesh(txy, tf, -1))
    data, idx, indptr = csr.download()
    q = np.repeat(np.arange(csr.n), np.diff(indptr))
    assert csr.n == tf.shape[0] and csr.m == sf.shape[0]
    assert np.array_equal(q, oq), "target indices differ"
    assert np.array_equal(idx, os_), "source indices differ"
    assert np.array_equal(data, oa), "areas not bit-exact"
    for t in np.nonzero(np.diff(indptr) > 1)[0]:
        assert (np.diff(idx[indptr[t]:indptr[t + 1]]) > 0).all()
    n_cand = dev_tree.last_candidates()
    assert n_cand >= oq.size
    return n_cand


def assert_meets_wave_edges(candidates):
    """The sweep has clipped less than one wave of pairs, between one and two, and more than two."""
    c = np.asarray(candidates)
    assert (c < 64).any() and ((c > 64) & (c < 128)).any() and (c > 128).any(), sorted(set(candidates))


def sweep(hip, tree, xr_option, txy, tf, settings):
    for options in settings:
        for name, value in options.items():
            xr_option(name, value)
        assert_meets_wave_edges([assert_parity(hip, tree, *first_faces(txy, tf, k)) for k in SWEEP])


def test_triangle_queries_across_wave_edges(hip, tree, xr_option):
    """clip_tri of both chains: the persistent k_clip_tri_queue (counts per block of target faces) and k_clip_tri<., 3>."""
    txy, tf = meshgen.triangle_mesh(36, 1, 30.0, 0.7)
    assert tf.shape[0] >= SWEEP[-1]
    sweep(hip, tree, xr_option, txy, tf, [{"overlap_fused": 1}, {"overlap_fused": 0}])


def test_quadrilateral_queries_across_wave_edges(hip, tree, xr_option):
    """Quadrilateral targets: the slot-loop clip inside the persistent kernel, k_clip_tri<., 4> and k_clip_small."""
    txy, tf = meshgen.quad_mesh(np.linspace(0.12, 0.88, 9), np.linspace(0.15, 0.85, 6))
    assert tf.shape[0] >= SWEEP[-1]
    sweep(hip, tree, xr_option, txy, tf,
          [{"overlap_fused": 1}, {"overlap_fused": 0, "clip_quad": 1}, {"overlap_fused": 0, "clip_quad": 0}])


def test_hexagon_query_through_the_generic_clip(hip, tree):
    """Six nodes per target face: k_clip (clip_v16), whose rows' runs of candidates are longer than a dense pair's."""
    txy, tf = hexagon_mesh(4, 3, 0.2, 0.2, 0.1)
    assert assert_parity(hip, tree, txy, tf) > 128

"""
GPU (-m gpu): dense meshes (at most four nodes per face) keep no float64 box array; the overlap kernels take a face's box from its
vertices (query_face_box, xugrid_amd/csrc/xr_geom.h) -- the one-thread search, the block-per-face search, the tile keys of the
assembly, and the query-order copy of an incoherently numbered target.  Every case: the weight matrix (ids and areas) bit for bit
the oracle's, absolute and relative.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_apply_equal, assert_overlap_parity
from xugrid_amd import meshgen

pytestmark = pytest.mark.gpu


def parity(hip, oracle, sxy, sf, txy, tf, **kw):
    """-> (candidates, nnz)"""
    assert_overlap_parity(hip, oracle, sxy, sf, txy, tf, relative=True, **kw)
    csr, _ = assert_overlap_parity(hip, oracle, sxy, sf, txy, tf, **kw)
    # (the tree mesh of that call is gone: the count comes from a build of its own)
    ms, mt = hip.engine.DeviceMesh(sxy, sf, kw.get("fill", -1)), hip.engine.DeviceMesh(txy, tf, kw.get("fill", -1))
    nnz = ms.overlap(mt, False).nnz
    assert nnz == csr.nnz
    return int(ms.last_candidates()), int(nnz)


def lattice_mesh(m):
    points, m = meshgen.jittered_lattice_points(m * m, 0, jitter=0.0)
    return points, meshgen._split_lattice(points, m)


def test_mesh_against_itself_and_shifted_by_a_node_spacing(hip, oracle):
    """A lattice-split mesh (2048 faces, spacing 1/32: every coordinate exact), against itself and against a copy shifted by exactly
    one node spacing: the neighbours' boxes touch exactly, so a box that came out one ulp different would show as a pair too many or
    too few.  Also at UTM-sized coordinates."""
    xy, faces = lattice_mesh(33)
    assert faces.shape[0] == 2048
    cand, nnz = parity(hip, oracle, xy, faces, xy, faces)
    assert nnz == faces.shape[0] and nnz <= cand
    for shift in ((1.0 / 32, 0.0), (0.0, 1.0 / 32), (1.0 / 32, -1.0 / 32)):
        parity(hip, oracle, xy, faces, xy + np.array(shift), faces)
    off = np.array([5.0e5, 6.0e6])  # spacing 32: still exact
    parity(hip, oracle, xy * 1024 + off, faces, xy * 1024 + off + np.array([32.0, 0.0]), faces)


def test_clockwise_faces_fill_values_and_zero_area_targets(hip, oracle):
    """A triangle source under quadrilateral and mixed targets (the box comes from 3 or 4 vertices by the face's length; the fill slot
    is never read), clockwise faces on both sides (the stored vertex order is reversed: the same minimum and maximum), and a triangle
    target with two zero-area triangles."""
    sxy, sf = meshgen.triangle_mesh(800, 2)
    qxy, qf = meshgen.quad_mesh(np.linspace(0.05, 0.95, 23), np.linspace(0.1, 0.9, 17))
    mxy, mf = meshgen.mixed_mesh(700, 3, 20.0, 0.8)
    assert (mf[:, 3] >= 0).any() and (mf[:, 3] < 0).any()
    parity(hip, oracle, sxy, sf[:, ::-1].copy(), qxy, qf[:, ::-1].copy())
    parity(hip, oracle, sxy, sf, mxy, mf)
    mf_cw = mf.copy()
    mf_cw[mf[:, 3] >= 0] = mf[mf[:, 3] >= 0][:, ::-1]
    mf_cw[mf[:, 3] < 0, :3] = mf[mf[:, 3] < 0][:, 2::-1]
    parity(hip, oracle, sxy, sf, mxy, mf_cw)
    # triangle target, every face clockwise, + a collinear triangle and one with a repeated node in the middle of the source
    txy, tf = meshgen.triangle_mesh(700, 4, 40.0, 0.75)
    n0 = txy.shape[0]
    txy = np.vstack([txy, [[0.30, 0.30], [0.40, 0.35], [0.50, 0.40]]])
    tf = np.vstack([tf[:, ::-1], [[n0, n0 + 1, n0 + 2], [n0, n0 + 2, n0 + 2]]])
    parity(hip, oracle, sxy, sf, txy, tf)


def test_shuffled_target_numbering(hip, oracle):
    """A shuffled target numbering: the engine sorts the target into its query order, whose arrays carry no box either (triangles and
    a mixed mesh).  The candidate count is the coherent numbering's: the same boxes, whatever the order."""
    rng = np.random.default_rng(42)
    sxy, sf = meshgen.triangle_mesh(1500, 0)
    txy, tf = meshgen.triangle_mesh(1500, 1, 30.0, 0.7)
    cand, nnz = parity(hip, oracle, sxy, sf, txy, tf)
    cand_s, nnz_s = parity(hip, oracle, sxy, sf[rng.permutation(sf.shape[0])], txy, tf[rng.permutation(tf.shape[0])])
    assert (cand_s, nnz_s) == (cand, nnz) and nnz <= cand
    mxy, mf = meshgen.mixed_mesh(1200, 5, 25.0, 0.8)
    parity(hip, oracle, sxy, sf, mxy, mf[rng.permutation(mf.shape[0])])


def test_big_target_faces(hip, oracle):
    """A triangle target with a few faces of far more than 16 hits: they take the block-per-face search on the side stream
    (test_overlap_long_rows_and_big_queries scaled down), which takes the face's box from the vertices it stages; their rows are
    placed with a tile key from the box of a run's middle face."""
    sxy, sf = meshgen.triangle_mesh(6000, 3)
    fxy, ff = meshgen.triangle_mesh(1000, 4, 10.0, 0.9)
    big = np.array([[0.02, 0.02], [0.98, 0.03], [0.97, 0.99], [0.03, 0.96], [0.5, 0.45]])
    n0 = fxy.shape[0]
    txy = np.vstack([fxy, big])
    tf = np.vstack([ff, [[n0, n0 + 1, n0 + 2], [n0, n0 + 2, n0 + 3], [n0, n0 + 1, n0 + 4], [n0 + 3, n0 + 4, n0 + 2]]])
    parity(hip, oracle, sxy, sf, txy, tf)
    # the big faces alone (four rows of thousands of entries), as triangles and as a mixed mesh's faces with a fill slot
    _, b_nnz = parity(hip, oracle, sxy, sf, txy, tf[-4:])
    assert b_nnz > 4 * 1000
    parity(hip, oracle, sxy, sf, txy, np.hstack([tf[-4:], np.full((4, 1), -1)]))


def test_tile_keys_feed_the_many_variable_apply(hip, oracle, xr_option):
    """A coherently numbered target's rows get a coarse Morton key from the box of a run's middle face -- written by k_assemble and
    k_place_big (big faces) in the one-round-trip pipeline and by k_search in the general chain (option "overlap_fused" = 0) -- and
    only the planned apply of eight or more variables reads the keys: it regroups the stored rows by them.  Both chains, triangle and
    mixed targets with big faces, 16 variables against the oracle.  (The keys order work and never enter a value: a wrong box would
    show as a key out of range or a mis-tiled, slower apply, not as a wrong number -- the boxes themselves are pinned by the pair sets
    of the cases above.)"""
    sxy, sf = meshgen.triangle_mesh(6000, 3)
    fxy, ff = meshgen.triangle_mesh(1000, 4, 10.0, 0.9)
    n0 = fxy.shape[0]
    txy = np.vstack([fxy, [[0.02, 0.02], [0.98, 0.03], [0.97, 0.99], [0.03, 0.96]]])
    tf = np.vstack([ff, [[n0, n0 + 1, n0 + 2], [n0, n0 + 2, n0 + 3]]])
    mxy, mf = meshgen.mixed_mesh(1200, 5, 25.0, 0.8)
    v = np.stack([meshgen.smooth_field(oracle.centroids(sxy, sf), k, nan_fraction=0.02) for k in range(16)])
    for fused in (None, 0):
        xr_option("overlap_fused", fused)
        for qxy, qf in ((txy, tf), (mxy, mf)):
            csr, (data, idx, indptr) = assert_overlap_parity(hip, oracle, sxy, sf, qxy, qf)
            assert_apply_equal(csr.apply(v, 0), oracle.regrid_csr("mean", v, data, idx, indptr, csr.n), indptr, "mean")
    xr_option("overlap_fused", None)


def test_dense_meshes_hold_no_box_array(hip):
    """What a prepared dense query mesh keeps on the device: nodes, connectivity, vertex blocks, lengths -- 32 bytes per face less
    than with a box array; a shuffled numbering adds the query-order permutation, vertex blocks and lengths, and no box either."""
    E = hip.engine
    sxy, sf = meshgen.triangle_mesh(1500, 0)
    txy, tf = meshgen.triangle_mesh(20_000, 1, 30.0, 0.7)
    F, m = tf.shape
    for faces, extra in ((tf, 0), (tf[np.random.default_rng(1).permutation(F)], F * (4 + 16 * m + 1))):
        mt = E.DeviceMesh(txy, faces)
        E.DeviceMesh(sxy, sf).overlap(mt)
        kept = txy.shape[0] * 16 + F * (4 * m + 16 * m + 1) + extra
        print("device bytes", mt.device_bytes(), "nodes + connectivity + vertex blocks + lengths", kept, "a box array", 32 * F)
        assert kept <= mt.device_bytes() < kept + 16 * F

"""
CPU: the numpy yardstick of the shard plan (tests/shard_cases.py) -- against the project's independent torch set-up code
(xugrid_amd/distributed.py) wherever the two state the same rule, against hand-made answers, and against its own properties;
and every case of tests/test_gpu_shard_plan.py reaches what it was made for.  All comparisons are exact.
"""
import numpy as np
import pytest
import torch

import shard_cases as sc
from xugrid_amd import meshgen
from xugrid_amd.distributed import _face_boxes_t, _partition_faces_t, _spread16, _targets_near_shard_t, _work_weights_t


def no_empty_face(c):
    return bool((c.rule.sn > 0).all() and (c.rule.tn > 0).all())


# ---- against the torch code -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SMALL_CASES)
def test_target_lists_equal_the_torch_filter(name):
    """_targets_near_shard_t on the boxes of the rank's faces, for every mode, world and rank of the case.  (Rows without a
    valid node are taken out before the torch code sees them: it has no rule for a box of (inf, -inf).)"""
    c = sc.case(name)
    sxy, txy = torch.from_numpy(c.sxy), torch.from_numpy(c.txy)
    t_ids = np.nonzero(c.rule.tn > 0)[0]
    tgt_boxes = _face_boxes_t(txy, torch.from_numpy(c.tf[t_ids])) if c.T else None
    for mode, world, rank in c.combinations():
        local_faces, local_targets = c.rule.lists(world, mode, rank)
        assert np.array_equal(local_faces, np.nonzero(c.rule.owner(world, mode) == rank)[0])
        if c.T == 0:
            assert local_targets.size == 0
            continue
        kept = local_faces[c.rule.sn[local_faces] > 0]
        expected = t_ids[_targets_near_shard_t(_face_boxes_t(sxy, torch.from_numpy(c.sf[kept])), tgt_boxes).numpy()]
        assert np.array_equal(local_targets, expected), (name, mode, world, rank, sc.first_difference(local_targets, expected))


@pytest.mark.parametrize("name", sc.SMALL_CASES)
def test_balanced_cost_equals_the_torch_weights(name):
    c = sc.case(name)
    if c.T == 0 or not no_empty_face(c):
        assert name == "no_node" or c.T == 0
        return
    r = c.rule
    expected = _work_weights_t(torch.from_numpy(np.column_stack([r.scx, r.scy])), torch.from_numpy(np.column_stack([r.tcx, r.tcy])))
    assert np.array_equal(r.balanced_cost(), expected.numpy())


@pytest.mark.parametrize("name", ("delaunay", "mixed", "stacked", "straddle_S1_T0"))
def test_hash_owners_equal_the_torch_partition(name):
    c = sc.case(name)
    centroids = torch.from_numpy(np.column_stack([c.rule.scx, c.rule.scy]))
    for world in (1, 2, 3, 8, 64, 4096):
        assert np.array_equal(c.rule.owner(world, "hash"), _partition_faces_t(centroids, world, "hash").numpy())


def test_interleave_equals_a_loop_over_the_bits():
    rng = np.random.default_rng(0)
    qx = np.concatenate([[0, 1023, 0, 1023, 1, 2, 512, 256, 128], rng.integers(0, 1024, 500)])
    qy = np.concatenate([[0, 1023, 1023, 0, 2, 1, 256, 512, 64], rng.integers(0, 1024, 500)])
    expected = []
    for x, y in zip(qx.tolist(), qy.tolist()):
        code = 0
        for b in range(10):
            if x & (1 << b):
                code += 4 ** b
            if y & (1 << b):
                code += 2 * 4 ** b
        expected.append(code)
    got = sc.interleave(qx, qy)
    assert np.array_equal(got, expected)
    assert np.array_equal(got, _spread16(torch.from_numpy(qx)).numpy() | (_spread16(torch.from_numpy(qy)).numpy() << 1))
    assert sc.interleave(1023, 0) == 0x55555 and sc.interleave(0, 1023) == 0xAAAAA and sc.interleave(1, 0) == 1 and sc.interleave(0, 1) == 2


# ---- known answers --------------------------------------------------------------------------------------------------------------
def test_four_quads_are_cut_in_z_order():
    """Faces (row-major) 0: lower left, 1: lower right, 2: upper left, 3: upper right -- already the Z order.  One unit of
    work each: in front of them 0, 1, 2, 3 of 4."""
    xy, faces = meshgen.quad_mesh([0.0, 1.0, 2.0], [0.0, 1.0, 2.0])
    rule = sc.ShardRule(xy, faces, xy, faces)
    assert np.array_equal(rule.morton_code(), [0, 0x55555, 0xAAAAA, 0xFFFFF])
    for mode in ("morton", "balanced"):  # (one target per source face everywhere: equal work)
        assert np.array_equal(rule.owner(4, mode), [0, 1, 2, 3])
        assert np.array_equal(rule.owner(2, mode), [0, 0, 1, 1])
        assert np.array_equal(rule.owner(3, mode), [0, 0, 1, 2])  # floor(k * 3 / 4)
        assert np.array_equal(rule.owner(1, mode), [0, 0, 0, 0])
    assert np.array_equal(rule.work("balanced"), [4096 * 5] * 4)
    # x and y swapped on the way in: the faces at (1, 0) and (0, 1) trade places on the curve
    swapped = sc.ShardRule(xy[:, ::-1], faces, xy, faces)
    assert np.array_equal(swapped.owner(4, "morton"), [0, 2, 1, 3])
    # every quad touches the middle of the raster: each rank keeps all four targets
    owner, lists = sc.shard_plan_numpy(xy, faces, xy, faces, 4, "morton")
    for rank in range(4):
        assert np.array_equal(lists(rank)[0], [rank]) and np.array_equal(lists(rank)[1], [0, 1, 2, 3])


def test_filter_keeps_what_the_boxes_reach():
    """A 1 x 8 row of unit quads as both meshes, W = 8 by hash: 128 cells over [0, 8] are 16 per quad; the box of quad r covers
    cells 16 r .. 16 (r + 1) inclusive (its right edge is the first cell of its neighbour), so rank r keeps r - 1, r, r + 1."""
    xy, faces = meshgen.quad_mesh(np.arange(9.0), [0.0, 1.0])
    owner, lists = sc.shard_plan_numpy(xy, faces, xy, faces, 8, "hash")
    for rank in range(8):
        expected = [t for t in (rank - 1, rank, rank + 1) if 0 <= t < 8]
        for form in ("paint", "diff"):
            assert np.array_equal(sc.shard_plan_numpy(xy, faces, xy, faces, 8, "hash", form)[1](rank)[1], expected)


def test_fixed_point_work():
    """3 source faces in one raster cell with 2 targets: rint(4096 (1 + 8 / 3)) = rint(15018.67) = 15019."""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [100.0, 100.0], [101.0, 100.0], [100.0, 101.0]])
    sf = np.array([[0, 1, 2]] * 3 + [[3, 4, 5]])
    tf = np.array([[0, 1, 2]] * 2)
    rule = sc.ShardRule(xy, sf, xy, tf)
    assert rule.n_grid == 4
    assert np.array_equal(rule.work("balanced"), [15019, 15019, 15019, 4096])
    assert np.array_equal(rule.work("morton"), [1, 1, 1, 1])
    assert np.array_equal(rule.owner(2, "balanced"), [0, 0, 0, 1])  # 45057 of 49153 in front of the last cell
    assert np.array_equal(rule.owner(4096, "balanced"), [0, 0, 0, 45057 * 4096 // 49153])


# ---- properties of the yardstick --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SMALL_CASES)
def test_partition_properties(name):
    c = sc.case(name)
    code = c.rule.morton_code()
    order = np.argsort(code, kind="stable")
    for mode in sc.MODES:
        for world in c.worlds:
            owner = c.rule.owner(world, mode)
            assert owner.shape == (c.S,) and owner.min() >= 0 and owner.max() < world
            if mode != "hash":
                assert (np.diff(owner[order]) >= 0).all()
                assert all(np.unique(owner[code == k]).size == 1 for k in np.unique(code)[:50])
            sizes = 0
            for rank in c.ranks(world, mode):
                local_faces, local_targets = c.rule.lists(world, mode, rank)
                assert (np.diff(local_faces) > 0).all() and (np.diff(local_targets) > 0).all()
                assert local_targets.size == 0 or (0 <= local_targets[0] and local_targets[-1] < c.T)
                sizes += local_faces.size
            if world <= 8:
                assert sizes == c.S


@pytest.mark.parametrize("name", sc.SMALL_CASES)
def test_painted_and_difference_forms_agree(name):
    c = sc.case(name)
    for mode, world, rank in c.combinations():
        mine = c.rule.owner(world, mode) == rank
        painted, by_difference = c.rule.targets(mine, "paint"), c.rule.targets(mine, "diff")
        assert np.array_equal(painted, by_difference), (name, mode, world, rank, sc.first_difference(painted, by_difference))


# ---- every case reaches what it was made for --------------------------------------------------------------------------------------
def test_stacked_fills_its_cells():
    c = sc.case("stacked")
    assert np.bincount(c.rule.morton_code()).max() >= 6
    assert np.bincount(sc.case("delaunay").rule.morton_code()).max() < 6


def test_outlier_leaves_ranks_without_a_face():
    c = sc.case("outlier")
    assert c.S == 301
    for mode in ("morton", "balanced"):
        counts = np.bincount(c.rule.owner(8, mode), minlength=8)
        assert (counts == 0).any() and counts[7] >= 1, counts
        empty = int(np.nonzero(counts == 0)[0][0])
        local_faces, local_targets = c.rule.lists(8, mode, empty)
        assert local_faces.size == 0 and local_targets.size == 0
    assert np.unique(c.rule.morton_code()).size <= 10


def test_column_has_no_extent_in_x():
    r = sc.case("column").rule
    assert r.src_bounds[0] == r.src_bounds[2] and r.src_bounds[1] < r.src_bounds[3]
    assert np.unique(r.morton_code() & 0x55555).size == 1


def test_diagonal_occupies_the_first_and_the_last_cell():
    r = sc.case("diagonal").rule
    assert np.array_equal(r.scx, r.scy)
    code = r.morton_code()
    assert code.min() == 0 and code.max() == (1 << 20) - 1


def test_no_node_faces_change_no_bounds():
    c, plain = sc.case("no_node"), sc.case("delaunay")
    assert (c.rule.sn == 0).sum() == 5 and (c.rule.tn == 0).sum() == 5 and c.S == plain.S + 5 and c.T == plain.T + 5
    shifted = sc.ShardRule(plain.sxy + 100.0, plain.sf, plain.txy + 100.0, plain.tf)
    assert c.rule.src_bounds == shifted.src_bounds and c.rule.tgt_bounds == shifted.tgt_bounds
    assert min(c.rule.src_bounds[:2]) > 99.0  # (0, 0) would have stretched them a hundredfold
    # such a face is still a source face: the first Morton cell, an owner, and no target ever
    empty = np.nonzero(c.rule.sn == 0)[0]
    assert (c.rule.morton_code()[empty] == 0).all()
    for mode in sc.MODES:
        assert np.isin(empty, np.concatenate([c.rule.lists(3, mode, r)[0] for r in range(3)])).all()
        assert not np.isin(np.nonzero(c.rule.tn == 0)[0], np.concatenate([c.rule.lists(3, mode, r)[1] for r in range(3)])).any()
    # the other faces' owners are those of the mesh without the spliced rows wherever the work is the same
    valid = c.rule.sn > 0
    assert np.array_equal(c.rule.morton_code()[valid], shifted.morton_code())


def test_clamp_reaches_the_limit():
    r = sc.case("clamp").rule
    work = r.work("balanced")
    assert r.n_grid == 4 and (work == 1 << 20).any() and work.max() == 1 << 20 and (work < 1 << 20).any()
    assert (sc.WORK_UNIT * r.balanced_cost()).max() > 1 << 20


def test_work_grids():
    assert sc.case("grid5").rule.n_grid == 5 and sc.case("grid5").S == 400
    assert sc.case("delaunay").rule.n_grid > 5
    assert sc.case("straddle_S1_T0").rule.n_grid == 4
    assert sc.work_grid(1024 * 1024) == 256 and sc.work_grid(4 * 1024 * 1024) == 256


def test_negative_has_ranks_without_targets():
    c = sc.case("negative")
    assert c.sxy.min() < -0.4 and c.sxy.max() > 0.4
    sizes = [c.rule.lists(8, "morton", rank)[1].size for rank in range(8)]
    assert min(sizes) == 0 and max(sizes) > 0, sizes


def test_straddle_sizes():
    sizes = {(sc.case(n).S, sc.case(n).T) for n in sc.SMALL_CASES if n.startswith("straddle")}
    assert sizes == set(sc.STRADDLE_SIZES) and (100, 156) in sizes and (1, 0) in sizes and (257, 300) in sizes


def test_modes_differ_on_delaunay():
    r = sc.case("delaunay").rule
    hashed, morton, balanced = (r.owner(8, mode) for mode in sc.MODES)
    assert (morton != balanced).any() and (morton != hashed).any() and (balanced != hashed).any()
    # more ranks than faces: owners still ascend along the curve and the last rank may well be empty
    assert np.unique(r.owner(4096, "morton")).size == np.unique(r.morton_code()).size


def test_number_of_comparisons():
    """what tests/test_gpu_shard_plan.py compares: (case, mode, world, rank)"""
    n = sum(len(sc.case(name).combinations()) for name in sc.SMALL_CASES) + 3 * 2
    assert n > 1000
    print("comparisons:", n)


def test_lattice1m():
    """the large case: its work raster is at the cap, one face per Morton cell, and one rank of one mode in both forms"""
    c = sc.case(sc.LARGE_CASE)
    assert c.S == 1 << 20 and c.T == 1 << 18 and c.rule.n_grid == 256 and c.worlds == (8,)
    code = c.rule.morton_code()
    assert np.array_equal(np.sort(code), np.arange(1 << 20))
    owner = c.rule.owner(8, "morton")
    assert np.array_equal(np.bincount(owner), [1 << 17] * 8)
    local_faces, by_difference = c.rule.lists(8, "morton", 7, "diff")
    _, painted = c.rule.lists(8, "morton", 7, "paint")
    assert np.array_equal(painted, by_difference) and 0 < painted.size < c.T // 2

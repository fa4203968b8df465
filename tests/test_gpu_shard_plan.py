"""
GPU (-m gpu): the shard plan of a rank on the device (csrc/xr_shard.hip: xr_shard_plan_dev) against the numpy restatement of its
rule in tests/shard_cases.py, array for array and without a tolerance: the owner of every source face, the rank's ascending
face list, its ascending target list and the two counts, for every mode, world and rank of every case.  The library is driven
through ``engine.shard_plan_dev`` on ``engine.DeviceArray`` buffers, in this process.
"""
import numpy as np
import pytest

import shard_cases as sc
from xugrid_amd import engine

pytestmark = pytest.mark.gpu

SENTINEL = -7  # what the output buffers hold before a call: nothing behind the returned counts may be written
_ON_DEVICE = {}


class DeviceCase:
    """the meshes of a case in HBM, uploaded once"""

    def __init__(self, c):
        self.c = c
        self.sxy, self.sf = engine.DeviceArray.from_host(c.sxy), engine.DeviceArray.from_host(c.sf)
        self.txy, self.tf = engine.DeviceArray.from_host(c.txy), engine.DeviceArray.from_host(c.tf)

    def plan(self, world, rank, mode, want_owner=True, src_m=None, n_src_face=None):
        """-> (local_faces buffer, local_targets buffer, owner buffer or None, n_faces, n_targets), all as downloaded"""
        c = self.c
        faces = engine.DeviceArray.from_host(np.full(max(c.S, 1), SENTINEL, dtype=np.int64))
        targets = engine.DeviceArray.from_host(np.full(max(c.T, 1), SENTINEL, dtype=np.int64))
        owner = engine.DeviceArray.from_host(np.full(max(c.S, 1), SENTINEL, dtype=np.int32)) if want_owner else None
        n_f, n_t = engine.shard_plan_dev(self.sxy.ptr, self.sf.ptr, c.S if n_src_face is None else n_src_face,
                                         c.sf.shape[1] if src_m is None else src_m, self.txy.ptr, self.tf.ptr, c.T, c.tf.shape[1],
                                         world, rank, mode, faces.ptr, targets.ptr, owner.ptr if want_owner else 0)
        return faces.download(), targets.download(), owner.download() if want_owner else None, n_f, n_t

    def unchanged(self):
        c = self.c
        return all(np.array_equal(dev.download().view(np.int64), host.view(np.int64))
                   for dev, host in ((self.sxy, c.sxy), (self.sf, c.sf), (self.txy, c.txy), (self.tf, c.tf)))


def on_device(name, hip):
    if name not in _ON_DEVICE:
        _ON_DEVICE[name] = DeviceCase(sc.case(name))
    return _ON_DEVICE[name]


def check_rank(d, mode, world, rank, expected_owner):
    """one (case, mode, world, rank): -> the two list buffers and the owner array of this call, as downloaded"""
    c = d.c
    where = f"{c.name}, {mode}, W = {world}, rank {rank}"
    faces, targets, owner, n_f, n_t = d.plan(world, rank, mode)
    owner = owner[:c.S]
    assert np.array_equal(owner, expected_owner), f"{where}: owner: {sc.first_difference(owner, expected_owner)}"
    expected_faces, expected_targets = c.rule.lists(world, mode, rank, c.form)
    assert (n_f, n_t) == (expected_faces.size, expected_targets.size), f"{where}: counts {(n_f, n_t)}, expected {(expected_faces.size, expected_targets.size)}"
    assert np.array_equal(faces[:n_f], np.nonzero(owner == rank)[0]), f"{where}: local_faces are not nonzero(owner == rank)"
    assert np.array_equal(faces[:n_f], expected_faces), f"{where}: local_faces: {sc.first_difference(faces[:n_f], expected_faces)}"
    assert np.array_equal(targets[:n_t], expected_targets), f"{where}: local_targets: {sc.first_difference(targets[:n_t], expected_targets)}"
    assert (faces[n_f:] == SENTINEL).all() and (targets[n_t:] == SENTINEL).all(), f"{where}: written behind the counts"
    if expected_faces.size == 0:
        assert (n_f, n_t) == (0, 0), f"{where}: a rank without a face keeps {n_t} targets"
    return faces, targets, owner


def check_case(d, mode):
    c = d.c
    for world in c.worlds:
        expected_owner = c.rule.owner(world, mode)
        ranks = c.ranks(world, mode)
        for rank in ranks:
            last = check_rank(d, mode, world, rank, expected_owner)
        again = check_rank(d, mode, world, ranks[-1], expected_owner)  # the same call once more: the same bytes
        assert all(np.array_equal(a, b) for a, b in zip(last, again)), f"{c.name}, {mode}, W = {world}: a second call differs"
        # without the owner array: the same lists
        faces, targets, _, n_f, n_t = d.plan(world, ranks[-1], mode, want_owner=False)
        assert np.array_equal(faces, last[0]) and np.array_equal(targets, last[1]), f"{c.name}, {mode}, W = {world}: owner_ptr = 0"
    assert d.unchanged(), f"{c.name}, {mode}: the inputs were written"


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("name", sc.SMALL_CASES)
def test_plan_equals_the_rule(hip, name, mode):
    check_case(on_device(name, hip), mode)


@pytest.mark.parametrize("mode", sc.MODES)
def test_plan_equals_the_rule_on_a_million_faces(hip, mode):
    """1024 x 1024 unit quads, one per Morton cell, with 512 x 512 over the middle: the work raster at its cap of 256, every tile
    of the 64-bit scan in use, W = 8, ranks 0 and 7."""
    check_case(on_device(sc.LARGE_CASE, hip), mode)


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("name", sc.FOLD_CASES)
def test_plan_equals_the_rule_at_256_and_257_partial_bounds(hip, name, mode):
    c = sc.case(name)
    assert c.S == 65_536 and c.S + c.T in (65_536, 65_736)
    check_case(on_device(name, hip), mode)


def test_empty_ranks_return_nothing(hip):
    d = on_device("outlier", hip)
    for mode in ("morton", "balanced"):
        counts = np.bincount(d.c.rule.owner(8, mode), minlength=8)
        assert (counts == 0).any()
        for rank in np.nonzero(counts == 0)[0]:
            faces, targets, _, n_f, n_t = d.plan(8, int(rank), mode)
            assert (n_f, n_t) == (0, 0) and (faces == SENTINEL).all() and (targets == SENTINEL).all()


# ---- arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world, rank, mode, src_m", [
    (0, 0, "morton", None), (4097, 0, "morton", None), (3, 3, "morton", None), (3, -1, "morton", None), (3, 0, 3, None),
    (3, 0, "morton", 0)])
def test_bad_arguments_raise(hip, monkeypatch, world, rank, mode, src_m):
    """all refused before any launch: the outputs stay as they were"""
    d = on_device("delaunay", hip)
    if mode == 3:
        monkeypatch.setitem(engine.SHARD_MODES, 3, 3)
    with pytest.raises(ValueError, match="xr_shard_plan_dev"):
        d.plan(world, rank, mode, src_m=src_m)
    assert d.unchanged()
    # the library goes on as before
    check_rank(d, "morton", 3, 1, d.c.rule.owner(3, "morton"))


def test_no_source_face(hip):
    d = on_device("delaunay", hip)
    for mode in sc.MODES:
        faces, targets, owner, n_f, n_t = d.plan(3, 1, mode, n_src_face=0)
        assert (n_f, n_t) == (0, 0)
        assert (faces == SENTINEL).all() and (targets == SENTINEL).all() and (owner == SENTINEL).all()

"""
The yardstick and the cases of the shard plan (csrc/xr_shard.hip: xr_shard_plan_dev, behind ``HipBackend.shard_plan``), shared by
tests/test_shard_cpu.py and tests/test_gpu_shard_plan.py.

``shard_plan_numpy`` restates the rule of include/xugrid_amd.h in float64 numpy and 64-bit integers, in the rule's operation
order, so that every comparison with the device is ``np.array_equal``:

  * face: centroid = sum of the valid nodes in connectivity order / their number, box = min / max of the valid nodes.  A face
    without a valid node has the centroid (0, 0) and no box; it takes no part in ANY bounds (of centroids or of boxes) and
    neither occupies nor receives a cell of the near-shard filter, but it is a source face like any other: its (0, 0) is cut
    against the bounds of the others (which clamps it into a border cell), it carries work and has an owner.
  * raster cell of a value: floor((v - lo) * (n / max(hi - lo, 1e-300))), clamped to [0, n - 1].
  * "hash": owner = face id mod world.
  * "morton" / "balanced": 1024 x 1024 cells over the bounds of the source centroids, code = x bits on the even and y bits on the
    odd positions; work of a face 1 ("morton") or max(1, min(rint(4096 (1 + 4 n_tgt / n_src)), 2^20)) ("balanced": both meshes
    counted on the n_grid-square raster over the joint centroid bounds, n_src taken as at least 1);
    owner = min(work of all cells in front of the face's cell * world // total work, world - 1).
  * near-shard filter: 128 x 128 cells over the bounds of the boxes of MY source faces and of all target faces; a target is kept
    iff the inclusive cell range of its box meets a cell that a box of my source faces covers.  ``form="paint"`` marks the
    covered cells rectangle by rectangle and looks every target's range up directly; ``form="diff"`` is the difference-array /
    integral-image form (the device's algorithm), kept for the one large case and shown equal to the painted form on all
    small ones by the CPU tests.
"""
import numpy as np

from xugrid_amd import meshgen

MODES = ("hash", "morton", "balanced")
MORTON_BITS = 10
MORTON_SIDE = 1 << MORTON_BITS
OCC_GRID = 128
WORK_UNIT = 4096.0
WORK_CLAMP = float(1 << 20)
TARGET_COST = 4.0
MAX_WORLD = 4096


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def face_geometry(xy, faces):
    """-> (cx, cy, number of valid nodes, (x0, y0, x1, y1)) of a dense (F, m) connectivity with -1 fill"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    faces = np.asarray(faces, dtype=np.int64)
    F, m = faces.shape
    sx, sy, n = np.zeros(F), np.zeros(F), np.zeros(F, dtype=np.int64)
    x0, y0, x1, y1 = np.full(F, np.inf), np.full(F, np.inf), np.full(F, -np.inf), np.full(F, -np.inf)
    for j in range(m):  # (connectivity order: ((0 + p0) + p1) + p2 ...)
        ok = faces[:, j] >= 0
        node = np.where(ok, faces[:, j], 0)
        x = xy[node, 0] if F else np.zeros(0)
        y = xy[node, 1] if F else np.zeros(0)
        sx, sy = np.where(ok, sx + x, sx), np.where(ok, sy + y, sy)
        n = n + ok
        x0, y0 = np.where(ok, np.minimum(x0, x), x0), np.where(ok, np.minimum(y0, y), y0)
        x1, y1 = np.where(ok, np.maximum(x1, x), x1), np.where(ok, np.maximum(y1, y), y1)
    count = np.maximum(n, 1).astype(np.float64)
    return sx / count, sy / count, n, (x0, y0, x1, y1)


def raster_cell(v, lo, hi, n):
    f = np.float64(n) / max(np.float64(hi) - np.float64(lo), 1e-300)
    return np.clip(np.floor((np.asarray(v, dtype=np.float64) - np.float64(lo)) * f), 0, n - 1).astype(np.int64)


def interleave(qx, qy):
    """Morton code of 10-bit cell coordinates: bit b of qx at position 2 b, bit b of qy at position 2 b + 1"""
    qx, qy = np.asarray(qx, dtype=np.int64), np.asarray(qy, dtype=np.int64)
    code = np.zeros(qx.shape, dtype=np.int64)
    for b in range(MORTON_BITS):
        code |= ((qx >> b) & 1) << (2 * b)
        code |= ((qy >> b) & 1) << (2 * b + 1)
    return code


def _lo(*arrays):
    return min(float(a.min(initial=np.inf)) for a in arrays)


def _hi(*arrays):
    return max(float(a.max(initial=-np.inf)) for a in arrays)


def work_grid(n_source_faces):
    return int(min(256, max(4, np.sqrt(n_source_faces / 16.0))))


class ShardRule:
    """The rule on one pair of meshes: everything that does not depend on (world, rank) is made once."""

    def __init__(self, sxy, sf, txy, tf):
        self.S, self.T = int(np.shape(sf)[0]), int(np.shape(tf)[0])
        self.scx, self.scy, self.sn, self.sbox = face_geometry(sxy, sf)
        self.tcx, self.tcy, self.tn, self.tbox = face_geometry(txy, tf)
        self.n_grid = work_grid(self.S)
        self._before = {}
        sv = self.sn > 0
        # bounds of the source centroids: faces without a valid node stay out
        self.src_bounds = (_lo(self.scx[sv]), _lo(self.scy[sv]), _hi(self.scx[sv]), _hi(self.scy[sv]))
        tv = self.tn > 0
        self.tgt_bounds = (_lo(self.tcx[tv]), _lo(self.tcy[tv]), _hi(self.tcx[tv]), _hi(self.tcy[tv]))

    # -- partition
    def morton_code(self):
        lox, loy, hix, hiy = self.src_bounds
        return interleave(raster_cell(self.scx, lox, hix, MORTON_SIDE), raster_cell(self.scy, loy, hiy, MORTON_SIDE))

    def work_cells(self):
        """cell of every source and every target face on the n_grid raster over the joint centroid bounds"""
        n = self.n_grid
        lox, loy = min(self.src_bounds[0], self.tgt_bounds[0]), min(self.src_bounds[1], self.tgt_bounds[1])
        hix, hiy = max(self.src_bounds[2], self.tgt_bounds[2]), max(self.src_bounds[3], self.tgt_bounds[3])
        cs = raster_cell(self.scy, loy, hiy, n) * n + raster_cell(self.scx, lox, hix, n)
        ct = raster_cell(self.tcy, loy, hiy, n) * n + raster_cell(self.tcx, lox, hix, n)
        return cs, ct

    def balanced_cost(self):
        """1 + 4 n_tgt / n_src of every source face's raster cell, before fixed point"""
        n = self.n_grid
        cs, ct = self.work_cells()
        n_src, n_tgt = np.bincount(cs, minlength=n * n), np.bincount(ct, minlength=n * n)
        return 1.0 + TARGET_COST * n_tgt[cs].astype(np.float64) / np.maximum(n_src[cs], 1).astype(np.float64)

    def work(self, mode):
        if mode == "morton":
            return np.ones(self.S, dtype=np.uint64)
        fixed = np.minimum(np.rint(WORK_UNIT * self.balanced_cost()), WORK_CLAMP)
        return np.maximum(fixed, 1.0).astype(np.uint64)

    def work_before(self, mode):
        """-> (work in all Morton cells in front of every face's cell, total work), uint64"""
        if mode not in self._before:
            code = self.morton_code()
            cell_work = np.zeros(MORTON_SIDE * MORTON_SIDE, dtype=np.uint64)
            np.add.at(cell_work, code, self.work(mode))
            inclusive = np.cumsum(cell_work, dtype=np.uint64)
            self._before[mode] = ((inclusive - cell_work)[code], int(inclusive[-1]) if self.S else 0)
        return self._before[mode]

    def owner(self, world, mode):
        assert 1 <= world <= MAX_WORLD and mode in MODES
        if mode == "hash":
            return np.arange(self.S, dtype=np.int64) % world
        before, total = self.work_before(mode)
        # (work <= 2^20 per face, S < 2^31, world <= 2^12: the product stays below 2^63)
        return np.minimum(before * np.uint64(world) // np.uint64(max(total, 1)), np.uint64(world - 1)).astype(np.int64)

    # -- near-shard filter
    def filter_cells(self, mine):
        """-> (cells (cx0, cy0, cx1, cy1) of my source faces' boxes, ids of the targets with a box, their cells)"""
        src = np.nonzero(mine & (self.sn > 0))[0]
        tgt = np.nonzero(self.tn > 0)[0]
        sb, tb = [b[src] for b in self.sbox], [b[tgt] for b in self.tbox]
        lox, loy, hix, hiy = _lo(sb[0], tb[0]), _lo(sb[1], tb[1]), _hi(sb[2], tb[2]), _hi(sb[3], tb[3])

        def cells(b):
            return (raster_cell(b[0], lox, hix, OCC_GRID), raster_cell(b[1], loy, hiy, OCC_GRID),
                    raster_cell(b[2], lox, hix, OCC_GRID), raster_cell(b[3], loy, hiy, OCC_GRID))

        return cells(sb), tgt, cells(tb)

    def targets(self, mine, form="paint"):
        empty = np.zeros(0, dtype=np.int64)
        if self.T == 0 or not (self.tn > 0).any() or not (mine & (self.sn > 0)).any():
            return empty
        (sx0, sy0, sx1, sy1), tgt, (tx0, ty0, tx1, ty1) = self.filter_cells(mine)
        if form == "paint":
            occupied = np.zeros((OCC_GRID, OCC_GRID), dtype=bool)
            for a, b, c, d in zip(sx0.tolist(), sy0.tolist(), sx1.tolist(), sy1.tolist()):
                occupied[b:d + 1, a:c + 1] = True
            hit = np.fromiter((occupied[b:d + 1, a:c + 1].any() for a, b, c, d in
                               zip(tx0.tolist(), ty0.tolist(), tx1.tolist(), ty1.tolist())), dtype=bool, count=tgt.size)
        elif form == "diff":
            diff = np.zeros((OCC_GRID + 1, OCC_GRID + 1), dtype=np.int64)
            np.add.at(diff, (sy0, sx0), 1)
            np.add.at(diff, (sy0, sx1 + 1), -1)
            np.add.at(diff, (sy1 + 1, sx0), -1)
            np.add.at(diff, (sy1 + 1, sx1 + 1), 1)
            occupied = diff.cumsum(0).cumsum(1)[:OCC_GRID, :OCC_GRID] > 0
            integral = np.zeros((OCC_GRID + 1, OCC_GRID + 1), dtype=np.int64)
            integral[1:, 1:] = occupied.cumsum(0).cumsum(1)
            hit = (integral[ty1 + 1, tx1 + 1] - integral[ty0, tx1 + 1] - integral[ty1 + 1, tx0] + integral[ty0, tx0]) > 0
        else:
            raise ValueError(form)
        return tgt[hit]

    def lists(self, world, mode, rank, form="paint"):
        """-> (local_faces, local_targets) of a rank: ascending global ids, int64"""
        assert 0 <= rank < world
        if self.S == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        mine = self.owner(world, mode) == rank
        return np.nonzero(mine)[0].astype(np.int64), self.targets(mine, form)


def shard_plan_numpy(sxy, sf, txy, tf, world, mode, form="paint"):
    """-> (owner int64 [S], lists): ``lists(rank)`` -> (local_faces, local_targets) of that rank"""
    rule = ShardRule(sxy, sf, txy, tf)
    return rule.owner(world, mode), lambda rank: rule.lists(world, mode, rank, form)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _delaunay():
    sxy, sf = meshgen.triangle_mesh(700, 0)
    txy, tf = meshgen.triangle_mesh(500, 1, 30.0, 0.6)  # (covers a part of the source)
    return sxy, sf, txy, tf


def _mixed():
    mxy, mf = meshgen.mixed_mesh(600, 2)
    assert mf.shape[1] == 4 and (mf[:, 3] < 0).any() and (mf[:, 3] >= 0).any()
    _, _, txy, tf = _delaunay()
    return mxy, mf, txy, tf


def _mixed_swapped():
    mxy, mf, txy, tf = _mixed()
    return txy, tf, mxy, mf


def _negative():
    sxy, sf, txy, tf = _delaunay()
    return sxy - 0.5, sf, txy, tf


def _utm():
    sxy, sf, txy, tf = _delaunay()
    origin = np.array([5.0e5, 5.8e6])
    return sxy * 1.0e4 + origin, sf, txy * 1.0e4 + origin, tf


def _stacked():
    sxy, sf, txy, tf = _delaunay()
    return sxy, np.ascontiguousarray(np.tile(sf, (6, 1))), txy, tf


def _outlier():
    pxy, pf = meshgen.triangle_mesh(200, 3)
    assert pf.shape[0] >= 300
    n = pxy.shape[0]
    far = 1.0e3 * (pxy[:, 0].max() - pxy[:, 0].min())
    sxy = np.concatenate([pxy, far + np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 0.5]])])
    sf = np.concatenate([pf[:300], [[n, n + 1, n + 2]]]).astype(np.int64)
    _, _, txy, tf = _delaunay()
    return sxy, sf, txy, tf


def _column():
    sxy, sf = meshgen.quad_mesh([0.0, 1.0], np.arange(301.0))
    _, _, txy, tf = _delaunay()
    return sxy, sf, txy * np.array([1.0, 300.0]), tf


def _diagonal():
    k = np.arange(300.0)
    # (quarters: both coordinate sums of a face are exact, so its centroid lies on y = x to the bit)
    sxy = np.stack([np.column_stack([k, k]), np.column_stack([k + 0.75, k]), np.column_stack([k, k + 0.75])], axis=1).reshape(-1, 2)
    sf = np.arange(900, dtype=np.int64).reshape(300, 3)
    _, _, txy, tf = _delaunay()
    return sxy, sf, txy * 300.0, tf


def _no_node():
    sxy, sf, txy, tf = _delaunay()

    def splice(f):
        rows = np.array([0, 100, 254, f.shape[0] // 2, f.shape[0] - 1])  # (row ids before insertion)
        return np.ascontiguousarray(np.insert(f, rows, -1, axis=0))

    return sxy + 100.0, splice(sf), txy + 100.0, splice(tf)


def _clamp():
    sxy, sf = meshgen.triangle_mesh(25, 5, delaunay=False)
    assert sf.shape[0] == 32
    keep = np.sort(np.random.default_rng(5).permutation(32)[:20])
    txy, tf = meshgen.triangle_mesh(3100, 6, 30.0, 0.6)
    assert tf.shape[0] >= 6000
    return sxy, np.ascontiguousarray(sf[keep]), txy, np.ascontiguousarray(tf[:6000])


def _grid5():
    sxy, sf = meshgen.triangle_mesh(256, 7)
    assert sf.shape[0] >= 400
    _, _, txy, tf = _delaunay()
    return sxy, np.ascontiguousarray(sf[:400]), txy, tf


def _straddle(S, T):
    def make():
        sxy, sf, txy, tf = _delaunay()
        return sxy, np.ascontiguousarray(sf[:S]), txy, np.ascontiguousarray(tf[:T])

    return make


def _fold(T):
    """65 536 source faces and T target faces: the bounds reduction writes 256 partials (T = 0) or 257, the last of them the
    target faces' alone, and one block folds them."""
    def make():
        sxy, sf = meshgen.triangle_mesh(33_000, 0)
        _, _, txy, tf = _delaunay()
        return sxy, np.ascontiguousarray(sf[:65_536]), txy, np.ascontiguousarray(tf[:T])

    return make


def _lattice1m():
    sxy, sf = meshgen.quad_mesh(np.arange(1025.0), np.arange(1025.0))
    txy, tf = meshgen.quad_mesh(256.0 + np.arange(513.0), 256.0 + np.arange(513.0))
    return sxy, sf, txy, tf


STRADDLE_SIZES = [(S, T) for S in (1, 255, 256, 257) for T in (0, 1, 300)] + [(100, 156)]
_BUILDERS = {
    "delaunay": _delaunay, "mixed": _mixed, "mixed_swapped": _mixed_swapped, "negative": _negative, "utm": _utm,
    "stacked": _stacked, "outlier": _outlier, "column": _column, "diagonal": _diagonal, "no_node": _no_node,
    "clamp": _clamp, "grid5": _grid5,
}
_BUILDERS.update({f"straddle_S{S}_T{T}": _straddle(S, T) for S, T in STRADDLE_SIZES})
SMALL_CASES = tuple(_BUILDERS)
LARGE_CASE = "lattice1m"
_BUILDERS[LARGE_CASE] = _lattice1m
FOLD_CASES = ("fold_T0", "fold_T200")
_BUILDERS.update({"fold_T0": _fold(0), "fold_T200": _fold(200)})
MANY_RANKS = ("delaunay", "outlier")  # also run with more ranks than a few, and more than faces
_MADE = {}


class Case:
    def __init__(self, name):
        self.name = name
        sxy, sf, txy, tf = _BUILDERS[name]()
        self.sxy, self.txy = np.ascontiguousarray(sxy, dtype=np.float64), np.ascontiguousarray(txy, dtype=np.float64)
        self.sf, self.tf = np.ascontiguousarray(sf, dtype=np.int64), np.ascontiguousarray(tf, dtype=np.int64)
        self.S, self.T = self.sf.shape[0], self.tf.shape[0]
        self.rule = ShardRule(self.sxy, self.sf, self.txy, self.tf)
        self.form = "diff" if name == LARGE_CASE else "paint"

    @property
    def worlds(self):
        if self.name == LARGE_CASE:
            return (8,)
        if self.name in FOLD_CASES:
            return (3,)
        return (1, 2, 3, 8) + ((64, 4096) if self.name in MANY_RANKS else ())

    def ranks(self, world, mode):
        """every rank of a small world; of a large one rank 0, rank 1, the first and the last rank without a face, the last
        rank with one and rank world - 1"""
        if self.name == LARGE_CASE:
            return [0, world - 1]
        if world <= 8:
            return list(range(world))
        counts = np.bincount(self.rule.owner(world, mode), minlength=world)
        empty, busy = np.nonzero(counts == 0)[0], np.nonzero(counts > 0)[0]
        picks = {0, 1, world - 1, int(busy[-1])}
        if empty.size:
            picks |= {int(empty[0]), int(empty[-1])}
        return sorted(picks)

    def combinations(self):
        """every (mode, world, rank) the case is compared at"""
        return [(mode, world, rank) for mode in MODES for world in self.worlds for rank in self.ranks(world, mode)]


def case(name):
    if name not in _MADE:
        _MADE[name] = Case(name)
    return _MADE[name]


def first_difference(got, expected):
    """a few words on where two id arrays part, for assertion messages"""
    got, expected = np.asarray(got), np.asarray(expected)
    if got.shape != expected.shape:
        n = min(got.size, expected.size)
        bad = np.nonzero(got[:n] != expected[:n])[0]
        at = int(bad[0]) if bad.size else n
        return f"lengths {got.size} and {expected.size}, first difference at index {at}"
    bad = np.nonzero(got != expected)[0]
    if bad.size == 0:
        return "equal"
    i = int(bad[0])
    return f"{bad.size} of {got.size} differ, first at index {i}: got {got[i]}, expected {expected[i]}"

"""
Yardstick and cases of the line snapping tests (xugrid_amd/snapgrid.py, csrc/xr_snapgrid.hip).

``frame_ref`` and ``winners_ref`` say what ``create_snap_to_grid_dataframe`` and ``snap_to_grid`` compute in this project's own
words, with numpy over the oracle's ``CellTree2d.intersect_edges``: tests/test_snapgrid_cpu.py pins them to what the reference's
``snap_to_edges`` gives for the same pieces (tests/golden/snapgrid_known.json, written by tests/golden/gen_snapgrid.py) and to the
expected values of the reference's own tests; tests/test_gpu_snapgrid.py compares the device with them, exactly.

The rule: vertices snap onto nodes (``snap_cases.snap_to_nodes_ref``); a segment joins consecutive vertices of one line; the
oracle cuts every segment into its pieces per face, ordered by (segment, face); a piece of non-zero extent, widened at both ends
by ``tolerance * max(|Ux|, |Uy|)`` along ``sign(U)``, snaps to an interior edge of its face iff the centroids ``a`` of the face
and ``b`` of the face across the edge lie on different sides of the piece (strictly left or not) AND the two widened end points
lie on different sides of ``a -> b``.  The edges of a face are taken in ascending id.  One row per (piece, edge); per edge the row
of greatest squared length wins, the first among equal ones.
"""
import numpy as np

import snap_cases

COLUMNS = ("line_index", "edge_index", "x0", "y0", "x1", "y1", "length")
FRAME_DTYPES = dict(line_index=np.int64, edge_index=np.int64, x0=np.float64, y0=np.float64, x1=np.float64, y1=np.float64,
                    length=np.float64)


# ---- restatement --------------------------------------------------------------------------------------------------------------------
def segments(xy, offsets):
    """-> (segments (n_seg, 2, 2), the line of each): consecutive vertices of one line."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    line = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    if len(xy) < 2:
        return np.empty((0, 2, 2)), np.empty(0, dtype=np.int64)
    same = line[1:] == line[:-1]
    return np.stack([xy[:-1][same], xy[1:][same]], axis=1), line[1:][same].astype(np.int64)


def _left_of(ax, ay, px, py, ux, uy):
    return ux * (ay - py) > uy * (ax - px)


def frame_ref(oracle, node_xy, faces, centroids, face_edge, edge_face, coords, offsets, max_snap_distance, tolerance=1e-12):
    """-> dict of the frame's columns, rows ordered by (segment, face, edge)."""
    node_xy = np.asarray(node_xy, dtype=np.float64)
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 2)
    face_edge, edge_face = np.asarray(face_edge), np.asarray(edge_face)
    if edge_face.shape[1] < 2:  # (a host table is as wide as the busiest edge)
        edge_face = np.column_stack([edge_face, np.full(len(edge_face), -1)])
    xs, ys, _, _ = snap_cases.snap_to_nodes_ref(coords[:, 0], coords[:, 1], node_xy[:, 0], node_xy[:, 1], max_snap_distance)
    seg, seg_line = segments(np.column_stack([xs, ys]), offsets)
    s, f, piece = oracle.CellTree2d(node_xy, faces).intersect_edges(seg)
    assert np.array_equal(np.lexsort((f, s)), np.arange(len(s)))  # ordered by (segment, face)
    p0, q0 = piece[:, 0], piece[:, 1]
    u = q0 - p0
    sign = np.sign(u)
    increase = tolerance * np.maximum(np.abs(u[:, 0]), np.abs(u[:, 1]))
    p = p0 - sign * increase[:, None]
    q = q0 + sign * increase[:, None]
    u2 = q - p
    a = np.asarray(centroids)[f]
    a_left = _left_of(a[:, 0], a[:, 1], p[:, 0], p[:, 1], u2[:, 0], u2[:, 1])
    nonzero = (u[:, 0] != 0) | (u[:, 1] != 0)
    big = np.iinfo(np.int64).max
    slots = np.sort(np.where(face_edge[f] < 0, big, face_edge[f].astype(np.int64)), axis=1)  # a face's edges ascending
    passes = np.zeros(slots.shape, dtype=bool)
    for k in range(slots.shape[1]):
        valid = nonzero & (slots[:, k] != big)
        e = np.where(valid, slots[:, k], 0)
        other = np.where(edge_face[e, 1] == f, edge_face[e, 0], edge_face[e, 1])
        valid &= other >= 0
        b = np.asarray(centroids)[np.where(valid, other, 0)]
        b_left = _left_of(b[:, 0], b[:, 1], p[:, 0], p[:, 1], u2[:, 0], u2[:, 1])
        v = b - a
        p_left = _left_of(p[:, 0], p[:, 1], a[:, 0], a[:, 1], v[:, 0], v[:, 1])
        q_left = _left_of(q[:, 0], q[:, 1], a[:, 0], a[:, 1], v[:, 0], v[:, 1])
        passes[:, k] = valid & (a_left != b_left) & (p_left != q_left)
    at, k = np.nonzero(passes)  # row-major: by piece, then by slot
    d = q0[at] - p0[at]
    return dict(line_index=seg_line[s[at]], edge_index=slots[at, k], x0=p0[at, 0], y0=p0[at, 1], x1=q0[at, 0], y1=q0[at, 1],
                length=d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def host_tables(oracle, node_xy, faces):
    """-> (centroids, face_edge, edge_face, n_edge) of a host mesh: the oracle's centroids and the host connectivity."""
    from xugrid_amd import connectivity

    edge_node, face_edge = connectivity.edge_connectivity(np.asarray(faces))
    return oracle.centroids(node_xy, faces), face_edge, connectivity.invert_dense(face_edge), len(edge_node)


def expected(oracle, name, tolerance=1e-12):
    """Case ``name`` through the restatement on host tables -> (frame, (line_index, edges, edge_lines), n_edge)."""
    node_xy, faces, coords, offsets, d = CASES[name]()
    centroids, face_edge, edge_face, n_edge = host_tables(oracle, node_xy, faces)
    frame = frame_ref(oracle, node_xy, faces, centroids, face_edge, edge_face, coords, offsets, d, tolerance)
    return frame, winners_ref(frame, n_edge), n_edge


def winners_ref(frame, n_edge):
    """-> (line_index float64 (n_edge,) NaN-filled, edges ascending, their lines): per edge the first row of greatest length."""
    edge, length = frame["edge_index"], frame["length"]
    order = np.lexsort((np.arange(len(edge)), -length, edge))
    first = np.ones(len(order), dtype=bool)
    first[1:] = edge[order][1:] != edge[order][:-1]
    rows = order[first]
    edges, lines = edge[rows].astype(np.int64), frame["line_index"][rows].astype(np.int64)
    line_index = np.full(n_edge, np.nan)
    line_index[edges] = lines
    return line_index, edges, lines


def gather_values(values, line_index):
    """values (n_line,) or (K, n_line) -> (n_edge,) or (K, n_edge), NaN where no line snapped."""
    values = np.asarray(values, dtype=np.float64)
    hit = ~np.isnan(line_index)
    out = np.full(values.shape[:-1] + line_index.shape, np.nan)
    out[..., hit] = values[..., line_index[hit].astype(np.int64)]
    return out


def contested(frame):
    """-> (edges that rows of more than one line name, those of them whose winner is not the lowest of their lines)."""
    edge, line = frame["edge_index"], frame["line_index"]
    n_edge = int(edge.max()) + 1 if len(edge) else 0
    _, edges, lines = winners_ref(frame, n_edge)
    lowest = np.full(n_edge, np.iinfo(np.int64).max)
    highest = np.full(n_edge, -1)
    np.minimum.at(lowest, edge, line)
    np.maximum.at(highest, edge, line)
    many = lowest[edges] != highest[edges]
    return edges[many], edges[many & (lines != lowest[edges])]


# ---- meshes: -> (node_xy (n, 2), faces (n_face, m) with -1 fill) ------------------------------------------------------------------
def quad_grid(xv, yv):
    """The quads of a rectilinear grid, nodes row by row along ``yv``."""
    xv, yv = np.asarray(xv, dtype=np.float64), np.asarray(yv, dtype=np.float64)
    nx, ny = len(xv) - 1, len(yv) - 1
    y, x = (a.ravel() for a in np.meshgrid(yv, xv, indexing="ij"))
    n = np.arange((nx + 1) * (ny + 1)).reshape(ny + 1, nx + 1)
    faces = np.stack([n[:-1, :-1], n[:-1, 1:], n[1:, 1:], n[1:, :-1]], axis=-1).reshape(-1, 4)
    return np.column_stack([x, y]), faces.astype(np.int64)


def reference_grid():
    """The 9 x 9 grid of 10-unit cells of the reference's tests (tests/test_snap.py:22-45): x ascends, y descends."""
    return quad_grid(np.arange(0.0, 91.0, 10.0), np.arange(90.0, -1.0, -10.0))


def jittered_lattice(n=15, seed=19, mixed=False):
    """An n x n node lattice over the unit square, every node moved by up to a fifth of the spacing; every cell is cut into two
    triangles, along alternating diagonals -- ``mixed``: every other cell stays a quad (m = 4, triangles padded with -1)."""
    rng = np.random.default_rng(seed)
    h = 1.0 / (n - 1)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    xy = np.column_stack([i.ravel() * h, j.ravel() * h]) + rng.uniform(-0.2 * h, 0.2 * h, (n * n, 2))
    node = np.arange(n * n).reshape(n, n)
    faces = []
    for r in range(n - 1):
        for c in range(n - 1):
            a, b, cc, d = node[r, c], node[r, c + 1], node[r + 1, c + 1], node[r + 1, c]
            if mixed and (r + c) % 2 == 0:
                faces.append([a, b, cc, d])
            elif (r + c) % 3 == 0:
                faces += [[a, b, d, -1], [b, cc, d, -1]]
            else:
                faces += [[a, b, cc, -1], [a, cc, d, -1]]
    faces = np.array(faces, dtype=np.int64)
    return xy, (faces if mixed else faces[:, :3].copy())


def widened(node_xy, faces, m):
    """The same faces in a table of ``m`` columns, -1 filled."""
    return node_xy, np.concatenate([faces, np.full((len(faces), m - faces.shape[1]), -1, dtype=faces.dtype)], axis=1)


# ---- lines: -> (coords (n, 2), offsets (n_line + 1)) ----------------------------------------------------------------------------------
def lines_of(*polylines):
    parts = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in polylines]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.empty((0, 2))), offsets


def random_lines(seed=19, n_line=40):
    """Polylines of 2-6 vertices that start in [-0.1, 1.1]^2 and take normal steps of sigma 0.18; one long segment through the
    middle at a slight slope; an exact copy of line 3 as the last line."""
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(n_line):
        k = int(rng.integers(2, 7))
        steps = rng.normal(0.0, 0.18, (k, 2))
        steps[0] = rng.uniform(-0.1, 1.1, 2)
        lines.append(np.cumsum(steps, axis=0))
    lines.append(np.array([[-0.2, 0.503], [1.2, 0.497]]))
    lines.append(lines[3].copy())
    return lines_of(*lines)


_Y = [82.0, 40.0, 0.0]
REFERENCE_LINES = {  # tests/test_snap.py:184-329, inputs; the expected counts are part of the goldens
    "single_line": [np.column_stack([[40.2] * 3, _Y])],
    "single_line_at_edge": [np.column_stack([[40.0] * 3, _Y])],
    "parallel_lines": [np.column_stack([[10.2] * 3, _Y]), np.column_stack([[30.2] * 3, _Y])],
    "series_lines": [[[40.2, 82.0], [40.2, 60.0]], [[40.2, 60.0], [40.2, 40.0]], [[40.2, 40.0], [40.2, 20.0]],
                     [[40.2, 20.0], [40.2, 0.0]]],
    "crossing_lines": [np.column_stack([[40.2] * 3, _Y]), np.column_stack([_Y, [40.2] * 3])],
    "closely_parallel": [np.column_stack([[19.0] * 3, _Y]), np.column_stack([[21.0] * 3, _Y])],
    "line_hits_edge_centroid": [[[12.0, 22.0], [18.0, 18.0]]],
}
STRIP = 300
# beside the one interior edge x = 1 of two unit quads, one line in either face: the pieces are the lines themselves
TIE_LOW, TIE_HIGH = [[0.9, 0.1], [0.9, 0.9]], [[1.1, 0.1], [1.1, 0.9]]
TIE_LONGER = [[1.1, 0.05], [1.1, 0.95]]


def _cases():
    """name -> () -> (node_xy, faces, coords, offsets, max_snap_distance)"""
    cases = {}
    for name, lines in REFERENCE_LINES.items():
        cases[f"ref_{name}"] = lambda lines=lines: reference_grid() + lines_of(*lines) + (0.5,)
    cases["random_triangles"] = lambda: jittered_lattice() + random_lines() + (0.02,)
    cases["random_mixed"] = lambda: jittered_lattice(mixed=True) + random_lines() + (0.02,)
    # the same faces in a table six columns wide: the mesh is stored as flat vertex blocks and no kernel knows its width
    cases["random_wide"] = lambda: widened(*jittered_lattice(mixed=True), 6) + random_lines() + (0.02,)
    # one segment across all faces of a strip of unit quads (a bucket of 299 rows), one along the outer boundary (exterior edges:
    # no rows), one along an interior edge (both faces report the piece)
    cases["strip"] = lambda: quad_grid(np.arange(STRIP + 1.0), [0.0, 1.0]) + lines_of(
        [[0.25, 0.3], [STRIP - 0.25, 0.7]], [[10.0, 0.0], [20.0, 0.0]], [[150.0, 0.0], [150.0, 1.0]]) + (0.05,)
    # A segment that only CROSSES the strip's interior edges separates no pair of centroids but near the middle of the strip.  The
    # long bucket comes from a strip two quads high with a segment along its middle line: one row per piece, about 300 rows of
    # one segment
    cases["strip_two_rows"] = lambda: quad_grid(np.arange(STRIP + 1.0), [0.0, 1.0, 2.0]) + lines_of(
        [[0.25, 0.9], [STRIP - 0.25, 1.1]], [[0.3, 1.2], [40.7, 0.8]]) + (0.05,)
    # an empty line, one vertex, a repeated vertex, two vertices onto one node, a line outside the mesh, an empty line at the end
    cases["degenerate"] = lambda: reference_grid() + lines_of(
        [], [[15.0, 15.0]], [[12.0, 33.0], [12.0, 33.0], [47.0, 33.0]], [[10.1, 10.1], [9.9, 9.8]], [[200.0, 200.0], [300.0, 250.0]],
        []) + (0.5,)
    cases["no_lines"] = lambda: reference_grid() + lines_of() + (0.5,)
    two = lambda: quad_grid([0.0, 1.0, 2.0], [0.0, 1.0])  # noqa: E731
    cases["tie_equal"] = lambda: two() + lines_of(TIE_LOW, TIE_HIGH) + (0.05,)
    cases["tie_later_longer"] = lambda: two() + lines_of(TIE_LOW, TIE_LONGER) + (0.05,)
    cases["tie_swapped"] = lambda: two() + lines_of(TIE_LONGER, TIE_LOW) + (0.05,)
    return cases


CASES = _cases()

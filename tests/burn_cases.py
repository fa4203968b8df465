"""Shared inputs and the host yardstick of the burn tests (CPU known-answer tests and GPU parity tests).

The yardstick restates in numpy, brute force over all segments, the rule ``burn_vector_geometry`` fixes for polygons
(DESIGN section 7): face f is in polygon g iff its centroid p passes, over ALL ring segments v0 -> v1 of g,

    on an edge:  |wx uy - wy ux| < tol sqrt(len2)  and  0 <= u.w <= len2        (w = v1 - v0, u = p - v0, len2 = w.w > 0)
    crossing:    (v0.y > p.y) != (v1.y > p.y)  and  p.x < wx (p.y - v0.y) / wy + v0.x

``on any edge or an odd number of crossings``.  numpy evaluates every product, sum and quotient in float64 one rounding at
a time, as the device code does (built without contraction), so the two are compared for equality.
"""
import numpy as np

from network_cases import burn_lines_case


def ring_segments(coords, ring_offsets, polygon_offsets=None):
    """(segments (n, 2, 2), owner (n,)) of cyclic rings: every vertex is joined to the next one of its ring, the last to the
    first.  owner: the ring, or its polygon when ``polygon_offsets`` is given."""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 2)
    ring_offsets = np.asarray(ring_offsets, dtype=np.int64)
    nxt = np.arange(1, coords.shape[0] + 1)
    owner = np.repeat(np.arange(ring_offsets.size - 1), np.diff(ring_offsets))
    last = ring_offsets[1:][np.diff(ring_offsets) > 0] - 1
    nxt[last] = ring_offsets[:-1][np.diff(ring_offsets) > 0]
    if polygon_offsets is not None:
        polygon_of_ring = np.repeat(np.arange(len(polygon_offsets) - 1), np.diff(polygon_offsets))
        owner = polygon_of_ring[owner]
    return np.stack((coords, coords[nxt]), axis=1), owner


def line_segments(coords, line_offsets):
    """(segments (n, 2, 2), line (n,)): consecutive vertices of one line (burn.py:166-178)."""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 2)
    line_offsets = np.asarray(line_offsets, dtype=np.int64)
    index = np.repeat(np.arange(line_offsets.size - 1), np.diff(line_offsets))
    valid = np.diff(index) == 0
    return np.stack((coords[:-1][valid], coords[1:][valid]), axis=1), index[1:][valid]


def points_in_segments(points, segments, tol, chunk_elements=1 << 21):
    """bool (n_point,): the rule of the module docstring over ``segments (n, 2, 2)``, chunked over the points."""
    points = np.asarray(points, dtype=np.float64)
    out = np.zeros(points.shape[0], dtype=bool)
    v0x, v0y, v1x, v1y = segments[:, 0, 0], segments[:, 0, 1], segments[:, 1, 0], segments[:, 1, 1]
    wx, wy = v1x - v0x, v1y - v0y
    len2 = wx * wx + wy * wy
    keep = len2 > 0
    v0x, v0y, v1y, wx, wy, len2 = v0x[keep], v0y[keep], v1y[keep], wx[keep], wy[keep], len2[keep]
    if len2.size == 0:
        return out
    reach = tol * np.sqrt(len2)
    step = max(1, chunk_elements // len2.size)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i0 in range(0, points.shape[0], step):
            px, py = points[i0:i0 + step, 0, None], points[i0:i0 + step, 1, None]
            ux, uy = px - v0x, py - v0y
            twice_area = np.abs(wx * uy - wy * ux)
            tpar = ux * wx + uy * wy
            on_edge = (twice_area < reach) & (tpar >= 0) & (tpar <= len2)
            crossing = ((v0y > py) != (v1y > py)) & (px < wx * (py - v0y) / wy + v0x)
            out[i0:i0 + step] = on_edge.any(axis=1) | (crossing.sum(axis=1) % 2 == 1)
    return out


def polygon_winner_numpy(centroids, coords, ring_offsets, polygon_offsets, tol):
    """Per face the highest index of a polygon whose segments its centroid passes, -1 for none."""
    segments, owner = ring_segments(coords, ring_offsets, polygon_offsets)
    winner = np.full(np.shape(centroids)[0], -1, dtype=np.int64)
    for g in range(len(polygon_offsets) - 1):  # (ascending: later polygons overwrite earlier ones)
        winner[points_in_segments(centroids, segments[owner == g], tol)] = g
    return winner


def interior_pairs(nodes, faces, segments, pairs):
    """The (segment, face) ``pairs`` without those whose segment lies exactly on the line of an edge of the (convex) face:
    such a piece runs along the face's boundary and does not make the face "touched" by a polygon."""
    segment_index, face_index = (np.asarray(a) for a in pairs)
    nodes, faces = np.asarray(nodes, dtype=np.float64), np.asarray(faces)
    along = np.zeros(segment_index.size, dtype=bool)
    s0, s1 = segments[segment_index, 0], segments[segment_index, 1]
    for k, f in enumerate(face_index):
        ring = nodes[faces[f][faces[f] >= 0]]
        a, b = ring, np.roll(ring, -1, axis=0)
        ex, ey = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
        c0 = ex * (s0[k, 1] - a[:, 1]) - ey * (s0[k, 0] - a[:, 0])
        c1 = ex * (s1[k, 1] - a[:, 1]) - ey * (s1[k, 0] - a[:, 0])
        along[k] = (((ex != 0) | (ey != 0)) & (c0 == 0) & (c1 == 0)).any()
    return segment_index[~along], face_index[~along]


def touched_winner(winner, owner, pairs):
    """``winner`` with the owners of the (segment, face) ``pairs`` of positive length folded in: per face the maximum."""
    segment_index, face_index = pairs
    out = winner.copy()
    np.maximum.at(out, face_index, owner[segment_index])
    return out


def burn_numpy(centroids, tol, fill=np.nan, polygons=None, polygon_pairs=None, lines=None, line_pairs=None, points=None,
               point_faces=None):
    """Last write wins, polygons then lines then points (burn.py:253-260), on the yardstick's polygon rule and on GIVEN
    (segment, face) pairs -- ``polygon_pairs`` over ``ring_segments`` for all_touched, ``line_pairs`` over ``line_segments``
    -- and GIVEN faces of the points (-1: outside, burns nothing)."""
    out = np.full(np.shape(centroids)[0], fill, dtype=np.float64)

    def values_of(parts, n_fixed, count):
        return np.ones(count) if len(parts) == n_fixed else np.asarray(parts[n_fixed], dtype=np.float64)

    if polygons is not None:
        coords, ring_offsets, polygon_offsets = polygons[:3]
        winner = polygon_winner_numpy(centroids, coords, ring_offsets, polygon_offsets, tol)
        if polygon_pairs is not None:
            winner = touched_winner(winner, ring_segments(coords, ring_offsets, polygon_offsets)[1], polygon_pairs)
        values = values_of(polygons, 3, len(polygon_offsets) - 1)
        out[winner >= 0] = values[winner[winner >= 0]]
    if lines is not None:
        coords, line_offsets = lines[:2]
        _, owner = line_segments(coords, line_offsets)
        values = values_of(lines, 2, len(line_offsets) - 1)
        segment_index, face_index = line_pairs
        winner = np.full(out.size, -1, dtype=np.int64)
        np.maximum.at(winner, face_index, owner[segment_index])
        out[winner >= 0] = values[winner[winner >= 0]]
    if points is not None:
        values = values_of(points, 1, np.shape(points[0])[0])
        point_faces = np.asarray(point_faces)
        winner = np.full(out.size, -1, dtype=np.int64)
        np.maximum.at(winner, point_faces[point_faces >= 0], np.nonzero(point_faces >= 0)[0])
        out[winner >= 0] = values[winner[winner >= 0]]
    return out


def ragged(rings_per_polygon):
    """[[ring, ...], ...] -> (coords, ring_offsets, polygon_offsets), the layout of shapely.to_ragged_array."""
    rings = [np.asarray(ring, dtype=np.float64).reshape(-1, 2) for polygon in rings_per_polygon for ring in polygon]
    coords = np.concatenate(rings) if rings else np.zeros((0, 2))
    ring_offsets = np.concatenate(([0], np.cumsum([len(ring) for ring in rings]))).astype(np.int64)
    polygon_offsets = np.concatenate(([0], np.cumsum([len(polygon) for polygon in rings_per_polygon]))).astype(np.int64)
    return coords, ring_offsets, polygon_offsets


def closed(ring):
    ring = np.asarray(ring, dtype=np.float64)
    return np.concatenate((ring, ring[:1]))


# the polygons of the reference's test_locate_polygon / test_locate_polygon_with_hole (tests/test_burn.py:81-118):
# (exterior, interiors, faces with all_touched=False, faces with all_touched=True)
LOCATE_POLYGON_CASES = (
    ([(0.5, 0.5), (2.5, 0.5), (0.5, 2.5)], [], [0, 1, 2, 3, 4, 6], [0, 1, 2, 3, 4, 6]),
    ([(0.75, 0.5), (2.5, 0.5), (0.75, 2.5)], [], [1, 2, 4], [0, 1, 2, 3, 4, 5, 6, 7]),
    ([(0.7, 0.7), (2.3, 0.7), (1.5, 2.3)], [[(1.4, 1.6), (1.5, 1.4), (1.6, 1.6)]], [], [0, 1, 2, 3, 4, 5, 7]),
)


def reference_burn_case():
    """tests/test_burn.py:17-79 of the reference: the 3 x 3 grid of unit quads (face id = 3 row + column) with its two
    polygons (closed rings, as shapely hands them out), three lines and three points.  -> dict of ``nodes``, ``faces``,
    ``polygons`` / ``lines`` / ``points`` (array tuples with values) and the expected outputs of tests/test_burn.py:120-195."""
    nodes, faces, _, _, lines_expected = burn_lines_case()
    square = closed([(0.0, 0.0), (2.0, 0.0), (2.0, 2.0), (0.0, 2.0)])
    ell = closed([(0.0, 2.0), (2.0, 2.0), (2.0, 0.0), (3.0, 0.0), (3.0, 3.0), (0.0, 3.0)])
    polygons = ragged([[square], [ell]]) + (np.array([0.0, 1.0]),)
    line_xy = np.array([[0.5, 0.5], [2.5, 0.5], [1.2, 1.5], [1.8, 1.5], [0.2, 2.2], [0.8, 2.8], [1.2, 2.2], [1.8, 2.8]])
    lines = (line_xy, np.array([0, 2, 4, 8], dtype=np.int64), np.array([0.0, 1.0, 2.0]))
    points = (np.array([[0.5, 0.5], [1.5, 0.5], [2.5, 2.5]]), np.array([0.0, 1.0, 3.0]))
    return dict(
        nodes=nodes, faces=faces, polygons=polygons, lines=lines, points=points,
        polygons_expected=np.array([0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0]),
        lines_expected=lines_expected,                                              # fill -1
        points_expected=np.array([0.0, 1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, 3.0]),  # fill -1
        mixed_expected=np.array([20.0, 21.0, 10.0, 0.0, 11.0, 1.0, 12.0, 12.0, 23.0]),  # lines + 10, points + 20
    )


def mixed_frame(case):
    """The mixed GeoDataFrame of tests/test_burn.py:180-195: line values + 10, point values + 20."""
    lines, points = case["lines"], case["points"]
    return case["polygons"], lines[:2] + (lines[2] + 10.0,), points[:1] + (points[1] + 20.0,)


# ---- the polygons of the tests at size (unit square meshes) -----------------------------------------------------------------
def star(centre, r_outer, r_inner, n_vertex, phase=0.0):
    angle = phase + 2.0 * np.pi * np.arange(n_vertex) / n_vertex
    r = np.where(np.arange(n_vertex) % 2 == 0, r_outer, r_inner)
    return np.column_stack((centre[0] + r * np.cos(angle), centre[1] + r * np.sin(angle)))


def at_size_polygons(seed=7):
    """60 random, overlapping polygons of 3 to 40 vertices (star-shaped about a random centre, some closed, some open), one
    star of 2000 vertices with two holes, and one tiny triangle (placed by the caller inside a single face: polygon 61)."""
    rng = np.random.default_rng(seed)
    polygons = []
    for k in range(60):
        n = int(rng.integers(3, 41))
        centre = rng.uniform(0.1, 0.9, 2)
        angle = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
        r = rng.uniform(0.03, 0.3, n)
        ring = np.column_stack((centre[0] + r * np.cos(angle), centre[1] + r * np.sin(angle)))
        polygons.append([closed(ring) if k % 2 else ring])
    hole_a = star((0.42, 0.5), 0.05, 0.03, 12)[::-1]
    hole_b = closed(star((0.6, 0.55), 0.04, 0.04, 9)[::-1])
    polygons.append([star((0.5, 0.5), 0.45, 0.2, 2000, 0.1), hole_a, hole_b])
    return polygons

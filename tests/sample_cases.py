"""Shared case builders and host yardsticks of the sampling tests (test_sample_cpu.py, test_gpu_sample.py): a brute-force
nearest search with the kernel's own arithmetic and tie rule, scipy's KDTree as the reference's route
(xugrid/ugrid/ugridbase.py:1261-1303), a numpy restatement of the section coordinates (ugridbase.py:1438-1452,
selection_utils.py:27-32) and the length of a line inside a convex hull."""
import numpy as np
from scipy.spatial import ConvexHull, KDTree

from network_cases import line_selection_cases


def grid2d_arrays():
    """The seven-node, four-face mesh of the reference's tests/test_ugrid2d.py (two unit quads under two triangles)."""
    nodes, faces, _ = line_selection_cases()
    return nodes, faces


def brute_nearest(points, queries, max_distance=np.inf, chunk=1024):
    """Id of the nearest of ``points`` per query, or -1: squared distance ``dx*dx + dy*dy`` in float64 (the kernel's
    arithmetic, no fused multiply-add), kept only STRICTLY below ``max_distance**2``, the lowest id among equal distances
    (``argmin`` returns the first minimum), -1 for a NaN query."""
    points = np.asarray(points, dtype=np.float64)
    queries = np.asarray(queries, dtype=np.float64).reshape(-1, 2)
    md2 = np.inf if np.isinf(max_distance) else max_distance * max_distance
    out = np.full(queries.shape[0], -1, dtype=np.int64)
    for i0 in range(0, queries.shape[0], chunk):
        q = queries[i0:i0 + chunk]
        dx = points[None, :, 0] - q[:, None, 0]
        dy = points[None, :, 1] - q[:, None, 1]
        d2 = dx * dx + dy * dy
        d2 = np.where(d2 < md2, d2, np.inf)  # (NaN compares false: a NaN query keeps nothing)
        j = np.argmin(d2, axis=1)
        found = np.isfinite(d2[np.arange(q.shape[0]), j])
        out[i0:i0 + chunk] = np.where(found, j, -1)
    return out


def kdtree_nearest(points, queries, max_distance=np.inf):
    """The reference's route: ``KDTree.query(distance_upper_bound=max_distance)``, a miss (index n) as -1.
    -> (index, unique): ``unique`` marks the queries whose nearest neighbour is unique in float64 -- the squared distances
    of scipy's first and second hit (k = 2, no bound) differ."""
    points = np.asarray(points, dtype=np.float64)
    tree = KDTree(points)
    _, index = tree.query(queries, distance_upper_bound=max_distance, workers=16)
    index = np.where(index == points.shape[0], -1, index).astype(np.int64)
    if points.shape[0] < 2:
        return index, np.ones(len(index), dtype=bool)
    _, two = tree.query(queries, k=2, workers=16)
    d = points[two] - np.asarray(queries, dtype=np.float64)[:, None, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    return index, d2[:, 0] != d2[:, 1]


def section_numpy(pieces, piece_segment, segments):
    """Midpoints (n, 2) and distance along the line s (n,) of clipped pieces (n, 2, 2): mid = 0.5 (p0 + p1),
    s = |mid - start of the piece's segment| + the summed length of the segments in front of it."""
    pieces = np.asarray(pieces, dtype=np.float64).reshape(-1, 2, 2)
    segments = np.asarray(segments, dtype=np.float64).reshape(-1, 2, 2)
    seg = np.asarray(piece_segment, dtype=np.int64)
    d = segments[:, 1] - segments[:, 0]
    length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    cumulative = np.zeros(len(segments))
    np.cumsum(length[:-1], out=cumulative[1:])
    mid = 0.5 * (pieces[:, 0] + pieces[:, 1])
    dm = mid - segments[seg, 0]
    return mid, np.sqrt(dm[:, 0] * dm[:, 0] + dm[:, 1] * dm[:, 1]) + cumulative[seg]


def length_inside_hull(points, segments):
    """Summed length of the parts of ``segments`` (m, 2, 2) inside the convex hull of ``points`` (Cyrus-Beck against the
    hull's counter-clockwise polygon)."""
    poly = np.asarray(points)[ConvexHull(points).vertices]  # (counter-clockwise in 2-D)
    a, b = poly, np.roll(poly, -1, axis=0)
    normal = np.column_stack([-(b[:, 1] - a[:, 1]), b[:, 0] - a[:, 0]])  # inward for a CCW polygon
    total = 0.0
    for p0, p1 in np.asarray(segments, dtype=np.float64):
        d = p1 - p0
        t0, t1 = 0.0, 1.0
        for ai, ni in zip(a, normal):
            num, den = np.dot(ni, p0 - ai), np.dot(ni, d)  # inside: num + t den >= 0
            if den == 0.0:
                if num < 0.0:
                    t0, t1 = 1.0, 0.0
            elif den > 0.0:
                t0 = max(t0, -num / den)
            else:
                t1 = min(t1, -num / den)
        if t1 > t0:
            total += (t1 - t0) * np.hypot(d[0], d[1])
    return total

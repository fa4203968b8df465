"""
Known answers of the line snapping tests: what the reference's own ``snap_to_edges`` (xugrid/ugrid/snapping.py:255-325) and the
code around it (:426-493, :540-542) give for the cases of tests/snapgrid_cases.py.

Runs ONLY on the build machine (needs the reference checkout next to the repository):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python -B <repo>/tests/golden/gen_snapgrid.py

snapping.py cannot be imported (top-level ``import xarray``, geopandas), so ``snap_to_edges``, ``lines_as_edges``, ``left_of``,
``to_vector``, ``as_point``, ``snap_to_nodes`` and ``_snap_to_nearest`` are lifted out of it with ``ast`` at run time;
``xugrid.ugrid.connectivity``, ``xugrid.core.sparse`` and ``xugrid.constants`` are imported (numba is absent: the reference's own
no-op decorator stands in).  The pieces come from the oracle's ``CellTree2d.intersect_edges`` (numba_celltree is absent); the
centroids, edges and adjacency from the reference's connectivity module; the frame and the winners are put together with pandas as
the reference does.  Only DATA is written: tests/golden/snapgrid_known.json.  The expected values of the reference's own tests
(tests/test_snap.py:184-329) are part of the file as data.
"""
import ast
import json
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd
from scipy.spatial import cKDTree

warnings.simplefilter("ignore")
OUT = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(OUT))
REF = os.environ.get("XUGRID_REFERENCE", os.path.join(os.path.dirname(REPO), "reference"))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, REPO)

pkg = types.ModuleType("xugrid")
pkg.__path__ = [f"{REF}/xugrid"]
sys.modules["xugrid"] = pkg
from xugrid.constants import NoOpNumba, Point, Vector  # noqa: E402
from xugrid.core.sparse import MatrixCSR, columns_and_values, row_slice  # noqa: E402
from xugrid.ugrid import connectivity  # noqa: E402
from xugrid.ugrid.connectivity import AdjacencyMatrix  # noqa: E402

import snapgrid_cases as sg  # noqa: E402
from oracle import oracle  # noqa: E402

IntDType = np.intp


def lift(path, names):
    fns = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in names]
    for fn in fns:
        fn.returns = None
        for a in fn.args.args + fn.args.kwonlyargs:
            a.annotation = None
    return fns


ns = {"np": np, "pd": pd, "cKDTree": cKDTree, "numba": NoOpNumba, "MatrixCSR": MatrixCSR, "columns_and_values": columns_and_values,
      "row_slice": row_slice, "Point": Point, "Vector": Vector, "connectivity": connectivity}
LIFTED = ("_snap_to_nearest", "snap_to_nodes", "to_vector", "as_point", "lines_as_edges", "left_of", "snap_to_edges")
exec(compile(ast.Module(body=lift(f"{REF}/xugrid/ugrid/snapping.py", LIFTED), type_ignores=[]), "reference", "exec"), ns)


def frame_and_winners(node_xy, faces, coords, offsets, max_snap_distance, tolerance=1e-12):
    """snapping.py:426-493 and :540-542 with arrays in place of the GeoDataFrame and the oracle in place of the celltree."""
    faces = faces.astype(IntDType)
    _, face_edge = connectivity.edge_connectivity(faces)
    A = connectivity.to_sparse(face_edge)
    n, m = A.shape
    face_edge_adjacency = AdjacencyMatrix(A.indices, A.indptr, A.nnz, n, m)
    edge_face = connectivity.invert_dense(face_edge)
    if edge_face.shape[1] < 2:
        edge_face = np.column_stack([edge_face, np.full(len(edge_face), -1, dtype=IntDType)])
    centroids = connectivity.centroids(faces, node_xy[:, 0], node_xy[:, 1])
    vertex_line = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    empty = dict(line_index=[], edge_index=[], x0=[], y0=[], x1=[], y1=[], length=[], edges=[], edge_lines=[])
    if len(coords) < 2:
        return empty
    x, y = ns["snap_to_nodes"](coords[:, 0], coords[:, 1], node_xy[:, 0], node_xy[:, 1], max_snap_distance, tiebreaker="nearest")
    line_edges, segment_line = ns["lines_as_edges"](np.column_stack([x, y]), vertex_line)
    line_index, face_indices, segment_edges = oracle.CellTree2d(node_xy, faces).intersect_edges(line_edges)
    size = len(face_indices) * faces.shape[1] + 1
    edge_index, segment_index = ns["snap_to_edges"](face_indices, segment_edges, face_edge_adjacency, edge_face, centroids,
                                                    np.empty(size, dtype=IntDType), np.empty(size, dtype=IntDType), tolerance)
    line_index = line_index[segment_index]
    segment_edges = segment_edges[segment_index]
    result = pd.DataFrame(data={
        "line_index": segment_line[line_index],
        "edge_index": edge_index,
        "x0": segment_edges[:, 0, 0],
        "y0": segment_edges[:, 0, 1],
        "x1": segment_edges[:, 1, 0],
        "y1": segment_edges[:, 1, 1],
        "length": ((segment_edges[:, 1] - segment_edges[:, 0]) ** 2).sum(axis=1),
    })
    out = {k: result[k].to_numpy() for k in sg.COLUMNS}
    if len(result):
        rows = result.groupby("edge_index").idxmax()["length"].to_numpy()
        out["edges"] = result["edge_index"].to_numpy()[rows]
        out["edge_lines"] = result["line_index"].to_numpy()[rows]
    else:
        out["edges"], out["edge_lines"] = [], []
    return out


def text(result):
    return {k: ([float(x) for x in np.asarray(v)] if np.asarray(v).dtype.kind == "f" and len(v) else [int(x) for x in np.asarray(v)])
            for k, v in result.items()}


# tests/test_snap.py:184-261, as they stand there: the counts of np.unique(uds["line_index"], return_counts=True), NaN last
EXPECTED_COUNTS = {
    "ref_single_line": [8, 172],
    "ref_single_line_at_edge": [8, 172],
    "ref_parallel_lines": [8, 8, 164],
    "ref_series_lines": [2, 2, 2, 2, 172],
    "ref_crossing_lines": [8, 8, 164],
    "ref_closely_parallel": [8, 172],
    "ref_line_hits_edge_centroid": [1, 179],
}
# :290-329: the lines at x = 19 and x = 21 carry [1, 2]; both name the same edges, and the sum per snapped edge is 3
DOCSTRING = {"case": "ref_closely_parallel", "my_variable": [1.0, 2.0], "sum_per_edge": 3.0}


def main():
    out = {"cases": {}, "reference_test": {"line_counts": EXPECTED_COUNTS, "docstring": DOCSTRING}}
    for name, case in sg.CASES.items():
        node_xy, faces, coords, offsets, d = case()
        result = frame_and_winners(node_xy, faces, coords, offsets, d)
        out["cases"][name] = text(result)
        print(name, "rows", len(result["edge_index"]), "edges", len(result["edges"]))
    with open(os.path.join(OUT, "snapgrid_known.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

"""
Known answers of the merge tests: what the reference's own functions return for the small cases of tests/partition_cases.py.

Runs ONLY on the build machine (needs the reference checkout next to the repository):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python -B <repo>/tests/golden/gen_partition.py

partitioning.py itself cannot be imported (top-level ``import xarray``), so ``labels_to_indices``, ``merge_nodes``,
``_merge_connectivity``, ``merge_faces`` and ``merge_edges`` are lifted out of the file with ``ast`` at run time and run on stub
grid objects that carry the attributes those functions read; ``connectivity.index_like`` and ``connectivity.edge_connectivity``
are imported.  Only DATA is written: tests/golden/partition_known.json (inputs come from partition_cases, outputs from the
reference).  NaN coordinates are written as the string "nan".
"""
import ast
import json
import os
import sys
import types
import warnings
from itertools import accumulate, chain

import numpy as np

warnings.simplefilter("ignore")
REF = os.environ.get("XUGRID_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

pkg = types.ModuleType("xugrid")
pkg.__path__ = [f"{REF}/xugrid"]
sys.modules["xugrid"] = pkg
from xugrid.ugrid import connectivity  # noqa: E402

import partition_cases as pc  # noqa: E402

src = open(f"{REF}/xugrid/ugrid/partitioning.py").read()
WANT = {"labels_to_indices", "merge_nodes", "_merge_connectivity", "merge_faces", "merge_edges"}
fns = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in WANT]
ns = {"np": np, "accumulate": accumulate, "chain": chain, "renumber": connectivity.renumber, "FILL_VALUE": -1, "IntDType": np.intp,
      "IntArray": np.ndarray, "List": list}
exec(compile(ast.Module(body=fns, type_ignores=[]), "partitioning", "exec"), ns)


class Grid:
    def __init__(self, xy, faces):
        self.node_x, self.node_y, self.face_node_connectivity = xy[:, 0], xy[:, 1], faces
        self.n_node, self.n_face, self.n_max_node_per_face = len(xy), len(faces), faces.shape[1]
        self.edge_node_connectivity = (connectivity.edge_connectivity(faces)[0] if len(faces) else np.zeros((0, 2), dtype=np.intp))
        self.n_edge = len(self.edge_node_connectivity)


def plain(a):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return [plain(row) for row in a] if a.ndim > 1 else [("nan" if np.isnan(v) else ("-0.0" if v == 0 and np.signbit(v) else float(v))) for v in a]
    return a.tolist()


def main():
    out = {"merge": {}, "index_like": {}}
    for name in pc.GOLDEN_CASES:
        grids = [Grid(xy, faces) for xy, faces in pc.partitions(name)]
        xy, node_indexes, node_inverse = ns["merge_nodes"](grids)
        faces, face_indexes = ns["merge_faces"](grids, node_inverse)
        edges, edge_indexes = ns["merge_edges"](grids, node_inverse)
        out["merge"][name] = dict(
            xy=plain(xy), node_indexes=[plain(i) for i in node_indexes], node_inverse=plain(node_inverse), faces=plain(faces),
            face_indexes=[plain(i) for i in face_indexes], edge_indexes=[plain(i) for i in edge_indexes],
            kept_edges_sorted=plain(np.sort(edges, axis=1)),
        )
        print(name, "nodes", len(xy), "faces", len(faces), "kept edges", len(edges))
    out["labels_to_indices"] = {"labels": [0, 1, 0, 2, 2], "indices": [plain(i) for i in ns["labels_to_indices"](np.array([0, 1, 0, 2, 2]))]}
    rows = np.array([[0.0, 1.0], [-0.0, 1.0], [np.nan, 1.0], [np.nan, 1.0], [2.0, -0.0], [2.0, 0.0]])
    u, index, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    out["unique_rows"] = {"rows": plain(rows), "n_unique": len(u), "index": plain(index), "inverse": plain(inverse.ravel())}
    for name, (a, b, tolerance) in pc.like_cases().items():
        out["index_like"][name] = {"index": plain(connectivity.index_like(a, b, tolerance)), "tolerance": tolerance}
    with open(os.path.join(OUT, "partition_known.json"), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

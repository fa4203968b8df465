"""
Known answers of the periodic tests: what the reference's own ``Ugrid2d.to_periodic`` and ``Ugrid2d.to_nonperiodic`` return for the
dense cases of tests/periodic_cases.py.

Runs ONLY on the build machine (needs the reference checkout next to the repository):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python -B <repo>/tests/golden/gen_periodic.py

ugrid2d.py itself cannot be imported (top-level ``import xarray``), so the two methods are lifted out of the class with ``ast`` at
run time and run on stub grids that carry the attributes they read; ``connectivity`` is imported.  ``obj`` is a stub whose
``isel`` hands the indexes back, ``pd`` a stub whose indexes are arrays.  Every grid gets DERIVED edges
(``connectivity.edge_connectivity``), the numbering grids of this project have; ``to_nonperiodic`` is fed the periodic grid the
reference returned.  Only DATA is written: tests/golden/periodic_known.json (inputs come from periodic_cases, outputs from the
reference); of a case with more than DIGEST_FROM faces every array is written as its shape, dtype and the SHA-256 of its bytes
instead of its values (periodic_cases.equals_known compares either form).  Fill slots never go to the reference (it maps them
to the last node: DESIGN section 7).
"""
import ast
import hashlib
import json
import os
import sys
import types
import warnings

import numpy as np

warnings.simplefilter("ignore")
OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("XUGRID_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference"))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

pkg = types.ModuleType("xugrid")
pkg.__path__ = [f"{REF}/xugrid"]
sys.modules["xugrid"] = pkg
from xugrid.ugrid import connectivity  # noqa: E402

import periodic_cases as pc  # noqa: E402

DIMS = ("node", "edge", "face")


class Grid:
    """What the two methods read of a Ugrid2d, and what they construct."""

    node_dimension, edge_dimension, face_dimension = DIMS
    name, _indexes, is_projected, crs, attrs = "mesh2d", None, False, None, None

    def __init__(self, node_x, node_y, face_node_connectivity, edge_node_connectivity=None, **ignored):
        self.node_x, self.node_y = np.asarray(node_x, dtype=np.float64), np.asarray(node_y, dtype=np.float64)
        self.face_node_connectivity = np.asarray(face_node_connectivity, dtype=np.intp)
        self.n_node, self.n_face = len(self.node_x), len(self.face_node_connectivity)
        self.given_edges = edge_node_connectivity  # (what to_periodic hands its result; the grid derives its own below)
        try:
            self._edge_node_connectivity = connectivity.edge_connectivity(self.face_node_connectivity)[0]
        except ValueError:  # (the faces the reference makes of a mixed mesh: no valid topology, never asked for its edges)
            self._edge_node_connectivity = None

    edge_node_connectivity = property(lambda self: self._edge_node_connectivity)
    node_coordinates = property(lambda self: np.column_stack([self.node_x, self.node_y]))  # (a fresh array per call)
    face_node_coordinates = property(lambda self: self.node_coordinates[self.face_node_connectivity])
    bounds = property(lambda self: (self.node_x.min(), self.node_y.min(), self.node_x.max(), self.node_y.max()))

    def _propagate_properties(self, other):
        pass


class Obj:
    dims = DIMS

    def isel(self, **indexes):
        return {k: np.asarray(v) for k, v in indexes.items()}


pd = types.SimpleNamespace(RangeIndex=lambda start, stop: np.arange(start, stop), Index=np.asarray)

src = open(f"{REF}/xugrid/ugrid/ugrid2d.py").read()
cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "Ugrid2d")
fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("to_periodic", "to_nonperiodic")]
for fn in fns:
    fn.returns = None
    for a in fn.args.args:
        a.annotation = None
ns = {"np": np, "pd": pd, "connectivity": connectivity, "Ugrid2d": Grid, "FILL_VALUE": -1}
exec(compile(ast.Module(body=fns, type_ignores=[]), "ugrid2d", "exec"), ns)


def plain(a):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return [plain(row) for row in a] if a.ndim > 1 else [float(v) for v in a]
    return a.tolist()


DIGEST_FROM = 1000  # faces: a larger case is written as digests of its arrays


def lexicographic(edges):
    """The node pairs (lower, higher) in lexicographic order, each once: the numbering of derived edges."""
    return np.unique(np.sort(edges, axis=1), axis=0)


def record(grid, indexes):
    return dict(xy=grid.node_coordinates, faces=grid.face_node_connectivity, node_index=indexes["node"], edge_index=indexes["edge"],
                face_index=indexes["face"], edges_sorted=lexicographic(grid.edge_node_connectivity))


def both(xy, faces, xmax):
    grid = Grid(xy[:, 0], xy[:, 1], faces)
    periodic, indexes = ns["to_periodic"](grid, Obj())
    out = {"to_periodic": record(periodic, indexes)}
    # the edges the reference itself kept, as node pairs: the new grid's derived edges, in another order
    out["to_periodic"]["given_edges_sorted"] = lexicographic(periodic.given_edges)
    try:
        nonperiodic, indexes = ns["to_nonperiodic"](periodic, xmax, Obj())
        out["to_nonperiodic"] = record(nonperiodic, indexes)
    except ValueError as e:
        out["to_nonperiodic"] = {"raises": str(e)}
    return out


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64 if np.asarray(a).dtype.kind == "f" else np.int64)
    return {"shape": list(a.shape), "dtype": a.dtype.name, "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def text(result, as_digest=False):
    return {k: (v if isinstance(v, (str, bool)) else digest(v) if as_digest else plain(v)) for k, v in result.items()}


def main():
    out = {"cases": {}}
    for name in pc.DENSE_CASES:
        results = both(*pc.mesh(name))
        out["cases"][name] = {direction: text(r, len(pc.mesh(name)[1]) > DIGEST_FROM) for direction, r in results.items()}
        print(name, "periodic nodes", len(results["to_periodic"]["xy"]))
    # the "symmetric edge" mesh of the reference's comment, already periodic
    xy, faces, xmax = pc.symmetric()
    grid = Grid(xy[:, 0], xy[:, 1], faces)
    try:
        nonperiodic, indexes = ns["to_nonperiodic"](grid, xmax, Obj())
        out["symmetric"] = dict(text(record(nonperiodic, indexes)), raises=False)
    except ValueError as e:
        out["symmetric"] = {"raises": str(e)}
    print("symmetric raises:", out["symmetric"]["raises"])
    # the fill slots of a mixed mesh in the reference: every -1 becomes the new id of the LAST node (why no golden holds one)
    xy, faces, _ = pc.mesh("mixed")
    periodic = ns["to_periodic"](Grid(xy[:, 0], xy[:, 1], faces))
    out["mixed_fill_slots_in_the_reference"] = plain(periodic.face_node_connectivity[faces == -1])
    with open(os.path.join(OUT, "periodic_known.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

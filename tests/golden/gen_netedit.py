"""
Known answers of the network-edit tests: what the reference's own ``Ugrid1d.topology_subset``, ``Ugrid1d.remove_self_loops``,
``Ugrid1d.refine_by_vertices`` and ``partitioning.merge_nodes`` / ``merge_edges`` return for the cases of tests/netedit_cases.py.

Runs ONLY on the build machine (needs the reference checkout next to the repository):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python -B <repo>/tests/golden/gen_netedit.py

ugrid1d.py and partitioning.py cannot be imported (top-level ``import xarray``), so the methods and functions are lifted out of
them with ``ast`` at run time and run on stub grids that carry the attributes they read; ``connectivity`` is imported, ``pd`` is a
stub whose indexes are arrays.  ``self.celltree.locate_points`` is STUBBED with the brute-force point-to-segment rule of
netedit_cases.locate_ref (numba_celltree is not available; the rule and the default tolerance are assumptions, DESIGN section
7) -- so the goldens pin everything the reference does AROUND the search, and the search itself only through the reference's own
test answers, which are part of the file as data.  Only DATA is written: tests/golden/netedit_known.json; an array of more than
DIGEST_FROM rows is written as its shape, dtype and the SHA-256 of its bytes (netedit_cases.equals_known compares either
form).  The merge cases with a NaN coordinate never go to the reference: np.unique sorts rows, and a NaN has no place in a sort.
"""
import ast
import json
import os
import sys
import types
import warnings
from itertools import accumulate

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

import netedit_cases as nc  # noqa: E402


class Idx(np.ndarray):
    """What the lifted code reads of a pandas index."""

    def __new__(cls, values):
        return np.asarray(values).view(cls)

    def equals(self, other):
        return bool(np.array_equal(np.asarray(self), np.asarray(other)))


pd = types.SimpleNamespace(Index=Idx, RangeIndex=lambda start, stop: Idx(np.arange(start, stop)))


class Tree:
    def __init__(self, grid):
        self.grid = grid

    def locate_points(self, vertices, tolerance):
        return nc.locate_ref(self.grid.node_coordinates, self.grid.edge_node_connectivity, np.asarray(vertices), tolerance)


class Grid:
    """What the lifted methods read of a Ugrid1d, and what they construct."""

    node_dimension, edge_dimension = "node", "edge"
    name, _indexes, is_projected, crs, _attrs, fill_value = "network1d", None, False, None, None, -1

    def __init__(self, node_x, node_y, fill_value, edge_node_connectivity, **ignored):
        self.node_x, self.node_y = np.asarray(node_x, dtype=np.float64), np.asarray(node_y, dtype=np.float64)
        self.edge_node_connectivity = np.asarray(edge_node_connectivity, dtype=np.intp).reshape(-1, 2)
        self.n_node, self.n_edge = len(self.node_x), len(self.edge_node_connectivity)

    node_coordinates = property(lambda self: np.column_stack([self.node_x, self.node_y]))
    celltree = property(lambda self: Tree(self))

    def _propagate_properties(self, other):
        pass


def lift(path, names, cls=None):
    body = ast.parse(open(path).read()).body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    fns = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    for fn in fns:
        fn.returns = None
        for a in fn.args.args + fn.args.kwonlyargs:
            a.annotation = None
    return fns


ns = {"np": np, "pd": pd, "connectivity": connectivity, "renumber": connectivity.renumber, "Ugrid1d": Grid, "FILL_VALUE": -1,
      "IntDType": np.intp, "accumulate": accumulate, "as_pandas_index": lambda index, n: Idx(index)}
fns = (lift(f"{REF}/xugrid/regrid/utils.py", ("alt_cumsum",))
       + lift(f"{REF}/xugrid/ugrid/ugrid1d.py", ("topology_subset", "remove_self_loops", "refine_by_vertices"), cls="Ugrid1d")
       + lift(f"{REF}/xugrid/ugrid/partitioning.py", ("merge_nodes", "_merge_connectivity", "merge_edges")))
exec(compile(ast.Module(body=fns, type_ignores=[]), "reference", "exec"), ns)


def grid_of(xy, edges):
    return Grid(xy[:, 0], xy[:, 1], -1, edges)


def text(result):
    out = {}
    for k, v in result.items():
        if isinstance(v, list):
            out[k] = [text({"a": a})["a"] for a in v]
            continue
        a = np.asarray(v)
        if len(a) > nc.DIGEST_FROM:
            out[k] = nc.digest(a)
        elif a.dtype.kind == "f":
            out[k] = [[float(x) for x in row] for row in a] if a.ndim > 1 else [float(x) for x in a]
        else:
            out[k] = a.tolist()
    return out


def main():
    out = {"subset": {}, "refine": {}, "merge": {}}
    for name, case in nc.SUBSET_CASES.items():
        xy, edges, index = case()
        sub, indexes = ns["topology_subset"](grid_of(xy, edges), index, return_index=True)
        out["subset"][name] = text(dict(xy=sub.node_coordinates, edges=sub.edge_node_connectivity, node_index=indexes["node"]))
    xy, edges = nc.self_loops()
    sub = ns["remove_self_loops"](grid_of(xy, edges))
    out["remove_self_loops"] = text(dict(xy=sub.node_coordinates, edges=sub.edge_node_connectivity))
    for name, case in nc.REFINE_CASES.items():
        xy, edges, vertices, tolerance, _ = case()
        grid, node_index = ns["refine_by_vertices"](grid_of(xy, edges), vertices, return_index=True, tolerance=tolerance)
        out["refine"][name] = text(dict(xy=grid.node_coordinates, edges=grid.edge_node_connectivity, node_index=node_index))
        print(name, "nodes", grid.n_node, "edges", grid.n_edge)
    # the reference's own test, inputs and answers, as data
    xy, edges, vertices = nc.known()
    out["reference_test"] = dict(text(dict(xy=xy, edges=edges, vertices=vertices)), expected_edges=nc.KNOWN_EDGES,
                                 expected_node_index=nc.KNOWN_NODE_INDEX, offset=[0.01, 0.0], offset_tolerance=0.01)
    for name, case in nc.MERGE_CASES.items():
        parts = case()
        if any(np.isnan(xy).any() for xy, _ in parts):
            continue
        grids = [grid_of(xy, e) for xy, e in parts]
        nodes, node_indexes, inverse = ns["merge_nodes"](grids)
        merged_edges, edge_indexes = ns["merge_edges"](grids, inverse)
        out["merge"][name] = text(dict(xy=nodes, edges=merged_edges, node_inverse=inverse, node_index=list(node_indexes),
                                       edge_index=list(edge_indexes)))
        print(name, "merged nodes", len(nodes), "edges", len(merged_edges))
    with open(os.path.join(OUT, "netedit_known.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

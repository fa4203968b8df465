"""
Known answers of the network fill: what the reference's own ``Ugrid1d._nearest_interpolate`` returns for the small cases of
tests/netfill_cases.py (KNOWN_CASES), on the nodes and on the edges.

Runs ONLY on the build machine (needs the reference checkout next to the repository):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python -B <repo>/tests/golden/gen_netfill.py

ugrid1d.py itself cannot be imported (top-level ``import xarray``), so the method is lifted out of the class with ``ast`` at run
time and run on a stub grid that carries the attributes it reads; ``connectivity`` is imported.  Only DATA is written:
tests/golden/netfill_known.json (inputs come from netfill_cases, outputs from the reference; NaN is written as null).
"""
import ast
import json
import os
import sys
import types
import warnings

import numpy as np
from scipy import sparse

warnings.simplefilter("ignore")
OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("XUGRID_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference"))
sys.path.insert(0, os.path.dirname(OUT))

pkg = types.ModuleType("xugrid")
pkg.__path__ = [f"{REF}/xugrid"]
sys.modules["xugrid"] = pkg
from xugrid.ugrid import connectivity  # noqa: E402

import netfill_cases as nc  # noqa: E402


class Grid:
    """What the method reads of a Ugrid1d."""

    node_dimension, edge_dimension = "node", "edge"

    def __init__(self, xy, edges):
        self.xy, self.edges = xy, edges.astype(np.intp)

    @property
    def edge_length(self):
        return nc.edge_length(self.xy, self.edges)

    @property
    def node_node_connectivity(self):
        return connectivity.node_node_connectivity(self.edges)

    @property
    def edge_edge_connectivity(self):
        node_edge = connectivity.invert_dense_to_sparse(self.edges)
        return connectivity.edge_edge_connectivity(self.edges, node_edge)


src = open(f"{REF}/xugrid/ugrid/ugrid1d.py").read()
cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "Ugrid1d")
fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_nearest_interpolate"]
for fn in fns:
    fn.returns = None
    for a in fn.args.args:
        a.annotation = None
ns = {"np": np, "sparse": sparse}
exec(compile(ast.Module(body=fns, type_ignores=[]), "ugrid1d", "exec"), ns)


def main():
    out = {"cases": {}}
    for name, (make, fraction, max_distance) in nc.KNOWN_CASES.items():
        xy, edges = make()
        grid = Grid(xy, edges)
        for facet in ("node", "edge"):
            data = nc.masked_data(nc.n_of(xy, edges, facet), fraction, seed=11)
            limit = np.inf if max_distance is None else max_distance
            filled = ns["_nearest_interpolate"](grid, data, facet, limit)
            out["cases"][f"{name}-{facet}"] = [None if np.isnan(v) else float(v) for v in filled]
            print(name, facet, "NaN before", int(np.isnan(data).sum()), "after", int(np.isnan(filled).sum()))
    with open(os.path.join(OUT, "netfill_known.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

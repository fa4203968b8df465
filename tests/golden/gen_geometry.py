"""
Known answers of the geometry tests: what the reference's own ``conversion.bounds2d_to_topology2d``, ``infer_interval_breaks``,
``polygons_to_faces``, ``linestrings_to_edges`` and ``Ugrid2d._from_intervals_helper`` return for the cases of
tests/geometry_cases.py.

Runs ONLY on the build machine (needs the reference checkout next to the repository):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python -B <repo>/tests/golden/gen_geometry.py

conversion.py and ugrid2d.py cannot be imported (top-level ``import xarray``), so the functions are lifted out with ``ast`` at
run time; ``connectivity`` is imported.  ``shapely`` is a stub whose ``get_coordinates(geometry, return_index=True)`` hands
back the arrays a ``Ragged`` geometry carries.  Only DATA is written: tests/golden/geometry_known.json (inputs come from
geometry_cases, outputs from the reference).
"""
import ast
import json
import os
import sys
import types
import warnings

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("XUGRID_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference"))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

pkg = types.ModuleType("xugrid")
pkg.__path__ = [f"{REF}/xugrid"]
sys.modules["xugrid"] = pkg
from xugrid.ugrid import connectivity  # noqa: E402

import geometry_cases as gc  # noqa: E402


class Ragged:
    """A stand-in for an array of shapely geometries: the vertices and the geometry each belongs to."""

    def __init__(self, coords, offsets):
        self.coords, self.n = coords, len(offsets) - 1
        self.index = np.repeat(np.arange(self.n), np.diff(offsets))

    def __len__(self):
        return self.n


shapely = types.SimpleNamespace(get_coordinates=lambda geometry, return_index=False: (geometry.coords, geometry.index))


def lift(path, names, cls=None):
    body = ast.parse(open(path).read()).body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    fns = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    for fn in fns:
        fn.returns, fn.decorator_list = None, []
        for a in fn.args.args:
            a.annotation = None
    return fns


class Made:
    def __init__(self, node_x, node_y, fill_value, face_nodes, name=None):
        self.faces = face_nodes


ns = {"np": np, "warnings": warnings, "shapely": shapely, "cross2d": connectivity.cross2d, "ragged_index": connectivity.ragged_index,
      "IntDType": np.intp, "FILL_VALUE": -1, "Ugrid2d": Made}
functions = lift(f"{REF}/xugrid/conversion.py", ("bounds2d_to_topology2d", "quad_area", "infer_interval_breaks", "_is_monotonic_and_increasing",
                                                 "_remove_last_vertex", "polygons_to_faces", "linestrings_to_edges", "contiguous_xy"))
functions += lift(f"{REF}/xugrid/ugrid/ugrid2d.py", ("_from_intervals_helper",), cls="Ugrid2d")
exec(compile(ast.Module(body=functions, type_ignores=[]), "reference", "exec"), ns)


def plain(a):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return [plain(row) for row in a] if a.ndim > 1 else [float(v) for v in a]
    return a.tolist()


def main():
    out = {"bounds": {}, "breaks": {}, "monotonic": {}, "lattices": {}, "polygons": {}, "lines": {}}
    for name, make in gc.BOUNDS_CASES.items():
        xb, yb = make()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            x, y, faces, index = ns["bounds2d_to_topology2d"](xb, yb)
        out["bounds"][name] = dict(xy=plain(np.column_stack([x, y])), faces=plain(faces), index=plain(index),
                                   warnings=[str(w.message) for w in caught if issubclass(w.category, UserWarning)])
        print(name, len(faces), "faces", len(x), "nodes", plain(index)[:8], len(caught), "warning(s)")
    for name, (ny, nx, x_dec, y_dec) in gc.LATTICE_CASES.items():
        if min(ny, nx) >= 2:  # (the reference's 2-D breaks fail along an axis of one element)
            cx, cy = gc.centres(ny, nx, x_dec, y_dec)
            xv = ns["infer_interval_breaks"](ns["infer_interval_breaks"](cx, axis=1, check_monotonic=True), axis=0)
            yv = ns["infer_interval_breaks"](ns["infer_interval_breaks"](cy, axis=1), axis=0, check_monotonic=True)
            out["breaks"][name] = dict(x=plain(xv), y=plain(yv), x1d=plain(ns["infer_interval_breaks"](cx[0], check_monotonic=True)))
        if name in gc.REFERENCE_LATTICES:
            x, y = gc.axis_lattice(ny, nx, x_dec, y_dec)
            out["lattices"][name] = plain(ns["_from_intervals_helper"](x.ravel(), y.ravel(), nx, ny, "mesh2d").faces)
    for name, coord in (("zigzag", [0.0, 2.0, 1.0]), ("flat", [1.0, 1.0, 2.0]), ("nan", [0.0, np.nan, 1.0])):
        try:
            ns["_is_monotonic_and_increasing"](np.array(coord))
            out["monotonic"][name] = True
        except ValueError as e:
            out["monotonic"][name] = str(e)
    for name, (coords, off) in gc.polygon_cases().items():
        if len(off) < 2:
            continue  # (the reference takes the maximum of an empty array)
        x, y, faces = ns["polygons_to_faces"](Ragged(coords, off))
        out["polygons"][name] = dict(xy=plain(np.column_stack([x, y])), faces=plain(faces))
    for name, (coords, off) in gc.line_cases().items():
        if len(coords) == 0:
            continue
        x, y, edges = ns["linestrings_to_edges"](Ragged(coords, off))
        out["lines"][name] = dict(xy=plain(np.column_stack([x, y])), edges=plain(edges))
    with open(os.path.join(OUT, "geometry_known.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

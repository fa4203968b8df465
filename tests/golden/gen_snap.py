"""
Known answers of the snapping tests: what the reference's own ``snap_nodes`` and ``snap_to_nodes`` (xugrid/ugrid/snapping.py)
return for the cases of tests/snap_cases.py.

Runs ONLY on the build machine (needs the reference checkout next to the repository):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python -B <repo>/tests/golden/gen_snap.py

snapping.py cannot be imported (top-level ``import xarray``, geopandas), so ``_snap_to_nearest``, ``snap_nodes`` and
``snap_to_nodes`` are lifted out of it with ``ast`` at run time; ``xugrid.core.sparse`` and ``xugrid.constants`` are imported
(numba is absent: the reference's own no-op decorator stands in), scipy and pandas are the installed ones.  Only DATA is
written: tests/golden/snap_known.json; an array of more than DIGEST_FROM rows is written as its shape, dtype and the SHA-256 of
its bytes (snap_cases.equals_known compares either form).  The expected values of the reference's own tests (tests/test_snap.py)
are part of the file as data, beside what the lifted functions return for the same inputs.
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
REF = os.environ.get("XUGRID_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference"))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

pkg = types.ModuleType("xugrid")
pkg.__path__ = [f"{REF}/xugrid"]
sys.modules["xugrid"] = pkg
from xugrid.constants import NoOpNumba  # noqa: E402
from xugrid.core.sparse import MatrixCSR, columns_and_values, row_slice  # noqa: E402

import snap_cases as sc  # noqa: E402


def lift(path, names):
    fns = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in names]
    for fn in fns:
        fn.returns = None
        for a in fn.args.args + fn.args.kwonlyargs:
            a.annotation = None
    return fns


ns = {"np": np, "pd": pd, "cKDTree": cKDTree, "numba": NoOpNumba, "MatrixCSR": MatrixCSR, "columns_and_values": columns_and_values,
      "row_slice": row_slice}
exec(compile(ast.Module(body=lift(f"{REF}/xugrid/ugrid/snapping.py", ("_snap_to_nearest", "snap_nodes", "snap_to_nodes")),
                        type_ignores=[]), "reference", "exec"), ns)


def text(result):
    out = {}
    for k, v in result.items():
        if v is None:
            out[k] = None
            continue
        a = np.asarray(v)
        if len(a) > sc.DIGEST_FROM:
            out[k] = sc.digest(a)
        elif a.dtype.kind == "f":
            out[k] = [float(x) for x in a]
        else:
            out[k] = a.tolist()
    return out


# tests/test_snap.py, the expected values as they stand there: (inverse, x, y) per distance; (x, y) per block
EXPECTED_NODES = {
    "ref_horizontal_0.1": (None, [0.0, 1.0, 2.0], [0.0, 0.0, 0.0]),
    "ref_horizontal_1.0": ([0, 0, 1], [0.0, 2.0], [0.0, 0.0]),
    "ref_horizontal_2.0": ([0, 0, 0], [0.0], [0.0]),
    "ref_diagonal_0.1": (None, [0.0, 1.0, 1.5], [0.0, 1.0, 1.5]),
    "ref_diagonal_0.71": ([0, 1, 1], [0.0, 1.0], [0.0, 1.0]),
    "ref_diagonal_1.42": ([0, 1, 1], [0.0, 1.5], [0.0, 1.5]),
    "ref_two_lines_0.1": ([0, 1, 1, 2], [0.0, 1.0, 2.0], [1.0, 0.0, 1.0]),
}
EXPECTED_TWO_LINES_EDGES = [[0, 1], [1, 2]]
EXPECTED_TO = {
    "ref_none_snapped": ([1.0, 2.0, 3.0], [1.0, 2.0, 3.0]),
    "ref_all_snapped": ([1.1, 2.1, 3.1], [1.1, 2.1, 3.1]),
    "ref_take_nearest": ([1.1, 2.1, 3.1], [1.1, 2.1, 3.1]),
    "ref_more_ties": ([1.01, 2.002, 3.01], [1.01, 2.002, 3.01]),
    "ref_exact_ties": ([1.01, 2.002, 3.01], [1.01, 2.002, 3.01]),
    "ref_multiple_ties": ([1.01, 2.002, 3.002], [1.01, 2.002, 3.002]),
}


def main():
    out = {"snap_nodes": {}, "snap_to_nodes": {}, "reference_test": {}}
    for name, case in sc.NODES_CASES.items():
        x, y, d = case()
        inverse, xs, ys = ns["snap_nodes"](x, y, d)
        out["snap_nodes"][name] = text(dict(inverse=inverse, x=xs, y=ys))
        print(name, "kept", len(xs), "of", len(x))
    for name, case in sc.TO_CASES.items():
        x, y, to_x, to_y, d = case()
        entry = {}
        try:
            xs, ys = ns["snap_to_nodes"](x, y, to_x, to_y, d)
            entry["no_tiebreaker"] = text(dict(x=xs, y=ys))
        except ValueError as e:
            entry["no_tiebreaker"] = {"raises": str(e)}
        xs, ys = ns["snap_to_nodes"](x, y, to_x, to_y, d, tiebreaker="nearest")
        entry["nearest"] = text(dict(x=xs, y=ys))
        out["snap_to_nodes"][name] = entry
        print(name, "ties" if "raises" in entry["no_tiebreaker"] else "")
    try:
        ns["snap_to_nodes"](sc._P, sc._P, sc._P, sc._P, 1.0, tiebreaker="first")
    except ValueError as e:
        out["bad_tiebreaker"] = {"tiebreaker": "first", "raises": str(e)}
    # 3.1 as the reference's test writes it: x + 0.1
    expected_to = {k: (list(np.asarray(v[0])), list(np.asarray(v[1]))) for k, v in EXPECTED_TO.items()}
    for k in ("ref_all_snapped", "ref_take_nearest"):
        expected_to[k] = ([float(v) for v in sc._P + 0.1], [float(v) for v in sc._P + 0.1])
    out["reference_test"] = {"snap_nodes": {k: {"inverse": v[0], "x": v[1], "y": v[2]} for k, v in EXPECTED_NODES.items()},
                             "two_lines_edges": EXPECTED_TWO_LINES_EDGES,
                             "snap_to_nodes": {k: {"x": v[0], "y": v[1]} for k, v in expected_to.items()}}
    with open(os.path.join(OUT, "snap_known.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

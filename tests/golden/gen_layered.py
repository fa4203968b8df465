"""
Golden vectors for the vertical overlaps of layered grids: the output of xugrid's own ``overlap_1d_nd``
(xugrid/regrid/overlap_1d.py:162-245) on the inputs where it is a valid oracle -- NaN-free columns of positive thickness
over a shared extent, one pair per target column, bounds that are multiples of 0.25 -- plus its own test case
(tests/test_regrid/test_overlap_1d.py::test_overlap_1d_nd) with the arrays that test expects.

    python tests/golden/gen_layered.py <directory holding the xugrid package>

xugrid's ``__init__`` imports xarray; a stub package whose ``__path__`` points at the checkout lets the two modules the
function needs be imported on their own (numba is optional there: its no-op stand-in is used when absent).  Only DATA is
written (layered_known.json): inputs come from tests/layered_cases.py, so they can be regenerated; the recorded outputs
are the reference's.  The generator asserts that the reference ran on every case it writes.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import layered_cases as C  # noqa: E402


def main(reference_root):
    pkg = types.ModuleType("xugrid")
    pkg.__path__ = [os.path.join(reference_root, "xugrid")]
    sys.modules["xugrid"] = pkg
    from xugrid.regrid.overlap_1d import overlap_1d_nd

    cases = {}

    def add(name, source_bounds, target_bounds, source_index, target_index, expected=None):
        try:
            source, target, overlap = overlap_1d_nd(source_bounds, target_bounds, source_index, target_index)
        except Exception as e:  # noqa: BLE001
            raise AssertionError(f"the reference did not run on case {name}: {e}") from e
        if expected is not None:
            assert np.array_equal(source, expected[0]) and np.array_equal(target, expected[1])
            assert np.allclose(overlap, expected[2])
        nan_to_none = lambda a: [[[None if np.isnan(v) else v for v in layer] for layer in col] for col in a.tolist()]  # noqa: E731
        cases[name] = {
            "source_bounds": nan_to_none(source_bounds), "target_bounds": nan_to_none(target_bounds),
            "source_index": np.asarray(source_index).tolist(), "target_index": np.asarray(target_index).tolist(),
            "source": source.tolist(), "target": target.tolist(), "overlap": overlap.tolist(),
        }
        print(name, len(overlap))

    for n_layer_s, n_layer_t in C.GOLDEN_LAYERS:
        add(f"shared_{n_layer_s}_{n_layer_t}", *C.golden_case(n_layer_s, n_layer_t))
    nan = np.nan
    add(
        "reference_test",
        np.array([[[0.0, 1.0], [2.0, 3.0], [nan, nan], [5.0, 6.0]]]),
        np.array([[[0.0, 10.0], [10.0, 20.0]], [[0.0, 2.5], [nan, nan]]]),
        np.array([0, 0]), np.array([0, 1]),
        expected=([0, 1, 3, 0, 1], [0, 0, 0, 2, 2], [1.0, 1.0, 1.0, 1.0, 0.5]),
    )
    with open(os.path.join(HERE, "layered_known.json"), "w") as f:
        json.dump(cases, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])

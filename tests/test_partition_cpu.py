"""
CPU: the numpy yardsticks of the merge tests (tests/partition_cases.py) give what the reference's own functions recorded in
tests/golden/partition_known.json (tests/golden/gen_partition.py) and the three answers the rule quotes; every ``index_like``
case the GPU tests use has unique keys and equal key sets, where pairing by key and the reference's pairing by sorted position
agree; and the host arithmetic of the key table (xugrid_amd/csrc/xr_merge_keys.h) runs stand-alone under the sanitizers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import partition_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def floats(rows):
    return np.array([[float(v) for v in row] for row in rows], dtype=np.float64).reshape(-1, 2)


@pytest.mark.parametrize("name", pc.GOLDEN_CASES)
def test_merge_restatement_is_the_reference(name):
    k, e = pc.known()["merge"][name], pc.expected(name)
    assert pc.same_bits(e["xy"], floats(k["xy"]))  # bit for bit: the kept zero keeps its sign, NaN stays NaN
    assert np.array_equal(e["faces"], np.array(k["faces"]).reshape(e["faces"].shape))
    assert np.array_equal(e["node_inverse"], k["node_inverse"])
    for key in ("node_indexes", "face_indexes", "edge_indexes"):
        assert len(e[key]) == len(k[key])
        for got, want in zip(e[key], k[key]):
            assert np.array_equal(got, np.array(want, dtype=np.int64)), key
    # the kept edges are edges of the merged grid, at the positions the yardstick names
    kept = np.array(k["kept_edges_sorted"], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(e["edges"][np.concatenate(e["edge_positions"])], kept)
    assert np.array_equal(np.sort(np.concatenate(e["edge_positions"])), np.arange(len(e["edges"])))  # each merged edge once


def test_anchor_answer():
    e = pc.expected("anchor")
    assert len(e["xy"]) == 12
    assert [i.tolist() for i in e["node_indexes"]] == [list(range(10)), [8, 9]]
    assert [i.tolist() for i in e["face_indexes"]] == [[0, 1, 2, 3], [0, 1]]
    assert e["faces"][-2:].tolist() == [[6, 7, 11, 10], [5, 6, 10, 9]]


def test_unique_rows_answer():
    k = pc.known()["unique_rows"]
    rows = floats(k["rows"])
    u, index, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    assert len(u) == k["n_unique"] == 4 and index.tolist() == k["index"] == [0, 4, 2, 3]
    assert inverse.ravel().tolist() == k["inverse"] == [0, 0, 2, 3, 1, 1]
    xy, node_indexes, node_inverse = pc.merge_nodes([(rows, None)])
    assert node_indexes[0].tolist() == [0, 2, 3, 4] and node_inverse.tolist() == [0, 0, 1, 2, 3, 3]
    assert pc.same_bits(xy, rows[[0, 2, 3, 4]])  # 0.0 of row 0 and -0.0 of row 4: the first of each pair, sign kept


def test_labels_answer():
    k = pc.known()["labels_to_indices"]
    assert k["indices"] == [[0, 2], [1], [3, 4]]
    assert [i.tolist() for i in pc.labels_to_indices(k["labels"])] == k["indices"]
    assert [i.tolist() for i in pc.labels_to_indices([2, 0, 2])] == [[1], [], [0, 2]]  # a label that does not occur
    assert pc.labels_to_indices(np.zeros(0, dtype=np.int64)) == []


@pytest.mark.parametrize("name", sorted(pc.like_cases()))
def test_index_like_cases_stay_inside_the_deviation(name):
    a, b, tolerance = pc.like_cases()[name]
    assert pc.like_inside_deviation(a, b, tolerance)
    index = pc.index_like(a, b, tolerance)
    assert np.array_equal(index, pc.known()["index_like"][name]["index"])
    assert (np.abs(a[index] - b) <= tolerance).all()
    if name.startswith("known"):
        assert index.tolist() == [3, 1, 0, 2]


def test_index_like_refusals_of_the_restatement():
    a = np.array([[0.0, 0.0], [1.0, 1.0]])
    with pytest.raises(ValueError, match="do not match in shape"):
        pc.index_like(a, a[:1], 0.0)
    with pytest.raises(ValueError, match="not identical after sorting"):
        pc.index_like(a, np.array([[0.0, 0.0], [1.1, 1.0]]), 0.0)
    with pytest.raises(ValueError, match="not identical after sorting"):
        pc.index_like(np.array([[0.0, 0.0], [0.0, 0.0]]), np.array([[0.0, 0.0], [0.0, 0.0]]), 0.0)


# ---- the host arithmetic of the key table, stand-alone under the sanitizers ----------------------------------------------------
@pytest.fixture(scope="module")
def keys_program(tmp_path_factory):
    compiler = next(c for c in ("c++", "g++", "clang++") if shutil.which(c))
    out = str(tmp_path_factory.mktemp("merge_keys") / "keys")
    source = os.path.join(ROOT, "tests", "native", "merge_keys_main.cpp")
    proc = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", out, source], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return out


def test_key_arithmetic_under_sanitizers(keys_program):
    """The program sorts every row with the network and with the in-place sort, inserts the rows into a table of the smallest
    and of the default capacity by the device's rule (sequentially) and prints the first occurrence of every row: the
    yardstick's, for faces of the cases and for coordinate rows with both zeros and NaN."""
    e = pc.expected("tri3_quad4")
    rows = pc.widened_faces(pc.partitions("tri3_quad4"), e["node_inverse"])
    k = pc.known()["unique_rows"]
    xy = floats(k["rows"])
    text = f"{len(rows)} {rows.shape[1]}\n" + "".join(" ".join(str(v) for v in row) + "\n" for row in rows)
    text += f"{len(xy)}\n" + "".join(f"{x!r} {y!r}\n" for x, y in xy.tolist())
    proc = subprocess.run([keys_program], input=text, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    lines = proc.stdout.strip().split("\n")
    kept, _ = pc.merge_rows(rows, np.array([0, len(rows)]))
    for line in lines[:2]:  # smallest capacity, default capacity
        rep = np.array(line.split(), dtype=np.int64)
        assert np.array_equal(np.nonzero(rep == np.arange(len(rows)))[0], kept)
        assert np.array_equal(np.sort(rows[rep], axis=1), np.sort(rows, axis=1))
    for line in lines[2:4]:
        assert np.array(line.split(), dtype=np.int64).tolist() == [0, 0, 2, 3, 4, 4]
    assert lines[4] == "capacity ok"

"""
CPU: the verdict on one attempt of the fused weight build (xugrid_amd/csrc/xr_overlap_tail.h: fused_outcome) -- the ONE function
k_publish_all sets the gate of an enqueued apply with and overlap_tri decides with after its read-back -- compiled as plain C++
(tests/host_fused_outcome.cpp against tests/host_shim/hip/hip_runtime.h) and table-tested at each boundary and for the
precedence: int32 range, then the general chain (error bit 0), then the big faces' queue, then the CSR's capacity, else final.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP, BIG = 1000, 50  # entries the CSR / pairs the big faces' queue have room for
INT32_MAX = 2**31 - 1

# (c_reg, c_big, n_pending, err, p_regular, p_big, cap, big_capacity) -> verdict
TABLE = [
    # the CSR's capacity: p_regular + p_big == cap fits, one more does not
    ((700, 10, 0, 0, 600, 400, CAP, BIG), "final"),
    ((700, 10, 0, 0, 601, 400, CAP, BIG), "grow_csr"),
    ((700, 10, 0, 0, CAP, 0, CAP, BIG), "final"),
    ((700, 10, 0, 0, CAP + 1, 0, CAP, BIG), "grow_csr"),
    ((700, 10, 0, 0, 0, CAP + 1, CAP, BIG), "grow_csr"),
    # ... summed in 64 bits: two int32 counts beyond 2^31 together do not wrap into "fits"
    ((700, 10, 0, 0, INT32_MAX, INT32_MAX, 2 * INT32_MAX, BIG), "final"),
    ((700, 10, 0, 0, INT32_MAX, INT32_MAX, 2 * INT32_MAX - 1, BIG), "grow_csr"),
    # the big faces' queue: c_big == big_capacity fits, one more does not
    ((700, BIG, 0, 0, 600, 400, CAP, BIG), "final"),
    ((700, BIG + 1, 0, 0, 600, 400, CAP, BIG), "grow_big"),
    # faces that found no room in it
    ((700, 10, 0, 0, 600, 300, CAP, BIG), "final"),
    ((700, 10, 1, 0, 600, 300, CAP, BIG), "grow_big"),
    # the error bits alone
    ((700, 10, 0, 1, 600, 300, CAP, BIG), "general"),
    ((700, 10, 0, 4, 600, 300, CAP, BIG), "grow_csr"),
    ((700, 10, 0, 5, 600, 300, CAP, BIG), "general"),
    # precedence: bit 0 beats everything below it
    ((700, BIG + 1, 1, 1, CAP + 1, 0, CAP, BIG), "general"),
    ((700, BIG + 1, 1, 5, CAP + 1, 0, CAP, BIG), "general"),
    # ... the big queue beats the CSR
    ((700, BIG + 1, 0, 4, 600, 300, CAP, BIG), "grow_big"),
    ((700, 10, 1, 4, CAP, 1, CAP, BIG), "grow_big"),
    ((700, BIG + 1, 0, 0, CAP, 1, CAP, BIG), "grow_big"),
    # ... and a pair count beyond the int32 range beats all of them
    ((-1, 10, 0, 0, 600, 300, CAP, BIG), "limit"),
    ((700, -1, 0, 0, 600, 300, CAP, BIG), "limit"),
    ((-(2**31), 10, 0, 0, 600, 300, CAP, BIG), "limit"),
    ((-1, BIG + 1, 1, 5, CAP + 1, 0, CAP, BIG), "limit"),
    ((700, -5, 1, 1, 600, 300, CAP, BIG), "limit"),
    # nothing at all is a final (empty) matrix; a bit no kernel sets decides nothing
    ((0, 0, 0, 0, 0, 0, 1, 1), "final"),
    ((700, 10, 0, 8, 600, 300, CAP, BIG), "final"),
]


@pytest.fixture(scope="module")
def outcomes(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_fused_outcome") / "host_fused_outcome")
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "host_shim"), "-I", os.path.join(ROOT, "xugrid_amd", "csrc"),
         os.path.join(ROOT, "tests", "host_fused_outcome.cpp"), "-o", exe])
    text = "".join(" ".join(str(x) for x in case) + "\n" for case, _ in TABLE)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(got) == len(TABLE)
    return got


@pytest.mark.parametrize("k", range(len(TABLE)))
def test_fused_outcome_table(outcomes, k):
    case, expected = TABLE[k]
    assert outcomes[k] == expected, case

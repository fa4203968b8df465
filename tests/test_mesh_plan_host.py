"""
CPU: what the host decides from a mesh's eight statistics before it allocates or launches anything
(xugrid_amd/csrc/xr_mesh_plan.h: index_grid, morton_cover, numbering_coherent) -- compiled as plain C++
(tests/host_mesh_plan.cpp against tests/host_shim/hip/hip_runtime.h) and table-tested against a restatement, below, of the
rule as mesh_build_index, mesh_query_order and tile_key_params spelled it out before the header existed.  Integers are compared
exactly, doubles bit for bit.
"""
import math
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_LEVELS, LEVEL_SHIFT = 24, 1  # xr_geom.h
XMIN, XMAX, YMIN, YMAX, SUM_EXTENT, MAX_EXTENT, MAX_DIAGONAL, SUM_JUMP = range(8)
INF = math.inf


def bits(x):
    return struct.pack("<d", x)


def cdiv(a, b):  # IEEE division (Python raises on a zero divisor)
    if b == 0.0:
        return math.nan if a == 0.0 or a != a else math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def cmax(a, b):  # std::max
    return b if a < b else a


# ---- the rule, restated ------------------------------------------------------------------------------------------------------
def ref_index_grid(s, F, sampled):
    xmin, xmax, ymin, ymax = s[0], s[1], s[2], s[3]
    n_ext = cmax(s[7], 1.0) if sampled else float(F)
    sum_ext = s[4] * cdiv(float(F), n_ext)
    max_ext = cmax(xmax - xmin, ymax - ymin) if sampled else s[5]
    W = xmax - xmin if F > 0 else 1.0
    H = ymax - ymin if F > 0 else 1.0
    if not W > 0:
        W = 1.0
    if not H > 0:
        H = 1.0
    h0 = 1.4 * sum_ext / float(F) if F > 0 else 1.0
    if not h0 > 0:
        h0 = cmax(W, H)
    max_cells0 = cmax(4.0 * float(F), 1024.0)
    doublings = 0
    while (math.floor(W / h0) + 1.0) * (math.floor(H / h0) + 1.0) > max_cells0:
        h0 *= 2.0
        doublings += 1
    inv_h0 = 1.0 / h0
    L = 1
    while L < MAX_LEVELS and not max_ext <= 0.999 * math.ldexp(h0, (L - 1) * LEVEL_SHIFT):
        L += 1
    total, levels = 0, []
    for l in range(L):
        inv_h = math.ldexp(inv_h0, -l * LEVEL_SHIFT)
        nx, ny = int(math.floor(W * inv_h)) + 1, int(math.floor(H * inv_h)) + 1
        if not total + nx * ny < 2**31:
            return None, doublings
        levels.append((total, nx, ny))
        total += nx * ny
    return ((xmin if F > 0 else 0.0, ymin if F > 0 else 0.0, h0, inv_h0), L, total, levels), doublings


def ref_morton_cover(s, F, extents, first, last):
    span = cmax(s[1] - s[0], s[3] - s[2])
    if not span > 0:
        span = 1.0
    h = cdiv(extents * s[4], float(F))
    if not h > 0:
        h = span
    b = first
    while b < last and math.ldexp(h, b) < span:
        b += 1
    return (s[0], s[2], float(1 << b) / (span * (1.0 + 1e-9))), 1 << b


def ref_coherent(s, F):
    mean_ext = s[4] / float(F) if F > 0 else 0.0
    mean_jump = s[7] / (float(F) * 63.0 / 64.0) if F > 0 else 0.0
    return F == 0 or mean_jump <= 4.0 * mean_ext


# ---- cases -------------------------------------------------------------------------------------------------------------------
def stats(x0=0.0, x1=1.0, y0=0.0, y1=1.0, sum_ext=0.0, max_ext=0.0, diag=0.0, last=0.0):
    return [x0, x1, y0, y1, sum_ext, max_ext, diag, last]


def square(F, cells, max_ext=None, **kw):
    """F faces of mean extent 1 (level-0 cell 1.4) on a square domain `cells` level-0 cells wide"""
    return stats(x1=1.4 * cells, y1=1.4 * cells, sum_ext=float(F), max_ext=1.0 if max_ext is None else max_ext, **kw)


H0 = 1.4 * 100.0 / 100.0  # level-0 cell of square(100, .)
up, down = (lambda v: math.nextafter(v, INF)), (lambda v: math.nextafter(v, -INF))

# (name, statistics, n_face, sampled, what the case is there for: None, or a check on (result, doublings))
GRID = [
    ("no faces", stats(x0=3.0, x1=3.0, y0=-2.0, y1=-2.0), 0, False, lambda r, d: r[0][:3] == (0.0, 0.0, 1.0) and r[3] == [(0, 2, 2)]),
    ("no faces, sampled", stats(last=0.0), 0, True, None),
    ("zero width", stats(x0=2.0, x1=2.0, y1=50.0, sum_ext=100.0, max_ext=1.0), 100, False, lambda r, d: r[3][0][1] == 1),
    ("zero height", stats(x0=-5.0, x1=45.0, y0=7.0, y1=7.0, sum_ext=100.0, max_ext=1.0), 100, False, lambda r, d: r[3][0][2] == 1),
    ("negative width (bounds of nothing)", stats(x0=INF, x1=-INF, y0=INF, y1=-INF), 5, False, None),
    ("zero mean extent: the domain is the cell", stats(x1=8.0, y1=3.0), 10, False, lambda r, d: r[0][2] == 8.0),
    ("1024-cell bound met: 32 x 32", square(100, 31.5), 100, False, lambda r, d: d == 0 and r[3][0][1:] == (32, 32)),
    ("1024-cell bound passed: 33 x 33", square(100, 32.5), 100, False, lambda r, d: d == 1 and r[0][2] == 2 * H0),
    ("1024-cell bound passed twice", square(100, 64.5), 100, False, lambda r, d: d == 2),
    ("4 n_face bound met: 63 x 63 of 4000", square(1000, 62.5), 1000, False, lambda r, d: d == 0 and r[3][0][1:] == (63, 63)),
    ("4 n_face bound passed: 64 x 64 of 4000", square(1000, 63.5), 1000, False, lambda r, d: d == 1),
    ("largest extent just below 0.999 h0", square(100, 20, max_ext=down(0.999 * H0)), 100, False, lambda r, d: r[1] == 1),
    ("largest extent at 0.999 h0", square(100, 20, max_ext=0.999 * H0), 100, False, lambda r, d: r[1] == 1),
    ("largest extent just above 0.999 h0", square(100, 20, max_ext=up(0.999 * H0)), 100, False, lambda r, d: r[1] == 2),
    ("largest extent just below 0.999 * 2 h0", square(100, 20, max_ext=down(0.999 * (2 * H0))), 100, False, lambda r, d: r[1] == 2),
    ("largest extent just above 0.999 * 2 h0", square(100, 20, max_ext=up(0.999 * (2 * H0))), 100, False, lambda r, d: r[1] == 3),
    ("levels saturate", square(100, 20, max_ext=1e30), 100, False, lambda r, d: r[1] == MAX_LEVELS),
    ("infinite extent saturates too", square(100, 20, max_ext=INF), 100, False, lambda r, d: r[1] == MAX_LEVELS),
    ("sampled, nothing looked at", stats(x1=100.0, y1=60.0, sum_ext=0.0, last=0.0), 200000, True, None),
    ("sampled, one face looked at", stats(x1=100.0, y1=60.0, sum_ext=0.25, max_ext=0.25, last=1.0), 200000, True,
     lambda r, d: r[0][2] == 1.4 * (0.25 * 200000.0) / 200000.0),
    ("sampled, the usual eighth", stats(x1=100.0, y1=60.0, sum_ext=6000.0, max_ext=0.5, last=25000.0), 200000, True, None),
    ("sampled: the domain bounds the extent", stats(x1=100.0, y1=60.0, sum_ext=6000.0, max_ext=1e9, last=25000.0), 200000, True,
     lambda r, d: r[1] < MAX_LEVELS),
    ("one level below 2^31 cells", square(2**30, 46000.5 - 1), 2**30, False, lambda r, d: r is not None and r[1] == 1),
    ("one level of 2^31 cells and more", square(2**30, 50000.5 - 1), 2**30, False, lambda r, d: r is None and d == 0),
    ("two levels reach 2^31 cells", square(2**30, 46000.5 - 1, max_ext=2.0), 2**30, False, lambda r, d: r is None),
    ("a plain triangle mesh", stats(x0=-1.5, x1=998.5, y0=20.0, y1=720.0, sum_ext=1.3e6, max_ext=9.5, last=7.0e6), 10**6, False, None),
]

TINY = 1e-9
# (name, statistics, n_face, extents per cell, first bits, max bits, n_side or None)
MORTON = [
    ("query order, coarse: first bits", stats(x1=10.0, y1=4.0, sum_ext=250.0), 100, 2.0, 1, 10, 2),
    ("query order, h * 2 == span: first bits", stats(x1=10.0, y1=4.0, sum_ext=250.0), 100, 2.0, 1, 10, 2),
    ("query order, h * 2 just short of span", stats(x1=up(10.0), y1=4.0, sum_ext=250.0), 100, 2.0, 1, 10, 4),
    ("query order, middle", stats(x0=-3.0, x1=97.0, y1=30.0, sum_ext=100.0), 100, 2.0, 1, 10, 64),
    ("query order, fine: max bits", stats(x1=10.0, y1=4.0, sum_ext=100 * TINY), 100, 2.0, 1, 10, 1024),
    ("query order, zero extent: one cell a side is not allowed", stats(x1=10.0, y1=4.0), 100, 2.0, 1, 10, 2),
    ("query order, no span", stats(x1=0.0, y1=0.0, sum_ext=1.0), 100, 2.0, 1, 10, None),
    ("tiles, coarse: no bits", stats(x1=10.0, y1=4.0, sum_ext=100.0), 100, 12.0, 0, 12, 1),
    ("tiles, h == span: no bits", stats(x1=12.0, y1=4.0, sum_ext=100.0), 100, 12.0, 0, 12, 1),
    ("tiles, middle", stats(x0=5.0, x1=1005.0, y0=-40.0, y1=700.0, sum_ext=1300.0), 1000, 12.0, 0, 12, 128),
    ("tiles, fine: max bits", stats(x1=10.0, y1=4.0, sum_ext=100 * TINY), 100, 12.0, 0, 12, 4096),
    ("tiles, no faces", stats(x1=0.0, y1=0.0), 0, 12.0, 0, 12, 1),
]

# (name, statistics, n_face, expected or None): 64 faces make the divisor of the jumps 63 exactly
COHERENT = [
    ("no faces", stats(), 0, True),
    ("mean jump == 4 mean extents", stats(sum_ext=32.0, last=126.0), 64, True),
    ("mean jump just above", stats(sum_ext=32.0, last=up(126.0)), 64, None),
    ("mean jump clearly above", stats(sum_ext=32.0, last=127.0), 64, False),
    ("mean jump just below", stats(sum_ext=32.0, last=down(126.0)), 64, True),
    ("no extent, no jump", stats(), 64, True),
    ("no extent, a jump", stats(last=1e-300), 64, False),
    ("a generator's numbering", stats(sum_ext=1.3e6, last=2.1e6), 10**6, True),
    ("a shuffled numbering", stats(sum_ext=1.3e6, last=3.3e8), 10**6, False),
]


def line(kind, s, F, *rest):
    return " ".join([kind] + [float(v).hex() for v in s] + [str(F)] + [v.hex() if isinstance(v, float) else str(int(v)) for v in rest]) + "\n"


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_mesh_plan") / "host_mesh_plan")
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "host_shim"), "-I", os.path.join(ROOT, "xugrid_amd", "csrc"),
         os.path.join(ROOT, "tests", "host_mesh_plan.cpp"), "-o", exe])
    text = "".join(line("grid", s, F, sampled) for _, s, F, sampled, _ in GRID)
    text += "".join(line("morton", s, F, e, first, last) for _, s, F, e, first, last, _ in MORTON)
    text += "".join(line("coherent", s, F) for _, s, F, _ in COHERENT)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(GRID) + len(MORTON) + len(COHERENT)
    return got


@pytest.mark.parametrize("k", range(len(GRID)), ids=[c[0] for c in GRID])
def test_index_grid(answers, k):
    name, s, F, sampled, check = GRID[k]
    ref, doublings = ref_index_grid(s, F, sampled)
    got = answers[k].split()
    if check is not None:
        assert check(ref, doublings), "the case does not reach the edge it is named for"
    if ref is None:
        assert got == ["fail"]
        return
    (doubles, L, total, levels) = ref
    assert got[0] == "ok"
    assert [bits(float.fromhex(v)) for v in got[1:5]] == [bits(v) for v in doubles], (got[1:5], [v.hex() for v in doubles])
    assert [int(v) for v in got[5:]] == [L, total] + [v for level in levels for v in level]


@pytest.mark.parametrize("k", range(len(MORTON)), ids=[c[0] for c in MORTON])
def test_morton_cover(answers, k):
    name, s, F, extents, first, last, n_side = MORTON[k]
    doubles, side = ref_morton_cover(s, F, extents, first, last)
    if n_side is not None:
        assert side == n_side, "the case does not reach the edge it is named for"
    got = answers[len(GRID) + k].split()
    assert [bits(float.fromhex(v)) for v in got[:3]] == [bits(v) for v in doubles], (got[:3], [v.hex() for v in doubles])
    assert [int(v) for v in got[3:]] == [side, 1]  # (n_run: the default, callers set their own)


@pytest.mark.parametrize("k", range(len(COHERENT)), ids=[c[0] for c in COHERENT])
def test_numbering_coherent(answers, k):
    name, s, F, expected = COHERENT[k]
    ref = ref_coherent(s, F)
    if expected is not None:
        assert ref == expected, "the case does not reach the edge it is named for"
    assert answers[len(GRID) + len(MORTON) + k] == ("1" if ref else "0")

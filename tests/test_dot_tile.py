"""CPU tests of dot diffusion's tiled form: hq_dot_reach2 and hq_dot_levels (plain C++, no
context, no GPU) against their numpy restatements (dot_tile_ref.py) and the values hq.h quotes,
their argument refusals, and the argument the kernel rests on -- a tile rendered from the window
its reach gives is the whole image's, pixel for pixel.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
from dot_ref import KNUTH8, dot, random_classes
from dot_tile_ref import column_major, levels, reach2, row_major, tiled
from hybridquantization_amd import _lib
from test_dither import _case

MATRICES = {
    "knuth8": KNUTH8, "perm4_44": random_classes(4, 44), "perm4_45": random_classes(4, 45),
    "perm8_2": random_classes(8, 2), "perm16_46": random_classes(16, 46), "row_major16": row_major(),
    "column_major16": column_major(),
}
# hq.h's and the design document's table: (above, below, left, right)
REACH = {"knuth8": (5, 5, 5, 5), "perm4_44": (7, 5, 2, 4), "perm4_45": (4, 4, 5, 4), "perm8_2": (6, 6, 10, 6),
         "perm16_46": (11, 7, 8, 6), "row_major16": (15, 1, 255, 17)}
DEPTH = {"knuth8": 15, "perm4_44": 10, "perm16_46": 17, "row_major16": 256}


def matrix_of(cls):
    m = _lib.hq_dot_classes()
    c = np.asarray(cls)
    m.n = c.shape[0]
    for i, v in enumerate(c.reshape(-1)):
        m.cls[i] = int(v)
    return m


def c_reach2(cls):
    v = [C.c_int(-9) for _ in range(4)]
    rc = hq.load().hq_dot_reach2(C.byref(matrix_of(cls)), *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


def c_levels(cls):
    level, depth = np.full(256, -9, np.int32), C.c_int(-9)
    rc = hq.load().hq_dot_levels(C.byref(matrix_of(cls)), _lib.iptr(level), C.byref(depth))
    return rc, level, depth.value


@pytest.mark.parametrize("name", list(MATRICES))
def test_reach2_is_the_restatement_and_its_rows_are_hq_dot_reach(name):
    cls = MATRICES[name]
    rc, got = c_reach2(cls)
    assert rc == _lib.HQ_OK
    assert got == reach2(cls)
    if name in REACH:
        assert got == REACH[name]
    above, below = C.c_int(0), C.c_int(0)
    assert hq.load().hq_dot_reach(C.byref(matrix_of(cls)), C.byref(above), C.byref(below)) == _lib.HQ_OK
    assert got[:2] == (above.value, below.value)
    assert hq.ImageManipulation.dotReach2(cls) == got


def test_reach2_of_random_permutations():
    for n in (4, 8, 16):
        for seed in range(6):
            cls = random_classes(n, 100 * n + seed)
            assert c_reach2(cls) == (_lib.HQ_OK, reach2(cls)), (n, seed)


@pytest.mark.parametrize("name", list(MATRICES))
def test_levels_are_the_restatement(name):
    cls = MATRICES[name]
    n = cls.shape[0]
    rc, level, depth = c_levels(cls)
    want, want_depth = levels(cls)
    assert rc == _lib.HQ_OK and depth == want_depth
    np.testing.assert_array_equal(level[:n * n].reshape(n, n), want)
    assert not level[n * n:].any()  # (the entries past n n)
    if name in DEPTH:
        assert depth == DEPTH[name]
    lv, d = hq.ImageManipulation.dotLevels(cls)
    np.testing.assert_array_equal(lv, want)
    assert d == want_depth


def test_column_major_is_row_major_transposed():
    a, b, l, r = c_reach2(row_major())[1]
    assert c_reach2(column_major())[1] == (l, r, a, b)
    assert c_levels(column_major())[2] == 256


def test_refusals_leave_the_outputs_untouched():
    lib = hq.load()
    bad = matrix_of(KNUTH8)
    bad.cls[3] = bad.cls[4]  # no permutation
    side = matrix_of(KNUTH8)
    side.n = 5
    good = matrix_of(KNUTH8)
    v = [C.c_int(-9) for _ in range(4)]
    ptrs = [C.byref(x) for x in v]
    for m in (bad, side):
        assert lib.hq_dot_reach2(C.byref(m), *ptrs) == _lib.HQ_ERR_ARG
    assert lib.hq_dot_reach2(None, *ptrs) == _lib.HQ_ERR_ARG
    for hole in range(4):
        args = list(ptrs)
        args[hole] = None
        assert lib.hq_dot_reach2(C.byref(good), *args) == _lib.HQ_ERR_ARG
    assert [x.value for x in v] == [-9] * 4
    level, depth = np.full(256, -9, np.int32), C.c_int(-9)
    for m in (bad, side):
        assert lib.hq_dot_levels(C.byref(m), _lib.iptr(level), C.byref(depth)) == _lib.HQ_ERR_ARG
    assert lib.hq_dot_levels(None, _lib.iptr(level), C.byref(depth)) == _lib.HQ_ERR_ARG
    assert lib.hq_dot_levels(C.byref(good), None, C.byref(depth)) == _lib.HQ_ERR_ARG
    assert lib.hq_dot_levels(C.byref(good), _lib.iptr(level), None) == _lib.HQ_ERR_ARG
    assert depth.value == -9 and (level == -9).all()


@pytest.mark.parametrize("name", ["knuth8", "perm4_44", "perm8_2", "perm16_46"])
def test_every_tile_rendered_from_its_window_is_the_whole_image(name):
    """45 x 37 noise, 16 x 16 tiles (3 x 3 of them, the last column and row partial), the
    window from the four-direction reach: 0 mismatches against dot_ref.dot.  With a window one
    pixel short on each side the argument must fail somewhere, else the test shows nothing."""
    w, h, K = 45, 37, 6
    cls = MATRICES[name]
    rgba, pal = _case(w, h, K, 7)
    want, _ = dot(rgba, pal, w, h, 1.0, cls)
    r = reach2(cls)
    np.testing.assert_array_equal(tiled(rgba, pal, w, h, 1.0, cls, 16, 16, r), want)
    if name == "knuth8":
        short = tiled(rgba, pal, w, h, 1.0, cls, 16, 16, (0, 0, 0, 0))
        assert np.count_nonzero(short != want) > 0

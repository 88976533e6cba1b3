"""CPU tests of dot diffusion on row-block shards: the reach of a class matrix (hq_dot_reach:
plain C++, no context, no GPU) against a numpy restatement, and the claim the shards rest on --
rendering the row window [r0 - above, r1 + below) alone, with the classes and the border rule
of the whole image, reproduces the whole image's indices on [r0, r1) exactly, and one row less
does not.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
from dot_ref import KNUTH8, NEIGHBOURS, class_image, dot, random_classes, weight_sums
from hybridquantization_amd import _lib
from test_dither import _case
from test_dot import _matrix

f32 = np.float32
ROWMAJOR4 = np.arange(16, dtype=np.int32).reshape(4, 4)
ROWMAJOR16 = np.arange(256, dtype=np.int32).reshape(16, 16)
PERM4 = random_classes(4, 44)


# ---------------------------------------------------------------------------
# The reach
# ---------------------------------------------------------------------------
def reach_ref(cls):
    """hq.h's hq_dot_reach, restated as a relaxation to the fixed point in place of one pass in
    ascending class: up[c] = max(0, max over lower neighbours p at (dx, dy) of up[p] - dy),
    down[c] likewise with + dy, on the torus; the maxima over the cells."""
    c = np.asarray(cls, np.int64)
    n = c.shape[0]
    up, down = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for _ in range(n * n + 1):  # (a path has at most n n - 1 steps)
        nu, nd = np.zeros_like(up), np.zeros_like(down)
        for dx, dy, _ in NEIGHBOURS:
            lower = np.roll(c, (-dy, -dx), (0, 1)) < c  # the neighbour at (x + dx, y + dy)
            nu = np.maximum(nu, np.where(lower, np.roll(up, (-dy, -dx), (0, 1)) - dy, 0))
            nd = np.maximum(nd, np.where(lower, np.roll(down, (-dy, -dx), (0, 1)) + dy, 0))
        if np.array_equal(nu, up) and np.array_equal(nd, down):
            return int(up.max()), int(down.max())
        up, down = nu, nd
    raise AssertionError("no fixed point: the class order is not a partial order")


def lib_reach(cls):
    a, b = C.c_int(-7), C.c_int(-7)
    n = np.asarray(cls).shape[0]
    assert hq.load().hq_dot_reach(C.byref(_matrix(n, cls)), C.byref(a), C.byref(b)) == _lib.HQ_OK
    return a.value, b.value


def test_reach_of_the_known_matrices():
    assert lib_reach(KNUTH8) == reach_ref(KNUTH8) == (5, 5)
    assert lib_reach(ROWMAJOR4) == reach_ref(ROWMAJOR4) == (3, 1)
    assert lib_reach(ROWMAJOR16) == reach_ref(ROWMAJOR16) == (15, 1)
    assert hq.ImageManipulation.dotReach() == (5, 5)
    assert hq.ImageManipulation.dotReach("knuth8") == (5, 5)
    assert hq.ImageManipulation.dotReach(ROWMAJOR16) == (15, 1)
    # a vertical flip swaps the sides
    assert lib_reach(ROWMAJOR16[::-1]) == reach_ref(ROWMAJOR16[::-1]) == (1, 15)


@pytest.mark.parametrize("n", [4, 8, 16])
def test_reach_of_random_permutations(n):
    past_side = 0
    for seed in range(40):
        cls = random_classes(n, 1000 * n + seed)
        got = lib_reach(cls)
        assert got == reach_ref(cls), (n, seed)
        assert 1 <= min(got) and max(got) <= n * n - 1
        past_side += max(got) > n
    if n == 4:
        assert past_side > 0  # paths cross tile borders: a 4 x 4 matrix can reach more than 4 rows
    print(f"n={n}: {past_side} of 40 permutations reach past their side; perm4(44) reaches {lib_reach(PERM4)}")


def test_reach_refusals_leave_the_outputs():
    lib = hq.load()
    a, b = C.c_int(-7), C.c_int(-7)
    ok = _matrix(8, KNUTH8)
    assert lib.hq_dot_reach(None, C.byref(a), C.byref(b)) == _lib.HQ_ERR_ARG
    assert lib.hq_dot_reach(C.byref(ok), None, C.byref(b)) == _lib.HQ_ERR_ARG
    assert lib.hq_dot_reach(C.byref(ok), C.byref(a), None) == _lib.HQ_ERR_ARG
    rep = KNUTH8.copy()
    rep[0, 0] = rep[7, 7]
    assert lib.hq_dot_reach(C.byref(_matrix(8, rep)), C.byref(a), C.byref(b)) == _lib.HQ_ERR_ARG
    assert lib.hq_dot_reach(C.byref(_matrix(5, np.arange(25))), C.byref(a), C.byref(b)) == _lib.HQ_ERR_ARG
    assert (a.value, b.value) == (-7, -7)
    with pytest.raises(ValueError):
        hq.ImageManipulation.dotReach(np.zeros((4, 5)))


# ---------------------------------------------------------------------------
# The window
# ---------------------------------------------------------------------------
def dot_window(rgba, pal4, w, H, s, classes, a0, a1):
    """hq.h's definition on the rows [a0, a1) of a (w, H) image alone -> idx int32 (a1 - a0, w).
    The class of a pixel comes from its row in the whole image and W(p) from the whole image's
    border; a source outside the window contributes nothing and is never read."""
    cls = KNUTH8 if classes is None else np.asarray(classes, np.int32)
    n = cls.shape[0]
    ci_full = class_image(cls, w, H)
    Wsum = weight_sums(ci_full)[a0:a1].astype(f32)
    ci = ci_full[a0:a1]
    hw = a1 - a0
    px = np.ascontiguousarray(np.asarray(rgba, f32)[:, :3]).reshape(H, w, 3)[a0:a1]
    pal = np.ascontiguousarray(np.asarray(pal4, f32).reshape(-1, 4))
    err = np.full((hw, w, 3), np.nan, f32)  # (never zeroed on the device: nothing unwritten may be read)
    idx = np.full((hw, w), -1, np.int32)
    s = f32(s)
    for k in range(n * n):
        Y, X = np.nonzero(ci == k)
        if Y.size == 0:
            continue  # a class without a pixel in the window
        cy, cx = (int(v[0]) for v in np.nonzero(cls == k))
        lower = sorted((int(cls[(cy + dy) % n, (cx + dx) % n]), dx, dy, wt) for dx, dy, wt in NEIGHBOURS
                       if cls[(cy + dy) % n, (cx + dx) % n] < k)
        a = np.zeros((Y.size, 3), f32)
        for _, dx, dy, wt in lower:
            PX, PY = X + dx, Y + dy
            ok = (PX >= 0) & (PX < w) & (PY >= 0) & (PY < hw)
            sx, sy = PX[ok], PY[ok]
            a[ok] = a[ok] + (f32(wt) * err[sy, sx]) / Wsum[sy, sx][:, None]
        v = np.minimum(np.maximum(px[Y, X] + s * a, f32(0)), f32(1))
        kk = o.assign(v, pal)[0]
        idx[Y, X] = kk
        err[Y, X] = v - pal[kk, :3]
    assert (idx >= 0).all() and not np.isnan(err).any()
    return idx


def window_rows(H, r0, r1, reach):
    return max(0, r0 - reach[0]), min(H, r1 + reach[1])


# (matrix, w, H, r0, r1): widths and first rows that are no multiples of the side; windows
# clipped by the top and by the bottom border; a shard of one row; 16 x 16 with its 15 rows above
SUFFICIENCY = [("knuth8", None, 21, 40, 13, 27), ("knuth8", None, 13, 37, 0, 9), ("knuth8", None, 13, 37, 30, 37),
               ("knuth8", None, 19, 30, 11, 12), ("perm4", PERM4, 11, 41, 17, 22), ("perm4", PERM4, 7, 29, 3, 26),
               ("rowmajor4", ROWMAJOR4, 10, 23, 9, 14), ("rowmajor16", ROWMAJOR16, 21, 50, 31, 35),
               ("rowmajor16", ROWMAJOR16, 18, 40, 7, 19), ("perm16", random_classes(16, 46), 20, 60, 27, 33)]


@pytest.mark.parametrize("name,cls,w,H,r0,r1", SUFFICIENCY)
def test_the_window_reproduces_the_whole_images_rows(name, cls, w, H, r0, r1):
    K = 5
    rgba, pal = _case(w, H, K, 7 * w + H)
    reach = reach_ref(KNUTH8 if cls is None else cls)
    a0, a1 = window_rows(H, r0, r1, reach)
    for s in (1.0, 0.5):
        whole = dot(rgba, pal, w, H, s, cls)[0].reshape(H, w)
        got = dot_window(rgba, pal, w, H, s, cls, a0, a1)
        np.testing.assert_array_equal(got[r0 - a0:r1 - a0], whole[r0:r1], err_msg=f"{name} s={s}")
    # the whole image as its own window is dot_ref.dot
    np.testing.assert_array_equal(dot_window(rgba, pal, w, H, 1.0, cls, 0, H), dot(rgba, pal, w, H, 1.0, cls)[0].reshape(H, w))


# The bound is tight, and a short apron shows: under the row-major 16 x 16 matrix (15 rows
# above) this image (mid-grey noise), two-colour palette and owned row 31 -- row 15 of its tile,
# the head of the longest paths -- were found by a search over seeds on the CPU: 6 of the row's 24
# indices change when the window starts at row 17 in the place of 16.
TIGHT = dict(w=24, H=40, r0=31, r1=32, seed=0, pal=((0.25, 0.25, 0.25, 0.0), (0.75, 0.75, 0.75, 0.0)))


def tight_case():
    t = TIGHT
    rng = np.random.default_rng(t["seed"])
    rgba = np.zeros((t["w"] * t["H"], 4), f32)
    rgba[:, :3] = rng.random((t["w"] * t["H"], 3), dtype=f32) * f32(0.2) + f32(0.4)
    return rgba, np.array(t["pal"], f32)


def test_one_row_less_above_changes_an_owned_index():
    t = TIGHT
    w, H, r0, r1 = t["w"], t["H"], t["r0"], t["r1"]
    rgba, pal = tight_case()
    above, below = reach_ref(ROWMAJOR16)
    assert (above, below) == (15, 1)
    whole = dot(rgba, pal, w, H, 1.0, ROWMAJOR16)[0].reshape(H, w)
    full = dot_window(rgba, pal, w, H, 1.0, ROWMAJOR16, r0 - above, r1 + below)
    np.testing.assert_array_equal(full[above:above + r1 - r0], whole[r0:r1])
    short = dot_window(rgba, pal, w, H, 1.0, ROWMAJOR16, r0 - above + 1, r1 + below)
    changed = int(np.count_nonzero(short[above - 1:above - 1 + r1 - r0] != whole[r0:r1]))
    print(f"{changed} of {(r1 - r0) * w} owned indices change with {above - 1} rows above")
    assert changed > 0

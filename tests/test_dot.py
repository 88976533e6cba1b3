"""CPU tests of dot diffusion: the restatement's two forms agree (dot_ref.py), strength 0 is
the plain argmin, the rendering does under S-CIELAB what error diffusion is for, and the
host side of the library (hq_dot_preset, hq_dot_classes_legal, hq_dot_barons: plain C++, no
context, no GPU) states the preset, the legality rule and the baron count as hq.h does.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
from dither_ref import cube_corners, ramp_image
from dot_ref import KNUTH8, barons, dot, dot_scatter, legal, random_classes
from hybridquantization_amd import _lib
from test_dither import _case, cost_of

SHAPES = [(1, 1), (1, 17), (17, 1), (3, 2), (8, 8), (9, 9), (13, 11), (23, 17)]
MATRICES = {"knuth8": None, "perm4": random_classes(4, 44)}


@pytest.mark.parametrize("s", [1.0, 0.5])
@pytest.mark.parametrize("matrix", list(MATRICES))
@pytest.mark.parametrize("w,h", SHAPES)
def test_class_form_equals_scatter_form(w, h, matrix, s):
    """Shapes smaller than the tile, one tile exactly, one pixel more, rows and columns without
    neighbours on two sides, and ordinary ones; Knuth's matrix and a 4 x 4 permutation."""
    rgba, pal = _case(w, h, 6, 10 * w + h)
    a, ua = dot(rgba, pal, w, h, s, MATRICES[matrix])
    b, ub = dot_scatter(rgba, pal, w, h, s, MATRICES[matrix])
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ua, ub)


@pytest.mark.parametrize("w,h,K", [(23, 17, 6), (64, 48, 16)])
def test_strength_zero_is_the_plain_argmin(w, h, K):
    rgba, pal = _case(w, h, K, 3)
    idx, used = dot(rgba, pal, w, h, 0.0)
    want_idx, want_used = o.assign(rgba, pal)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(used, want_used)


def test_ramp_costs_less_dot_diffused():
    """The 64 x 64 RGB ramp under the eight cube corners at 72 dpi / 45 cm, dE76: at strength 1
    at most 0.6 of the nearest-colour cost (0.514 measured), at 0.5 below it."""
    w = h = 64
    rgba, pal = ramp_image(w, h), cube_corners()
    f = o.design_filters(72, 45.0)
    lab = o.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    plain = cost_of(*o.assign(rgba, pal), pal, lab, f, w, h)
    costs = {s: cost_of(*dot(rgba, pal, w, h, s), pal, lab, f, w, h) for s in (0.5, 1.0)}
    print(f"plain {plain!r}, dot-diffused {costs!r}, ratio at 1: {costs[1.0] / plain:.3f}")
    assert costs[1.0] <= 0.6 * plain
    assert costs[0.5] < plain


def test_noise_image_changes_a_fifth_of_its_indices():
    w, h, K = 97, 53, 16
    R, G, B = o.synthetic_image(w, h, 5)
    rgba = o.inline_rgba(R, G, B).reshape(-1, 4)
    pal = o.synthetic_palette(K, 16).reshape(K, 4)
    idx, _ = dot(rgba, pal, w, h, 1.0)
    changed = float(np.mean(idx != o.assign(rgba, pal)[0]))
    print(f"{changed:.3f} of the indices change")
    assert changed >= 0.2


# ---------------------------------------------------------------------------
# The library's host side, through ctypes: no context, no GPU
# ---------------------------------------------------------------------------
def _matrix(n, cls):
    m = _lib.hq_dot_classes()
    m.n = n
    for i, v in enumerate(np.asarray(cls).reshape(-1)[:256]):
        m.cls[i] = int(v)
    return m


def test_the_preset_is_knuths_matrix():
    lib = hq.load()
    m = _lib.hq_dot_classes()
    m.n = -5
    assert lib.hq_dot_preset(0, C.byref(m)) == _lib.HQ_OK
    assert m.n == 8
    np.testing.assert_array_equal(np.array(m.cls[:64]).reshape(8, 8), KNUTH8)
    assert legal(8, KNUTH8) and lib.hq_dot_classes_legal(C.byref(m)) == 1
    assert lib.hq_dot_barons(C.byref(m)) == 2 == barons(KNUTH8)
    np.testing.assert_array_equal(hq.ImageManipulation.diffusionClasses("knuth8"), KNUTH8)
    for bad in (-1, 1, 7):
        assert lib.hq_dot_preset(bad, C.byref(m)) == _lib.HQ_ERR_ARG
    assert lib.hq_dot_preset(0, None) == _lib.HQ_ERR_ARG
    with pytest.raises(ValueError):
        hq.ImageManipulation.diffusionClasses("bayer")


@pytest.mark.parametrize("n", [4, 8, 16])
def test_random_permutations_are_legal_and_their_barons_counted(n):
    lib = hq.load()
    for seed in range(12):
        cls = random_classes(n, 100 * n + seed)
        m = _matrix(n, cls)
        assert legal(n, cls) and lib.hq_dot_classes_legal(C.byref(m)) == 1
        assert lib.hq_dot_barons(C.byref(m)) == barons(cls), (n, seed)


def test_illegal_matrices_are_refused():
    lib = hq.load()
    assert lib.hq_dot_classes_legal(None) == 0
    for n in (3, 5, 32):
        cls = np.arange(256) % max(n * n, 1)
        assert not legal(n, cls)
        assert lib.hq_dot_classes_legal(C.byref(_matrix(n, cls))) == 0
    for n in (4, 8, 16):
        ok = random_classes(n, n).reshape(-1)
        rep = ok.copy()
        rep[1] = rep[n * n - 1]  # a repeated class
        out = ok.copy()
        out[int(np.argmax(ok))] = n * n  # a class outside 0 .. n n - 1
        neg = ok.copy()
        neg[int(np.argmin(ok))] = -1
        for bad in (rep, out, neg):
            assert not legal(n, bad)
            m = _matrix(n, bad)
            assert lib.hq_dot_classes_legal(C.byref(m)) == 0
            assert lib.hq_dot_barons(C.byref(m)) == -1
        assert lib.hq_dot_classes_legal(C.byref(_matrix(n, ok))) == 1

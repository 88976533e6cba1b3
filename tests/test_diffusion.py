"""CPU tests of the diffusion kernels beyond Floyd-Steinberg (hq_diffuse_population): the
library's preset table, legality rule and (R, S) classification against diffusion_ref.py's
restatement of hq.h, and the restatement's two forms -- the wavefront order t = x + S y is the
raster order for S = 2 and S = 3.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
from diffusion_ref import (POSITIONS, PRESET_CLASS, PRESETS, classify, diffuse, diffuse_raster, legal, preset,
                           single_tap, wavefronts)
from dither_ref import cube_corners, ramp_image
from hybridquantization_amd import _lib

# (the last three: the GPU tests' images narrower than the tap window that cross a strip of 64 rows)
EDGE_SHAPES = [(1, 5), (2, 3), (5, 1), (23, 17), (1, 130), (2, 129), (3, 66)]
# twelve distinct weights, div = their sum + 3
TWELVE = (np.array([[0, 0, 0, 11, 2], [7, 3, 12, 5, 1], [4, 9, 6, 10, 8]], np.int64), 81)


def c_taps(w, div):
    t = _lib.hq_diffusion_taps()
    for dy in range(3):
        for i in range(5):
            t.w[dy][i] = int(w[dy][i])
    t.div = int(div)
    return t


def lib_classify(w, div):
    R, S = C.c_int(-1), C.c_int(-1)
    rc = hq.load().hq_diffusion_classify(C.byref(c_taps(w, div)), C.byref(R), C.byref(S))
    return rc, R.value, S.value


def _case(w, h, K, seed):
    R, G, B = o.synthetic_image(w, h, seed)
    return o.inline_rgba(R, G, B).reshape(-1, 4), o.synthetic_palette(K, seed + 1).reshape(K, 4)


def test_the_preset_table():
    assert tuple(PRESETS) == _lib.DIFFUSION_PRESETS and len(PRESETS) == 8
    for i, name in enumerate(PRESETS):
        t = _lib.hq_diffusion_taps()
        assert hq.load().hq_diffusion_preset(i, C.byref(t)) == _lib.HQ_OK
        w, div = preset(name)
        np.testing.assert_array_equal(np.array([list(r) for r in t.w]), w, err_msg=name)
        assert t.div == div
        pw, pdiv = hq.ImageManipulation.diffusionPreset(name)
        np.testing.assert_array_equal(pw, w)
        assert pdiv == div and pw.dtype == np.int32
        assert legal(w, div) and int(w.sum()) == (6 if name == "atkinson" else div)
    t = _lib.hq_diffusion_taps()
    for bad in (-1, 8):
        assert hq.load().hq_diffusion_preset(bad, C.byref(t)) == _lib.HQ_ERR_ARG
    assert hq.load().hq_diffusion_preset(0, None) == _lib.HQ_ERR_ARG
    with pytest.raises(ValueError):
        hq.ImageManipulation.diffusionPreset("floyd")


def test_the_legality_rule():
    lib = hq.load()
    cases = [preset(n) for n in PRESETS] + [TWELVE, (TWELVE[0], 78), (TWELVE[0], 77), (np.zeros((3, 5), np.int64), 1)]
    for dy in range(3):
        for dx in range(-2, 3):
            for wt in (1, -1, 2 ** 31 - 1):
                for div in (0, 1, -1, 2 ** 31 - 1):
                    w = np.zeros((3, 5), np.int64)
                    w[dy, dx + 2] = wt
                    cases.append((w, div))
    big = np.full((3, 5), 2 ** 31 - 1, np.int64)
    big[0, :3] = 0
    cases.append((big, 2 ** 31 - 1))  # (the sum passes int32)
    seen = set()
    for w, div in cases:
        want = legal(w, div)
        seen.add(want)
        assert lib.hq_diffusion_taps_legal(C.byref(c_taps(w, div))) == int(want), (w, div)
        rc, R, S = lib_classify(w, div)
        assert (rc == _lib.HQ_OK) == want and ((R, S) == classify(w) if want else (R, S) == (-1, -1)), (w, div)
    assert seen == {True, False}
    assert lib.hq_diffusion_taps_legal(None) == 0
    # the twelve legal positions are exactly the twelve that may hold a weight
    assert [(dy, dx) for dy in range(3) for dx in range(-2, 3) if legal(*single_tap(dy, dx))] == POSITIONS


def test_the_classification_of_every_preset():
    for name in PRESETS:
        w, div = preset(name)
        assert classify(w) == PRESET_CLASS[name], name
        assert lib_classify(w, div) == (_lib.HQ_OK,) + PRESET_CLASS[name], name
    assert classify(TWELVE[0]) == (2, 3) and lib_classify(*TWELVE) == (_lib.HQ_OK, 2, 3)
    want = {(0, 1): (1, 2), (0, 2): (1, 2), (1, -2): (1, 3), (1, -1): (1, 2), (1, 0): (1, 2), (1, 1): (1, 2),
            (1, 2): (1, 2)}
    for dy, dx in POSITIONS:
        w, div = single_tap(dy, dx)
        assert classify(w) == want.get((dy, dx), (2, 2)) and lib_classify(w, div)[1:] == classify(w), (dy, dx)
    assert {classify(preset(n)[0]) for n in PRESETS} == {(1, 2), (1, 3), (2, 2), (2, 3)}


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("w,h", EDGE_SHAPES)
def test_wavefront_order_is_raster_order(w, h, S):
    """Each pixel once; every source of a pixel -- up to (x + S - 1, y - 1) and (x + 2, y - 2), and the
    row's own (x - 1, y), (x - 2, y) -- lies on an earlier wavefront; and the two forms of the
    restatement agree on tap sets of that slope, with and without a second row."""
    order = np.full((h, w), -1)
    for t, (ys, xs) in enumerate(wavefronts(w, h, S)):
        assert np.all(order[ys, xs] == -1)
        order[ys, xs] = t
    assert np.all(order >= 0)
    for y in range(h):
        for x in range(w):
            for sy, sx in [(y, x - 1), (y, x - 2)] + [(y - 1, x + d) for d in range(-2, S)] + \
                          [(y - 2, x + d) for d in range(-2, 3)]:
                if 0 <= sy < h and 0 <= sx < w:
                    assert order[sy, sx] < order[y, x]
    rgba, pal = _case(w, h, 6, 10 * w + h)
    for name in [n for n in PRESETS if PRESET_CLASS[n][1] == S] + ["twelve"]:
        taps, div = TWELVE if name == "twelve" else preset(name)
        if classify(taps)[1] > S:
            continue
        for s in (1.0, 0.37):
            a, ua = diffuse(rgba, pal, w, h, s, taps, div, slope=S)
            b, ub = diffuse_raster(rgba, pal, w, h, s, taps, div)
            np.testing.assert_array_equal(a, b, err_msg=f"{name} s={s}")
            np.testing.assert_array_equal(ua, ub)


def test_strength_zero_is_the_plain_argmin():
    w, h, K = 23, 17, 6
    rgba, pal = _case(w, h, K, 3)
    for name in PRESETS:
        idx, used = diffuse(rgba, pal, w, h, 0.0, *preset(name))
        want_idx, want_used = o.assign(rgba, pal)
        np.testing.assert_array_equal(idx, want_idx)
        np.testing.assert_array_equal(used, want_used)


def test_ramp_costs_less_under_every_preset():
    """The 64 x 64 ramp under the eight cube corners (DESIGN.md 14's case): every preset's rendering
    costs strictly less than the nearest-colour one.  No order among the kernels is asserted."""
    w = h = 64
    rgba, pal = ramp_image(w, h), cube_corners()
    f = o.design_filters(72, 45.0)
    lab = o.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)

    def cost_of(idx, used):
        err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
        return o.average_array(err) + o.compute_penalty(used, 2.0)

    plain = cost_of(*o.assign(rgba, pal))
    for name in PRESETS:
        cost = cost_of(*diffuse(rgba, pal, w, h, 1.0, *preset(name)))
        print(f"{name}: {cost!r}, plain {plain!r}, ratio {cost / plain:.3f}")
        assert cost < plain, name

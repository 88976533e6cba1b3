"""CPU tests of the dithered rendering's restatement (dither_ref.py): its two forms agree,
strength 0 is the plain argmin, and error diffusion does what it is for under S-CIELAB --
the cost of the rendering drops, because the blur that precedes dE removes high-frequency
error and leaves the nearest-colour rendering's low-frequency error untouched.
"""

import numpy as np
import pytest

import oracle as o
from dither_ref import cube_corners, dither, dither_raster, ramp_image

# (the last three: the GPU tests' images narrower than the tap window that cross a strip of 64 rows)
EDGE_SHAPES = [(1, 5), (2, 3), (5, 1), (3, 70), (23, 17), (1, 130), (2, 129), (3, 66)]


def _case(w, h, K, seed):
    R, G, B = o.synthetic_image(w, h, seed)
    return o.inline_rgba(R, G, B).reshape(-1, 4), o.synthetic_palette(K, seed + 1).reshape(K, 4)


def cost_of(idx, used, pal, lab, f, w, h, delta=2.0):
    err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
    return o.average_array(err) + o.compute_penalty(used, delta)


@pytest.mark.parametrize("s", [1.0, 0.5])
@pytest.mark.parametrize("w,h", EDGE_SHAPES)
def test_wavefront_form_equals_raster_form(w, h, s):
    """Shapes without a left, right or upper neighbour, a column strip taller than it is
    wide (every wavefront one pixel per two rows) and one ordinary shape."""
    rgba, pal = _case(w, h, 6, 10 * w + h)
    a, ua = dither(rgba, pal, w, h, s)
    b, ub = dither_raster(rgba, pal, w, h, s)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ua, ub)
    assert len(np.unique(a)) > 1 or w * h < 4


@pytest.mark.parametrize("w,h,K", [(23, 17, 6), (64, 48, 16)])
def test_strength_zero_is_the_plain_argmin(w, h, K):
    rgba, pal = _case(w, h, K, 3)
    idx, used = dither(rgba, pal, w, h, 0.0)
    want_idx, want_used = o.assign(rgba, pal)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(used, want_used)


def test_ramp_costs_less_dithered():
    """A 64 x 64 RGB ramp under the eight cube corners at 72 dpi / 45 cm, dE76: the dithered
    rendering's cost is at most 0.6 of the nearest-colour one's (about half)."""
    w = h = 64
    rgba, pal = ramp_image(w, h), cube_corners()
    f = o.design_filters(72, 45.0)
    lab = o.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    plain = cost_of(*o.assign(rgba, pal), pal, lab, f, w, h)
    costs = {s: cost_of(*dither(rgba, pal, w, h, s), pal, lab, f, w, h) for s in (0.5, 1.0)}
    print(f"plain {plain!r}, dithered {costs!r}, ratio at 1: {costs[1.0] / plain:.3f}")
    assert costs[1.0] <= 0.6 * plain
    assert costs[0.5] < plain


def test_noise_image_changes_a_quarter_of_its_indices():
    w, h, K = 97, 53, 16
    R, G, B = o.synthetic_image(w, h, 5)
    rgba = o.inline_rgba(R, G, B).reshape(-1, 4)
    pal = o.synthetic_palette(K, 16).reshape(K, 4)
    idx, _ = dither(rgba, pal, w, h, 1.0)
    changed = float(np.mean(idx != o.assign(rgba, pal)[0]))
    print(f"{changed:.3f} of the indices change")
    assert changed >= 0.25

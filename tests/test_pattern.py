"""CPU tests of the pattern-dithering restatement (pattern_ref.py): the luminance order against
hand values, and the rule's two identities with the nearest colour."""

import numpy as np
import pytest

import oracle as o
from ordered_ref import bayer
from pattern_ref import luminance_order, pattern

TIES = np.array([[0.25, 0, 0, 0], [0, 0.25, 0, 0], [1, 1, 0, 0], [1, 1, 2.0 ** -26, 0], [0.25, 0, 0, 0]], np.float32)


def test_luminance_order_hand_values():
    # green .587 > red .299 > blue .114 > black; the two reds tie and keep their order
    pal = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    rank, color = luminance_order(pal)
    assert rank.tolist() == [4, 2, 1, 3, 0] and color.tolist() == [4, 2, 1, 3, 0]
    # TIES: colours 2 and 3 differ and have one Y (the blue term is absorbed); 0 and 4 are one colour
    rank, color = luminance_order(TIES)
    assert color.tolist() == [0, 4, 1, 2, 3] and rank.tolist() == [0, 2, 3, 4, 1]


@pytest.mark.parametrize("n,strength", [(1, 1.0), (1, 0.3), (16, 0.0), (64, 0.0)])
def test_identities_with_the_nearest_colour(n, strength):
    w, h = 13, 7
    rgba = o.inline_rgba(*o.synthetic_image(w, h, seed=3)).reshape(-1, 4)
    pal = o.synthetic_palette(6, 9).reshape(-1, 4)
    idx, used = pattern(rgba, pal, w, h, n, strength)
    want = o.assign(rgba, pal)
    np.testing.assert_array_equal(idx, want[0])
    np.testing.assert_array_equal(used, want[1])


def test_the_list_averages_to_the_pixel():
    """A grey between two palette colours: the list holds both in the pixel's proportion, darker first,
    so the map's low thresholds give the dark colour and every entry count is n times the proportion."""
    pal = np.array([[1, 1, 1, 0], [0, 0, 0, 0]], np.float32)
    rgba = np.full((16 * 16, 4), 0.25, np.float32)
    idx, _ = pattern(rgba, pal, 16, 16, 16, 1.0)
    assert np.count_nonzero(idx == 0) == 64  # a quarter white: the Bayer map's 64 highest thresholds
    m = bayer(4).reshape(-1)
    np.testing.assert_array_equal(idx == 0, m >= np.sort(m)[192])

"""CPU tests of ordered dithering: hq_bayer_map (host-only) against the restatement's integer
rule, the restatement (ordered_ref.py) at amplitude 0, and what the feature is for -- under
S-CIELAB the ordered rendering of a ramp costs about half the nearest-colour one's.
"""

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
from dither_ref import cube_corners, ramp_image
from hybridquantization_amd import _lib
from ordered_ref import bayer, bayer_rank, ordered
from test_dither import cost_of


@pytest.mark.parametrize("L", range(7))
def test_bayer_map_equals_the_restatement(L):
    n = 1 << L
    B = bayer_rank(L)
    np.testing.assert_array_equal(np.sort(B.reshape(-1)), np.arange(n * n))  # a permutation
    got = hq.ImageManipulation.bayerMap(L)
    assert got.shape == (n, n) and got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), bayer(L).view(np.uint32))
    # (B + 0.5) / n^2 - 0.5 exactly: the float64 value is the float32 one
    np.testing.assert_array_equal(got.astype(np.float64), (B + 0.5) / (n * n) - 0.5)
    assert got.min() == -0.5 + 0.5 / (n * n) and got.max() == 0.5 - 0.5 / (n * n)


def test_bayer_map_of_side_two_and_argument_checks():
    np.testing.assert_array_equal(hq.ImageManipulation.bayerMap(1), [[-0.375, 0.125], [0.375, -0.125]])
    lib = hq.load()
    buf = np.full(4, 7.0, np.float32)
    for bad in (-1, 7, 64):
        assert lib.hq_bayer_map(bad, _lib.fptr(buf)) == _lib.HQ_ERR_ARG
    assert lib.hq_bayer_map(1, None) == _lib.HQ_ERR_ARG
    assert np.all(buf == 7.0)


def test_ordered_amplitude_is_the_lattice_spacing():
    f = hq.ImageManipulation.orderedAmplitude
    assert f(8) == 1.0 and f(2) == 1.0 and f(1) == 1.0
    assert f(27) == pytest.approx(0.5) and f(64) == pytest.approx(1.0 / 3.0) and f(256) == pytest.approx(1 / (256 ** (1 / 3) - 1))


@pytest.mark.parametrize("w,h,K", [(23, 17, 6), (64, 48, 16)])
def test_amplitude_zero_is_the_plain_argmin(w, h, K):
    R, G, B = o.synthetic_image(w, h, 3)
    rgba = o.inline_rgba(R, G, B).reshape(-1, 4)
    pal = o.synthetic_palette(K, 4).reshape(K, 4)
    idx, used = ordered(rgba, pal, w, h, 0.0)
    want_idx, want_used = o.assign(rgba, pal)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(used, want_used)


def test_ramp_costs_less_ordered():
    """A 64 x 64 RGB ramp under the eight cube corners at 72 dpi / 45 cm, dE76, amplitude 1,
    Bayer 16 x 16: at most 0.6 of the nearest-colour rendering's cost (measured: 0.549)."""
    w = h = 64
    rgba, pal = ramp_image(w, h), cube_corners()
    f = o.design_filters(72, 45.0)
    lab = o.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    plain = cost_of(*o.assign(rgba, pal), pal, lab, f, w, h)
    cost = cost_of(*ordered(rgba, pal, w, h, 1.0, bayer(4)), pal, lab, f, w, h)
    print(f"plain {plain!r}, ordered {cost!r}, ratio {cost / plain:.3f}")
    assert cost <= 0.6 * plain


def test_shard_rows_are_the_whole_images_rows():
    """The restatement's y0: rows [20, 53) on their own equal those rows of the whole image."""
    w, h, K = 97, 53, 16
    R, G, B = o.synthetic_image(w, h, 5)
    rgba = o.inline_rgba(R, G, B).reshape(-1, 4)
    pal = o.synthetic_palette(K, 16).reshape(K, 4)
    whole, _ = ordered(rgba, pal, w, h, (0.3, 0.0, 0.7))
    part, _ = ordered(rgba[20 * w:], pal, w, h - 20, (0.3, 0.0, 0.7), y0=20)
    np.testing.assert_array_equal(part, whole[20 * w:])
    assert np.mean(whole != o.assign(rgba, pal)[0]) > 0.05

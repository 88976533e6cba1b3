"""CPU checks behind tests/test_long_filters_gpu.py: the dpi -> halfSize table of
its boundary cases, libhq's host-only filter design at those lengths, and the
checkers it leans on (oracle.shard_partial, oracle.reflect_index and the float64
exact_pixel_err) at the sizes it uses them: shards shorter than their halo and
images as small as the half-width."""

import ctypes

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
from hybridquantization_amd import _lib
from test_gpu import exact_pixel_err

# dpi at 45 cm -> halfSize: the dispatch boundaries of launch_cost_tiled_generic
TABLE = [(157, 24), (164, 25), (416, 64), (422, 65), (616, 95), (622, 96), (823, 127), (829, 128)]


@pytest.mark.parametrize("dpi,half", TABLE)
def test_dpi_to_half_size_table(dpi, half):
    f = o.design_filters(dpi, 45.0)
    assert f.half == half and f.taps == 2 * half + 1
    assert f.k1.shape == (f.taps, 4) and f.k3.shape == (f.taps,)


def test_ordinary_long_geometry():
    assert o.design_filters(300, 50.0).half == 51


@pytest.mark.parametrize("dpi", [416, 422, 823])
def test_design_filters_bitexact_with_oracle_at_long_filters(dpi):
    """test_design_filters_bitexact_with_oracle stops at 41 taps; here 129, 131
    and 255 (up-sampled by 2, 2 and 1: SP:79-88)."""
    k1, k2, k3, ak3, il = hq.design_filters(dpi, 45.0, hq.Whitepoint.D65)
    f = o.design_filters(dpi, 45.0)
    np.testing.assert_array_equal(k1, f.k1)
    np.testing.assert_array_equal(k2, f.k2)
    np.testing.assert_array_equal(k3, f.k3)
    np.testing.assert_array_equal(ak3, f.absk3)
    np.testing.assert_array_equal(il, f.illum)


def test_829_dpi_is_refused_at_255_taps():
    """257 taps: one step past the generic path's kMaxTaps."""
    lib = hq.load()
    buf = np.zeros(4 * 255, np.float32)
    taps = ctypes.c_int()
    p = _lib.fptr(buf)
    assert lib.hq_design_filters(829, 45.0, 1, 255, p, p, p, p, ctypes.byref(taps), p) == _lib.HQ_ERR_UNSUPPORTED
    assert taps.value == 257
    assert not buf.any()  # nothing written
    k1 = np.zeros(4 * 255, np.float32)
    k2, il = k1.copy(), np.zeros(3, np.float32)
    k3, ak3 = np.zeros(255, np.float32), np.zeros(255, np.float32)
    assert lib.hq_design_filters(823, 45.0, 1, 255, _lib.fptr(k1), _lib.fptr(k2), _lib.fptr(k3), _lib.fptr(ak3),
                                 ctypes.byref(taps), _lib.fptr(il)) == _lib.HQ_OK
    assert taps.value == 255  # the largest accepted


def test_shard_partial_with_shards_shorter_than_the_halo():
    """oracle.shard_partial at halfSize 25 on a 60 x 40 image: shards shorter than
    the halo (the extended window clipped on both sides), single-row shards at
    both borders (reflection inside the window).  Each shard runs the full
    image's fp32 operations on its rows, so the fp64 sums add up to
    eval_palette's error image and the used flags OR to its flags."""
    f = o.design_filters(164, 45.0)
    assert f.half == 25
    w, h, K = 60, 40, 12
    R, G, B = o.synthetic_image(w, h, seed=3)
    rgb = o.inline_rgba(R, G, B)[:, :3]
    lab = o.srgb_to_scielab(R, G, B, f, w)
    pal = o.synthetic_palette(K, 8)
    _, parts = o.eval_palette(rgb, lab, pal, f, w, return_parts=True)
    err = parts["err"].astype(np.float64).reshape(h, w)
    for bounds in ([0, 20, 40], [0, 13, 26, 40], [0, 5, 10, 15, 20, 25, 30, 35, 40], [0, 1, 2, 39, 40]):
        total, used = 0.0, np.zeros(K, bool)
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            s, u = o.shard_partial(rgb, lab, pal, f, w, h, r0, r1)
            assert abs(s - err[r0:r1].sum()) <= 1e-12 * err[r0:r1].sum(), (r0, r1)
            total += s
            used |= np.asarray(u) > 0
        assert abs(total - err.sum()) <= 1e-12 * err.sum()
        np.testing.assert_array_equal(used, np.asarray(parts["used"]) > 0)


@pytest.mark.parametrize("half", [10, 25, 127])
def test_reflection_at_the_smallest_image(half):
    """n == half: every window reflects at both ends and stays inside (CL:256-263
    reflects once); n == half - 1 does not."""
    idx = o.reflect_index(half, half)
    assert idx.min() == 0 and idx.max() == half - 1
    assert idx[0, 0] == half - 1 and idx[half - 1, 2 * half] == 0
    with pytest.raises(ValueError):
        o.reflect_index(half - 1, half)


def test_exact_pixel_err_at_the_smallest_image():
    """The float64 reference on a half x (half + 1) image: finite, and within fp32
    rounding of the oracle's own error image."""
    f = o.design_filters(164, 45.0)
    w, h, K = f.half, f.half + 1, 8
    R, G, B = o.synthetic_image(w, h, seed=5)
    rgb = o.inline_rgba(R, G, B)[:, :3]
    lab = o.srgb_to_scielab(R, G, B, f, w)
    pal = o.synthetic_palette(K, 9)
    _, parts = o.eval_palette(rgb, lab, pal, f, w, return_parts=True)
    ex = exact_pixel_err(parts["idx"], pal, lab, f, w, h)
    assert ex.shape == (w * h,) and np.isfinite(ex).all()
    np.testing.assert_allclose(parts["err"], ex, rtol=0, atol=2e-4)

"""The illuminant axis, without a GPU: conditions on the inputs of tests/test_illuminant_gpu.py,
checked with the oracles alone, so that the GPU tests cannot pass vacuously -- both segments of
Opp->Lab are populated in every component at every illuminant, the illuminants give different
LabRefs and costs (a component ignored on both sides of a comparison would show), and the
numpy oracle's LabRef follows a float64 statement of it at every illuminant.
"""

import itertools

import numpy as np
import pytest

import c_oracle
import hybridquantization_amd as hq
import illuminant_ref as ir
import oracle as o
from test_gpu import exact_pixel_err

DELTA3 = float(o.LABDELTA3)


def test_the_set():
    """D50's bits are the oracle's; every illuminant other than D65 differs from it in X and Z;
    and Yn: D65, D50 and A all have Yn = 1 exactly (the scaling of the Y row is invisible at
    them), dimD65 and brightD50 are the two with Yn != 1, one below and one above."""
    ills = ir.ills()
    assert tuple(ills) == ir.NAMES
    np.testing.assert_array_equal(ills["D50"].view(np.uint32), o.D50.view(np.uint32))
    np.testing.assert_array_equal(ills["D65"].view(np.uint32), o.D65.view(np.uint32))
    for name, il in ills.items():
        assert il.dtype == np.float32 and il.shape == (3,) and np.all(np.isfinite(il)) and np.all(il > 0)
        if name != "D65":
            assert il[0] != ills["D65"][0] and il[2] != ills["D65"][2], name
            # differs from D65 in component 1, or is one of the Yn = 1 white points
            assert il[1] != ills["D65"][1] or name in ("D50", "A"), name
    assert [n for n, il in ills.items() if il[1] != np.float32(1)] == ["dimD65", "brightD50"]
    assert ills["dimD65"][1] == np.float32(0.8) and ills["brightD50"][1] == np.float32(1.25)


def test_both_lab_segments_are_populated_at_every_illuminant():
    """The candidate of the dark case (the oracle's argmin of the 64-colour palette with dark
    colours), filtered in float64: per illuminant and per component X/Xn, Y/Yn, Z/Zn, at least
    500 of the 5141 pixels at or below delta^3 and at least 500 above it; at A the largest Z/Zn
    is above 2."""
    R, G, B, rgba = ir.dark_image()
    w, h = ir.DARK_W, ir.DARK_H
    assert w * h == 5141
    pal = ir.dark_palette(64)
    idx, _ = c_oracle.assign(rgba, pal)
    for name in ir.NAMES:
        f = ir.filters(name)
        t = ir.t_of_lab(exact_pixel_err(idx, pal, None, f, w, h, lab_only=True))
        below = (t <= DELTA3).sum(0)
        print(f"{name}: pixels at or below delta^3 (X, Y, Z) {below.tolist()} of {w * h}; largest t {t.max(0).round(3).tolist()}")
        assert np.all(below >= 500) and np.all(w * h - below >= 500), (name, below)
        if name == "A":
            assert t[:, 2].max() > 2.0


def test_illuminants_give_distinct_labrefs_and_costs():
    """Pairwise: the oracle's costs of one palette differ by more than 1e-3 relative and the
    LabRefs by more than 1e-2 somewhere -- an illuminant component ignored by the library and
    by the oracle it is compared with could not pass at all five."""
    R, G, B, rgba = ir.dark_image()
    w = ir.DARK_W
    pal = ir.dark_palette(64)
    labs = {n: ir.oracle_labref(n) for n in ir.NAMES}
    costs = {n: c_oracle.eval_palette(rgba, labs[n], pal, ir.filters(n), w) for n in ir.NAMES}
    print("oracle costs:", {n: round(c, 6) for n, c in costs.items()})
    for a, b in itertools.combinations(ir.NAMES, 2):
        assert abs(costs[a] - costs[b]) > 1e-3 * max(costs[a], costs[b]), (a, b)
        assert np.abs(labs[a][:, :3] - labs[b][:, :3]).max() > 1e-2, (a, b)


@pytest.mark.parametrize("name", ir.NAMES)
def test_numpy_oracle_labref_follows_float64(name):
    """oracle.srgb_to_scielab (fp32, the reference's order) within 1e-3 of illuminant_ref's
    float64 LabRef, and the C oracle within the same."""
    R, G, B, _ = ir.dark_image()
    f = ir.filters(name)
    ex = ir.labref_exact(name)
    d_np = np.abs(o.srgb_to_scielab(R, G, B, f, ir.DARK_W)[:, :3] - ex).max()
    d_c = np.abs(ir.oracle_labref(name)[:, :3] - ex).max()
    print(f"{name}: LabRef max |numpy oracle - float64| {d_np:.3g}, |C oracle - float64| {d_c:.3g}")
    assert d_np <= 1e-3 and d_c <= 1e-3


def test_design_filters_reports_the_white_point():
    for wp, want in ((hq.Whitepoint.D65, o.D65), (hq.Whitepoint.D50, o.D50)):
        np.testing.assert_array_equal(hq.design_filters(72, 45.0, wp)[4].view(np.uint32), want.view(np.uint32))

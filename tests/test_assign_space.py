"""Option "assign_space" without a GPU: the fp32 restatement the GPU tests use as their
yardstick against published CIELAB values and float64, the geometry the option's text states
(the coordinates are an isotropic scale of Lab; where the sRGB cube lands per illuminant), the
C surface's declarations, and the Python arguments' ValueErrors, which are raised before
anything runs."""

import os

import numpy as np
import pytest

import assign_space_ref as ar
import hybridquantization_amd as hq
import illuminant_ref as ir
from hybridquantization_amd import _lib
from hybridquantization_amd.scielab_processor import quantization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_against_published_lab():
    """The sRGB primaries and white under D65, to 0.01, in float64 and in the fp32 restatement."""
    rgb = np.array([k + (0.0,) for k in ar.PUBLISHED], np.float32)
    want = np.array(list(ar.PUBLISHED.values()))
    for fn in (ar.lab_f64, ar.lab_f32):
        got = fn(rgb, ar.PUBLISHED_D65)
        assert np.abs(got - want).max() <= 0.01, (fn.__name__, got)


@pytest.mark.parametrize("name", ["D65", "D50", "dimD65"])
def test_restatement_against_float64(name):
    """fp32 against float64 over the GPU test's colour sets: a few ulp of f times 500."""
    il = ir.ills()[name]
    for key, cols in ar.colour_sets().items():
        d = ar.dist(ar.coords_f32(cols, il), ar.coords_f64(cols, il)) * 256.0
        print(f"{name} {key}: |fp32 - float64| in dE76 max {d.max():.3g} mean {d.mean():.3g}")
        assert 0 < d.max() <= 2e-4


def test_coordinates_are_an_isotropic_scale_of_lab():
    cols = ar.colour_sets()["random4096"]
    il = ir.ills()["D65"]
    lab, q = ar.lab_f64(cols, il), ar.coords_f64(cols, il)
    np.testing.assert_allclose(ar.dist(q[:-1], q[1:]) * 256.0, ar.dist(lab[:-1], lab[1:]), rtol=1e-12)


def test_where_the_srgb_cube_lands():
    """Inside [0, 1]^3 under D65 and D50 (the extremes are corners of the cube); under illuminant A
    saturated blues leave it through b < -128."""
    lat = ar.colour_sets()["lattice17"]
    for name in ("D65", "D50"):
        q = ar.coords_f64(lat, ir.ills()[name])
        assert q.min() >= 0.0 and q.max() <= 1.0, (name, q.min(), q.max())
    q = ar.coords_f64(lat, ir.ills()["A"])
    blue = ar.coords_f64(np.array([[0, 0, 1, 0]], np.float32), ir.ills()["A"])[0]
    assert q[:, 2].min() < 0.0 and blue[2] < 0.0 and q[:, :2].min() >= 0.0


def test_c_surface():
    assert _lib.SIGNATURES["hq_assign_coords"][1][1:] == [_lib.C.c_int, _lib._f, _lib.C.c_int64, _lib._f]
    with open(os.path.join(ROOT, "include", "hq.h")) as f:
        text = f.read()
    assert "int hq_assign_coords(hq_ctx *ctx, int space, const float *rgba4, int64_t n, float *out4);" in text
    assert '"assign_space"' in text
    hq.load()  # (binds hq_assign_coords: the built library exports it)


def test_python_arguments_raise_before_anything_runs(monkeypatch):
    """A bad assignSpace, or "lab" with a rendering that keeps the sRGB rule, is a ValueError
    from findBestQuantization and quantization before a context is asked for anything: no
    library call is made (every entry of the loaded library is replaced by one that fails)."""
    IM = hq.ImageManipulation
    assert IM.assignSpaceValue("rgb") == 0 and IM.assignSpaceValue("lab") == 1
    for bad in ("Lab", "xyz", 1, None, b"lab"):
        with pytest.raises(ValueError):
            IM.assignSpaceValue(bad)
    calls = []
    m = IM.__new__(IM)  # no hq_create: the checks need no context
    m._require = lambda: calls.append("require") or (_ for _ in ()).throw(AssertionError("ran"))
    sw = hq.SWASA(population=2, imax=4, seed=1)
    img = np.zeros(4 * 64, np.float32)
    args = (img, None, 8, 4, sw, None, None, None)
    with pytest.raises(ValueError):
        m.findBestQuantization(*args, assignSpace="cielab")
    for kw in (dict(dither=0.5), dict(dot=1.0), dict(ordered=0.25), dict(ordered=(0.1, 0.1, 0.1)),
               dict(dither=0.5, ditherSearch=True), dict(ordered=0.25, orderedSearch=True),
               dict(dot=1.0, dotSearch="device"), dict(dot=1.0, dotSearch=True)):
        with pytest.raises(ValueError, match="assignSpace"):
            m.findBestQuantization(*args, assignSpace="lab", **kw)
    with pytest.raises(ValueError):
        m.assignCoords(np.zeros((2, 4), np.float32), space="hsv")
    assert calls == []
    made = []
    monkeypatch.setattr("hybridquantization_amd.scielab_processor.ImageManipulation.__init__",
                        lambda self, *a, **k: made.append(1))
    planar = np.zeros((3, 64), np.float32)
    with pytest.raises(ValueError):
        quantization(planar, 8, 4, sw, assignSpace="oklab")
    for kw in (dict(dither=1.0), dict(ordered=0.3), dict(dot=0.5), dict(dot=0.5, dotSearch=True),
               dict(pyramid=((2, 4), (1, 4)))):
        with pytest.raises(ValueError, match="assignSpace"):
            quantization(planar, 8, 4, sw, assignSpace="lab", **kw)
    assert made == []

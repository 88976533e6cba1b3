"""Option "assign_space": what the tests hold the library to (tests/test_assign_space.py,
tests/test_assign_space_gpu.py).  No GPU here.

The argmin coordinates of a colour (R, G, B) in space 1 are (L, a + 128, b + 128) / 256 of its
unfiltered CIELAB under an illuminant: sRGB decode (CL:85-87), RGB2XYZm (CL:77), division by the
white point, f(t) with its linear segment (CL:137), L = 116 fy - 16, a = 500 (fx - fy),
b = 200 (fy - fz).  Two statements of it:

  lab_f64 / coords_f64   float64 from the fp32 inputs (colour, matrix constants, illuminant):
                         the value every fp32 evaluation approximates;
  coords_f32             a plain fp32 numpy restatement, one rounding per operation, the cube
                         root numpy's: the yardstick of row a4's kind of bar -- the
                         device's distance from float64 is held to a multiple of this one's.
"""

import numpy as np

import oracle as o

f32 = np.float32

# CIELAB of the sRGB primaries and white under D65, as published for the sRGB matrix whose
# white is (0.95047, 1, 1.08883) (Lindbloom's tables).  libhq's own D65 has Zn = 1.0883
# (SP:20), which moves b by up to 0.03: the published values are checked under PUBLISHED_D65.
PUBLISHED_D65 = np.array([0.95047, 1.0, 1.08883], np.float32)
PUBLISHED = {
    (1.0, 0.0, 0.0): (53.2408, 80.0925, 67.2032),
    (0.0, 1.0, 0.0): (87.7347, -86.1827, 83.1793),
    (0.0, 0.0, 1.0): (32.2970, 79.1875, -107.8602),
    (1.0, 1.0, 1.0): (100.0, 0.0, 0.0),
}


def _rgb3(rgb):
    a = np.asarray(rgb, np.float32)
    a = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(-1, 4)
    return np.ascontiguousarray(a[:, :3])


def lab_f64(rgb, illum):
    """CIELAB (n, 3) float64 of fp32 colours (n, 3 or 4) under the fp32 illuminant."""
    d = np.float64
    p = _rgb3(rgb).astype(d)
    lin = np.where(p <= 0.04045, p / 12.92, ((p + 0.055) / 1.055) ** float(f32(2.4)))
    t = lin @ o.RGB2XYZM.astype(d).T / np.asarray(illum, np.float32)[:3].astype(d)
    f = np.where(t > d(o.LABDELTA3), np.cbrt(t), (d(o.KAPPA) * t + 16.0) / 116.0)
    return np.stack([116.0 * f[:, 1] - 16.0, 500.0 * (f[:, 0] - f[:, 1]), 200.0 * (f[:, 1] - f[:, 2])], -1)


def coords_of_lab(lab):
    lab = np.asarray(lab)
    return (lab + np.array([0.0, 128.0, 128.0], lab.dtype)) / lab.dtype.type(256.0)


def coords_f64(rgb, illum):
    return coords_of_lab(lab_f64(rgb, illum))


def lab_f32(rgb, illum):
    """The fp32 restatement: every operation rounded once to fp32, in the order written."""
    p = _rgb3(rgb)
    with np.errstate(invalid="ignore"):  # (numpy's own fp32 pow, not the oracle's float64 one)
        hi = np.power((p + f32(0.055)) / f32(1.055), f32(2.4)).astype(f32)
    lin = np.where(p <= f32(0.04045), p / f32(12.92), hi).astype(f32)
    inv = (f32(1.0) / np.asarray(illum, f32)[:3]).astype(f32)
    t = np.stack([o.dot3(lin, o.RGB2XYZM[i]) * inv[i] for i in range(3)], -1).astype(f32)
    with np.errstate(invalid="ignore"):
        root = np.cbrt(t).astype(f32)
    lin_seg = ((f32(o.KAPPA) * t + f32(16.0)) / f32(116.0)).astype(f32)
    f = np.where(t > f32(o.LABDELTA3), root, lin_seg).astype(f32)
    L = f32(116.0) * f[:, 1] - f32(16.0)
    a = f32(500.0) * (f[:, 0] - f[:, 1])
    b = f32(200.0) * (f[:, 1] - f[:, 2])
    return np.stack([L, a, b], -1).astype(f32)


def coords_f32(rgb, illum):
    return coords_of_lab(lab_f32(rgb, illum)).astype(f32)


def dist(a, b):
    """Euclidean distance per row, float64."""
    return np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).sum(-1))


def colour_sets():
    """name -> (n, 4) float32 colours: the 8 cube corners, a 17^3 lattice, 4096 random colours."""
    corners = np.array([[r, g, b, 0] for r in (0, 1) for g in (0, 1) for b in (0, 1)], np.float32)
    ax = (np.arange(17, dtype=np.float32) / f32(16))
    lat = np.zeros((17 ** 3, 4), np.float32)
    lat[:, :3] = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rnd = np.zeros((4096, 4), np.float32)
    rnd[:, :3] = np.random.default_rng(29).random((4096, 3), dtype=np.float32)
    return {"corners": corners, "lattice17": lat, "random4096": rnd}


def nearest_lab_de76(pix_rgb, pal_rgb, illum):
    """Per pixel: min over the palette of dE76(Lab(pixel), Lab(colour)) in float64, and its index."""
    lp, lc = lab_f64(pix_rgb, illum), lab_f64(pal_rgb, illum)
    d2 = ((lp[:, None, :] - lc[None, :, :]) ** 2).sum(-1)
    return np.sqrt(d2.min(1)), d2.argmin(1)

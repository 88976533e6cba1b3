"""The illuminant axis of the tests (tests/test_illuminant.py, tests/test_illuminant_gpu.py):
the set of white points, the oracle's filters under each, the shared dark 97 x 53 case, and a
float64 statement of LabRef.  No GPU here; everything is computed once and handed out
read-only.

The set.  D65 is the control: every other GPU test runs under it.  D50 is the reference's other
white point (SP:19-21).  A (1.0985, 1, 0.35585) is a caller-given illuminant far from both: Z/Zn
reaches 2.1, outside the (delta^3, ~1.1] that the cube root of the hot path was measured over.
All three have Yn = 1 exactly, so none of them can tell a Y row divided by Yn from one that is
not: dimD65 = 0.8 D65 (Yn = 0.8) and brightD50 = 1.25 D50 (Yn = 1.25) are there for that.
"""

from dataclasses import replace

import numpy as np

import c_oracle
import hybridquantization_amd as hq
import oracle as o

NAMES = ("D65", "D50", "A", "dimD65", "brightD50")
DARK_W, DARK_H, DARK_SEED = 97, 53, 150
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def ills():
    """name -> float32[3], in NAMES' order.  D50 comes from the library's filter design
    (hq_design_filters, host code), as a caller gets it."""
    def make():
        d65 = o.D65.copy()
        d50 = np.asarray(hq.design_filters(72, 45.0, hq.Whitepoint.D50)[4], np.float32).copy()
        out = {"D65": d65, "D50": d50, "A": np.array([1.0985, 1.0, 0.35585], np.float32),
               "dimD65": (d65 * np.float32(0.8)).astype(np.float32),
               "brightD50": (d50 * np.float32(1.25)).astype(np.float32)}
        for a in out.values():
            a.setflags(write=False)
        return out
    return _once("ills", make)


def filters(name, dpi=72, vd=45.0):
    """The oracle's filters at (dpi, vd) with the illuminant `name`: what every oracle reads."""
    base = _once(("filters", dpi, vd), lambda: o.design_filters(dpi, vd))
    return replace(base, illum=ills()[name].copy())


def dark_image():
    """(R, G, B, rgba) of the dark 97 x 53 case."""
    def make():
        from test_gpu import _dark_case
        R, G, B = _dark_case(DARK_W, DARK_H, seed=DARK_SEED)
        return R, G, B, o.inline_rgba(R, G, B)
    return _once("dark", make)


def dark_palette(K=64):
    def make():
        from test_gpu import _pal_with_dark
        return _pal_with_dark(K, 997 if K == 64 else 997 + K)
    return _once(("pal", K), make)


def labref_f64(R, G, B, f, w):
    """LabRef in float64 from the fp32 pixels and taps: sRGB -> linear (CL:85-87) -> RGB2XYZm
    (CL:77-90) -> XYZ2Oppm (CL:110-116) -> the three filter pairs with reflection (IM:319-346:
    conv = V1 H1 opp + V2 H2 opp, conv.x += V|3| H3 opp.x; CL:256-263) -> Opp->Lab (CL:124-145,
    X / Xn as the reference divides).  The matrices are the fp32 constants; nothing goes through
    RGB2Oppm.  -> (n, 3) float64."""
    d = np.float64
    rgb = np.stack([np.asarray(c, np.float32) for c in (R, G, B)], -1).astype(d)
    n = rgb.shape[0]
    h = n // w
    lin = np.where(rgb <= 0.04045, rgb / 12.92, ((rgb + 0.055) / 1.055) ** float(np.float32(2.4)))
    xyz = lin @ o.RGB2XYZM.astype(d).T
    opp = (xyz @ o.XYZ2OPPM.astype(d).T).reshape(h, w, 3)
    half = f.half
    hidx, vidx = o.reflect_index(w, half), o.reflect_index(h, half)
    k1, k2 = f.k1[:, :3].astype(d), f.k2[:, :3].astype(d)
    k3, ak3 = np.asarray(f.k3, d), np.asarray(f.absk3, d)
    t1 = np.zeros((h, w, 3)); t2 = np.zeros((h, w, 3)); t3 = np.zeros((h, w))
    for t in range(2 * half + 1):
        src = opp[:, hidx[:, t], :]
        t1 += src * k1[t]
        t2 += src * k2[t]
        t3 += src[..., 0] * k3[t]
    conv = np.zeros((h, w, 3))
    for t in range(2 * half + 1):
        r = vidx[:, t]
        conv += t1[r] * k1[t] + t2[r] * k2[t]
        conv[..., 0] += t3[r] * ak3[t]
    t_ = conv.reshape(-1, 3) @ o.OPP2XYZM.astype(d).T / np.asarray(f.illum[:3], d)
    fx = np.where(t_ > d(o.LABDELTA3), np.cbrt(t_), (d(o.KAPPA) * t_ + 16.0) / 116.0)
    return np.stack([116.0 * fx[:, 1] - 16.0, 500.0 * (fx[:, 0] - fx[:, 1]), 200.0 * (fx[:, 1] - fx[:, 2])], -1)


def t_of_lab(lab):
    """(X/Xn, Y/Yn, Z/Zn) back from a float64 Lab (n, 3): f = ((L + 16) / 116, a / 500 + fy,
    fy - b / 200), t = f^3 above f = 6/29 (t = delta^3 there), else (116 f - 16) / kappa."""
    lab = np.asarray(lab, np.float64)
    fy = (lab[:, 0] + 16.0) / 116.0
    f = np.stack([lab[:, 1] / 500.0 + fy, fy, fy - lab[:, 2] / 200.0], -1)
    return np.where(f > 6.0 / 29.0, f ** 3, (116.0 * f - 16.0) / np.float64(o.KAPPA))


def oracle_labref(name, case="dark", nthreads=1):
    """The C oracle's LabRef (n, 4) float32 of a case under the illuminant `name`."""
    def make():
        R, G, B, w = case_image(case)[:4]
        return c_oracle.srgb_to_scielab(R, G, B, filters(name), w, nthreads=nthreads)
    return _once(("lab", name, case), make)


def case_image(case):
    """(R, G, B, w, h, rgba) of "dark" or of a golden case's name."""
    def make():
        if case == "dark":
            R, G, B, rgba = dark_image()
            return R, G, B, DARK_W, DARK_H, rgba
        from test_gpu import load_case
        g, R, G, B = load_case(case)
        return R, G, B, int(g["w"]), int(g["h"]), o.inline_rgba(R, G, B)
    return _once(("case", case), make)


def labref_exact(name, case="dark"):
    def make():
        R, G, B, w = case_image(case)[:4]
        return labref_f64(R, G, B, filters(name), w)
    return _once(("lab64", name, case), make)

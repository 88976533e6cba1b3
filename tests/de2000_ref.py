"""CIEDE2000 (Sharma, Wu & Dalal, Color Res. Appl. 30(1), 2005; kL = kC = kH = 1)
stated plainly in numpy: the checker of libhq's HQ_DE_CIEDE2000.

    ciede2000(L1, a1, b1, L2, a2, b2, dtype=np.float64, other_branch=False)

Every operation runs in `dtype` (float64: the truth; float32: the plain
single-precision statement that serves as the yardstick of what fp32 allows).
Sample 1 is the reference colour, sample 2 the candidate; the result is
symmetric in the two.

The formula is discontinuous where the two hues are 180 degrees apart: there
dh' jumps between +180 and -180 (dH' changes sign) and the mean hue h-bar'
jumps by 180.  `other_branch=True` evaluates every pair on the other side of
that decision (|h'1 - h'2| <= 180 taken as > 180 and the reverse), so a pixel
within rounding of the jump can be compared with both neighbouring values.
"""
import json
import os

import numpy as np

SHARMA_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ciede2000_sharma.json")


def sharma_table():
    """The 34 pairs of Sharma's Table 1: (L1, a1, b1, L2, a2, b2, dE00) as float64 [34, 7]."""
    with open(SHARMA_JSON) as f:
        return np.asarray(json.load(f)["rows"], np.float64)


def _hue_deg(b, ap, t):
    h = np.degrees(np.arctan2(b, ap)).astype(t)
    h = np.where(h < 0, h + t(360), h)
    return np.where((b == 0) & (ap == 0), t(0), h).astype(t)


def hue_gap_deg(L1, a1, b1, L2, a2, b2):
    """|h'1 - h'2| in degrees (float64), NaN where C'1 C'2 = 0 (no hue difference is defined)."""
    p = _parts(L1, a1, b1, L2, a2, b2, np.float64)
    return np.where(p["C1p"] * p["C2p"] == 0, np.nan, np.abs(p["h1"] - p["h2"]))


def _parts(L1, a1, b1, L2, a2, b2, dtype):
    t = np.dtype(dtype).type
    L1, a1, b1, L2, a2, b2 = (np.asarray(v).astype(t) for v in (L1, a1, b1, L2, a2, b2))
    C1 = np.sqrt(a1 * a1 + b1 * b1)
    C2 = np.sqrt(a2 * a2 + b2 * b2)
    Cb = (C1 + C2) / t(2)
    Cb7 = Cb ** 7
    G = t(0.5) * (t(1) - np.sqrt(Cb7 / (Cb7 + t(25.0 ** 7))))
    a1p = (t(1) + G) * a1
    a2p = (t(1) + G) * a2
    C1p = np.sqrt(a1p * a1p + b1 * b1)
    C2p = np.sqrt(a2p * a2p + b2 * b2)
    return dict(L1=L1, L2=L2, C1p=C1p, C2p=C2p, h1=_hue_deg(b1, a1p, t), h2=_hue_deg(b2, a2p, t))


def ciede2000(L1, a1, b1, L2, a2, b2, dtype=np.float64, other_branch=False):
    t = np.dtype(dtype).type
    p = _parts(L1, a1, b1, L2, a2, b2, dtype)
    L1, L2, C1p, C2p, h1, h2 = p["L1"], p["L2"], p["C1p"], p["C2p"], p["h1"], p["h2"]
    with np.errstate(invalid="ignore", divide="ignore"):
        dLp = L2 - L1
        dCp = C2p - C1p
        zero = (C1p * C2p) == 0
        dh = h2 - h1
        near = np.abs(dh) <= t(180)
        if other_branch:
            near = ~near
        dh_far = np.where(dh > 0, dh - t(360), dh + t(360))
        dhp = np.where(zero, t(0), np.where(near, dh, dh_far)).astype(t)
        dHp = t(2) * np.sqrt(C1p * C2p) * np.sin(np.radians(dhp / t(2)).astype(t))
        Lb = (L1 + L2) / t(2)
        Cbp = (C1p + C2p) / t(2)
        hs = h1 + h2
        hb_far = np.where(hs < t(360), (hs + t(360)) / t(2), (hs - t(360)) / t(2))
        hb = np.where(zero, hs, np.where(near, hs / t(2), hb_far)).astype(t)
        rad = lambda d: np.radians(d).astype(t)  # noqa: E731
        T = (t(1) - t(0.17) * np.cos(rad(hb - t(30))) + t(0.24) * np.cos(rad(t(2) * hb))
             + t(0.32) * np.cos(rad(t(3) * hb + t(6))) - t(0.20) * np.cos(rad(t(4) * hb - t(63))))
        dth = t(30) * np.exp(-(((hb - t(275)) / t(25)) ** 2))
        Cbp7 = Cbp ** 7
        Rc = t(2) * np.sqrt(Cbp7 / (Cbp7 + t(25.0 ** 7)))
        d50 = (Lb - t(50)) ** 2
        SL = t(1) + t(0.015) * d50 / np.sqrt(t(20) + d50)
        SC = t(1) + t(0.045) * Cbp
        SH = t(1) + t(0.015) * Cbp * T
        RT = -np.sin(rad(t(2) * dth)) * Rc
        tl, tc, th = dLp / SL, dCp / SC, dHp / SH
        e2 = tl * tl + tc * tc + th * th + RT * tc * th
        return np.sqrt(np.maximum(e2, t(0))).astype(t)

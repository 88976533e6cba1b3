"""CPU checks behind tests/test_fast_path_gpu.py: the dpi -> halfSize table of
every fast half-width 0 .. 24, the trim-window rule on every designed geometry
the suite runs, the caller-supplied filter sets (asymmetric, wide k1, unit
tap) and what makes them a test -- the float64 reference moves far beyond the
bars when the taps are read mirrored or k3 and |k3| change places -- and the
conditions of the dE94 and CIEDE2000 rules (NaN share, pixels at the hue
jump) on the oracle alone, at the images and palettes the GPU module uses."""

import dataclasses

import numpy as np
import pytest

import c_oracle
import de2000_ref as d
import oracle as o
from test_gpu import _dark_case, _de94_exact, _pal_with_dark, exact_pixel_err

VD = 45.0
# dpi at 45 cm whose filters have halfSize 0, 1, .. 24 (index = halfSize)
DPI_45 = [4, 9, 15, 21, 28, 34, 41, 47, 54, 60, 67, 73, 80, 86, 93, 99, 105, 112, 118, 125, 131, 138, 144, 151, 157]
# the designed geometries the suite names elsewhere (test_viewing_geometry_vs_oracle, the default)
NAMED = [(72, 45.0, 10), (96, 60.0, 19), (150, 30.0, 15), (72, 30.0, 7), (100, 55.0, 18), (96, 70.0, 22),
         (200, 30.0, 20)]
LONG = (300, 50.0, 51)
BUCKETS = (10, 15, 19, 24)
# hq_cost_layout.h, trim_w: the narrow k1.x / k1.y / k1.z filters' significant half-windows per bucket
TRIM_W = {10: (3, 4, 5), 15: (4, 5, 7), 19: (5, 7, 9), 24: (6, 9, 12)}
# hq_cost_layout.h, kVTapMax: |tap| x 2^16 stays within f16's largest finite value
TAP_MAX = 65504.0 / 65536.0

_DESIGNED = {}


def designed(dpi, vd=VD):
    if (dpi, vd) not in _DESIGNED:
        _DESIGNED[(dpi, vd)] = o.design_filters(dpi, vd)
    return _DESIGNED[(dpi, vd)]


def designed_half(half):
    f = designed(*((LONG[0], LONG[1]) if half == LONG[2] else (DPI_45[half], VD)))
    assert f.half == half
    return f


def bucket(half):
    return next((hb for hb in BUCKETS if half <= hb), 0)


def trim_window_ok(f):
    """The rule of hq_cost_layout.h / trim_window_ok: outside the bucket's
    half-window every tap of k1.x, k1.y, k1.z is at most 1e-9 of that
    channel's peak (then `trim` 1 may skip those taps)."""
    hb = bucket(f.half)
    if not hb:
        return False
    dist = np.abs(np.arange(f.taps) - f.half)
    for ch in range(3):
        k = np.abs(f.k1[:, ch])
        if (k[dist > TRIM_W[hb][ch]] > np.float32(1e-9) * k.max()).any():
            return False
    return True


def fits_split(f):
    taps = np.concatenate([f.k1[:, :3].ravel(), f.k2[:, :3].ravel(), f.k3, f.absk3])
    return bool((np.abs(taps) <= TAP_MAX).all())  # (False for NaN)


# ---------------------------------------------------------------------------
# Caller-supplied filter sets (hq_set_filters takes any taps)
# ---------------------------------------------------------------------------
KINDS = ("asymmetric", "wide-k1", "unit-tap", "neg-tap")


def caller_filters(kind, half):
    """asymmetric: the designed taps of `half` times a ramp 0.5 .. 1 per channel
    and filter, rising and falling mixed; k3 times a falling ramp, absk3 =
    0.9 |designed k3| times a rising one (not |k3|).  Every ramp is <= 1, so no
    |tap| exceeds the designed one.  wide-k1: k1 = k2's wide profile per channel,
    scaled to k1's own tap sum (the stencil keeps its gain at DC; the trim
    window fails).  unit-tap: k1's centre tap
    (1, 1, 1), nothing else: the stencil is the identity and the candidate's Lab
    is plain CIELAB of the palette colour.  neg-tap: the same with -1.5 (both
    passes: the opponent colour times 2.25)."""
    f = designed_half(half)
    T = f.taps
    up = np.linspace(0.5, 1.0, T).astype(np.float32)
    down = up[::-1].copy()
    k1, k2, k3, ak3 = f.k1.copy(), f.k2.copy(), f.k3.copy(), f.absk3.copy()
    if kind == "asymmetric":
        for ch, (r1, r2) in enumerate(((up, down), (down, up), (up, down))):
            k1[:, ch] *= r1
            k2[:, ch] *= r2
        k3 = (k3 * down).astype(np.float32)
        ak3 = (np.float32(0.9) * np.abs(f.k3) * up).astype(np.float32)
    elif kind == "wide-k1":
        for ch in range(3):
            k1[:, ch] = f.k2[:, ch] * (f.k1[:, ch].sum(dtype=np.float64) / f.k2[:, ch].sum(dtype=np.float64))
    elif kind in ("unit-tap", "neg-tap"):
        k1, k2, k3, ak3 = np.zeros_like(k1), np.zeros_like(k2), np.zeros_like(k3), np.zeros_like(ak3)
        k1[half, :3] = 1.0 if kind == "unit-tap" else -1.5
    else:
        raise ValueError(kind)
    return dataclasses.replace(f, k1=k1, k2=k2, k3=k3, absk3=ak3, ofilters=None)


def mirrored(f):
    """Every filter read back to front (t <-> 2 half - t)."""
    return dataclasses.replace(f, k1=f.k1[::-1].copy(), k2=f.k2[::-1].copy(), k3=f.k3[::-1].copy(),
                               absk3=f.absk3[::-1].copy())


def k3_swapped(f):
    """k3 and |k3| in each other's pass."""
    return dataclasses.replace(f, k3=f.absk3.copy(), absk3=f.k3.copy())


def high_frequency_image(w, h, seed):
    """Neighbouring pixels far apart in colour: each channel a checkerboard of
    two levels with a random 8-bit offset, so a fill shifted by one byte shows."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    planes = []
    for ch in range(3):
        board = ((xx + (ch + 1) * yy) % 2).astype(np.float32)
        v = np.clip(np.round(40 + 150 * board + rng.integers(0, 60, (h, w))), 0, 255)
        planes.append((v / 255.0).astype(np.float32).reshape(-1))
    return planes


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("half", range(25))
def test_dpi_table_every_half_width(half):
    f = designed(DPI_45[half])
    assert f.half == half and f.taps == 2 * half + 1
    assert bucket(half) == (10 if half <= 10 else 15 if half <= 15 else 19 if half <= 19 else 24)
    assert fits_split(f)
    if half > 0:  # the table holds the first dpi of each half-width
        assert designed(DPI_45[half] - 1).half == half - 1


def test_designed_geometries_satisfy_the_trim_window():
    """Every designed geometry the suite runs on the fast path keeps
    trim_window_ok: the dispatch's `trim && trim_ok` is `trim` there, and only a
    caller's filters (wide-k1 below) reach the other branch."""
    for half in range(25):
        assert trim_window_ok(designed(DPI_45[half])), half
    for dpi, vd, half in NAMED:
        f = designed(dpi, vd)
        assert f.half == half and trim_window_ok(f), (dpi, vd)
    assert designed(LONG[0], LONG[1]).half == LONG[2]


def test_largest_designed_tap():
    """The largest designed tap over half-widths 0 .. 24, 4 dpi's single k1.x
    tap, is inside the split-f16 range; 1.0 is not."""
    peak = max(float(np.abs(np.concatenate([f.k1.ravel(), f.k2.ravel(), f.k3, f.absk3])).max())
               for f in (designed(dpi) for dpi in DPI_45))
    assert peak == float(np.abs(designed(4).k1[:, 0]).max())
    assert 0.98 < peak < TAP_MAX < 1.0
    assert np.float32(TAP_MAX) * np.float32(65536.0) == np.float32(65504.0)


def test_tap_range_bound_in_f16():
    """tap x 2^16 as f16: finite at the bound, infinite for a unit tap (numpy's
    float16 rounds to nearest even, as the library's host_f16 does)."""
    with np.errstate(over="ignore"):
        assert float(np.float16(np.float32(TAP_MAX) * np.float32(65536.0))) == 65504.0
        assert np.isinf(np.float16(np.float32(1.0) * np.float32(65536.0)))
        assert np.isinf(np.float16(np.float32(-1.5) * np.float32(65536.0)))
        for dpi in DPI_45:
            f = designed(dpi)
            taps = np.concatenate([f.k1.ravel(), f.k2.ravel(), f.k3, f.absk3]) * np.float32(65536.0)
            assert np.isfinite(taps.astype(np.float16)).all()


@pytest.mark.parametrize("half", [7, 10, 15, 24, 51])
def test_caller_filter_sets(half):
    f = designed_half(half)
    peak = float(np.abs(np.concatenate([f.k1.ravel(), f.k2.ravel(), f.k3, f.absk3])).max())
    a = caller_filters("asymmetric", half)
    for name in ("k1", "k2", "k3"):
        assert (np.abs(getattr(a, name)) <= np.abs(getattr(f, name))).all()
    assert (a.absk3 <= np.abs(f.k3)).all()
    assert float(np.abs(np.concatenate([a.k1.ravel(), a.k2.ravel(), a.k3, a.absk3])).max()) <= peak
    assert not np.array_equal(a.absk3, np.abs(a.k3))
    for name in ("k1", "k2"):  # no channel is symmetric any more
        for ch in range(3):
            k = getattr(a, name)[:, ch]
            assert not np.allclose(k, k[::-1], rtol=1e-3, atol=0)
    assert fits_split(a) and fits_split(caller_filters("wide-k1", half))
    if half <= 24:
        assert not trim_window_ok(caller_filters("wide-k1", half))
    for kind in ("unit-tap", "neg-tap"):
        u = caller_filters(kind, half)
        assert not fits_split(u) and u.half == half and np.count_nonzero(u.k1) == 3
        assert not (u.k2.any() or u.k3.any() or u.absk3.any())


def _image_and_refs(f, w, h, K):
    R, G, B = _dark_case(w, h, seed=w + h)
    rgb = o.inline_rgba(R, G, B)
    lab = o.srgb_to_scielab(R, G, B, f, w)
    pal = _pal_with_dark(K, 900 + w)
    idx, _ = o.assign(rgb[:, :3], pal)
    return rgb, lab, pal, idx


@pytest.mark.parametrize("half", [7, 10, 24])
def test_asymmetric_taps_give_the_suite_teeth(half):
    """On a 77 x 45 image the float64 per-pixel dE under the asymmetric taps read
    mirrored, or with k3 and |k3| swapped, is more than 10x the per-pixel bar
    (2e-4) away on more than 90 % of the pixels, and its sum more than 100x the
    sum bar (1e-5 relative): a kernel that reads its taps back to front, or the
    wrong k3, cannot pass test_caller_filters.  With the designed (symmetric)
    taps the mirrored reading stays inside the per-pixel bar."""
    w, h, K = 77, 45, 64
    f = caller_filters("asymmetric", half)
    rgb, lab, pal, idx = _image_and_refs(f, w, h, K)
    ex = exact_pixel_err(idx, pal, lab, f, w, h)
    for name, g in (("mirrored", mirrored(f)), ("k3 <-> |k3|", k3_swapped(f))):
        other = exact_pixel_err(idx, pal, lab, g, w, h)
        far = float((np.abs(other - ex) > 10 * 2e-4).mean())
        rel = abs(other.sum() - ex.sum()) / ex.sum()
        print(f"half {half} {name}: {far:.4f} of the pixels beyond 2e-3, sum off by {rel:.3g}")
        assert far > 0.9, (name, far)
        assert rel > 100 * 1e-5, (name, rel)
    # (the designed taps are symmetric to fp32 rounding of their design)
    sym = designed_half(half)
    np.testing.assert_allclose(exact_pixel_err(idx, pal, lab, sym, w, h),
                               exact_pixel_err(idx, pal, lab, mirrored(sym), w, h), rtol=0, atol=2e-4)


def test_unit_tap_is_plain_cielab():
    """unit-tap: the float64 candidate Lab is Opp -> Lab of the palette colour of
    each pixel; neg-tap: of 2.25 times its opponent colour."""
    w, h, K, half = 33, 21, 16, 10
    for kind, scale in (("unit-tap", 1.0), ("neg-tap", 2.25)):
        f = caller_filters(kind, half)
        rgb, lab, pal, idx = _image_and_refs(f, w, h, K)
        got = exact_pixel_err(idx, pal, lab, f, w, h, lab_only=True)
        p = pal[:, :3].astype(np.float64)
        lin = np.where(p <= 0.04045, p / 12.92, ((p + 0.055) / 1.055) ** float(np.float32(2.4)))
        xyz = scale * (lin @ o.RGB2OPPM.astype(np.float64).T)[idx] @ o.OPP2XYZM.astype(np.float64).T / f.illum[:3]
        fx = np.where(xyz > o.LABDELTA3, np.cbrt(xyz), (o.KAPPA * xyz + 16.0) / 116.0)
        want = np.stack([116 * fx[:, 1] - 16, 500 * (fx[:, 0] - fx[:, 1]), 200 * (fx[:, 1] - fx[:, 2])], -1)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def test_high_frequency_image_separates_neighbours():
    for w, h in ((300, 45), (303, 93), (535, 45)):
        R, G, B = high_frequency_image(w, h, seed=w)
        idx, _ = o.assign(np.stack([R, G, B], -1), o.synthetic_palette(256, 11))
        idx = idx.reshape(h, w)
        assert (idx[:, 1:] != idx[:, :-1]).mean() >= 0.5


# (filters, half, w, h, palette sizes and their index j in the GPU module's seeds 900 + j + w)
_CONDITION_CASES = (
    [("designed", half, 301, 93, ((64, 0), (256, 1))) for half in (7, 10, 12, 15, 17, 19, 21, 24)]  # test_instance_matrix
    + [("designed", half, 535, 45, ((64, 0), (256, 1))) for half in (7, 10)]                          # its 256-column form
    + [("designed", 10, w, 45, ((300, 0), (4200, 0))) for w in (300, 301, 302)]                      # test_chunked_cost_matrix
    + [("designed", 10, 301, 45, ((513, 0), (1100, 1), (2100, 0), (8192, 1)))]                       # (its other chunk counts)
    + [("asymmetric", 10, 301, 93, ((64, 0), (256, 1)))])                                            # test_caller_filters


@pytest.mark.parametrize("kind,half,w,h,pals", _CONDITION_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}x{c[3]}-K{c[4][0][0]}" for c in _CONDITION_CASES])
def test_de94_and_de2000_conditions_hold_on_the_oracle(kind, half, w, h, pals):
    """The dE94 NaN share (2e-3) and the CIEDE2000 exclusion cap (2e-3 of the
    pixels within 0.5 degrees of the hue jump) are conditions of the GPU tests'
    rules: the oracle alone (ciede94_f32, de2000_ref) stays inside them on every
    image, half-width and palette on which test_fast_path_gpu.py applies those
    rules -- both half-widths of each bucket of test_instance_matrix, the
    chunked matrix's three widths at K = 300 and 4200, and the asymmetric set
    (the unit tap's plain CIELAB has hue-aligned pairs on 2.5e-3 to 5.8e-3 of the
    pixels: test_caller_filters runs the other dE types on the asymmetric set
    only; test_fast_path_shards compares shards with the full image and does
    not apply the rules)."""
    f = designed_half(half) if kind == "designed" else caller_filters(kind, half)
    R, G, B = _dark_case(w, h, seed=w + h)
    rgb = o.inline_rgba(R, G, B)
    lab = c_oracle.srgb_to_scielab(R, G, B, f, w)
    ref64 = [lab[:, i].astype(np.float64) for i in range(3)]
    for K, j in pals:
        pal = _pal_with_dark(K, 900 + j + w)
        idx, _ = c_oracle.assign(rgb, pal)
        e94 = o.ciede94_f32(lab, o.candidate_scielab(idx, pal, f, w, h))
        cand64 = exact_pixel_err(idx, pal, lab, f, w, h, lab_only=True)
        _, dH2, dab2 = _de94_exact(lab, cand64)
        nan = np.isnan(e94)
        gap = d.hue_gap_deg(*ref64, *[cand64[:, i] for i in range(3)])
        excl = float((np.abs(gap - 180.0) < 0.5).mean())
        print(f"{kind} half {half} {w}x{h} K={K}: dE94 NaN share {nan.mean():.3g}, at the hue jump {excl:.3g}")
        assert nan.mean() < 2e-3
        assert (np.abs(dH2) <= 1e-3 * (np.sqrt(dab2) + 1.0))[nan].all()
        assert excl < 2e-3

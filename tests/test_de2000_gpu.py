"""HQ_DE_CIEDE2000 through the C ABI (the Python mirror) on the GPU: libhq's own
dE type (the reference's branch is empty, CL:227-230) against the formula of
Sharma, Wu & Dalal (2005) as tests/de2000_ref.py states it in float64, with
its plain float32 form on the oracle's fp32 Lab as the yardstick of what
single precision allows.

The formula jumps where the two hues are 180 degrees apart (dH' changes sign,
h-bar' moves by 180 degrees).  A pixel whose float64 hues are within 0.5
degrees of that is compared with the float64 value of either side; such pixels
stay below 2e-3 of every case (asserted on the float64 side).
"""

import ctypes as C

import numpy as np
import pytest

import c_oracle
import de2000_ref as d
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from test_gpu import GOLD, _dark_case, _pal_with_dark, exact_pixel_err, load_case  # noqa: F401

pytestmark = pytest.mark.gpu

DE00 = hq.deltaETypes.CIEDE2000
EXCL_DEG = 0.5     # |  |h'1 - h'2| - 180 | below this (float64): either branch's value
EXCL_CAP = 2e-3    # share of such pixels per case
FP32_ABS = 2e-5    # the formula's own fp32 evaluation (a plain fp32 statement: <= 1.3e-5)


def _threads():
    import os
    return max(1, min(16, len(os.sched_getaffinity(0))))


@pytest.fixture(scope="module")
def filt():
    return o.design_filters()


def _ctx(gpu, rgba, lab, w, illum, de=DE00, dpi=72, vd=45.0, **opts):
    m = pr.Context(de, device=gpu)
    hq.ScielabProcessor(dpi, vd, hq.Whitepoint.D65, None, m)
    for k, v in opts.items():
        m.setOption(k, v)
    m.setImage(rgba.reshape(-1), None if lab is None else lab.reshape(-1), w, illum)
    return m


def _inline(lab3):
    out = np.zeros((len(lab3), 4), np.float32)
    out[:, :3] = lab3
    return out


def _cols(x):
    return [x[:, i] for i in range(x.shape[1])]


# ---------------------------------------------------------------------------
# 1. Sharma's table through computeError (error_image_kernel<2>)
# ---------------------------------------------------------------------------
def _compute_error(m, lab1, lab2):
    img = np.zeros(4 * len(lab1), np.float32)
    mean = m.computeError(_inline(lab1).reshape(-1), _inline(lab2).reshape(-1), img)
    return mean, img.reshape(-1, 4)


def _err_from_image(img):
    """e from the error image (255 - e)^2 / 255^2 (e < 255)."""
    return 255.0 - 255.0 * np.sqrt(img[:, 0].astype(np.float64))


@pytest.fixture(scope="module")
def de00_ctx(gpu):
    m = pr.Context(DE00, device=gpu)
    assert m.getOpenCLAvailable()
    yield m
    m.close()


def _table_values(m, lab1, lab2):
    """dE of each pair, one pair per call (the returned mean is that pair's dE)."""
    return np.array([_compute_error(m, lab1[i:i + 1], lab2[i:i + 1])[0] for i in range(len(lab1))])


def test_sharma_table_through_compute_error(de00_ctx):
    """The 34 published pairs: |GPU - table| <= 1e-4 (5e-5 the table's rounding,
    5e-5 for fp32: a plain fp32 statement is within 1e-5 of float64 here, which
    leaves 5x for the hardware's transcendentals), as one Lab image pair and
    one pair per call.  Pairs 10 and 14 sit exactly on the 180 degree jump:
    either neighbouring value passes.  Swapping the samples: within 2e-5."""
    m = de00_ctx
    t = d.sharma_table()
    lab1, lab2, want = t[:, 0:3], t[:, 3:6], t[:, 6]
    alt = want.copy()
    alt[9], alt[13] = 7.2195, 4.7461
    e = _table_values(m, lab1, lab2)
    diff = np.minimum(np.abs(e - want), np.abs(e - alt))
    print("per pair |gpu - table|:", np.array2string(diff, precision=2), "worst", diff.max())
    assert np.isfinite(e).all()
    assert diff.max() <= 1e-4
    # the 34 pairs as one image pair: the mean, and each pixel through the error image
    mean, img = _compute_error(m, lab1, lab2)
    assert abs(mean - e.mean()) <= 1e-6 * e.mean()
    want_img = ((255.0 - e) ** 2 / 255.0 ** 2)
    np.testing.assert_allclose(img[:, 0], want_img, rtol=2e-6)  # (255 - e)^2 / 255^2 of the same e, in fp32
    np.testing.assert_array_equal(img[:, 1], img[:, 0])
    np.testing.assert_array_equal(img[:, 2], img[:, 0])
    assert not img[:, 3].any()
    # swapped samples
    es = _table_values(m, lab2, lab1)
    print("swap: worst", np.abs(es - e).max())
    assert np.abs(es - e).max() <= 2e-5


def test_identical_grey_and_degenerate_pairs(de00_ctx):
    """Identical inputs give exactly 0.0; grey/grey gives |dL| / S_L and
    grey/chromatic is finite: both match float64 (C'1 C'2 = 0: dh' = 0 and
    h-bar' = h'1 + h'2)."""
    m = de00_ctx
    rng = np.random.default_rng(11)
    n = 4096
    lab = np.c_[rng.uniform(0, 100, n), rng.uniform(-110, 110, n), rng.uniform(-110, 110, n)].astype(np.float32)
    lab[:64, 1:] = 0          # greys
    lab[64:128, 1] = 0        # on the b axis
    lab[128:192, 2] = 0       # on the a axis
    mean, img = _compute_error(m, lab, lab)
    assert mean == 0.0
    assert (img[:, 0] == 1.0).all()  # (255 - 0)^2 / 255^2
    # grey / grey, grey / chromatic, chromatic / grey, and hues exactly opposite on an axis
    grey = lab.copy()
    grey[:, 1:] = 0
    other = np.roll(lab, 1, axis=0)
    opp = lab.copy()
    opp[:, 1:] = -opp[:, 1:]
    for name, (x, y) in {"grey/grey": (grey, np.roll(grey, 1, axis=0)), "grey/chromatic": (grey, other),
                         "chromatic/grey": (other, grey)}.items():
        mean, img = _compute_error(m, x, y)
        e = _err_from_image(img)
        ref = d.ciede2000(*_cols(x.astype(np.float64)), *_cols(y.astype(np.float64)))
        assert np.isfinite(mean) and np.isfinite(img).all(), name
        # (the error image holds (255 - e)^2 / 255^2 in fp32: e to ~2e-5 absolute)
        print(name, "worst |gpu - float64| via the error image", np.abs(e - ref).max())
        np.testing.assert_allclose(e, ref, rtol=0, atol=1e-4, err_msg=name)
        assert abs(mean - ref.mean()) <= 2e-6 * ref.mean(), name
    # one pair per call gives the pair's dE itself: grey/grey is |dL| / S_L
    for i in (0, 1, 2, 70, 130):
        e = _compute_error(m, grey[i:i + 1], np.roll(grey, 1, axis=0)[i:i + 1])[0]
        L1, L2 = float(grey[i, 0]), float(np.roll(grey, 1, axis=0)[i, 0])
        sl = 1 + 0.015 * ((L1 + L2) / 2 - 50) ** 2 / np.sqrt(20 + ((L1 + L2) / 2 - 50) ** 2)
        assert abs(e - abs(L1 - L2) / sl) <= 2e-6 * max(e, 1.0)
    mean, img = _compute_error(m, lab, opp)  # exactly opposite hues: the jump itself, both sides finite
    assert np.isfinite(mean) and np.isfinite(img).all()
    e = _err_from_image(img)
    c64 = _cols(lab.astype(np.float64)) + _cols(opp.astype(np.float64))
    ref = np.minimum(np.abs(e - d.ciede2000(*c64)), np.abs(e - d.ciede2000(*c64, other_branch=True)))
    assert ref.max() <= 2e-4  # via the fp32 error image, at dE up to ~150


# ---------------------------------------------------------------------------
# 2. Per-pixel dE against float64 (the pattern of test_pixel_errors_de94_vs_oracle)
# ---------------------------------------------------------------------------
_CASES = {}


def _case(name):
    """Inputs and CPU references of a case, computed once and shared by its variants."""
    if name in _CASES:
        return _CASES[name]
    if name.startswith("case_"):
        g, R, G, B = load_case(name)
        w, h = int(g["w"]), int(g["h"])
        dpi, vd = 72, 45.0
        f = o.design_filters()
        pals = [p for p in g["palettes"]]
        lab = g["lab"].astype(np.float32)
    else:
        dims, geo = name.split("_")[1], name.split("_")[2]
        w, h = (int(v) for v in dims.split("x")) if "x" in dims else (int(dims), int(dims))
        dpi, vd = {"9660": (96, 60.0), "7245": (72, 45.0), "15030": (150, 30.0), "30050": (300, 50.0)}[geo]
        f = o.design_filters(dpi, vd)
        R, G, B = _dark_case(w, h, seed=w + h)
        pals = [_pal_with_dark(64, 900 + w), _pal_with_dark(256, 901 + w)]
        lab = c_oracle.srgb_to_scielab(R, G, B, f, w, nthreads=_threads())
    rgba = o.inline_rgba(R, G, B)
    ref64 = _cols(lab[:, :3].astype(np.float64))
    per_pal = []
    for pal in pals:
        _, parts = c_oracle.eval_palette(rgba, lab, pal, f, w, nthreads=_threads(), return_parts=True)
        cand64 = exact_pixel_err(parts["idx"], pal, lab, f, w, h, lab_only=True)
        cand32 = o.candidate_scielab(parts["idx"], pal, f, w, h).reshape(-1, 4)[:, :3].astype(np.float32)
        ex = d.ciede2000(*ref64, *_cols(cand64))
        ex_other = d.ciede2000(*ref64, *_cols(cand64), other_branch=True)
        gap = d.hue_gap_deg(*ref64, *_cols(cand64))
        excl = np.abs(gap - 180.0) < EXCL_DEG  # (NaN gap, C'1 C'2 = 0: no hue difference, not excluded)
        yard = d.ciede2000(*_cols(lab[:, :3]), *_cols(cand32), dtype=np.float32).astype(np.float64)
        for a in (ex, ex_other, excl, yard):
            a.setflags(write=False)
        per_pal.append(dict(pal=pal, idx=parts["idx"], ex=ex, ex_other=ex_other, excl=excl, yard=yard))
    _CASES[name] = dict(w=w, h=h, dpi=dpi, vd=vd, f=f, rgba=rgba, lab=lab, pals=per_pal)
    return _CASES[name]


def _dist(e, ref):
    """|e - float64|, for the pixels set aside against the nearer of the two branches."""
    dd = np.abs(e - ref["ex"])
    return np.where(ref["excl"], np.minimum(dd, np.abs(e - ref["ex_other"])), dd)


@pytest.mark.parametrize("variant", [(0, 16, 1), (0, 16, 0), (0, 8, 1), (1, 16, 1), (2, 16, 1)])
@pytest.mark.parametrize("case", ["case_97x53_k64", "dark_193x131_7245", "dark_256_9660", "dark_200x136_15030",
                                  "dark_160x144_30050"])
def test_pixel_errors_de2000_vs_float64(gpu, case, variant):
    """(cost_variant, cost_rows, trim): cost16w (trimmed and not), cost_mfma, the
    LDS-tiled generic pair and the per-pixel generic pair; tap buckets 10, 19
    and 15, and halfSize 51 (300 dpi / 50 cm), which takes the matrix-core
    generic pair whatever the variant.  Indices bit-exact; no NaN or inf; every
    pixel's |GPU - float64| at most 2x the yardstick's worst |fp32 - float64|
    plus 2e-5, its mean at most 1.5x the yardstick's mean plus 2e-5 (the 2x and
    1.5x are dE76's and dE94's bars, resting on the same split-f16 argument;
    2e-5 covers the formula's own fp32 evaluation), pixels within 0.5 degrees
    of the 180 degree jump against either branch; the cost against the float64
    mean within 1e-5."""
    c = _case(case)
    w = c["w"]
    m = _ctx(gpu, c["rgba"], c["lab"], w, c["f"].illum, dpi=c["dpi"], vd=c["vd"], pixel_err=1,
             cost_variant=variant[0], cost_rows=variant[1], trim=variant[2])
    for ref in c["pals"]:
        pal = ref["pal"]
        K = pal.shape[0]
        share = float(ref["excl"].mean())
        assert share < EXCL_CAP, f"{case} K={K}: {share:.3g} of the pixels within {EXCL_DEG} degrees of the jump"
        cost = m.computeQuantizationErrorPopulation([pal.reshape(-1)], 2.0)[0]
        np.testing.assert_array_equal(m.getIndices(0), ref["idx"].astype(np.uint8))
        err = m.getPixelErrors(0)
        assert np.isfinite(err).all() and np.isfinite(cost)
        keep = ~ref["excl"]
        d_gpu, d_yard = _dist(err.astype(np.float64), ref), _dist(ref["yard"], ref)
        stats = (f"{case} K={K} variant {variant}: set aside {int(ref['excl'].sum())} px ({share:.2g}); "
                 f"|gpu-f64| max {d_gpu[keep].max():.3g} mean {d_gpu[keep].mean():.3g}"
                 f" (set aside: max {d_gpu[~keep].max() if (~keep).any() else 0:.3g}); "
                 f"|fp32-f64| max {d_yard[keep].max():.3g} mean {d_yard[keep].mean():.3g}")
        print(stats)
        bar = 2 * d_yard[keep].max() + FP32_ABS
        assert d_gpu[keep].max() <= bar, stats
        assert d_gpu[keep].mean() <= 1.5 * d_yard[keep].mean() + FP32_ABS, stats
        assert d_gpu.max() <= bar, stats  # the pixels set aside: the same bar, either branch
        # the cost (IM:736-768 mean + penalty): float64 mean, a pixel set aside at the branch the GPU took
        # (Both branches are correct values there, and the GPU's choice only decides which of
        # the two float64 values stands in the mean: it cannot absorb an error of the GPU's,
        # since every such pixel is held to `bar` against the branch chosen, just above.  The
        # choice moves `want` by at most sum|ex_other - ex| / n over the < 2e-3 of the pixels
        # set aside, printed below as `branch slack` beside the 1e-5 bar.)
        slack = float(np.abs(ref["ex_other"] - ref["ex"])[ref["excl"]].sum()) / ref["excl"].size
        print(f"{case} K={K}: branch slack {slack:.3g} of a mean {float(ref['ex'].mean()):.3g}")
        near_other = ref["excl"] & (np.abs(err - ref["ex_other"]) < np.abs(err - ref["ex"]))
        used = np.bincount(ref["idx"], minlength=K)[:K] > 0
        want = float(np.where(near_other, ref["ex_other"], ref["ex"]).mean()) + 2.0 * float(np.count_nonzero(~used))
        assert abs(cost - want) <= 1e-5 * want, stats
    m.close()


# ---------------------------------------------------------------------------
# 3. Costs: fast path against generic, used flags and penalty against a CIE76 context
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(97, 53), (193, 131)])
@pytest.mark.parametrize("rows,tw,trim", [(16, 128, 1), (16, 256, 1), (8, 128, 1), (16, 128, 0)])
def test_de2000_fast_path_matches_generic(gpu, filt, w, h, rows, tw, trim):
    """_compare_fast_generic's shape for CIE76, on CIEDE2000: costs of the fast
    path and the generic pair within 1e-6 relative, per pixel within 2e-4, no
    NaN; edge and partial tiles at both sizes, two tile rows and columns at
    193 x 131."""
    R, G, B = o.synthetic_image(w, h, seed=w)
    m = _ctx(gpu, o.inline_rgba(R, G, B), None, w, filt.illum, trim=trim, cost_rows=rows, cost_tw=tw, pixel_err=1)
    for K in (16, 64, 256):
        p = o.synthetic_palette(K, 7 + K)
        cost, err = {}, {}
        for variant in (0, 1):
            m.setOption("cost_variant", variant)
            cost[variant] = m.computeQuantizationErrorPopulation([p.reshape(-1)], 2.0)[0]
            err[variant] = m.getPixelErrors(0)
        assert np.isfinite(err[0]).all() and np.isfinite(err[1]).all()
        print(f"K={K}: per pixel worst {np.abs(err[0] - err[1]).max():.3g}, costs {cost[0]!r} {cost[1]!r}")
        np.testing.assert_allclose(err[0], err[1], rtol=0, atol=2e-4)
        np.testing.assert_allclose(cost[0], cost[1], rtol=1e-6)
    m.close()


@pytest.mark.parametrize("w,h", [(97, 53), (193, 131)])
def test_de2000_used_flags_and_penalty_as_cie76(gpu, filt, w, h):
    """The argmin is nearest in RGB whatever the dE type: used flags, indices and
    so the penalty delta * #unused equal a CIE76 context's on the same palettes."""
    R, G, B = o.synthetic_image(w, h, seed=w + 1)
    rgba = o.inline_rgba(R, G, B)
    pals = np.stack([o.synthetic_palette(256, 31 + p) for p in range(3)])
    pals[1, 200:] = pals[1, 3]  # duplicates: never chosen (strict <), so unused
    out = {}
    for de in (hq.deltaETypes.CIE76, DE00):
        m = _ctx(gpu, rgba, None, w, filt.illum, de=de, pixel_err=1)
        costs, used = m.computeQuantizationErrorPopulation(pals.reshape(3, -1), 2.0, return_used=True)
        means = [float(m.getPixelErrors(p).astype(np.float64).mean()) for p in range(3)]
        out[de] = (costs, used, [m.getIndices(p) for p in range(3)], means)
        m.close()
    a, b = out[hq.deltaETypes.CIE76], out[DE00]
    np.testing.assert_array_equal(a[1], b[1])
    for p in range(3):
        np.testing.assert_array_equal(a[2][p], b[2][p])
        unused = int(np.count_nonzero(a[1][p] == 0))
        assert unused >= (56 if p == 1 else 0)
        for costs, means in ((a[0], a[3]), (b[0], b[3])):  # cost - mean dE = 2 * #unused on both
            assert abs((costs[p] - means[p]) - 2.0 * unused) <= 1e-5 * costs[p]
    assert np.all(np.abs(a[0] - b[0]) > 1e-3 * a[0])  # and the dE part differs


# ---------------------------------------------------------------------------
# 4. The other paths, each against the generic exhaustive path of the same context
# ---------------------------------------------------------------------------
def _exhaustive(m, pals, P):
    for k, v in (("chunked", 0), ("grid", 0), ("cost_variant", 1)):
        m.setOption(k, v)
    costs, used = m.computeQuantizationErrorPopulation(pals.reshape(P, -1), 2.0, return_used=True)
    return costs, used, [m.getIndices32(p) for p in range(P)]


@pytest.mark.parametrize("K,opts", [(300, {"lists16": 0}), (600, {}), (300, {"chunked": 0})],
                         ids=["K300-grid-per-chunk", "K600-lists16", "K300-32bit-indices"])
def test_de2000_wide_palettes_match_exhaustive(gpu, filt, K, opts):
    w, h, P = 160, 96, 2
    R, G, B = o.synthetic_image(w, h, seed=K)
    pals = np.stack([o.synthetic_palette(K, 500 + p) for p in range(P)])
    m = _ctx(gpu, o.inline_rgba(R, G, B), None, w, filt.illum, **opts)
    costs, used = m.computeQuantizationErrorPopulation(pals.reshape(P, -1), 2.0, return_used=True)
    idx = [m.getIndices32(p) for p in range(P)]
    assert np.isfinite(costs).all()
    ref = _exhaustive(m, pals, P)
    m.close()
    np.testing.assert_allclose(costs, ref[0], rtol=1e-6)
    np.testing.assert_array_equal(used, ref[1])
    for p in range(P):
        np.testing.assert_array_equal(idx[p], ref[2][p])


@pytest.mark.parametrize("K", [16, 600])
def test_de2000_nonfinite_palette(gpu, filt, K):
    """A palette with NaN and inf colours takes the generic path by itself: the
    same indices, used flags and cost (NaN where a NaN colour is chosen, else
    equal to 1e-6) as with the exhaustive generic path forced."""
    w, h = 96, 64
    R, G, B = o.synthetic_image(w, h, seed=3)
    rgba = o.inline_rgba(R, G, B)
    pal = o.synthetic_palette(K, 5).copy()
    pal[3, 1] = np.nan
    pal[7, 0] = np.inf
    if K > 256:
        pal[256, 2] = np.nan
    good = o.synthetic_palette(K, 6)
    pals = np.stack([pal, good])
    m = _ctx(gpu, rgba, None, w, filt.illum)
    costs, used = m.computeQuantizationErrorPopulation(pals.reshape(2, -1), 2.0, return_used=True)
    idx = [m.getIndices32(p) for p in range(2)]
    ref = _exhaustive(m, pals, 2)
    m.close()
    ref_idx, _ = c_oracle.assign(rgba, pal)
    np.testing.assert_array_equal(idx[0], ref_idx.astype(np.uint32))
    np.testing.assert_array_equal(used, ref[1])
    for p in range(2):
        np.testing.assert_array_equal(idx[p], ref[2][p])
    assert np.isfinite(costs[1])
    assert np.isnan(costs[0]) == np.isnan(ref[0][0])
    np.testing.assert_allclose(costs, ref[0], rtol=1e-6, equal_nan=True)


def test_de2000_population_equals_single_evaluations(gpu, filt):
    """P = 5 in one launch equals five single evaluations bit for bit (the
    fixed-point sum is order-free)."""
    w, h, K, P = 97, 53, 64, 5
    R, G, B = o.synthetic_image(w, h, seed=12)
    m = _ctx(gpu, o.inline_rgba(R, G, B), None, w, filt.illum)
    pals = np.stack([o.synthetic_palette(K, 40 + p) for p in range(P)]).reshape(P, -1)
    costs, used = m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
    for p in range(P):
        c1, u1 = m.computeQuantizationErrorPopulation(pals[p:p + 1], 2.0, return_used=True)
        assert c1[0] == costs[p]
        np.testing.assert_array_equal(u1[0], used[p])
    m.close()


@pytest.mark.parametrize("cost_variant", [0, 2])
def test_de2000_row_block_shards_sum_to_full(gpu, filt, cost_variant):
    """97 x 53 split at an odd row (27): the two shards' hq_eval_population_partial
    sums add up to the full image's within 1e-9 relative, the used flags to the
    same set.

    The per-pixel generic pair (cost_variant 2, the reference's summation
    order) does not depend on where a tile starts.  The default tiled path
    (cost_variant 0, cost16w) does: a pixel at another row of its tile has its
    taps at other K slots of the split-f16 matrix-core products.  So a
    CIEDE2000 shard's 16-row tiles sit on the full image's tile grid, with the
    rows above the shard's first row masked: row 27's
    shard starts its tiles at row 16.  With tiles from the shard's first row
    the sums were -8.5e-9 and 1.8e-9 relative from the full image's."""
    w, h, K, P = 97, 53, 32, 2
    R, G, B = o.synthetic_image(w, h, seed=4)
    rgba = o.inline_rgba(R, G, B)
    pals = np.stack([o.synthetic_palette(K, 60 + p) for p in range(P)]).reshape(P, -1)
    lib = hq.load()

    def partial(r0, r1):
        m = pr.Context(DE00, device=gpu)
        hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
        m.setOption("cost_variant", cost_variant)
        m.setImage(rgba.reshape(-1), None, w, filt.illum, row_begin=r0, row_end=r1)
        out = np.zeros(P * (1 + K))
        hq._lib.check(lib.hq_eval_population_partial(m.ctx, hq._lib.fptr(pals), P, K, hq._lib.dptr(out)), m.ctx)
        m.close()
        return out.reshape(P, 1 + K)

    full = partial(0, h)
    acc = partial(0, 27) + partial(27, h)
    print(f"cost_variant {cost_variant}: (shards - full) / full = {((acc[:, 0] - full[:, 0]) / full[:, 0]).tolist()}")
    assert np.isfinite(full).all()
    np.testing.assert_array_equal(acc[:, 1:] > 0, full[:, 1:] > 0)
    np.testing.assert_allclose(acc[:, 0], full[:, 0], rtol=1e-9)


def test_de2000_palette_split_slices_sum_to_full(gpu, filt):
    """The palette split's slices without a communicator (test options
    slice_ranks / slice_rank, as test_palette_slices_sum_to_full): the two
    ranks' slices of P = 4 together give the full evaluation's sums bit for bit."""
    w, h, K, P = 97, 53, 32, 4
    R, G, B = o.synthetic_image(w, h, seed=14)
    pals = np.stack([o.synthetic_palette(K, 70 + p) for p in range(P)]).reshape(P, -1)
    lib = hq.load()
    m = _ctx(gpu, o.inline_rgba(R, G, B), None, w, filt.illum)

    def partial():
        out = np.zeros(P * (1 + K))
        hq._lib.check(lib.hq_eval_population_partial(m.ctx, hq._lib.fptr(pals), P, K, hq._lib.dptr(out)), m.ctx)
        return out.reshape(P, 1 + K)

    full = partial()
    m.setOption("slice_ranks", 2)
    acc = np.zeros_like(full)
    for r in range(2):
        m.setOption("slice_rank", r)
        acc += partial()
    m.close()
    np.testing.assert_array_equal(acc, full)


# ---------------------------------------------------------------------------
# 5. Search
# ---------------------------------------------------------------------------
def _search(m, lib, P, K, imax, seed, chunks):
    sw = hq.SWASA(population=P, imax=imax, seed=seed, t0=0.05)
    params = sw.params()
    handle = C.c_void_p()
    hq._lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(handle)), m.ctx)
    traj = []
    best = np.zeros(4 * K, np.float32)
    err, it, ran = C.c_double(), C.c_int(), C.c_int()
    for chunk in chunks:
        hq._lib.check(lib.hq_search_run(handle, chunk, C.byref(ran)), m.ctx)
        hq._lib.check(lib.hq_search_best(handle, hq._lib.fptr(best), C.byref(err), C.byref(it)), m.ctx)
        traj.append((best.copy(), err.value, it.value, ran.value))
    pr.check_search(m, handle, P, K, ran=True)  # device-resident exactly when sa_device is 1
    lib.hq_search_destroy(handle)
    return traj


def test_de2000_device_search_matches_host_driven(gpu, filt):
    """64 x 48, K = 16, P = 4, imax 60: the device-resident loop and the
    host-driven one (sa_device 0) give the same best palette, best error and
    iteration after every run() call (1 iteration at a time at first, then to
    imax), and the best error is hq_eval_population's cost of the best palette."""
    g, R, G, B = load_case("case_64x48_k16")
    w = int(g["w"])
    m = _ctx(gpu, o.inline_rgba(R, G, B), None, w, filt.illum)
    lib = hq.load()
    res = {}
    for dev in (0, 1):
        m.setOption("sa_device", dev)
        res[dev] = _search(m, lib, 4, 16, 60, 21, (1, 1, 1, 1, 1, 1, 14, 20, 30))
    for a, b in zip(res[0], res[1]):
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
        np.testing.assert_array_equal(a[0], b[0])
    best, err, it, _ = res[1][-1]
    assert it == 60 and np.isfinite(err) and err > 0
    assert len({t[1] for t in res[1]}) > 1  # the best improved along the way
    cost = m.computeQuantizationErrorPopulation([best], 2.0)[0]
    m.close()
    assert cost == err


def test_cie94_search_still_as_before(gpu, filt):
    """Guards the three-way dispatch from the dE94 side: a CIE94 search on the
    same image ends NaN or not exactly as its population evaluation says (the
    reference's unclamped dH, CL:222), host-driven and device-resident alike,
    and never with CIEDE2000's values."""
    g, R, G, B = load_case("case_64x48_k16")
    w = int(g["w"])
    rgba = o.inline_rgba(R, G, B)
    lib = hq.load()
    m = _ctx(gpu, rgba, None, w, filt.illum, de=hq.deltaETypes.CIE94)
    res = {}
    for dev in (0, 1):
        m.setOption("sa_device", dev)
        res[dev] = _search(m, lib, 4, 16, 60, 21, (20, 40))[-1]
    assert res[0][1] == res[1][1] or (np.isnan(res[0][1]) and np.isnan(res[1][1]))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    best, err = res[1][0], res[1][1]
    m.setOption("pixel_err", 1)
    cost = m.computeQuantizationErrorPopulation([best], 2.0)[0]
    nan_px = bool(np.isnan(m.getPixelErrors(0)).any())
    m.close()
    # the oracle's fp32 dE94 of the golden palettes: which of them have a NaN pixel is dE94's own business
    assert np.isnan(cost) == nan_px
    if not np.isnan(err):
        assert cost == err
    m2 = _ctx(gpu, rgba, None, w, filt.illum)
    c2 = m2.computeQuantizationErrorPopulation([best], 2.0)[0]
    m2.close()
    assert np.isfinite(c2) and c2 != cost


# ---------------------------------------------------------------------------
# 6. Dispatch guard
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_three_de_types_give_three_costs(gpu, variant):
    """Same image and palettes, three contexts: three different costs, CIE76's
    the golden fixture's (1e-6) -- a dispatch that routed type 2 into an
    existing kernel would repeat one of the others."""
    g, R, G, B = load_case("case_97x53_k64")
    w = int(g["w"])
    rgba = o.inline_rgba(R, G, B)
    pals = g["palettes"]
    P = len(pals)
    costs = {}
    for de in (hq.deltaETypes.CIE76, hq.deltaETypes.CIE94, DE00):
        m = _ctx(gpu, rgba, g["lab"], w, o.design_filters().illum, de=de, cost_variant=variant, pixel_err=1)
        costs[de] = m.computeQuantizationErrorPopulation(pals.reshape(P, -1), 2.0)
        if de == hq.deltaETypes.CIE94:  # its cost may be NaN (CL:222): compare the finite pixels' mean instead
            e94 = np.stack([m.getPixelErrors(p) for p in range(P)])
        m.close()
    np.testing.assert_allclose(costs[hq.deltaETypes.CIE76], g["costs"], rtol=1e-6)
    c76, c00 = costs[hq.deltaETypes.CIE76], costs[DE00]
    assert np.isfinite(c00).all()
    pen = 2.0 * (g["used"] == 0).sum(1)
    m94 = np.array([np.nanmean(e94[p].astype(np.float64)) for p in range(P)]) + pen
    print("dE76", c76, "dE94 (finite pixels)", m94, "dE2000", c00)
    for x, y in ((c76, c00), (m94, c00), (c76, m94)):
        assert np.all(np.abs(x - y) > 1e-2 * np.abs(x))

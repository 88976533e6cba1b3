"""Option "assign_space" on the GPU: CIELAB nearest-colour assignment on every argmin path.

Under value 1 the argmin kernels rank by the coordinates (L, a + 128, b + 128) / 256 of the
pixels and of the palette colours (tests/assign_space_ref.py states them).  What is held here:

 1. hq_assign_coords against float64, at row a4's bar relative to the fp32 restatement;
 2. the argmin is the existing argmin, bit for bit: a plain context whose image is the first
    one's coordinates and whose palettes are the first one's palettes' coordinates gives the
    same indices and used flags, over K, P, the grid resolutions and both image forms;
 3. the cost and every pixel's dE are the stencil cost of that index image (the oracle's
    candidate_scielab on the indices, not its own argmin), at test_gpu.py's bars;
 4. identity: an image made of the palette's colours, and value 0 after value 1;
 5. pointwise minimality under a one-tap filter;
 6. device-resident, captured and host-driven searches agree;
 7. state: the image, the illuminant, shards, a reduced image, a search's latch;
 8. the refusals.

Images: 97 x 53 noise and 96 x 64 blobs.
"""

import ctypes as C

import numpy as np
import pytest

import assign_space_ref as ar
import c_oracle
import de2000_ref as d00
import hybridquantization_amd as hq
import illuminant_ref as ir
import oracle as o
from hybridquantization_amd import _lib
from test_de2000_gpu import EXCL_DEG, FP32_ABS, _cols
from test_gpu import _threads, exact_pixel_err
from test_lloyd_gpu import blob_image

pytestmark = pytest.mark.gpu

DE76, DE00 = hq.deltaETypes.CIE76, hq.deltaETypes.CIEDE2000
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = _lib.HQ_OK, _lib.HQ_ERR_ARG, _lib.HQ_ERR_STATE, _lib.HQ_ERR_UNSUPPORTED
NW, NH = 97, 53
BW, BH = 96, 64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dbits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def new_ctx(gpu, de=DE76, dpi=72, vd=45.0, **opts):
    m = hq.ImageManipulation(de, device=gpu)
    sp = hq.ScielabProcessor(dpi, vd, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    for k, v in opts.items():
        m.setOption(k, v)
    return m


@pytest.fixture()
def ctxs(gpu):
    made = []

    def make(*a, **kw):
        made.append(new_ctx(gpu, *a, **kw))
        return made[-1]

    yield make
    for m in made:
        m.close()


_ONCE = {}


def once(key, make):
    if key not in _ONCE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ONCE[key] = v
    return _ONCE[key]


def noise(form="u8"):
    """The 97 x 53 noise image, inline RGBA: "u8" on the k/255 lattice (the packed form),
    "planar" the same pixels moved off it by less than half a step (the planar form)."""
    def make():
        rgba = o.inline_rgba(*o.synthetic_image(NW, NH, seed=7))
        if form == "planar":
            off = np.random.default_rng(3).random((NW * NH, 3), dtype=np.float32) * np.float32(1.5e-3)
            rgba[:, :3] = np.clip(rgba[:, :3] + off, 0.0, 1.0)
        return rgba
    return once(("noise", form), make)


def blobs():
    return once("blobs", lambda: blob_image(BW, BH, seed=11)[0])


def pals_of(P, K, seed):
    return np.stack([o.synthetic_palette(K, seed + p).reshape(-1) for p in range(P)]).astype(np.float32)


def indices(m, p, K):
    return m.getIndices(p).astype(np.uint32) if K <= 256 else m.getIndices32(p)


def evaluated(m, pals, err=False):
    P, K = pals.shape[0], pals.shape[1] // 4
    costs, used = m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
    return dict(costs=costs, used=used, idx=[indices(m, p, K) for p in range(P)],
                err=[m.getPixelErrors(p) for p in range(P)] if err else [])


def assert_same(a, b, msg=""):
    np.testing.assert_array_equal(dbits(a["costs"]), dbits(b["costs"]), err_msg=f"{msg}: costs")
    np.testing.assert_array_equal(a["used"], b["used"], err_msg=f"{msg}: used flags")
    for x, y in zip(a["idx"], b["idx"]):
        np.testing.assert_array_equal(x, y, err_msg=f"{msg}: indices")
    assert len(a["err"]) == len(b["err"])
    for x, y in zip(a["err"], b["err"]):
        np.testing.assert_array_equal(bits(x), bits(y), err_msg=f"{msg}: per-pixel dE")


# ---------------------------------------------------------------------------
# 1. Coordinates against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["D65", "D50", "dimD65"])
def test_coordinates_against_float64(ctxs, name):
    """hq_assign_coords on the 8 cube corners, a 17^3 lattice and 4096 random colours under D65,
    D50 and dimD65 (Yn = 0.8): the distance from the float64 coordinates at most 2x the fp32
    restatement's worst and 1.5x its mean (row a4's bar), in units of dE76.  Space "rgb" copies."""
    m = ctxs()
    il = ir.ills()[name]
    m.setImage(np.zeros(4 * 16 * 16, np.float32), None, 16, il)  # (the illuminant is the image's)
    for key, cols in ar.colour_sets().items():
        got = m.assignCoords(cols, "lab")
        assert got.shape == cols.shape and not got[:, 3].any()
        ex = ar.coords_f64(cols, il)
        d_dev, d_ref = ar.dist(got[:, :3], ex) * 256.0, ar.dist(ar.coords_f32(cols, il), ex) * 256.0
        stats = (f"{name} {key}: |gpu-float64| max {d_dev.max():.3g} mean {d_dev.mean():.3g}; "
                 f"|fp32-float64| max {d_ref.max():.3g} mean {d_ref.mean():.3g}")
        print(stats)
        assert d_dev.max() <= 2 * d_ref.max(), stats
        assert d_dev.mean() <= 1.5 * d_ref.mean(), stats
        same = m.assignCoords(cols, "rgb")
        np.testing.assert_array_equal(bits(same[:, :3]), bits(cols[:, :3]))
        assert not same[:, 3].any()
    if name != "D65":  # not D65's coordinates under another name
        lat = ar.colour_sets()["lattice17"]
        assert np.abs(m.assignCoords(lat)[:, :3] - ar.coords_f32(lat, ir.ills()["D65"])).max() > 1e-3


# ---------------------------------------------------------------------------
# 2. The argmin is the existing argmin, bit for bit
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(gpu):
    """form -> (the context under assign_space 1 holding the noise image in that form, a plain
    context whose image is the first one's coordinates), made once."""
    made = {}
    for form in ("u8", "planar"):
        a, b = new_ctx(gpu, assign_space=1), new_ctx(gpu)
        rgba = noise(form)
        a.setImage(rgba.reshape(-1), None, NW, a.illum)
        b.setImage(a.assignCoords(rgba).reshape(-1), None, NW, b.illum)
        made[form] = (a, b)
    yield made
    for a, b in made.values():
        a.close()
        b.close()


def with_duplicates(pals):
    """Exact duplicate colours in palette 0: colour 3 again at 7 and at the last index, colour 0 at 5."""
    pals = pals.copy()
    c = pals[0].reshape(-1, 4)
    c[7], c[-1], c[5] = c[3], c[3], c[0]
    return pals


ARGMIN_CASES = [(16, 2, 32), (16, 5, 0), (16, 2, 16), (16, 5, 64), (256, 5, 32), (256, 2, 0), (256, 2, 16),
                (256, 2, 64), (300, 2, 32), (300, 5, 32), (1100, 2, 32), (1100, 5, 32)]


@pytest.mark.parametrize("form", ["u8", "planar"])
@pytest.mark.parametrize("K,P,grid", ARGMIN_CASES)
def test_argmin_is_the_existing_argmin(pair, form, K, P, grid):
    """K 16 and 256 (grid + assign), 300 (per-chunk grids), 1100 (the native 16-bit lists); the
    pruned argmin under value 1 also equals the exhaustive one (grid 0) at K <= 256.  The cross
    K x P x grid is sampled, not run in full: every value of K, P and grid occurs and both image
    forms run every case, but not every combination (K = 256 meets grid 0, 16 and 64 at P = 2 only)."""
    a, b = pair[form]
    pals = with_duplicates(pals_of(P, K, 40 + K))
    coords = np.stack([a.assignCoords(p.reshape(-1, 4)).reshape(-1) for p in pals])
    a.setOption("grid", grid)
    b.setOption("grid", grid)
    ea, eb = evaluated(a, pals), evaluated(b, coords)
    path = a.lastPath()
    assert path["pixels"] == "planar" and b.lastPath()["pixels"] == "planar"
    assert path["grid"] == ("none" if grid == 0 else "lists16" if K == 1100 else "build_grid")
    np.testing.assert_array_equal(ea["used"], eb["used"])
    for p in range(P):
        np.testing.assert_array_equal(ea["idx"][p], eb["idx"][p], err_msg=f"palette {p}")
        assert ea["idx"][p].max() < K
    if K <= 256 and grid != 0:
        a.setOption("grid", 0)
        e0 = evaluated(a, pals)
        for p in range(P):
            np.testing.assert_array_equal(ea["idx"][p], e0["idx"][p], err_msg=f"pruned vs exhaustive, palette {p}")
    # and it is not the sRGB assignment
    rgb_idx, _ = c_oracle.assign(noise(form), pals[1].reshape(-1, 4), nthreads=_threads())
    assert np.count_nonzero(rgb_idx != ea["idx"][1]) > NW * NH // 50


# ---------------------------------------------------------------------------
# 3. Cost for that index image
# ---------------------------------------------------------------------------
def cost_refs(geo, K):
    """Filters, LabRef and palette of a cost case (CPU), shared by its dE types."""
    def make():
        dpi, vd = {"7245": (72, 45.0), "30050": (300, 50.0)}[geo]
        f = o.design_filters(dpi, vd)
        rgba = noise("u8")
        lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, NW, nthreads=_threads())
        return dpi, vd, f, lab, pals_of(1, K, 70 + K)
    return once(("cost", geo, K), make)


@pytest.mark.parametrize("de", [DE76, DE00], ids=["de76", "de2000"])
@pytest.mark.parametrize("geo", ["7245", "30050"])
@pytest.mark.parametrize("K", [16, 300])
def test_cost_is_that_of_the_index_image(ctxs, K, geo, de):
    """The indices are test 2's matter; here the cost and every pixel's dE are the stencil cost of
    those indices: dE76 within 2e-4 of the oracle's error image, at most 2x the oracle's worst
    distance from float64 and 1.5x its mean, the cost within 1e-6 (1e-5 on the long filter) of
    the oracle's; CIEDE2000 at test_de2000_gpu's bars against float64."""
    dpi, vd, f, lab, pals = cost_refs(geo, K)
    m = ctxs(de, dpi, vd, assign_space=1, pixel_err=1)
    m.setImage(noise("u8").reshape(-1), lab.reshape(-1), NW, m.illum)
    e = evaluated(m, pals, err=True)
    idx, pal, err = e["idx"][0].astype(np.int64), pals[0].reshape(-1, 4), e["err"][0]
    cand32 = o.candidate_scielab(idx, pal, f, NW, NH)
    used = np.bincount(idx, minlength=K)[:K] > 0
    np.testing.assert_array_equal(e["used"][0], used.astype(np.int32))
    penalty = 2.0 * float(np.count_nonzero(~used))
    if de == DE76:
        e_orc = o.ciede76(lab, cand32)
        ex = exact_pixel_err(idx, pal, lab, f, NW, NH)
        d_gpu, d_orc = np.abs(err - ex), np.abs(e_orc - ex)
        stats = (f"K={K} {geo} dE76: |gpu-exact| max {d_gpu.max():.3g} mean {d_gpu.mean():.3g}; "
                 f"|oracle-exact| max {d_orc.max():.3g} mean {d_orc.mean():.3g}")
        print(stats)
        np.testing.assert_allclose(err, e_orc, rtol=0, atol=2e-4, err_msg=stats)
        assert d_gpu.max() <= 2 * d_orc.max(), stats
        assert d_gpu.mean() <= 1.5 * d_orc.mean(), stats
        want = o.average_array(e_orc) + penalty
        assert abs(e["costs"][0] - want) <= (1e-6 if geo == "7245" else 1e-5) * want, (e["costs"][0], want)
        return
    ref64 = _cols(lab[:, :3].astype(np.float64))
    cand64 = exact_pixel_err(idx, pal, lab, f, NW, NH, lab_only=True)
    ex = d00.ciede2000(*ref64, *_cols(cand64))
    ex_other = d00.ciede2000(*ref64, *_cols(cand64), other_branch=True)
    excl = np.abs(d00.hue_gap_deg(*ref64, *_cols(cand64)) - 180.0) < EXCL_DEG
    yard = d00.ciede2000(*_cols(lab[:, :3]), *_cols(cand32.reshape(-1, 4)[:, :3].astype(np.float32)),
                         dtype=np.float32).astype(np.float64)

    def dist(v):
        dd = np.abs(v - ex)
        return np.where(excl, np.minimum(dd, np.abs(v - ex_other)), dd)

    keep = ~excl
    d_gpu, d_yard = dist(err.astype(np.float64)), dist(yard)
    stats = (f"K={K} {geo} dE2000: set aside {int(excl.sum())}; |gpu-f64| max {d_gpu[keep].max():.3g} mean "
             f"{d_gpu[keep].mean():.3g}; |fp32-f64| max {d_yard[keep].max():.3g} mean {d_yard[keep].mean():.3g}")
    print(stats)
    bar = 2 * d_yard[keep].max() + FP32_ABS
    assert np.isfinite(err).all()
    assert d_gpu.max() <= bar, stats
    assert d_gpu[keep].mean() <= 1.5 * d_yard[keep].mean() + FP32_ABS, stats
    near_other = excl & (np.abs(err - ex_other) < np.abs(err - ex))
    want = float(np.where(near_other, ex_other, ex).mean()) + penalty
    assert abs(e["costs"][0] - want) <= 1e-5 * want, stats


# ---------------------------------------------------------------------------
# 4. Identity
# ---------------------------------------------------------------------------
def test_an_image_of_the_palettes_colours(ctxs):
    """Every pixel is exactly one of the palette's 8 distinct colours: its nearest colour is
    itself in either space, so value 1 gives value 0's indices, used flags, per-pixel dE and
    cost, bit for bit."""
    rng = np.random.default_rng(5)
    by = rng.integers(0, 256, (8, 3))
    pal = np.zeros((8, 4), np.float32)
    pal[:, :3] = by.astype(np.float32) / np.float32(255)
    assert len({tuple(c) for c in by}) == 8
    rgba = pal[rng.integers(0, 8, NW * NH)]
    out = []
    for v in (0, 1):
        m = ctxs(assign_space=v, pixel_err=1)
        m.setImage(rgba.reshape(-1), None, NW, m.illum)
        out.append(evaluated(m, pal.reshape(1, -1), err=True))
    assert_same(out[1], out[0], "assign_space 1 vs 0")
    assert out[0]["used"].all()


@pytest.mark.parametrize("K", [16, 300])
def test_value_0_after_value_1_is_a_fresh_context(ctxs, K):
    pals = pals_of(3, K, 11)
    fresh = ctxs(pixel_err=1)
    fresh.setImage(noise().reshape(-1), None, NW, fresh.illum)
    want = evaluated(fresh, pals, err=True)
    m = ctxs(pixel_err=1, assign_space=1)
    m.setImage(noise().reshape(-1), None, NW, m.illum)
    lab = evaluated(m, pals, err=True)
    assert any(np.any(x != y) for x, y in zip(lab["idx"], want["idx"]))
    m.setOption("assign_space", 0)
    got = evaluated(m, pals, err=True)
    assert_same(got, want, "value 0 after value 1")
    if K <= 256:
        assert m.lastPath()["pixels"] == "u8"
    m.setOption("assign_space", 1)
    assert_same(evaluated(m, pals, err=True), lab, "value 1 again")


def test_illuminant_a_pixels_outside_the_cube(ctxs):
    """Under illuminant A saturated blues have b < -128, a coordinate below 0: those pixels take the
    argmin's exact loop for pixels outside the cube.  Indices against the float64 nearest colour in
    CIELAB, wherever the runner-up is not within 1e-3 dE76 of it."""
    il = ir.ills()["A"]
    rgba = noise("u8").copy()
    rgba[3::11, :3] = np.array([20, 10, 245], np.float32) / np.float32(255)
    rgba[::7, :3] = [0.0, 0.0, 1.0]
    pal = pals_of(1, 16, 61)
    c = pal[0].reshape(-1, 4)
    c[5, :3] = [0.0, 0.0, 1.0]
    c[9, :3] = np.array([0, 0, 230], np.float32) / np.float32(255)
    q = ar.coords_f64(rgba, il)
    outside = q.min(1) < 0.0
    assert outside.sum() > 500 and ar.coords_f64(c, il).min() < 0.0
    lp, lc = ar.lab_f64(rgba, il), ar.lab_f64(c, il)
    dd = np.sqrt(((lp[:, None, :] - lc[None, :, :]) ** 2).sum(-1))
    order = np.sort(dd, axis=1)
    clear = order[:, 1] - order[:, 0] > 1e-3
    want = dd.argmin(1)
    for grid in (32, 0):
        m = ctxs(assign_space=1, grid=grid)
        m.setImage(rgba.reshape(-1), None, NW, il)
        idx = evaluated(m, pal)["idx"][0]
        assert clear.mean() > 0.99
        np.testing.assert_array_equal(idx[clear], want[clear], err_msg=f"grid {grid}")
        assert (idx[::7] == 5).all()
        assert np.count_nonzero(outside & clear) > 500


# ---------------------------------------------------------------------------
# 5. Pointwise minimality
# ---------------------------------------------------------------------------
ONE_TAP = ([[[1.0], [0.0], [0.0]], [[1.0], [0.0]], [[1.0], [0.0]]], [0.0])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pointwise_minimality_under_a_one_tap_filter(gpu, seed):
    """One tap of weight 1 on all three channels, dE76: a pixel's dE is then the dE76 between
    its own Lab and its colour's, so the colour nearest in CIELAB minimises it pointwise.
    tau: twice the largest distance from float64 the value 0 evaluation of the same case shows
    (two candidates each carry that error)."""
    K = 16
    rgba = noise("u8")
    pal = pals_of(1, K, 500 + seed)
    il = o.D65
    out = {}
    for v in (0, 1):
        m = hq.ImageManipulation(DE76, device=gpu)
        try:
            m.updateOpenCLFilters(*ONE_TAP)
            m.setOption("pixel_err", 1)
            m.setOption("assign_space", v)
            m.setImage(rgba.reshape(-1), None, NW, il)
            out[v] = evaluated(m, pal, err=True)
        finally:
            m.close()
    lp, lc = ar.lab_f64(rgba, il), ar.lab_f64(pal.reshape(-1, 4), il)
    e0, e1 = out[0]["err"][0].astype(np.float64), out[1]["err"][0].astype(np.float64)
    ex0 = ar.dist(lp, lc[out[0]["idx"][0].astype(np.int64)])
    tau = 2.0 * float(np.abs(e0 - ex0).max())
    best, _ = ar.nearest_lab_de76(rgba, pal.reshape(-1, 4), il)
    print(f"palette {seed}: tau {tau:.3g}; max(e1 - e0) {float((e1 - e0).max()):.3g}; max(e1 - min) "
          f"{float((e1 - best).max()):.3g}; cost {out[1]['costs'][0]:.6f} vs {out[0]['costs'][0]:.6f}; "
          f"{int(np.count_nonzero(out[0]['idx'][0] != out[1]['idx'][0]))} pixels reassigned")
    assert tau < 1e-2
    assert np.all(e1 <= e0 + tau)
    assert np.all(e1 <= best + tau)
    assert out[1]["costs"][0] <= out[0]["costs"][0]
    assert np.count_nonzero(out[0]["idx"][0] != out[1]["idx"][0]) > 50


# ---------------------------------------------------------------------------
# 6. The searches agree
# ---------------------------------------------------------------------------
class Search:
    """hq_search_* through ctypes."""

    def __init__(self, m, K, P, seed=17, imax=40):
        self.m, self.K, self.P, self.lib = m, K, P, hq.load()
        self.sw = hq.SWASA(population=P, imax=imax, seed=seed, t0=0.05)
        params = self.sw.params()
        self.h = C.c_void_p()
        _lib.check(self.lib.hq_search_create(m.ctx, C.byref(params), K, self.sw.seed, C.byref(self.h)), m.ctx)

    def run(self, n):
        ran = C.c_int(-5)
        rc = self.lib.hq_search_run(self.h, n, C.byref(ran))
        return rc, ran.value

    def best(self):
        best = np.zeros(4 * self.K, np.float32)
        err, it = C.c_double(), C.c_int()
        _lib.check(self.lib.hq_search_best(self.h, _lib.fptr(best), C.byref(err), C.byref(it)), self.m.ctx)
        return best, err.value, it.value

    def close(self):
        self.lib.hq_search_destroy(self.h)


def searched(m, K, P, runs=(20,), lloyd=0, repair=0, resident=None):
    s = Search(m, K, P)
    try:
        if resident is not None:
            assert m.searchInfo(s.h)["device_resident"] == resident
        if lloyd:
            _lib.check(s.lib.hq_search_set_lloyd(s.h, lloyd), m.ctx)
        if repair:
            _lib.check(s.lib.hq_search_set_repair(s.h, repair, -1), m.ctx)
        for n in runs:
            assert s.run(n) == (OK, n), m._lib.hq_last_error(m.ctx)
        return s.best()
    finally:
        s.close()


def assert_same_best(a, b, msg):
    np.testing.assert_array_equal(bits(a[0]), bits(b[0]), err_msg=f"{msg}: best colours")
    assert dbits(a[1]) == dbits(b[1]) and a[2] == b[2], (msg, a[1:], b[1:])


SEARCH_CASES = {"k16": (16, {}, 0), "k600": (600, {}, 0), "k16_lloyd2": (16, dict(lloyd=2), 0),
                "k16_repair3": (16, dict(repair=3), 0), "k16_fixed2": (16, {}, 2)}


@pytest.mark.parametrize("case", SEARCH_CASES)
def test_the_searches_agree(ctxs, case):
    """20 iterations of P = 3 under value 1: device-resident, captured (sa_graph 1) and
    host-driven (sa_device 0) give the same best colours, error and iteration, bit for bit; 7 + 13
    iterations equal 20; the best error is hq_eval_population's of the best colours within 1e-6."""
    K, moves, nfixed = SEARCH_CASES[case]
    P = 3
    got = {}
    for mode, opts in (("device", {}), ("graph", dict(sa_graph=1)), ("host", dict(sa_device=0))):
        m = ctxs(assign_space=1, **opts)
        m.setImage(blobs().reshape(-1), None, BW, m.illum)
        if nfixed:
            m.setFixedColors([[0, 0, 0], [1, 0, 1]][:nfixed])
        got[mode] = searched(m, K, P, resident=mode != "host", **moves)
        if mode == "device":
            got["split"] = searched(m, K, P, runs=(7, 13), **moves)
            cost = m.computeQuantizationErrorPopulation(got[mode][0].reshape(1, -1), 2.0)[0]
            assert abs(cost - got[mode][1]) <= 1e-6 * cost, (cost, got[mode][1])
            assert m.lastPath()["pixels"] == "planar"
    for mode in ("graph", "host", "split"):
        assert_same_best(got[mode], got["device"], f"{case}: {mode} vs device-resident")
    assert got["device"][2] == 20 and np.isfinite(got["device"][1])
    if nfixed:
        np.testing.assert_array_equal(got["device"][0].reshape(-1, 4)[:2, :3], [[0, 0, 0], [1, 0, 1]])
    # and the search under value 0 is another search
    m0 = ctxs()
    m0.setImage(blobs().reshape(-1), None, BW, m0.illum)
    if nfixed:
        m0.setFixedColors([[0, 0, 0], [1, 0, 1]][:nfixed])
    assert dbits(searched(m0, K, P, **moves)[1]) != dbits(got["device"][1])


def test_the_host_callback_search_agrees(ctxs):
    """hq_swasa_search_host with the context's evaluation as its callback equals the host-driven
    hq_search_* under value 1."""
    K, P = 16, 3
    m = ctxs(assign_space=1, sa_device=0)
    m.setImage(blobs().reshape(-1), None, BW, m.illum)
    want = searched(m, K, P, resident=False)
    sw = hq.SWASA(population=P, imax=40, seed=17, t0=0.05)
    best, err, _ = sw.search_host(K, lambda ps: m.computeQuantizationErrorPopulation(ps.reshape(P, -1), sw.delta),
                                  iterations=20)
    np.testing.assert_array_equal(bits(best), bits(want[0]))
    assert dbits(err) == dbits(want[1])


# ---------------------------------------------------------------------------
# 7. State
# ---------------------------------------------------------------------------
def test_option_before_and_after_the_image(ctxs):
    pals = pals_of(2, 16, 21)
    a = ctxs(assign_space=1, pixel_err=1)
    a.setImage(noise().reshape(-1), None, NW, a.illum)
    b = ctxs(pixel_err=1)
    b.setImage(noise().reshape(-1), None, NW, b.illum)
    b.setOption("assign_space", 1)
    assert_same(evaluated(a, pals, err=True), evaluated(b, pals, err=True), "option before vs after hq_set_image")


def test_a_new_image_or_illuminant_rebuilds_the_coordinates(ctxs):
    pals = pals_of(2, 16, 22)
    d50 = ir.ills()["D50"]
    steps = [(noise("u8"), NW, None), (blobs(), BW, None), (blobs(), BW, d50), (noise("planar"), NW, d50)]
    live = ctxs(assign_space=1, pixel_err=1)
    seen = []
    for rgba, w, il in steps:
        il = live.illum if il is None else il
        live.setImage(rgba.reshape(-1), None, w, il)
        got = evaluated(live, pals, err=True)
        fresh = ctxs(assign_space=1, pixel_err=1)
        fresh.setImage(rgba.reshape(-1), None, w, il)
        assert_same(got, evaluated(fresh, pals, err=True), f"step {len(seen)}")
        seen.append(got)
    # the illuminant alone moved the assignment (same image, D65 -> D50)
    assert any(np.any(x != y) for x, y in zip(seen[1]["idx"], seen[2]["idx"]))


def test_the_coordinates_are_made_once_per_image(ctxs):
    """The "coords" stage counts the coordinate kernel: none under value 0, one for any number of
    evaluations of an image under value 1, one more after a new image."""
    lib = hq.load()
    pals = pals_of(2, 16, 25)

    def launches(m):
        ms, n = C.c_double(), C.c_int64()
        _lib.check(lib.hq_profile_get(m.ctx, b"coords", C.byref(ms), C.byref(n)), m.ctx)
        return n.value

    m = ctxs()
    lib.hq_profile_enable(m.ctx, 1)
    m.setImage(noise().reshape(-1), None, NW, m.illum)
    evaluated(m, pals)
    assert launches(m) == 0
    m.setOption("assign_space", 1)
    want = evaluated(m, pals)
    evaluated(m, pals)
    assert launches(m) == 1
    m.setOption("assign_space", 0)
    evaluated(m, pals)
    m.setOption("assign_space", 1)
    assert_same(evaluated(m, pals), want, "the coordinates outlive value 0")
    assert launches(m) == 1
    m.setImage(blobs().reshape(-1), None, BW, m.illum)
    evaluated(m, pals)
    assert launches(m) == 2


@pytest.mark.parametrize("K", [16, 300])
def test_two_row_block_shards_add_up(ctxs, K):
    pals = pals_of(2, K, 23)
    P = 2
    whole = ctxs(assign_space=1)
    whole.setImage(noise().reshape(-1), None, NW, whole.illum)
    full = whole._populationCall(whole._lib.hq_eval_population_partial, pals, ())
    full_idx = [indices(whole, p, K) for p in range(P)]
    parts = []
    for r0, r1 in ((0, 27), (27, NH)):
        sh = ctxs(assign_space=1)
        sh.setImage(noise().reshape(-1), None, NW, sh.illum, row_begin=r0, row_end=r1)
        parts.append(sh._populationCall(sh._lib.hq_eval_population_partial, pals, ()))
        for p in range(P):
            np.testing.assert_array_equal(indices(sh, p, K)[:NW * (r1 - r0)], full_idx[p][NW * r0:NW * r1])
    np.testing.assert_allclose(parts[0][:, 0] + parts[1][:, 0], full[:, 0], rtol=1e-6)
    np.testing.assert_array_equal((parts[0][:, 1:] != 0) | (parts[1][:, 1:] != 0), full[:, 1:] != 0)


def test_a_reduced_image(ctxs):
    """hq_set_image_reduced (f = 2) under value 1 equals a context given the reduced image."""
    pals = pals_of(2, 16, 24)
    src = ctxs()
    src.setImage(blobs().reshape(-1), None, BW, src.illum)
    red = ctxs(assign_space=1, pixel_err=1)
    red.setImageReduced(src, 2)
    got = evaluated(red, pals, err=True)
    given = ctxs(assign_space=1, pixel_err=1)
    given.setImage(red.getImage(), None, red.w, given.illum)
    assert_same(got, evaluated(given, pals, err=True), "reduced vs given")
    # and a context that had coordinates of another image before the reduction
    red2 = ctxs(assign_space=1, pixel_err=1)
    red2.setImage(noise().reshape(-1), None, NW, red2.illum)
    evaluated(red2, pals)
    red2.setImageReduced(src, 2)
    assert_same(evaluated(red2, pals, err=True), got, "reduced after another image")


@pytest.mark.parametrize("device", [1, 0])
def test_a_search_latches_the_option(ctxs, device):
    m = ctxs(assign_space=1, sa_device=device)
    m.setImage(blobs().reshape(-1), None, BW, m.illum)
    want = searched(m, 16, 3, runs=(5, 5))
    s = Search(m, 16, 3)
    try:
        assert s.run(5) == (OK, 5)
        before = s.best()
        m.setOption("assign_space", 0)
        rc, ran = s.run(5)
        assert rc == ERR_STATE and ran == 0
        assert b"recreate the search" in m._lib.hq_last_error(m.ctx)
        assert_same_best(s.best(), before, "a refused run")
        m.setOption("assign_space", 1)
        assert s.run(5) == (OK, 5)
        assert_same_best(s.best(), want, "after the option is restored")
    finally:
        s.close()


# ---------------------------------------------------------------------------
# 8. Refusals
# ---------------------------------------------------------------------------
def test_refusals(ctxs):
    """Under value 1 every call that keeps the sRGB rule returns HQ_ERR_UNSUPPORTED with a message
    naming the option, writes no output and leaves the context usable; under value 0 it succeeds."""
    lib = hq.load()
    m = ctxs(assign_space=1, pixel_err=1)
    m.setImage(noise().reshape(-1), None, NW, m.illum)
    P, K = 2, 16
    pals = pals_of(P, K, 31)
    before = evaluated(m, pals, err=True)
    amp = np.full(3, 0.25, np.float32)
    taps = _lib.hq_diffusion_taps()
    _lib.check(lib.hq_diffusion_preset(_lib.DIFFUSION_PRESETS.index("jarvis"), C.byref(taps)))
    fp, dp, ip_ = _lib.fptr, _lib.dptr, _lib.iptr
    ctx = m.ctx

    def outputs():
        return np.full(P, -7.0), np.full((P, K), -7, np.int32), np.full((P, 1 + K), -7.0)

    calls = {
        "hq_dither_population": lambda c, u, r: lib.hq_dither_population(ctx, fp(pals), P, K, 1.0, 2.0, dp(c), ip_(u)),
        "hq_diffuse_population": lambda c, u, r: lib.hq_diffuse_population(ctx, fp(pals), P, K, C.byref(taps), 1.0, 2.0,
                                                                           dp(c), ip_(u)),
        "hq_dot_population": lambda c, u, r: lib.hq_dot_population(ctx, fp(pals), P, K, None, 1.0, 2.0, dp(c), ip_(u)),
        "hq_dot_population_partial": lambda c, u, r: lib.hq_dot_population_partial(ctx, fp(pals), P, K, None, 1.0, dp(r)),
        "hq_ordered_population": lambda c, u, r: lib.hq_ordered_population(ctx, fp(pals), P, K, fp(amp), 2.0, dp(c), ip_(u)),
        "hq_ordered_population_partial": lambda c, u, r: lib.hq_ordered_population_partial(ctx, fp(pals), P, K, fp(amp),
                                                                                           dp(r)),
    }
    for name, call in calls.items():
        c, u, r = outputs()
        assert call(c, u, r) == ERR_UNSUPPORTED, name
        assert b"assign_space" in lib.hq_last_error(ctx), name
        assert (c == -7).all() and (u == -7).all() and (r == -7).all(), name
    # K > 16384: the wide path
    wide = pals_of(1, 16385, 32)
    c = np.full(1, -7.0)
    u = np.full((1, 16385), -7, np.int32)
    assert lib.hq_eval_population(ctx, fp(wide), 1, 16385, 2.0, dp(c), ip_(u)) == ERR_UNSUPPORTED
    assert b"assign_space" in lib.hq_last_error(ctx) and (c == -7).all() and (u == -7).all()
    # K > 256 off the chunked path (enqueue_wide reads colours): grid 0, option chunked 0
    mid = pals_of(1, 300, 34)
    for opt, off, on in (("grid", 0, 32), ("chunked", 0, 1)):
        m.setOption(opt, off)
        c, u = np.full(1, -7.0), np.full((1, 300), -7, np.int32)
        assert lib.hq_eval_population(ctx, fp(mid), 1, 300, 2.0, dp(c), ip_(u)) == ERR_UNSUPPORTED, opt
        assert b"assign_space" in lib.hq_last_error(ctx) and (c == -7).all() and (u == -7).all(), opt
        m.setOption(opt, on)
        assert lib.hq_eval_population(ctx, fp(mid), 1, 300, 2.0, dp(c), ip_(u)) == OK, opt
    # a search: the ordered and the dot-diffused cost
    s = Search(m, K, 3)
    try:
        assert lib.hq_search_set_ordered(s.h, fp(amp)) == ERR_UNSUPPORTED and b"assign_space" in lib.hq_last_error(ctx)
        assert lib.hq_search_set_dot(s.h, None, 1.0) == ERR_UNSUPPORTED and b"assign_space" in lib.hq_last_error(ctx)
        assert s.run(3) == (OK, 3)
    finally:
        s.close()
    # the context is as usable as before
    assert_same(evaluated(m, pals, err=True), before, "after the refusals")
    # other values of the option
    for bad in (2, -1):
        assert lib.hq_set_option(ctx, b"assign_space", bad) == ERR_ARG
    assert_same(evaluated(m, pals, err=True), before, "after a refused value")
    # under value 0 the same calls succeed
    m.setOption("assign_space", 0)
    for name, call in calls.items():
        c, u, r = outputs()
        assert call(c, u, r) == OK, (name, lib.hq_last_error(ctx))
        assert np.isfinite(c).all() and np.isfinite(r).all() and ((c != -7).all() or (r != -7).all()), name
    c = np.full(1, -7.0)
    assert lib.hq_eval_population(ctx, fp(wide), 1, 16385, 2.0, dp(c), None) == OK and np.isfinite(c[0]) and c[0] > 0
    s = Search(m, K, 3)
    try:
        assert lib.hq_search_set_ordered(s.h, fp(amp)) == OK
        assert lib.hq_search_set_ordered(s.h, None) == OK
        assert lib.hq_search_set_dot(s.h, None, 1.0) == OK
    finally:
        s.close()


# ---------------------------------------------------------------------------
# The served scope beyond the evaluation, and the Python surface
# ---------------------------------------------------------------------------
def test_sums_errors_and_polishes_work_from_the_lab_assignment(ctxs):
    """hq_cluster_sums counts value 1's assignment and sums RGB; hq_refine_population and
    hq_repair_population equal the loops spelt out with the public calls."""
    m = ctxs(assign_space=1)
    rgba = blobs()
    m.setImage(rgba.reshape(-1), None, BW, m.illum)
    P, K = 2, 16
    pals = pals_of(P, K, 33)
    e = evaluated(m, pals)
    sums, den = m.clusterSums(P, K)
    by = np.rint(rgba[:, :3].astype(np.float64) * 255).astype(np.int64)
    for p in range(P):
        idx = e["idx"][p].astype(np.int64)
        np.testing.assert_array_equal(sums[p, :, 3], np.bincount(idx, minlength=K))
        for ch in range(3):
            np.testing.assert_array_equal(sums[p, :, ch], np.bincount(idx, weights=by[:, ch], minlength=K).astype(np.int64))
    assert den == 255
    cur = m.centroidsFromSums(sums, den, pals)
    want = m.computeQuantizationErrorPopulation(cur, 2.0)
    got = m.refinePopulation(pals, 1, 2.0, keep_best=False)
    np.testing.assert_array_equal(bits(got[0]), bits(cur))
    np.testing.assert_array_equal(dbits(got[1]), dbits(want))
    m.setOption("pixel_err", 1)
    m.computeQuantizationErrorPopulation(pals, 2.0)
    err, worst = m.clusterErrors(P, K)
    moved, n = m.reseedUnused(err, worst, pals)
    m.setOption("pixel_err", 0)
    rep = m.repairPopulation(pals, 1, 2.0, keep_best=False)
    np.testing.assert_array_equal(bits(rep[0]), bits(moved))


def test_python_surface(gpu):
    """findBestQuantization(assignSpace="lab") is the search under value 1 and puts the option
    back; quantization renders the image from the index image of the best palette's evaluation."""
    from hybridquantization_amd.scielab_processor import makeinline, quantization
    rgba = blobs()
    planar = np.ascontiguousarray(rgba[:, :3].T)
    sw = hq.SWASA(population=3, imax=40, seed=17, t0=0.05)
    q, best, err = quantization(planar, BW, 8, sw, iterations=10, device=gpu, assignSpace="lab")
    q0, best0, err0 = quantization(planar, BW, 8, hq.SWASA(population=3, imax=40, seed=17, t0=0.05), iterations=10,
                                   device=gpu)
    assert np.isfinite(err) and err != err0
    m = hq.ImageManipulation(DE76, device=gpu)
    try:
        sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
        m.illum = sp.illuminant
        lab = sp.sRGBToScielab(planar, BW)  # (LabRef as quantization makes it)
        m.setOption("assign_space", 1)
        m.setImage(rgba.reshape(-1), lab, BW, m.illum)
        want = searched(m, 8, 3, runs=(10,))
        np.testing.assert_array_equal(bits(best), bits(want[0]))
        assert dbits(err) == dbits(want[1])
        m.computeQuantizationErrorPopulation(best.reshape(1, -1), 0.0)
        table = best.reshape(-1, 4)[:, :3]
        np.testing.assert_array_equal(bits(q.T), bits(table[m.getIndices(0)]))
        # hq_quantize keeps the sRGB rule whatever the option says
        np.testing.assert_array_equal(bits(m.quantize(makeinline(planar), best0)), bits(makeinline(q0)))
        m.setOption("assign_space", 0)
        m.findBestQuantization(rgba.reshape(-1), lab, BW, 8, hq.SWASA(population=3, imax=40, seed=17, t0=0.05),
                               None, None, m.illum, iterations=10, assignSpace="lab")
        assert dbits(m.bestError) == dbits(want[1]) and m._assign_space == 0
        assert m.lastPath()["pixels"] == "planar"
        m.computeQuantizationErrorPopulation(best.reshape(1, -1), 0.0)
        assert m.lastPath()["pixels"] == "u8"
    finally:
        m.close()

"""One long-lived context against fresh ones ("Context reuse and its tests").

2a  every state class of tests/reuse_walk.py on two fresh contexts: the same bits, and
    right against the oracle, dither_ref, lloyd_ref, reseed_ref and seed_ref;
2b  one context through the walk over every ordered pair of classes, bit for bit the
    fresh outputs at every step;
2c  the read-back getters after "pixel_err" was off, after hq_set_image and hq_set_filters,
    and after a search run of no iterations;
2d  a search interrupted by other calls on its context against one that is not;
2e  a context handed from thread to thread, and four contexts side by side.

Every comparison with a fresh context is exact equality of bits.  The only tolerance is
COST_BAR in 2a.
"""

import ctypes as C
import functools
import threading

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
import reuse_walk as rw
from hybridquantization_amd import _lib
from lloyd_ref import cluster_sums_ref, q32
from mask_ref import inside, live_tiles_brute, masked_cluster_sums, masked_histogram
from reseed_ref import cluster_errors_ref
from seed_ref import coord_byte, coord_float, histogram_ref
from test_fast_path_gpu import DEFAULTS as FAST_DEFAULTS
from test_lloyd_gpu import blob_image
from test_seed_gpu import Search

pytestmark = pytest.mark.gpu

DE = {"de76": hq.deltaETypes.CIE76, "de2000": hq.deltaETypes.CIEDE2000}
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = _lib.HQ_OK, _lib.HQ_ERR_ARG, _lib.HQ_ERR_STATE, _lib.HQ_ERR_UNSUPPORTED
# The oracle's cost against the device's.  The path tests hold it to 1e-5 relative
# (test_fast_path_gpu._eval76, test_long_filters_gpu.test_index_widths_long_filters,
# test_dither_gpu.test_indices_used_and_costs_against_the_restatement) or to 1e-6
# (test_gpu.py's K > 256 tests); no class here is held looser than 1e-6, the figure hq.h
# gives for the cost across the paths.
COST_BAR = 1e-6


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


# ---------------------------------------------------------------------------
# Driving a context
# ---------------------------------------------------------------------------
def new_ctx(gpu, de=DE["de76"]):
    m = pr.Context(de, device=gpu)
    assert m.getOpenCLAvailable()
    m.cur_filters = m.cur_image = None
    return m


def enter(m, cls):
    """Brings the context to the class's state with the fewest calls: every option,
    hq_set_filters when the filters differ, hq_set_image when the filters or the image do,
    and -- at every step, since classes that share an image set none between them -- the
    class's mask and threshold map, or none."""
    for name, v in cls["opts"].items():
        m.setOption(name, v)
    if m.cur_filters != cls["filters"]:
        dpi, vd, half = cls["filters"]
        sp = hq.ScielabProcessor(dpi, vd, hq.Whitepoint.D65, None, m)
        assert m.halfSize == half
        m.illum, m.cur_filters, m.cur_image = sp.illuminant, cls["filters"], None
    if m.cur_image != (cls["image"], cls["lab"]):
        lab = rw.oracle_lab(cls).reshape(-1) if cls["lab"] == "oracle" else None
        r0, r1 = rw.rows(cls)
        m.setImage(rw.image(cls).reshape(-1), lab, cls["image"][1], m.illum, r0, r1)
        m.cur_image = (cls["image"], cls["lab"])
    m.setMask(rw.mask_of(cls))
    m.setDitherMap(rw.map_of(cls))


def raw_sums(m, P, K):
    sums, den = np.full((P, K, 4), -7, np.int64), C.c_int64(-7)
    rc = hq.load().hq_cluster_sums(m.ctx, P, K, _lib.i64ptr(sums), C.byref(den))
    return rc, sums, den.value


def raw_errors(m, P, K):
    err, worst = np.full((P, K, 4), -7, np.int64), np.full((P, K, 4), -7, np.float32)
    rc = hq.load().hq_cluster_errors(m.ctx, P, K, _lib.i64ptr(err), _lib.fptr(worst))
    return rc, err, worst


def check_class_path(m, cls):
    """The record of the pass just made against tests/path_ref.py's statement for the class's own
    options, image form, palettes and mask: a path decision left over from the class before
    (the chunk count, the palette range, the live-tile list, the image form) shows here even
    where the fall-back's results are the same."""
    kind, w, h, _, _ = cls["image"]
    kw = dict(pal_fits=pr.palette_fits(rw.palettes(cls)), image_u8=kind == "lattice", rows=rw.rows(cls),
              kind="dither" if cls["op"] == "dither" else "full", ordered=cls["op"] == "ordered")
    if cls["mask"] is not None:
        tw, th, _ = pr.fast_tiles(cls["opts"], cls["filters"][2], w, h)
        kw.update(mask="mask", live_tiles=len(live_tiles_brute(rw.mask_of(cls), w, h, tw, th)))
    return pr.check(m, cls["K"], cls["P"], cls["name"], opts=cls["opts"], **kw)


def operate(m, cls):
    """The class's operation and every read-back -> {name: array}, in a fixed order."""
    P, K, pals = cls["P"], cls["K"], rw.palettes(cls)
    out = {}
    if cls["op"] == "partial":
        part = np.full(P * (1 + K), -7.0)
        _lib.check(hq.load().hq_eval_population_partial(m.ctx, _lib.fptr(pals), P, K, _lib.dptr(part)), m.ctx)
        out["partial"] = part
    elif cls["op"] == "dither":
        out["costs"], out["used"] = m.ditherPopulation(pals, cls["strength"], 2.0, return_used=True)
    elif cls["op"] == "ordered":
        out["costs"], out["used"] = m.orderedPopulation(pals, cls["amp"], 2.0, return_used=True)
    else:
        out["costs"], out["used"] = m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
    check_class_path(m, cls)
    for p in rw.local_palettes(cls):
        out[f"indices32[{p}]"] = m.getIndices32(p)
    if cls["opts"]["pixel_err"]:
        for p in rw.local_palettes(cls):
            out[f"pixel_errors[{p}]"] = m.getPixelErrors(p)
    out["mask_info"] = np.array(m.maskInfo(), np.int64)  # (n_full, n_owned, tiles_run, tiles_all)
    out["labref"] = m.getLabRef()
    cells, den = m.colorHistogram(3)
    out["histogram"], out["histogram_den"] = cells, np.int64(den)
    rc, sums, den = raw_sums(m, P, K)
    out["cluster_sums_status"], out["cluster_sums"], out["cluster_sums_den"] = np.int64(rc), sums, np.int64(den)
    rc, err, worst = raw_errors(m, P, K)
    out["cluster_errors_status"], out["cluster_errors"], out["cluster_errors_worst"] = np.int64(rc), err, worst
    return out


def first_difference(got, want):
    if list(got) != list(want):
        return f"outputs {list(got)} vs {list(want)}"
    for name in want:
        if not np.array_equal(bits(got[name]), bits(want[name])):
            return name
    return None


_FRESH = {}


def fresh(gpu, de, name):
    """The class's outputs on a context that has done nothing else; computed once, read-only."""
    if (de, name) not in _FRESH:
        m = new_ctx(gpu, DE[de])
        try:
            enter(m, rw.by_name(name))
            out = operate(m, rw.by_name(name))
        finally:
            m.close()
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _FRESH[(de, name)] = out
    return _FRESH[(de, name)]


def test_option_table_covers_the_path_tests_defaults():
    for name, v in FAST_DEFAULTS.items():
        assert rw.OPTION_DEFAULTS[name] == v, name


# ---------------------------------------------------------------------------
# 2a. Fresh against fresh, and against the oracle
# ---------------------------------------------------------------------------
def sums_allowed(cls):
    """hq_cluster_sums serves the class: the whole image, not dithered (by diffusion or by a
    threshold map), not sliced."""
    return cls["op"] not in ("dither", "ordered") and cls["opts"]["slice_ranks"] == 1


@pytest.mark.parametrize("name", rw.NAMES)
@pytest.mark.parametrize("de", list(DE))
def test_fresh_contexts_agree_and_are_right(gpu, de, name):
    cls = rw.by_name(name)
    P, K, (_, w, h, _, _), (r0, r1) = cls["P"], cls["K"], cls["image"], rw.rows(cls)
    n_own = w * (r1 - r0)
    a = fresh(gpu, de, name)
    m = new_ctx(gpu, DE[de])
    try:
        enter(m, cls)
        b = operate(m, cls)
    finally:
        m.close()
    assert first_difference(b, a) is None, f"{name}: two fresh contexts differ in {first_difference(b, a)}"

    # indices, used flags and costs against the oracle (the argmin does not depend on the dE type)
    lab = np.zeros((w * h, 4), np.float32)
    lab[r0 * w:r1 * w] = a["labref"].reshape(-1, 4)[:n_own]  # (hq_get_labref: the owned rows first)
    ref = rw.oracle_outputs(cls, lab if cls["lab"] == "device" else None)
    local = list(rw.local_palettes(cls))
    for p in local:
        np.testing.assert_array_equal(a[f"indices32[{p}]"][:n_own], ref["idx"][p].astype(np.uint32), err_msg=f"{name} p={p}")
    if cls["op"] == "partial":
        part = a["partial"].reshape(P, 1 + K)
        for p in range(P):
            np.testing.assert_array_equal(part[p, 1:] > 0, ref["used"][p] > 0, err_msg=f"{name} p={p}")
            if p not in local:
                assert np.all(part[p] == 0.0)
        got, want = part[local, 0], np.array([ref["sum"][p] for p in local])
    else:
        np.testing.assert_array_equal(a["used"] > 0, np.stack(ref["used"]) > 0, err_msg=name)
        got, want = a["costs"], np.array(ref["cost"], np.float64)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    if de == "de76":
        rel = np.abs(got - want) / np.abs(want)
        print(f"{name}: cost or sum against the oracle, relative {rel.max():.3g} (bar {COST_BAR:.3g})")
        assert np.all(rel <= COST_BAR), (name, got, want)

    # the exact integer outputs against their numpy restatements
    rgb = rw.image(cls)[r0 * w:r1 * w, :3]
    by = np.rint(rgb.astype(np.float64) * 255).astype(np.int64)
    den = int(a["histogram_den"])
    assert den == (255 if cls["image"][0] == "lattice" else 1 << 32)
    px = by if den == 255 else q32(rgb)
    coords = coord_byte(by, 3) if den == 255 else coord_float(rgb, 3)
    mask = rw.mask_of(cls)  # (the masked classes hold the whole image)
    np.testing.assert_array_equal(a["histogram"], histogram_ref(coords, px, 3) if mask is None
                                  else masked_histogram(coords, px, 3, mask), err_msg=name)
    whole = (r0, r1) == (0, h)
    n_in = w * h if mask is None else int(inside(mask).sum())
    assert tuple(a["mask_info"][:2]) == (n_in, n_own if mask is None else n_in)
    if mask is not None:  # the rectangle leaves whole tiles dead: the fast cost launch skips them
        assert 0 < a["mask_info"][2] < a["mask_info"][3], a["mask_info"]
    if sums_allowed(cls):
        assert a["cluster_sums_status"] == OK and a["cluster_sums_den"] == den
        for p in range(P):
            idx = a[f"indices32[{p}]"][:n_own]
            np.testing.assert_array_equal(a["cluster_sums"][p], cluster_sums_ref(idx, px, K) if mask is None
                                          else masked_cluster_sums(idx, px, K, mask), err_msg=f"{name} p={p}")
    else:
        assert a["cluster_sums_status"] in (ERR_STATE, ERR_UNSUPPORTED) and np.all(a["cluster_sums"] == -7)
    if sums_allowed(cls) and cls["opts"]["pixel_err"]:
        assert a["cluster_errors_status"] == OK
        for p in range(P):
            want_err, want_rgb = cluster_errors_ref(a[f"indices32[{p}]"][:n_own], a[f"pixel_errors[{p}]"][:n_own], rgb,
                                                    rw.palettes(cls)[p].reshape(K, 4), pos0=r0 * w)
            np.testing.assert_array_equal(a["cluster_errors"][p], want_err, err_msg=f"{name} p={p}")
            np.testing.assert_array_equal(bits(a["cluster_errors_worst"][p]), bits(want_rgb), err_msg=f"{name} p={p}")
    else:
        assert a["cluster_errors_status"] in (ERR_STATE, ERR_UNSUPPORTED) and np.all(a["cluster_errors"] == -7)
        assert np.all(a["cluster_errors_worst"] == -7)
    if mask is not None:  # (no masked error statistic exists, whatever "pixel_err" says)
        assert a["cluster_errors_status"] == ERR_UNSUPPORTED
    assert whole or name == "shard"


# ---------------------------------------------------------------------------
# 2b. The walk
# ---------------------------------------------------------------------------
WALK = rw.euler_walk(len(rw.CLASSES))


@pytest.mark.parametrize("de", list(DE))
def test_walk_over_every_transition(gpu, de):
    """One context through all 211 steps (210 transitions: every ordered pair of the fifteen
    classes once); at every step every output is the fresh context's, bit for bit."""
    assert len(WALK) == 211
    m = new_ctx(gpu, DE[de])
    try:
        prev = None
        for n, ci in enumerate(WALK):
            cls = rw.CLASSES[ci]
            want = fresh(gpu, de, cls["name"])
            enter(m, cls)
            diff = first_difference(operate(m, cls), want)
            assert diff is None, (f"step {n}: {cls['name']} after {prev['name'] if prev else 'nothing'} differs "
                                  f"from a fresh context in {diff}")
            prev = cls
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 2c. Stale read-backs
# ---------------------------------------------------------------------------
def plain_ctx(gpu, **opts):
    m = new_ctx(gpu)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    for name, v in opts.items():
        m.setOption(name, v)
    return m


def lattice(w, h, seed):
    R, G, B = o.synthetic_image(w, h, seed=seed)
    return o.inline_rgba(R, G, B).reshape(-1)


def pals_of(P, K, seed):
    return np.stack([o.synthetic_palette(K, seed + p).reshape(-1) for p in range(P)]).astype(np.float32)


def raw_getters(m, n, p=0):
    """The three getters on buffers prefilled with -7 / 249 -> {name: (status, buffer)}."""
    lib = hq.load()
    i8, i32, e = np.full(n, 249, np.uint8), np.full(n, 0xFFFFFFF9, np.uint32), np.full(n, -7.0, np.float32)
    return {"hq_get_indices": (lib.hq_get_indices(m.ctx, p, _lib.u8ptr(i8)), i8),
            "hq_get_indices32": (lib.hq_get_indices32(m.ctx, p, i32.ctypes.data_as(C.POINTER(C.c_uint32))), i32),
            "hq_get_pixel_errors": (lib.hq_get_pixel_errors(m.ctx, p, _lib.fptr(e)), e)}


def assert_refused(got, what):
    for name, (rc, buf) in got.items():
        untouched = np.all(buf == (-7.0 if buf.dtype == np.float32 else 249 if buf.dtype == np.uint8 else 0xFFFFFFF9))
        assert rc == ERR_STATE and untouched, (f"{what}: {name} returned status {rc} and "
                                               f"{'left the buffer alone' if untouched else 'wrote stale data'}")


def test_pixel_errors_of_an_evaluation_that_stored_none(gpu):
    """97 x 53, P = 3, K = 16: population A with pixel_err 1, population B with pixel_err 0,
    pixel_err 1 again: no error image of B exists, and A's is not B's."""
    w, h, P, K = 97, 53, 3, 16
    img, A, B = lattice(w, h, 3), pals_of(P, K, 11), pals_of(P, K, 29)
    f = plain_ctx(gpu, pixel_err=1)
    f.setImage(img, None, w, f.illum)
    f.computeQuantizationErrorPopulation(B, 2.0)
    want = [f.getPixelErrors(p) for p in range(P)]
    f.close()
    m = plain_ctx(gpu, pixel_err=1)
    try:
        m.setImage(img, None, w, m.illum)
        m.computeQuantizationErrorPopulation(A, 2.0)
        errs_a = [m.getPixelErrors(p) for p in range(P)]
        assert not any(np.array_equal(a, b) for a, b in zip(errs_a, want))
        m.setOption("pixel_err", 0)
        m.computeQuantizationErrorPopulation(B, 2.0)
        m.setOption("pixel_err", 1)
        for p in range(P):
            rc, buf = raw_getters(m, w * h, p)["hq_get_pixel_errors"]
            stale = np.array_equal(bits(buf), bits(errs_a[p]))
            assert rc == ERR_STATE and np.all(buf == -7.0), (
                f"palette {p}: status {rc}, " + ("population A's error image returned for B" if stale else "buffer written"))
        rc, _, _ = raw_errors(m, P, K)
        assert rc == ERR_STATE
        m.computeQuantizationErrorPopulation(B, 2.0)
        for p in range(P):
            np.testing.assert_array_equal(bits(m.getPixelErrors(p)), bits(want[p]))
    finally:
        m.close()


@pytest.mark.parametrize("sizes", ["large_to_small", "small_to_large"])
@pytest.mark.parametrize("by", ["hq_set_image", "hq_set_filters"])
def test_getters_after_the_image_or_filters_changed(gpu, by, sizes):
    """An evaluation on one image, then hq_set_image of another (or hq_set_filters of the
    same taps, which drops the image): nothing of the old evaluation may be read at the new
    geometry.  Afterwards everything equals a fresh context's."""
    big, small = (97, 53, 3), (64, 48, 7)
    (w1, h1, s1), (w2, h2, s2) = (big, small) if sizes == "large_to_small" else (small, big)
    P, K = 3, 16
    pals = pals_of(P, K, 11)
    img1, img2 = lattice(w1, h1, s1), lattice(w2, h2, s2)

    def read_all(m):
        out = {"costs": m.computeQuantizationErrorPopulation(pals, 2.0)}
        for p in range(P):
            out[f"i8[{p}]"], out[f"i32[{p}]"], out[f"e[{p}]"] = m.getIndices(p), m.getIndices32(p), m.getPixelErrors(p)
        out["sums"], _ = m.clusterSums(P, K)
        out["errors"], out["worst"] = m.clusterErrors(P, K)
        return out

    f = plain_ctx(gpu, pixel_err=1)
    f.setImage(img2, None, w2, f.illum)
    want = read_all(f)
    f.close()
    m = plain_ctx(gpu, pixel_err=1)
    lib = hq.load()
    try:
        m.setImage(img1, None, w1, m.illum)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        if by == "hq_set_image":
            m.setImage(img2, None, w2, m.illum)
            n = w2 * h2
        else:
            k = m._filters
            _lib.check(lib.hq_set_filters(m.ctx, k[0].shape[0], *(_lib.fptr(a) for a in k)), m.ctx)
            n = w1 * h1  # (the geometry is still the first image's; the image itself is gone)
        assert_refused(raw_getters(m, n), f"after {by}")
        assert raw_sums(m, P, K)[0] == ERR_STATE and raw_errors(m, P, K)[0] == ERR_STATE
        if by == "hq_set_filters":
            m.setImage(img2, None, w2, m.illum)
            assert_refused(raw_getters(m, w2 * h2), "after hq_set_filters and hq_set_image")
        assert first_difference(read_all(m), want) is None, first_difference(read_all(m), want)
    finally:
        m.close()


def test_getters_after_a_failed_evaluation_and_after_a_search(gpu):
    """A palette-slice evaluation that is refused after the buffers were sized (slice_ranks 2,
    P = 3) ends the read-backs until the next evaluation.  After hq_search_run the index
    getters answer (the last candidates' images, as hq.h says) and hq_get_pixel_errors is
    HQ_ERR_STATE until the next evaluation call."""
    w, h, P, K = 64, 48, 3, 16
    pals = pals_of(P, K, 11)
    m = plain_ctx(gpu, pixel_err=1)
    try:
        m.setImage(lattice(w, h, 7), None, w, m.illum)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        m.setOption("slice_ranks", 2)
        part = np.full(P * (1 + K), -7.0)
        assert hq.load().hq_eval_population_partial(m.ctx, _lib.fptr(pals), P, K, _lib.dptr(part)) == ERR_ARG
        m.setOption("slice_ranks", 1)
        assert_refused(raw_getters(m, w * h), "after a refused evaluation")
        m.computeQuantizationErrorPopulation(pals, 2.0)
        assert all(rc == OK for rc, _ in raw_getters(m, w * h).values())
        s = Search(m, K, hq.SWASA(population=P, imax=20, seed=4, t0=0.05), None)
        try:
            assert s.run(3) == 3
            got = raw_getters(m, w * h)
            assert got["hq_get_indices"][0] == OK and got["hq_get_indices32"][0] == OK
            np.testing.assert_array_equal(got["hq_get_indices"][1], got["hq_get_indices32"][1])
            assert got["hq_get_indices"][1].max() < K
            assert_refused({"hq_get_pixel_errors": got["hq_get_pixel_errors"]}, "after hq_search_run")
        finally:
            s.close()
    finally:
        m.close()


@pytest.mark.parametrize("grows", [True, False], ids=["larger_image", "same_image"])
def test_index_getter_after_a_search_run_of_no_iterations(gpu, grows):
    """A device-resident search (P = 2, K = 16) created on 64 x 48; [the image replaced by
    193 x 131;] an evaluation of P = 1 and its indices read; hq_search_run(s, 0).  The run
    enqueues nothing, so nothing it does may make hq_get_indices answer from memory nobody
    wrote: where it had to grow the index buffer for its own two palettes (the larger image)
    the getter either refuses with the buffer untouched or returns the bytes read before;
    where nothing grows it answers HQ_OK with those bytes."""
    K = 16
    (w1, h1, s1), (w2, h2, s2) = (64, 48, 7), (193, 131, 9)
    m = plain_ctx(gpu, sa_device=1)
    try:
        m.setImage(lattice(w1, h1, s1), None, w1, m.illum)
        s = Search(m, K, hq.SWASA(population=2, imax=20, seed=4, t0=0.05), None)
        try:
            w, h = (w2, h2) if grows else (w1, h1)
            if grows:
                m.setImage(lattice(w2, h2, s2), None, w2, m.illum)
            m.computeQuantizationErrorPopulation(pals_of(1, K, 11), 2.0)
            before = m.getIndices(0).copy()
            assert before.shape == (w * h,) and before.max() < K
            assert s.run(0) == 0
            buf = np.full(w * h, 249, np.uint8)
            rc = hq.load().hq_get_indices(m.ctx, 0, _lib.u8ptr(buf))
            print(f"grows={grows}: hq_get_indices after hq_search_run(s, 0) returned {rc}, "
                  f"{'the bytes read before' if np.array_equal(buf, before) else 'untouched' if np.all(buf == 249) else 'other bytes'}")
            if grows:
                assert (rc == ERR_STATE and np.all(buf == 249)) or (rc == OK and np.array_equal(buf, before)), rc
            else:
                assert rc == OK and np.array_equal(buf, before), rc
        finally:
            s.close()
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 2d. A search that is interrupted equals one that is not
# ---------------------------------------------------------------------------
SW, SH, SP = 96, 64, 4
CHUNKS = (7, 1, 12, 10)
# name: (K, lloyd every, repair every, from a median cut)
KINDS = {"plain": (16, 0, 0, False), "lloyd3": (16, 3, 0, False), "lloyd2_repair4": (8, 2, 4, False),
         "mediancut": (16, 0, 0, True), "k600": (600, 0, 0, False)}
# (kind, sa_device, sa_graph): host-driven, device-resident, device-resident from a captured graph
VARIANTS = [(k, d, g) for k in KINDS for d, g in ((0, 0), (1, 0), (1, 1))]
_SEARCH_REF = {}


@functools.lru_cache(maxsize=None)
def search_image():
    return blob_image(SW, SH, seed=11)[0].reshape(-1)


@functools.lru_cache(maxsize=None)
def other_image():
    return lattice(70, 40, 21)


def start_search(m, kind, seed=31, K=None):
    K0, lloyd, repair, cut = KINDS[kind]
    K = K0 if K is None else K
    pop = None
    if cut:
        cells, den = m.colorHistogram(5)
        pal, _ = m.medianCut(cells, 5, den, K)
        pop = np.tile(pal, (SP, 1))
    s = Search(m, K, hq.SWASA(population=SP, imax=100, seed=seed, t0=0.05), pop)
    if lloyd:
        assert s.lib.hq_search_set_lloyd(s.h, lloyd) == OK
    if repair:
        assert s.lib.hq_search_set_repair(s.h, repair, -1) == OK
    return s


def search_ctx(gpu, device, graph):
    m = plain_ctx(gpu, sa_device=device, sa_graph=graph)
    m.setImage(search_image(), None, SW, m.illum)
    return m


def trajectory(gpu, kind, device, graph, chunks, seed=31, K=None):
    """The best (palette, error, iteration) after every chunk on a fresh context with nothing
    in between; computed once per variant."""
    key = (kind, device, graph, chunks, seed, K)
    if key not in _SEARCH_REF:
        m = search_ctx(gpu, device, graph)
        try:
            s = start_search(m, kind, seed, K)
            try:
                out = []
                for n in chunks:
                    assert s.run(n) == n
                    out.append(s.best())
            finally:
                s.close()
        finally:
            m.close()
        _SEARCH_REF[key] = out
    return _SEARCH_REF[key]


def same_best(a, b):
    return a[2] == b[2] and bits(np.float64(a[1])) == bits(np.float64(b[1])) and np.array_equal(bits(a[0]), bits(b[0]))


class Interruptions:
    """The nine interruptions, numbered as in DESIGN.md; `second` is the second search of 9."""

    def __init__(self, gpu, m, kind, device, graph):
        self.gpu, self.m, self.kind, self.device, self.graph, self.second = gpu, m, kind, device, graph, None
        self.lib = hq.load()

    def run(self, i):
        m, lib = self.m, self.lib
        if self.second is not None and self.second[1] == 3:  # the second search's other two iterations
            assert self.second[0].run(2) == 2
            self.second[1] = 5
        if i == 1:
            m.computeQuantizationErrorPopulation(pals_of(7, 300, 5), 2.0)
            assert m.getIndices32(6).max() < 300
        elif i == 2:
            m.setOption("pixel_err", 1)
            m.computeQuantizationErrorPopulation(pals_of(1, 16, 9), 2.0)
            m.clusterSums(1, 16)
            m.clusterErrors(1, 16)
            m.setOption("pixel_err", 0)
        elif i == 3:
            m.ditherPopulation(pals_of(2, 16, 13), 1.0, 2.0)
        elif i == 4:
            n = 500
            rng = np.random.default_rng(4)
            R, G, B = (rng.random(n, dtype=np.float32) for _ in range(3))
            rgba = o.inline_rgba(R, G, B).reshape(-1)
            m.colorHistogram(4)
            m.XYZtoScielab(m.RGBtoXYZ(R, G, B), None, None, 25, m.illum)
            m.computeError(rgba, m.quantize(rgba, pals_of(1, 16, 3)[0]))
        elif i == 5:
            pals, part = pals_of(3, 16, 17), np.full(3 * 17, -7.0)
            m.setOption("slice_ranks", 2)
            assert lib.hq_eval_population_partial(m.ctx, _lib.fptr(pals), 3, 16, _lib.dptr(part)) == ERR_ARG
            m.setOption("slice_ranks", 1)
        elif i == 6:
            assert lib.hq_profile_enable(m.ctx, 1) == OK
            m.computeQuantizationErrorPopulation(pals_of(2, 16, 19), 2.0)
            assert lib.hq_profile_reset(m.ctx) == OK and lib.hq_profile_enable(m.ctx, 0) == OK
        elif i == 7:  # options documented as not changing results; left changed
            for name, v in (("grid", 64), ("grid", 16), ("assign_blocks_per_cu", 32), ("gen_hrow4", 0), ("gen_vtile2", 0)):
                m.setOption(name, v)
        elif i == 8:
            m.setImage(other_image(), None, 70, m.illum)
            m.computeQuantizationErrorPopulation(pals_of(2, 16, 23), 2.0)
            m.setImage(search_image(), None, SW, m.illum)
        elif i == 9:
            self.second = [start_search(m, "plain", seed=77, K=8), 0]
            assert self.second[0].run(3) == 3
            self.second[1] = 3

    def finish(self):
        """The second search, after its five iterations, against a fresh context's."""
        if self.second is None:
            return
        s, done = self.second
        if done == 3:
            assert s.run(2) == 2
        want = trajectory(self.gpu, "plain", self.device, self.graph, (3, 2), seed=77, K=8)[-1]
        assert same_best(s.best(), want), "the second search on the context differs from a fresh context's"

    def close(self):
        if self.second is not None:
            self.second[0].close()
            self.second = None


@pytest.mark.parametrize("first", [1, 4, 7])
@pytest.mark.parametrize("kind,device,graph", VARIANTS, ids=[f"{k}-dev{d}-graph{g}" for k, d, g in VARIANTS])
def test_interrupted_search_equals_uninterrupted(gpu, kind, device, graph, first):
    """96 x 64 blobs, P = 4, 30 iterations in chunks of 7, 1, 12 and 10; after each chunk the
    best palette, error and iteration equal the uninterrupted search's bit for bit, and one of
    the nine interruptions runs on the context: `first`, first + 1, .. (cyclically), so the
    three values of `first` put each of the nine before at least one chunk."""
    want = trajectory(gpu, kind, device, graph, CHUNKS)
    m = search_ctx(gpu, device, graph)
    try:
        s = start_search(m, kind)
        inter = Interruptions(gpu, m, kind, device, graph)
        try:
            for j, n in enumerate(CHUNKS):
                assert s.run(n) == n
                i = (first - 1 + j) % 9 + 1
                before = f"after interruption {(first - 2 + j) % 9 + 1}" if j else "before any interruption"
                assert same_best(s.best(), want[j]), (f"chunk {j} ({n} iterations) {before}: best "
                                                      f"{s.best()[1:]} vs uninterrupted {want[j][1:]}")
                inter.run(i)
            assert same_best(s.best(), want[-1]), "the best changed without a run"
            inter.finish()
        finally:
            inter.close()
            s.close()
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 2e. Threads
# ---------------------------------------------------------------------------
def in_thread(fn, *args):
    """Runs fn(*args) in a thread of its own, joined before the next starts."""
    box = {}

    def body():
        try:
            box["value"] = fn(*args)
        except BaseException as e:  # noqa: BLE001 (handed to the caller's thread)
            box["error"] = e
    t = threading.Thread(target=body)
    t.start()
    t.join(120)
    assert not t.is_alive(), "the thread did not come back"
    if "error" in box:
        raise box["error"]
    return box.get("value")


@pytest.mark.parametrize("graph", [0, 1])
def test_context_handed_from_thread_to_thread(gpu, graph):
    """hq.h: one host thread per context at a time.  Created in the main thread, image set in a
    second, evaluated in a third, 10 device-resident search iterations in a fourth, read back
    in the main thread: everything equals the same calls made from one thread."""
    w, h, P, K = 97, 53, 3, 16
    img, pals = lattice(w, h, 3), pals_of(P, K, 11)

    def steps(call):
        m = plain_ctx(gpu, sa_device=1, sa_graph=graph, pixel_err=1)
        try:
            out = {}
            call(m.setImage, img, None, w, m.illum)
            out["costs"], out["used"] = call(m.computeQuantizationErrorPopulation, pals, 2.0, True)

            def search():
                s = Search(m, K, hq.SWASA(population=P, imax=50, seed=6, t0=0.05), None)
                try:
                    assert s.run(10) == 10
                    return s.best()
                finally:
                    s.close()
            best, err, it = call(search)
            out["best"], out["best_error"], out["iteration"] = best, np.float64(err), np.int64(it)
            for p in range(P):
                out[f"indices[{p}]"] = m.getIndices32(p)
            out["labref"] = m.getLabRef()
            out["histogram"], _ = m.colorHistogram(3)
            out["costs_again"] = m.computeQuantizationErrorPopulation(pals, 2.0)
            out["errors[0]"] = m.getPixelErrors(0)
            return out
        finally:
            m.close()

    serial = steps(lambda fn, *a: fn(*a))
    handed = steps(in_thread)
    assert first_difference(handed, serial) is None, first_difference(handed, serial)
    assert np.array_equal(bits(serial["costs"]), bits(serial["costs_again"]))


def test_four_contexts_side_by_side(gpu):
    """Four threads, each with a context of its own on one device, started together: three
    rounds each of u8-fast, long-filter, lists16 and dither, every round the class's fresh
    outputs bit for bit."""
    names = ["u8-fast", "long-filter", "lists16", "dither"]
    want = {n: fresh(gpu, "de76", n) for n in names}
    for n in names:  # (the inputs are made once, before the threads start)
        rw.image(rw.by_name(n)), rw.palettes(rw.by_name(n))
    barrier = threading.Barrier(len(names))
    found = {}

    def body(name):
        try:
            cls = rw.by_name(name)
            m = new_ctx(gpu)
            try:
                barrier.wait(60)
                for rnd in range(3):
                    enter(m, cls)
                    diff = first_difference(operate(m, cls), want[name])
                    if diff is not None:
                        found[name] = f"round {rnd}: differs from a fresh context in {diff}"
                        return
            finally:
                m.close()
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            barrier.abort()
            found[name] = repr(e)

    threads = [threading.Thread(target=body, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads), "a thread did not come back"
    assert not found, found

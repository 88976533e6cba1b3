"""Pixel weights on the GPU (hq_set_weights): the weighted cost against the library's own
error image, zeros and ones against the mask bit for bit, dE94's NaN under weight 0, the
weighted sums and histogram against numpy exactly (the wave shortcuts and the accumulator
fields at their bound included), shards, the search, the seed, the arguments, the refusals
and the Python surface.  Restatements: weights_ref.py."""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import path_ref as pr
from hybridquantization_amd import _lib
from lloyd_ref import DEN32, q32
from mask_ref import two_tone_image
from seed_ref import coord_byte, coord_float, median_cut_ref
from test_mask_gpu import (AH, AK, AP, AW, BH, BW, DE00, DE76, DE94, DELTA, LONG, SAMP, SHAPES, caller_filters,
                           designed_half, filter_ctx, indices, new_ctx, noise, pals_of, partial_of, path_under, plain, set_image, u32,
                           u64)
from weights_ref import (LIMIT, as_int64, live_tile_count, nonzero, weight_maps, weight_sum, weighted_cluster_sums,
                         weighted_histogram, weighted_sum)

pytestmark = pytest.mark.gpu


def check_cost(m, wmap, costs, used, msg, w_full=None, delta=DELTA):
    """Check 1: |cost W - delta #unused W - S| <= 1e-6 S + 2^-20 n_nz, S the float64 sum of w e over
    the library's own error image of the owned rows ("pixel_err" 1 in force), W the weight sum of
    the full image, n_nz the owned pixels of non-zero weight.  The first term is the project's bar
    for a cost, the second acc_add's 2^-20 resolution: at most one partial per pixel.  wmap: the
    owned rows' weights."""
    n_nz = nonzero(wmap)
    W = weight_sum(wmap) if w_full is None else w_full
    for p in range(len(costs)):
        S = weighted_sum(m.getPixelErrors(p)[:np.asarray(wmap).size], wmap)  # (a shard: its owned rows come first)
        unused = int(np.count_nonzero(np.asarray(used[p]) == 0))
        miss, bound = abs(costs[p] * W - delta * unused * W - S), 1e-6 * S + 2.0 ** -20 * n_nz
        print(f"{msg} p={p}: cost {costs[p]!r}, S {S!r}, W {W}, n_nz {n_nz}, miss {miss:.3e}, bound {bound:.3e}")
        assert miss <= bound, f"{msg} p={p}"


def sweep_maps(m, pals, w, h, msg, evaluate=plain, tile=(128, 16), de2000=False, maps=None, each=None):
    """Every weight map of the shape on the context m (image set, "pixel_err" 1): the unweighted
    evaluation first; under each map the indices, the used flags and the error image keep their
    bits and the cost satisfies check 1; with "pixel_err" 0 the cost's bits are the same with and
    without the tile skip, and the skipping launch ran the restated number of live tiles.  maps:
    name -> map instead of weight_maps'; each(name, map, skip): called after each of those two
    evaluations.  -> dict(fin, costs0, covers: name -> (the map as set, its costs))."""
    Pn, K = pals.shape[0], pals.shape[1] // 4
    m.setWeights(None)
    costs0, used0 = evaluate(m, pals)
    errs0 = [m.getPixelErrors(p) for p in range(Pn)]
    idx0 = [indices(m, p, K) for p in range(Pn)]
    fin = np.all([np.isfinite(e) for e in errs0], axis=0)  # (dE94: the pixels whose dE is a number)
    covers = {}
    for name, wmap in (weight_maps(w, h) if maps is None else maps).items():
        if not fin.all():
            wmap = np.where(fin.reshape(h, w), wmap, 0).astype(np.uint8)
            if not wmap.any():
                continue
        m.setWeights(wmap)
        costs, used = evaluate(m, pals)
        np.testing.assert_array_equal(used, used0, err_msg=f"{msg} {name}")
        for p in range(Pn):
            np.testing.assert_array_equal(u32(m.getPixelErrors(p)), u32(errs0[p]), err_msg=f"{msg} {name} p={p}")
            np.testing.assert_array_equal(indices(m, p, K), idx0[p], err_msg=f"{msg} {name} p={p}")
        check_cost(m, wmap, costs, used, f"{msg} {name}")
        covers[name] = (wmap, costs)
        assert m.weightsInfo() == (weight_sum(wmap),) * 2
        info = m.maskInfo()
        assert info[0] == info[1] == nonzero(wmap) and info[2] == info[3]
        m.setOption("pixel_err", 0)
        for skip in (1, 0):
            m.setOption("mask_skip", skip)
            c2, u2 = evaluate(m, pals)
            np.testing.assert_array_equal(u64(c2), u64(costs), err_msg=f"{msg} {name} mask_skip {skip}")
            np.testing.assert_array_equal(u2, used0)
            run, every = m.maskInfo()[2:]
            if every:  # (0, 0: the generic pair, which never skips)
                live = live_tile_count(wmap, w, h, *tile, de2000=de2000)
                assert every == live_tile_count(np.ones((h, w)), w, h, *tile, de2000=de2000)
                assert run == (live if skip else every), (msg, name, skip, run, live, every)
            if each is not None:
                each(name, wmap, skip)
        m.setOption("mask_skip", 1)
        m.setOption("pixel_err", 1)
    m.setWeights(None)
    c3, _ = evaluate(m, pals)
    np.testing.assert_array_equal(c3, costs0, err_msg=f"{msg}: the weights cleared")  # (dE94: NaN equals NaN)
    return dict(fin=fin, costs0=costs0, covers=covers)


# ---------------------------------------------------------------------------
# 1. Cost against the library's own error image: every shape, every map, every path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_cost_against_the_error_image(gpu, name):
    w, h, K, Pn, fkey = SHAPES[name]
    m = new_ctx(gpu, pixel_err=1) if fkey is None else filter_ctx(gpu, caller_filters("asymmetric", 0))
    try:
        set_image(m, noise(w, h, 5 if (w, h) == (AW, AH) else w + h), w)
        sweep_maps(m, pals_of(K, 16 if K == 16 else 3 * K + w, Pn), w, h, name)
    finally:
        m.close()


A_PATHS = {
    "cost_rows8": (DE76, {"cost_rows": 8}, plain, (108, 8)),
    "cost_tw256": (DE76, {"cost_tw": 256}, plain, (256, 16)),
    "cost_variant1": (DE76, {"cost_variant": 1}, plain, None),
    "cost_variant2": (DE76, {"cost_variant": 2}, plain, None),
    "de94": (DE94, {}, plain, (128, 16)),
    "de2000": (DE00, {}, plain, (128, 16)),
    "de2000_rows8": (DE00, {"cost_rows": 8}, plain, (108, 8)),
    "dithered": (DE76, {}, lambda m, pals: m.ditherPopulation(pals, 0.75, DELTA, return_used=True), (128, 16)),
    "ordered": (DE76, {}, lambda m, pals: m.orderedPopulation(pals, (0.3, 0.0, 0.7), DELTA, return_used=True), (128, 16)),
}


@pytest.mark.parametrize("name", list(A_PATHS))
def test_cost_paths_on_A(gpu, name):
    """Shape A on the other cost paths, dE types and renderings: every map (dE94: each map with
    weight 0 on the pixels whose dE is NaN for a palette)."""
    de, opts, evaluate, tile = A_PATHS[name]
    m = new_ctx(gpu, de, pixel_err=1, **opts)
    try:
        set_image(m, noise(AW, AH), AW)
        sweep_maps(m, pals_of(AK, 16), AW, AH, name, evaluate=evaluate, tile=tile or (128, 16), de2000=de == DE00)
        if tile is None:
            assert m.maskInfo()[2:] == (0, 0)
    finally:
        m.close()


def test_cost_on_a_long_filter(gpu):
    """A half-width-51 set: the generic pair, the exact double product."""
    w = h = 64
    m = filter_ctx(gpu, designed_half(LONG[2]))
    try:
        set_image(m, noise(w, h), w)
        sweep_maps(m, pals_of(16, 16, 2), w, h, "half 51")
        m.setWeights(weight_maps(w, h)["noise"])
        plain(m, pals_of(16, 16, 2))
        assert m.maskInfo()[2:] == (0, 0)
    finally:
        m.close()


def test_a_uniform_map_is_the_unweighted_cost_within_the_bar(gpu):
    """Not bit for bit (each fma rounds c e + part where the plain kernel rounds e + part), but
    within the project's 1e-6 relative bar for a cost."""
    pals = pals_of(AK, 16)
    m = new_ctx(gpu)
    try:
        set_image(m, noise(AW, AH), AW)
        want = plain(m, pals)[0]
        for c in (2, 37, 255):
            m.setWeights(np.full((AH, AW), c, np.uint8))
            got = plain(m, pals)[0]
            print(f"uniform {c}: {got.tolist()} against {want.tolist()}")
            assert np.all(np.abs(got - want) <= 1e-6 * want)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 2. Zeros and ones is the mask, bit for bit; all ones is the unmasked library
# ---------------------------------------------------------------------------
def _search(gpu, maps, runs=(30,), opts=None, lloyd=0, amp=None, given=None, probe=None, trace=False, setter="setWeights"):
    """A search on A under maps[0]; maps[i] is set before run i (None: nothing set).  setter: a
    name, or one per map."""
    lib = hq.load()
    m = new_ctx(gpu, **(opts or {}))
    setters = [setter] * len(maps) if isinstance(setter, str) else list(setter)
    try:
        set_image(m, noise(AW, AH), AW)
        getattr(m, setters[0])(maps[0])
        sw = hq.SWASA(population=AP, imax=100, seed=9, t0=0.05)
        params, h = sw.params(), C.c_void_p()
        if given is None:
            _lib.check(lib.hq_search_create(m.ctx, C.byref(params), AK, sw.seed, C.byref(h)), m.ctx)
        else:
            _lib.check(lib.hq_search_create_from(m.ctx, C.byref(params), AK, sw.seed, _lib.fptr(given), C.byref(h)), m.ctx)
        pr.check_search(m, h, AP, AK)  # device-resident exactly when sa_device is 1
        try:
            if amp is not None:
                _lib.check(lib.hq_search_set_ordered(h, _lib.fptr(np.ascontiguousarray(amp, np.float32))), m.ctx)
            if lloyd:
                _lib.check(lib.hq_search_set_lloyd(h, lloyd), m.ctx)
            tr = []
            for i, n in enumerate(runs):
                if i:
                    j = min(i, len(maps) - 1)
                    getattr(m, setters[j])(maps[j])
                ran = C.c_int()
                _lib.check(lib.hq_search_run(h, n, C.byref(ran)), m.ctx)
                assert ran.value == n
                best, err, it = np.zeros(4 * AK, np.float32), C.c_double(), C.c_int()
                _lib.check(lib.hq_search_best(h, _lib.fptr(best), C.byref(err), C.byref(it)), m.ctx)
                tr.append(err.value)
            pr.check_search(m, h, AP, AK, ran=True)  # ... and captured exactly when sa_graph is 1
            if probe:
                probe(m, best, err.value)
            return (best, err.value, it.value) + ((tr,) if trace else ())
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()


def _same_search(a, b, msg):
    np.testing.assert_array_equal(u32(a[0]), u32(b[0]), err_msg=msg)
    assert a[1:] == b[1:], (msg, a[1:], b[1:])


def _everything(m, pals):
    Pn, K = pals.shape[0], pals.shape[1] // 4
    costs, used = plain(m, pals)
    out = dict(costs=u64(costs), used=used, sums=m.clusterSums(Pn, K), hist=m.colorHistogram(4),
               part=u64(partial_of(m, pals)))
    got, c2, u2, trace = m.refinePopulation(pals, 2, DELTA, keep_best=False, return_trace=True)
    out.update(refined=u32(got), refined_costs=u64(c2), refined_used=u2, trace=u64(trace))
    return out


def _assert_everything_equal(a, b, msg):
    for k in a:
        for x, y in zip(a[k] if isinstance(a[k], tuple) else (a[k],), b[k] if isinstance(b[k], tuple) else (b[k],)):
            np.testing.assert_array_equal(x, y, err_msg=f"{msg}: {k}")


@pytest.mark.parametrize("img_u8", [1, 0])
def test_zeros_and_ones_is_the_mask_bit_for_bit(gpu, img_u8):
    rgba, pals = noise(AW, AH), pals_of(AK, 16)
    zo = weight_maps(AW, AH)["zeros_ones"]
    a, b = new_ctx(gpu, img_u8=img_u8), new_ctx(gpu, img_u8=img_u8)
    try:
        for c in (a, b):
            set_image(c, rgba, AW)
        fresh = _everything(a, pals)
        a.setMask(zo)
        b.setWeights(zo)
        want = _everything(a, pals)
        _assert_everything_equal(want, _everything(b, pals), "zeros and ones")
        assert not np.array_equal(want["costs"], fresh["costs"])
        assert b.maskInfo() == a.maskInfo() and b.weightsInfo() == a.weightsInfo() == (int(zo.sum()),) * 2
        b.setWeights(np.ones((AH, AW), np.uint8))
        _assert_everything_equal(fresh, _everything(b, pals), "all ones")
        assert b.weightsInfo() == (AW * AH, AW * AH) and b.maskInfo() == (AW * AH, AW * AH, 4, 4)
        b.setWeights(zo)
        for x in ("cost_rows", 16), ("cost_rows", 8), ("cost_variant", 1):  # both fast kernels; the generic pair
            for c in (a, b):
                c.setOption(*x)
            b.setWeights(zo)
            np.testing.assert_array_equal(u64(plain(a, pals)[0]), u64(plain(b, pals)[0]), err_msg=str(x))
            # equal outputs from different kernels: the masked instance there, the weighted one here
            pa, pb = path_under(a, pals, zo, f"mask {x}"), path_under(b, pals, zo, f"weights {x}", weighted=True)
            assert (pa["cost_instance"], pb["cost_instance"]) == ("masked", "weighted"), x
            own = ("cost_instance", "sequence", "previous_pass", "previous_cost")  # (each context's own)
            assert {k: v for k, v in pa.items() if k not in own} == {k: v for k, v in pb.items() if k not in own}
            assert pa["cost"] == {("cost_rows", 16): "cost16w", ("cost_rows", 8): "cost_mfma"}.get(x, "tiled_generic")
    finally:
        a.close()
        b.close()
    opts = {"img_u8": img_u8}
    masked = _search(gpu, [zo], opts=opts, lloyd=3, setter="setMask")
    _same_search(masked, _search(gpu, [zo], opts=opts, lloyd=3), "a 30-iteration search")


# ---------------------------------------------------------------------------
# 3. dE94's NaN under weight 0
# ---------------------------------------------------------------------------
def test_nan_under_weight_zero(gpu):
    """test_nan_outside_the_mask's palettes (dE94 on A, 69 .. 76: several pixels whose dE is NaN).
    The cost is a number when every such pixel weighs 0, and NaN when one of them weighs 1."""
    pals = pals_of(AK, 69, 8)
    m = new_ctx(gpu, DE94, pixel_err=1)
    try:
        set_image(m, noise(AW, AH), AW)
        for opts in ({}, {"cost_rows": 8}, {"cost_variant": 1}):
            for k, v in opts.items():
                m.setOption(k, v)
            m.setWeights(None)  # (which pixels are NaN hangs on the last bits: per path)
            plain(m, pals)
            errs = [m.getPixelErrors(p) for p in range(8)]
            fin = np.all([np.isfinite(e) for e in errs], axis=0)
            assert np.count_nonzero(~fin) >= 1
            wmap = np.where(fin.reshape(AH, AW), weight_maps(AW, AH)["hgrad"] | 1, 0).astype(np.uint8)
            m.setWeights(wmap)
            costs, used = plain(m, pals)
            assert np.all(np.isfinite(costs)), opts
            check_cost(m, wmap, costs, used, f"dE94, weight 0 on the pixels without a number {opts}")
            one = wmap.copy()
            bad = int(np.flatnonzero(~fin)[0])
            one.reshape(-1)[bad] = 1
            m.setWeights(one)
            costs = plain(m, pals)[0]
            hit = [p for p in range(8) if not np.isfinite(errs[p][bad])]
            assert hit and all(np.isnan(costs[p]) for p in hit), opts
            for k in opts:
                m.setOption(k, {"cost_rows": 16, "cost_variant": 0}[k])
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 4. Sums and histogram equal numpy exactly
# ---------------------------------------------------------------------------
def _pixels(rgba, img_u8, bits=4):
    """(integer pixels (n, 3), den, cell coordinates) of a k/255 image in that form."""
    by = np.rint(rgba[:, :3].astype(np.float64) * 255).astype(np.int64)
    if img_u8:
        return by, 255, coord_byte(by, bits)
    return q32(rgba[:, :3]), DEN32, coord_float(rgba[:, :3], bits)


def _check_sums_and_hist(m, pals, px, den, coords, wmap, msg):
    Pn, K = pals.shape[0], pals.shape[1] // 4
    plain(m, pals)
    sums, d = m.clusterSums(Pn, K)
    assert d == den
    for p in range(Pn):
        want = as_int64(weighted_cluster_sums(m.getIndices32(p), px, K, wmap))
        np.testing.assert_array_equal(sums[p], want, err_msg=f"{msg} p={p}")
    assert np.all(sums[..., 3].sum(1) == weight_sum(wmap))
    cells, d = m.colorHistogram(4)
    assert d == den
    np.testing.assert_array_equal(cells, as_int64(weighted_histogram(coords, px, 4, wmap)), err_msg=msg)
    return sums, cells


@pytest.mark.parametrize("K", [16, 300, 1024])
@pytest.mark.parametrize("img_u8", [1, 0])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_sums_and_histogram_equal_numpy(gpu, shape, img_u8, K):
    w, h = (AW, AH) if shape == "A" else (BW, BH)
    rgba = noise(w, h, 5 if shape == "A" else w + h)
    px, den, coords = _pixels(rgba, img_u8)
    Pn = 2 if K == 16 else 1
    pals = pals_of(K, 16 if K == 16 else 3 * K + w, Pn)
    maps = weight_maps(w, h)
    m = new_ctx(gpu, img_u8=img_u8)
    try:
        set_image(m, rgba, w)
        for name in (maps if K == 16 and shape == "A" else ("hgrad", "vgrad", "noise")):
            m.setWeights(maps[name])
            _check_sums_and_hist(m, pals, px, den, coords, maps[name], f"{shape} img_u8 {img_u8} K {K} {name}")
        # a uniform map: exactly c times the unweighted sums and cells
        m.setWeights(None)
        plain(m, pals)
        sums0, cells0 = m.clusterSums(Pn, K)[0], m.colorHistogram(4)[0]
        for c in (3, 255):
            m.setWeights(np.full((h, w), c, np.uint8))
            plain(m, pals)
            sums, cells = m.clusterSums(Pn, K)[0], m.colorHistogram(4)[0]
            np.testing.assert_array_equal(sums, c * sums0)
            np.testing.assert_array_equal(cells, c * cells0)
            if img_u8:  # c s / (255 c n) and s / (255 n): one real quotient of exact doubles
                np.testing.assert_array_equal(u32(m.centroidsFromSums(sums, den, pals)),
                                              u32(m.centroidsFromSums(sums0, den, pals)))
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 5. The shortcuts: uniform waves under non-uniform weights
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("img_u8", [1, 0])
def test_the_wave_shortcuts_add_weights(gpu, img_u8):
    """A single-colour 64 x 64 image: every wave of the sums and the histogram kernel is `full`
    and uniform, so the shortcut's count is the wave's weight sum (256 would be wrong under the
    gradient).  A zero in the map takes its wave off the shortcut.  Then the two-tone image."""
    w = h = 64
    flat = np.zeros((w * h, 4), np.float32)
    flat[:, :3] = np.asarray([51, 102, 204], np.float32) / np.float32(255)
    maps = weight_maps(w, h)
    pals = pals_of(AK, 16)
    m = new_ctx(gpu, img_u8=img_u8)
    try:
        set_image(m, flat, w)
        for name in ("hgrad", "vgrad", "all255", "noise"):
            wmap = maps[name] | 1 if name.endswith("grad") else maps[name]  # (| 1: every wave full)
            m.setWeights(wmap)
            sums, cells = _check_sums_and_hist(m, pals, *_pixels(flat, img_u8), wmap, f"flat img_u8 {img_u8} {name}")
            assert np.count_nonzero(cells[:, 3]) == 1 and cells[:, 3].sum() == weight_sum(wmap)
        rgba, _, left = two_tone_image(w, 32)
        set_image(m, rgba, w)
        for wmap in (weight_maps(w, 32)["hgrad"], (left * 254 + 1).astype(np.uint8)):
            m.setWeights(wmap)
            _check_sums_and_hist(m, pals_of(4, 16, 2), *_pixels(rgba, img_u8), wmap, f"two-tone img_u8 {img_u8}")
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 6. The accumulator fields at their bound (option "cent_span" at its cap)
# ---------------------------------------------------------------------------
WHITE_BLACK = np.asarray([[1, 1, 1, 0, 0, 0, 0, 0]], np.float32)


def test_packed_fields_at_the_span_cap(gpu):
    """260 x 260 white pixels of weight 255 in one colour: 67,600 x 65,025 = 4,395,690,000 > 2^32,
    so a 32-bit field would carry if one workgroup took them all; the cap (2^16 pixels) splits
    them.  The results do not depend on the span."""
    w = h = 260
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = 1.0
    n = w * h
    m = new_ctx(gpu, img_u8=1)
    try:
        set_image(m, rgba, w)
        m.setWeights(np.full((h, w), 255, np.uint8))
        for span in (0, 1024, 1 << 16, 1 << 30):
            m.setOption("cent_span", span)
            plain(m, WHITE_BLACK)
            sums, den = m.clusterSums(1, 2)
            assert den == 255
            assert sums[0].tolist() == [[255 * 255 * n] * 3 + [255 * n], [0, 0, 0, 0]], span
        m.setWeights(None)  # ... and without weights, where the cap is 2^22
        plain(m, WHITE_BLACK)
        assert m.clusterSums(1, 2)[0][0].tolist() == [[255 * n] * 3 + [n], [0, 0, 0, 0]]
        with pytest.raises(_lib.HQError):
            m.setOption("cent_span", -1)
    finally:
        m.close()


def test_planar_words_and_the_2_31_refusal(gpu):
    """2904 x 2900 pixels of 1.0 (q = 2^32): weight 254 sums to 2,139,086,400 < 2^31, accepted and
    exact at 2^32 times that (below 2^63); weight 255 sums to 2,147,508,000 >= 2^31 and is refused
    on the planar form, accepted and exact on the packed one."""
    w, h = 2904, 2900
    n = w * h
    assert n >= 1 << 23 and 254 * n < LIMIT <= 255 * n
    rgba = np.zeros((n, 4), np.float32)
    rgba[:, :3] = 1.0
    lib = hq.load()
    m = new_ctx(gpu, img_u8=0)
    try:
        set_image(m, rgba, w)
        m.setOption("cent_span", 1 << 30)  # (clamped to the planar weighted form's cap)
        m.setWeights(np.full((h, w), 254, np.uint8))
        assert m.weightsInfo() == (254 * n, 254 * n)
        plain(m, WHITE_BLACK)
        sums, den = m.clusterSums(1, 2)
        assert den == DEN32 and sums[0].tolist() == [[DEN32 * 254 * n] * 3 + [254 * n], [0, 0, 0, 0]]
        cells, den = m.colorHistogram(2)
        assert den == DEN32 and cells[-1].tolist() == [DEN32 * 254 * n] * 3 + [254 * n]
        assert np.count_nonzero(cells[:-1]) == 0
        m.setOption("cent_span", 0)
        np.testing.assert_array_equal(m.clusterSums(1, 2)[0], sums)

        m.setWeights(np.full((h, w), 255, np.uint8))
        assert m.weightsInfo() == (255 * n, 255 * n)
        costs = plain(m, WHITE_BLACK)[0]  # (the cost itself has no such limit)
        assert np.isfinite(costs[0])
        out, d = np.full((1, 2, 4), -7, np.int64), C.c_int64(-7)
        assert lib.hq_cluster_sums(m.ctx, 1, 2, _lib.i64ptr(out), C.byref(d)) == _lib.HQ_ERR_UNSUPPORTED
        assert np.all(out == -7) and d.value == -7
        hcells = np.full((64, 4), -7, np.int64)
        assert lib.hq_color_histogram(m.ctx, 2, _lib.i64ptr(hcells), C.byref(d)) == _lib.HQ_ERR_UNSUPPORTED
        assert np.all(hcells == -7) and d.value == -7
        sw = hq.SWASA(population=1, imax=100, seed=9, t0=0.05)
        params, s, ran = sw.params(), C.c_void_p(), C.c_int(-1)
        m.setWeights(np.full((h, w), 254, np.uint8))
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), 2, sw.seed, C.byref(s)), m.ctx)
        try:
            _lib.check(lib.hq_search_set_lloyd(s, 1), m.ctx)
            m.setWeights(np.full((h, w), 255, np.uint8))
            best0, e0 = np.zeros(8, np.float32), C.c_double()
            _lib.check(lib.hq_search_best(s, _lib.fptr(best0), C.byref(e0), None), m.ctx)
            assert lib.hq_search_run(s, 1, C.byref(ran)) == _lib.HQ_ERR_UNSUPPORTED and ran.value == 0
            best1, e1 = np.zeros(8, np.float32), C.c_double()
            _lib.check(lib.hq_search_best(s, _lib.fptr(best1), C.byref(e1), None), m.ctx)
            np.testing.assert_array_equal(u32(best0), u32(best1))
            assert e0.value == e1.value
        finally:
            lib.hq_search_destroy(s)
        # the packed form of the same image and weights
        m.setOption("img_u8", 1)
        plain(m, WHITE_BLACK)
        sums, den = m.clusterSums(1, 2)
        assert den == 255 and sums[0].tolist() == [[255 * 255 * n] * 3 + [255 * n], [0, 0, 0, 0]]
        cells, den = m.colorHistogram(2)
        assert den == 255 and cells[-1].tolist() == [255 * 255 * n] * 3 + [255 * n]
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 7. Shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("de", [DE76, DE00], ids=["de76", "de2000"])
def test_shards_add_up(gpu, de):
    rgba, pals = noise(AW, AH), pals_of(AK, 16)
    maps = weight_maps(AW, AH)
    lower = maps["noise"].copy()  # nothing in rows [0, 20)
    lower[:20] = 0
    m = new_ctx(gpu, de, pixel_err=1)
    try:
        for name, wmap in (("hgrad", maps["hgrad"]), ("vgrad", maps["vgrad"]), ("noise", maps["noise"]), ("lower", lower)):
            set_image(m, rgba, AW)
            m.setWeights(wmap)
            whole = partial_of(m, pals)
            wsums, whist = m.clusterSums(AP, AK)[0], m.colorHistogram(4)[0]
            W = weight_sum(wmap)
            parts, sums, hist, w_owned = [], 0, 0, 0
            for r0, r1 in ((0, 20), (20, AH)):
                set_image(m, rgba, AW, row_begin=r0, row_end=r1)
                m.setWeights(wmap)  # the FULL image's map on every shard
                part = partial_of(m, pals)
                parts.append(part)
                assert m.weightsInfo() == (W, weight_sum(wmap[r0:r1]))
                assert m.maskInfo()[:2] == (nonzero(wmap), nonzero(wmap[r0:r1]))
                w_owned += m.weightsInfo()[1]
                # the shard's partial is check 1 with nothing to divide by: cost W = partial
                check_cost(m, wmap[r0:r1], part[:, 0], np.ones((AP, 1)), f"{name} rows {r0}..{r1}", w_full=1.0)
                sums, hist = sums + m.clusterSums(AP, AK)[0], hist + m.colorHistogram(4)[0]
                if name == "lower" and r0 == 0:  # (every tile runs, "pixel_err" 1, and adds nothing)
                    assert np.all(part[:, 0] == 0.0) and m.weightsInfo()[1] == 0
            assert w_owned == W
            np.testing.assert_array_equal(sums, wsums, err_msg=name)
            np.testing.assert_array_equal(hist, whist, err_msg=name)
            for p in range(AP):
                s = parts[0][p, 0] + parts[1][p, 0]
                print(f"{name} p={p}: shards {s!r}, whole {whole[p, 0]!r}")
                assert abs(s - whole[p, 0]) <= 1e-6 * whole[p, 0]
    finally:
        m.close()


def test_a_single_rank_communicator(gpu):
    rgba, pals, wmap = noise(AW, AH), pals_of(AK, 16), weight_maps(AW, AH)["noise"]
    m, c = new_ctx(gpu), new_ctx(gpu)
    try:
        c.initComm(1, 0, hq.ImageManipulation.commUniqueId())
        for x in (m, c):
            set_image(x, rgba, AW)
            x.setWeights(wmap)
        a, b = plain(m, pals), plain(c, pals)
        np.testing.assert_array_equal(u64(a[0]), u64(b[0]))
        np.testing.assert_array_equal(a[1], b[1])
        assert c.maskInfo() == m.maskInfo() and c.weightsInfo() == m.weightsInfo()
    finally:
        m.close()
        c.close()


# ---------------------------------------------------------------------------
# 8. Search and seed
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "lloyd2", "ordered", "from"])
def test_search_forms_agree_and_runs_compose(gpu, kind):
    wmap = weight_maps(AW, AH)["noise"]
    kw = {"plain": {}, "lloyd2": {"lloyd": 2}, "ordered": {"amp": SAMP},
          "from": {"given": np.clip(pals_of(AK, 16), 0.0, 1.0), "lloyd": 3}}[kind]

    def reproduces(m, best, err):
        m.setOption("pixel_err", 1)
        pal = best.reshape(1, -1)
        costs, used = (m.orderedPopulation(pal, SAMP, DELTA, return_used=True) if kind == "ordered" else plain(m, pal))
        check_cost(m, wmap, [err], used, f"{kind}: the search's best error")
        assert abs(costs[0] - err) <= 1e-6 * err

    dev = _search(gpu, [wmap], probe=reproduces, **kw)
    assert dev[2] == 30
    _same_search(dev, _search(gpu, [wmap], opts={"sa_device": 0}, **kw), "host-driven")
    _same_search(dev, _search(gpu, [wmap], runs=(10, 20), **kw), "10 + 20 iterations")
    _same_search(dev, _search(gpu, [wmap], opts={"sa_graph": 1}, **kw), "sa_graph 1")
    unweighted = _search(gpu, [None], **kw)
    assert unweighted[1] != dev[1]  # another objective


def test_a_map_changed_between_runs(gpu):
    maps = weight_maps(AW, AH)
    seq = [maps["noise"], maps["hgrad"], None]
    dev = _search(gpu, seq, runs=(10, 10, 10))
    _same_search(dev, _search(gpu, seq, runs=(10, 10, 10), opts={"sa_device": 0}), "maps changed, host-driven")
    _same_search(dev, _search(gpu, seq, runs=(10, 10, 10), opts={"sa_graph": 1}), "maps changed, sa_graph 1")
    assert dev[1] != _search(gpu, [maps["noise"]], runs=(10, 10, 10))[1]
    # mask, then weights, then mask: what each run is under is the last one set
    mix, how = [maps["zeros_ones"], maps["noise"], maps["zeros_ones"]], ["setMask", "setWeights", "setMask"]
    a = _search(gpu, mix, runs=(10, 10, 10), setter=how)
    _same_search(a, _search(gpu, mix, runs=(10, 10, 10), setter=["setWeights"] * 3), "zeros and ones through either call")
    _same_search(a, _search(gpu, mix, runs=(10, 10, 10), setter=how, opts={"sa_device": 0}), "mixed, host-driven")


def test_the_weights_steer_the_seed(gpu):
    """The two-tone image under a map that is heavy on the blue half: the median cut of the
    weighted histogram is seed_ref's on the restated weighted cells, and it beats the whole
    image's seed under the weighted cost."""
    w, h, K, bits = 64, 32, 4, 5
    rgba, by, left = two_tone_image(w, h)
    wmap = (left * 254 + 1).astype(np.uint8)  # 255 on the left, 1 on the right
    m = new_ctx(gpu)
    try:
        set_image(m, rgba, w)
        cells, den = m.colorHistogram(bits)
        whole, _ = m.medianCut(cells, bits, den, K)
        m.setWeights(wmap)
        cells, den = m.colorHistogram(bits)
        want_cells = as_int64(weighted_histogram(coord_byte(by, bits), by, bits, wmap))
        np.testing.assert_array_equal(cells, want_cells)
        seeded, made = m.medianCut(cells, bits, den, K)
        want, wmade = median_cut_ref(want_cells, bits, 255, K)
        assert made == wmade == K
        np.testing.assert_array_equal(u32(seeded), u32(want))
        assert not np.array_equal(seeded, whole)
        costs = plain(m, np.stack([seeded, whole]))[0]
        print(f"weighted cost of the weighted seed {costs[0]!r}, of the whole image's seed {costs[1]!r}")
        assert costs[0] < costs[1]
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 9. Arguments, refusals and the Python surface
# ---------------------------------------------------------------------------
def test_set_weights_arguments(gpu):
    lib = hq.load()
    m = new_ctx(gpu)
    try:
        ones = np.ones(AW * AH, np.uint8)
        assert lib.hq_set_weights(None, _lib.u8ptr(ones), AW, AH) == _lib.HQ_ERR_ARG
        assert lib.hq_set_weights(m.ctx, None, 0, 0) == _lib.HQ_OK  # nothing set, no image: a fresh context's state
        assert lib.hq_set_weights(m.ctx, _lib.u8ptr(ones), AW, AH) == _lib.HQ_ERR_STATE
        assert m.weightsInfo() == (0, 0) and m.maskInfo() == (0, 0, 0, 0)
        set_image(m, noise(AW, AH), AW)
        assert m.weightsInfo() == (AW * AH, AW * AH)
        maps = weight_maps(AW, AH)
        good = maps["noise"]
        m.setWeights(good)
        W, n = weight_sum(good), nonzero(good)
        for bad in (lambda: lib.hq_set_weights(m.ctx, _lib.u8ptr(ones), AH, AW),
                    lambda: lib.hq_set_weights(m.ctx, _lib.u8ptr(ones), AW, AH - 1),
                    lambda: lib.hq_set_weights(m.ctx, _lib.u8ptr(np.zeros(AW * AH, np.uint8)), AW, AH),
                    lambda: lib.hq_set_mask(m.ctx, _lib.u8ptr(np.zeros(AW * AH, np.uint8)), AW, AH)):
            assert bad() == _lib.HQ_ERR_ARG
            assert m.weightsInfo() == (W, W) and m.maskInfo()[:2] == (n, n)  # the state in force stays
        for none in (None, None), (C.byref(C.c_int64()), None):
            assert lib.hq_weights_info(m.ctx, *none) == _lib.HQ_OK
        assert lib.hq_weights_info(None, None, None) == _lib.HQ_ERR_ARG
        # Python: bool and 2-D maps, any integer dtype, values 0 .. 255; None clears
        pals = pals_of(AK, 16)
        want = plain(m, pals)[0]
        for form in (good.reshape(-1).astype(np.int64), good.astype(np.int16), good.astype(np.uint32)):
            m.setWeights(form)
            np.testing.assert_array_equal(u64(plain(m, pals)[0]), u64(want))
        m.setWeights(maps["zeros_ones"].astype(bool))
        assert m.weightsInfo() == (int(maps["zeros_ones"].sum()),) * 2
        for wrong in (good.astype(np.float32), good[:-1], good.T, good.reshape(1, AH, AW), good.astype(np.int64) + 1,
                      good.astype(np.int64) - 1):
            with pytest.raises(ValueError):
                m.setWeights(wrong)
        assert m.weightsInfo() == (int(maps["zeros_ones"].sum()),) * 2  # (a ValueError changes nothing)
        # mask and weights are one piece of state: the last wins, None to either clears
        m.setWeights(good)
        m.setMask(maps["zeros_ones"])
        assert m.weightsInfo() == m.maskInfo()[:2] == (int(maps["zeros_ones"].sum()),) * 2
        masked = plain(m, pals)[0]
        m.setWeights(good)
        assert m.weightsInfo() == (W, W) and m.maskInfo()[:2] == (n, n)
        np.testing.assert_array_equal(u64(plain(m, pals)[0]), u64(want))
        m.setMask(maps["zeros_ones"])
        np.testing.assert_array_equal(u64(plain(m, pals)[0]), u64(masked))
        m.setWeights(None)
        assert m.weightsInfo() == m.maskInfo()[:2] == (AW * AH, AW * AH)
        m.setWeights(good)
        m.setMask(None)
        assert m.weightsInfo() == (AW * AH, AW * AH)
        unweighted = plain(m, pals)[0]
        m.setWeights(good)
        set_image(m, noise(AW, AH), AW)  # a map belongs to an image
        assert m.weightsInfo() == m.maskInfo()[:2] == (AW * AH, AW * AH)
        np.testing.assert_array_equal(u64(plain(m, pals)[0]), u64(unweighted))
    finally:
        m.close()


def test_refusals_leave_outputs_and_state_untouched(gpu):
    lib = hq.load()
    pals, wmap = pals_of(AK, 16), weight_maps(AW, AH)["noise"]
    amp = np.asarray(SAMP, np.float32)
    m = new_ctx(gpu, pixel_err=1)
    try:
        set_image(m, noise(AW, AH), AW)
        m.setWeights(wmap)
        plain(m, pals)

        def state():
            return ([m.getIndices(p) for p in range(AP)] + [m.getPixelErrors(p) for p in range(AP)] +
                    [m.clusterSums(AP, AK)[0]])

        held, path = state(), m.lastPath()
        assert path["sequence"] == 1 and path["cost_instance"] == "weighted"
        costs, used = np.full(AP, -7.0), np.full((AP, AK), -7, np.int32)
        part = np.full((AP, 1 + AK), -7.0)
        scratch = pals.copy()
        calls = {
            "eval": lambda: lib.hq_eval_population(m.ctx, _lib.fptr(pals), AP, AK, DELTA, _lib.dptr(costs), _lib.iptr(used)),
            "partial": lambda: lib.hq_eval_population_partial(m.ctx, _lib.fptr(pals), AP, AK, _lib.dptr(part)),
            "ordered": lambda: lib.hq_ordered_population(m.ctx, _lib.fptr(pals), AP, AK, _lib.fptr(amp), DELTA,
                                                         _lib.dptr(costs), _lib.iptr(used)),
            "dither": lambda: lib.hq_dither_population(m.ctx, _lib.fptr(pals), AP, AK, 0.5, DELTA, _lib.dptr(costs),
                                                       _lib.iptr(used)),
            "refine": lambda: lib.hq_refine_population(m.ctx, _lib.fptr(scratch), AP, AK, 1, DELTA, 1,
                                                       _lib.dptr(costs), _lib.iptr(used), None),
        }
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            for what, call in calls.items():
                if name == "palette_split" and what == "refine":
                    continue  # (palette_split without a communicator slices nothing there; see below)
                assert call() == _lib.HQ_ERR_UNSUPPORTED, (name, what, lib.hq_last_error(m.ctx))
                if what in ("eval", "partial"):  # (the renderings refuse a slice on grounds of their own)
                    assert b"pixel weights" in lib.hq_last_error(m.ctx)
            m.setOption(name, 0 if name == "palette_split" else 1)
        m.setOption("palette_split", 1)
        assert calls["refine"]() == _lib.HQ_ERR_UNSUPPORTED  # its evaluations refuse
        m.setOption("palette_split", 0)
        assert np.all(costs == -7.0) and np.all(used == -7) and np.all(part == -7.0)
        np.testing.assert_array_equal(u32(scratch), u32(pals))
        for a, b in zip(held, state()):
            np.testing.assert_array_equal(a, b)
        err, worst = np.full((AP, AK, 4), -7, np.int64), np.full((AP, AK, 4), -7.0, np.float32)
        assert lib.hq_cluster_errors(m.ctx, AP, AK, _lib.i64ptr(err), _lib.fptr(worst)) == _lib.HQ_ERR_UNSUPPORTED
        assert b"hq_set_weights" in lib.hq_last_error(m.ctx)
        p2 = pals.copy()
        assert lib.hq_repair_population(m.ctx, _lib.fptr(p2), AP, AK, 1, DELTA, -1, 1, _lib.dptr(costs), _lib.iptr(used),
                                        None) == _lib.HQ_ERR_UNSUPPORTED
        assert b"hq_set_weights" in lib.hq_last_error(m.ctx)
        assert np.all(err == -7) and np.all(worst == -7.0) and np.all(costs == -7.0) and np.all(used == -7)
        np.testing.assert_array_equal(u32(p2), u32(pals))
        for a, b in zip(held, state()):
            np.testing.assert_array_equal(a, b)
        assert m.lastPath() == path  # no refused call enqueued a pass
        m.setWeights(None)  # with nothing set both answer
        assert lib.hq_cluster_errors(m.ctx, AP, AK, _lib.i64ptr(err), _lib.fptr(worst)) == _lib.HQ_OK
    finally:
        m.close()


@pytest.mark.parametrize("sa_device", [1, 0])
def test_search_refusals(gpu, sa_device):
    lib = hq.load()
    wmap = weight_maps(AW, AH)["noise"]
    m = new_ctx(gpu, sa_device=sa_device)
    try:
        set_image(m, noise(AW, AH), AW)
        sw = hq.SWASA(population=AP, imax=100, seed=9, t0=0.05)
        params, h, ran = sw.params(), C.c_void_p(), C.c_int(-1)
        m.setWeights(wmap)
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            assert lib.hq_search_create(m.ctx, C.byref(params), AK, sw.seed, C.byref(h)) == _lib.HQ_ERR_UNSUPPORTED
            assert not h
            m.setOption(name, 0 if name == "palette_split" else 1)
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), AK, sw.seed, C.byref(h)), m.ctx)
        try:
            def best():
                b, e, it = np.zeros(4 * AK, np.float32), C.c_double(), C.c_int()
                _lib.check(lib.hq_search_best(h, _lib.fptr(b), C.byref(e), C.byref(it)), m.ctx)
                return b, e.value, it.value

            assert lib.hq_search_set_repair(h, 2, -1) == _lib.HQ_ERR_UNSUPPORTED
            assert b"pixel weights" in lib.hq_last_error(m.ctx)
            assert lib.hq_search_set_repair(h, 0, -1) == _lib.HQ_OK
            _lib.check(lib.hq_search_run(h, 3, C.byref(ran)), m.ctx)
            assert ran.value == 3
            m.setWeights(None)
            assert lib.hq_search_set_repair(h, 2, -1) == _lib.HQ_OK  # a period set with nothing in force ...
            m.setWeights(wmap)
            before = best()
            assert lib.hq_search_run(h, 1, C.byref(ran)) == _lib.HQ_ERR_UNSUPPORTED  # ... iteration 4 would repair
            assert ran.value == 0
            _same_search(before, best(), "the refused run")
            m.setOption("slice_ranks", 2)
            assert lib.hq_search_set_repair(h, 0, -1) == _lib.HQ_OK
            assert lib.hq_search_run(h, 1, C.byref(ran)) == _lib.HQ_ERR_UNSUPPORTED and ran.value == 0
            m.setOption("slice_ranks", 1)
            _same_search(before, best(), "the refused run on a slice")
            _lib.check(lib.hq_search_run(h, 2, C.byref(ran)), m.ctx)
            assert ran.value == 2 and best()[2] == 5
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()


def test_find_best_quantization_and_quantization_with_weights(gpu):
    w, h, K = 64, 32, 4
    rgba, _, left = two_tone_image(w, h)
    wmap = (left * 254 + 1).astype(np.uint8)
    W = weight_sum(wmap)
    m = new_ctx(gpu)
    try:
        sw = hq.SWASA(population=2, imax=100, seed=4)
        best = {}
        for name, kw in (("weighted", dict(weights=wmap)), ("flat_i64", dict(weights=wmap.reshape(-1).astype(np.int64))),
                         ("plain", {}), ("seeded", dict(weights=wmap, init="mediancut", lloydSteps=2, lloydEvery=3))):
            best[name] = np.asarray(m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum,
                                                           iterations=10, **kw), np.float32)
            if name == "plain":
                assert m.weightsInfo() == (w * h, w * h)  # setImage dropped the map
                continue
            assert m.weightsInfo() == (W, W) and m.maskInfo()[:2] == (w * h, w * h)
            m.setOption("pixel_err", 1)
            costs, used = plain(m, best[name].reshape(1, -1))
            check_cost(m, wmap, [m.bestError], used, name, delta=sw.delta)
            m.setOption("pixel_err", 0)
        np.testing.assert_array_equal(u32(best["weighted"]), u32(best["flat_i64"]))
        assert not np.array_equal(best["weighted"], best["plain"])
        assert m.seedError >= m.bestError
        for kw in (dict(repairEvery=2), dict(repairSteps=1), dict(mask=left), dict(mask=left, repairEvery=2)):
            set_image(m, rgba, w)
            with pytest.raises(ValueError):
                m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum, iterations=2, weights=wmap, **kw)
            assert m.weightsInfo() == (w * h, w * h)  # (raised before anything ran)
        with pytest.raises(ValueError):
            m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum, iterations=2,
                                   weights=wmap.astype(np.float32))
    finally:
        m.close()
    image = np.stack([rgba[:, 0], rgba[:, 1], rgba[:, 2]])
    q, pal, err = hq.quantization(image, w, K, hq.SWASA(population=2, imax=100, seed=4), device=gpu, iterations=10,
                                  weights=wmap)
    assert q.shape == image.shape and np.isfinite(err) and pal.shape == (4 * K,)
    with pytest.raises(ValueError):
        hq.quantization(image, w, K, hq.SWASA(population=2, imax=100, seed=4), device=gpu, iterations=2, weights=wmap,
                        mask=left)

"""The pixel mask on the GPU (hq_set_mask): the masked cost against the library's own
error image and the oracle, the identities, the tile skip, dE94's NaN outside the
mask, the masked sums and histogram, shards, the search, the seed, the refusals and
the Python surface.  Restatements: mask_ref.py."""

import ctypes as C

import numpy as np
import pytest

import c_oracle
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from hybridquantization_amd import _lib
from lloyd_ref import DEN32, q32
from mask_ref import (inside, live_tiles, masked_cluster_sums, masked_histogram, masked_sum, masks_for, rectangle,
                      two_tone_image)
from seed_ref import coord_byte, coord_float
from test_dither_gpu import new_ctx, noise, pals_of
from test_fast_path import LONG, caller_filters, designed_half
from test_fast_path_gpu import _ctx as filter_ctx

pytestmark = pytest.mark.gpu

DE76, DE94, DE00 = hq.deltaETypes.CIE76, hq.deltaETypes.CIE94, hq.deltaETypes.CIEDE2000
AW, AH, AK, AP = 97, 53, 16, 3
BW, BH, BK, BP = 300, 40, 16, 2
DELTA = 2.0


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def set_image(m, rgba, w, **kw):
    m.setImage(rgba.reshape(-1), None, w, m.illum, **kw)


def plain(m, pals):
    return m.computeQuantizationErrorPopulation(pals, DELTA, return_used=True)


def path_under(m, pals, cover, label, weighted=False):
    """The record of the last pass of `pals` against tests/path_ref.py under the mask or weight map
    `cover` (None: neither): the instance (plain / masked / weighted) and the tiles that ran."""
    Pn, K = pals.shape[0], pals.shape[1] // 4
    kw = {}
    if cover is not None:
        tw, th, _ = pr.fast_tiles(m.options, m.halfSize, m.w, m.h)
        on = (np.asarray(cover).reshape(m.h, m.w) != 0).astype(np.uint8)
        kw = dict(mask="weights" if weighted else "mask", live_tiles=len(live_tiles(on, m.w, m.h, tw, th)))
    return pr.check(m, K, Pn, label, **kw)


def indices(m, p, K):
    return m.getIndices(p) if K <= 256 else m.getIndices32(p)


def partial_of(m, pals):
    Pn, K = pals.shape[0], pals.shape[1] // 4
    part = np.zeros((Pn, 1 + K), np.float64)
    _lib.check(hq.load().hq_eval_population_partial(m.ctx, _lib.fptr(pals), Pn, K, _lib.dptr(part)), m.ctx)
    return part


def check_cost(m, mask, costs, used, msg, n_full=None, delta=DELTA):
    """Check 1: |cost N - delta #unused N - S| <= 1e-6 S + 2^-20 n_in, S the float64 sum of the
    library's own error image over the mask ("pixel_err" 1 in force).  The first term is the
    project's bar for a cost, the second acc_add's 2^-20 resolution: every in-mask pixel lies in
    at most one partial, and empty partials add exact zeros."""
    n_in = int(inside(mask).sum())
    N = n_in if n_full is None else n_full
    for p in range(len(costs)):
        S = masked_sum(m.getPixelErrors(p), mask)
        unused = int(np.count_nonzero(np.asarray(used[p]) == 0))
        miss, bound = abs(costs[p] * N - delta * unused * N - S), 1e-6 * S + 2.0 ** -20 * n_in
        print(f"{msg} p={p}: cost {costs[p]!r}, S {S!r}, n_in {n_in}, miss {miss:.3e}, bound {bound:.3e}")
        assert miss <= bound, f"{msg} p={p}"


def sweep_masks(m, pals, w, h, msg, evaluate=plain, masks=None, extra=None, skip_bits=True, tile=None, de2000=False,
                each=None):
    """Every mask of the shape on the context m (image set, "pixel_err" 1): the unmasked
    evaluation first; under each mask the indices and the error image keep their bits and the
    cost satisfies check 1; with "pixel_err" 0 the cost's bits are the same with and without
    the tile skip.  masks: name -> mask instead of masks_for's; tile = (tw, th) of the fast
    launch: the skipping launch ran the restated number of live tiles, the other one all;
    each(name, mask, skip): called after each of those two evaluations.
    -> dict(fin, costs0, covers: name -> (the mask as set, its costs))."""
    Pn, K = pals.shape[0], pals.shape[1] // 4
    m.setMask(None)
    costs0, used0 = evaluate(m, pals)
    errs0 = [m.getPixelErrors(p) for p in range(Pn)]
    idx0 = [indices(m, p, K) for p in range(Pn)]
    fin = np.all([np.isfinite(e) for e in errs0], axis=0)  # (dE94: the pixels whose dE is a number)
    worst = int(np.argmax(np.where(fin, errs0[0], -1.0)))
    ms = dict(masks_for(w, h, worst=worst) if masks is None else masks)
    ms.update(extra or {})
    covers = {}
    for name, mask in ms.items():
        if not fin.all():
            mask = (inside(mask) & fin).astype(np.uint8).reshape(h, w)
            if not mask.any():
                continue
        m.setMask(mask)
        costs, used = evaluate(m, pals)
        np.testing.assert_array_equal(used, used0, err_msg=f"{msg} {name}")
        for p in range(Pn):
            np.testing.assert_array_equal(u32(m.getPixelErrors(p)), u32(errs0[p]), err_msg=f"{msg} {name} p={p}")
            np.testing.assert_array_equal(indices(m, p, K), idx0[p], err_msg=f"{msg} {name} p={p}")
        check_cost(m, mask, costs, used, f"{msg} {name}")
        covers[name] = (mask, costs)
        info = m.maskInfo()
        assert info[0] == info[1] == int(inside(mask).sum()) and info[2] == info[3]
        if name == "ones" and fin.all():
            np.testing.assert_array_equal(u64(costs), u64(costs0), err_msg=f"{msg}: all ones is no mask")
        if skip_bits:
            m.setOption("pixel_err", 0)
            for skip in (1, 0):
                m.setOption("mask_skip", skip)
                c2, u2 = evaluate(m, pals)
                np.testing.assert_array_equal(u64(c2), u64(costs), err_msg=f"{msg} {name} mask_skip {skip}")
                np.testing.assert_array_equal(u2, used0)
                if tile is not None:
                    live = len(live_tiles(mask, w, h, *tile, de2000=de2000))
                    every = len(live_tiles(np.ones((h, w), np.uint8), w, h, *tile, de2000=de2000))
                    assert m.maskInfo()[2:] == (live if skip else every, every), (msg, name, skip, m.maskInfo(), live, every)
                if each is not None:
                    each(name, mask, skip)
            m.setOption("mask_skip", 1)
            m.setOption("pixel_err", 1)
    m.setMask(None)
    c3, _ = evaluate(m, pals)
    np.testing.assert_array_equal(c3, costs0, err_msg=f"{msg}: the mask cleared")  # (dE94: NaN equals NaN)
    return dict(fin=fin, costs0=costs0, covers=covers)


# ---------------------------------------------------------------------------
# 1. Cost against the library's own error image: every shape, every mask
# ---------------------------------------------------------------------------
SHAPES = {
    "A_97x53": (AW, AH, AK, AP, None),
    "B_300x40": (BW, BH, BK, BP, None),
    "C_5x1": (5, 1, 6, 2, "caller0"),
    "C_1x5": (1, 5, 6, 2, "caller0"),
    "C_2x3": (2, 3, 6, 2, "caller0"),
    "D_64x64_k300": (64, 64, 300, 1, None),   # chunked palettes, per-chunk grids
    "D_64x64_k1024": (64, 64, 1024, 1, None),  # chunked palettes, native lists
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_cost_against_the_error_image(gpu, name):
    w, h, K, Pn, fkey = SHAPES[name]
    m = new_ctx(gpu, pixel_err=1) if fkey is None else filter_ctx(gpu, caller_filters("asymmetric", 0))
    try:
        set_image(m, noise(w, h, 5 if (w, h) == (AW, AH) else w + h), w)
        extra = {"rect": rectangle(BW, BH, 130, 250, 17, 30)} if name.startswith("B") else None
        sweep_masks(m, pals_of(K, 16 if K == 16 else 3 * K + w, Pn), w, h, name, extra=extra)
    finally:
        m.close()


A_PATHS = {
    "cost_rows8": (DE76, {"cost_rows": 8}, plain),
    "cost_tw256": (DE76, {"cost_tw": 256}, plain),
    "cost_variant1": (DE76, {"cost_variant": 1}, plain),
    "cost_variant2": (DE76, {"cost_variant": 2}, plain),
    "de94": (DE94, {}, plain),
    "de2000": (DE00, {}, plain),
    "de2000_rows8": (DE00, {"cost_rows": 8}, plain),
    "dithered": (DE76, {}, lambda m, pals: m.ditherPopulation(pals, 0.75, DELTA, return_used=True)),
    "ordered": (DE76, {}, lambda m, pals: m.orderedPopulation(pals, (0.3, 0.0, 0.7), DELTA, return_used=True)),
}


@pytest.mark.parametrize("name", list(A_PATHS))
def test_cost_paths_on_A(gpu, name):
    """Shape A on the other cost paths, dE types and renderings: every mask (dE94: each mask
    without the pixels whose dE is NaN for a palette, the way of check 5)."""
    de, opts, evaluate = A_PATHS[name]
    m = new_ctx(gpu, de, pixel_err=1, **opts)
    try:
        set_image(m, noise(AW, AH), AW)
        sweep_masks(m, pals_of(AK, 16), AW, AH, name, evaluate=evaluate)
    finally:
        m.close()


def test_cost_on_a_long_filter(gpu):
    """A half-width-51 set: the generic pair, which never skips (maskInfo's tiles are 0)."""
    w = h = 64
    m = filter_ctx(gpu, designed_half(LONG[2]))
    try:
        set_image(m, noise(w, h), w)
        sweep_masks(m, pals_of(16, 16, 2), w, h, "half 51")
        m.setMask(masks_for(w, h)["bernoulli"])
        plain(m, pals_of(16, 16, 2))
        assert m.maskInfo()[2:] == (0, 0)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 2. Cost against the oracle
# ---------------------------------------------------------------------------
def test_masked_cost_against_the_oracle(gpu):
    """A masked mean cannot be further from the oracle's than the worst pixel is: 2e-4, the
    per-pixel bar of test_pixel_errors_vs_oracle."""
    f = o.design_filters(72, 45.0)
    rgba, pals = noise(AW, AH), pals_of(AK, 16)
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, AW)
    mask = masks_for(AW, AH)["bernoulli"]
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), lab.reshape(-1), AW, m.illum)
        m.setMask(mask)
        costs, used = plain(m, pals)
        for p in range(AP):
            pal = pals[p].reshape(AK, 4)
            err = o.ciede76(lab, o.candidate_scielab(m.getIndices(p).astype(np.int32), pal, f, AW, AH))
            want = masked_sum(err, mask) / int(inside(mask).sum()) + DELTA * int(np.count_nonzero(used[p] == 0))
            print(f"p={p}: masked cost {costs[p]!r}, oracle {want!r}, distance {abs(costs[p] - want):.3e}")
            assert abs(costs[p] - want) <= 2e-4
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 3. Identities, bit for bit
# ---------------------------------------------------------------------------
def _everything(m, pals):
    Pn, K = pals.shape[0], pals.shape[1] // 4
    costs, used = plain(m, pals)
    return dict(costs=u64(costs), used=used, sums=m.clusterSums(Pn, K), hist=m.colorHistogram(4),
                part=u64(partial_of(m, pals)))


def _assert_everything_equal(a, b, msg):
    for k in a:
        for x, y in zip(a[k] if isinstance(a[k], tuple) else (a[k],), b[k] if isinstance(b[k], tuple) else (b[k],)):
            np.testing.assert_array_equal(x, y, err_msg=f"{msg}: {k}")


@pytest.mark.parametrize("img_u8", [1, 0])
def test_all_ones_and_no_mask_are_the_unmasked_library(gpu, img_u8):
    rgba, pals = noise(AW, AH), pals_of(AK, 16)
    fresh, m = new_ctx(gpu, img_u8=img_u8), new_ctx(gpu, img_u8=img_u8)
    try:
        for c in (fresh, m):
            set_image(c, rgba, AW)
        want = _everything(fresh, pals)
        assert m.maskInfo() == (AW * AH, AW * AH, 0, 0)
        m.setMask(np.ones((AH, AW), np.uint8))
        _assert_everything_equal(want, _everything(m, pals), "all ones")
        assert m.maskInfo() == (AW * AH, AW * AH, 4, 4)
        plain(m, pals)  # the masked instance over every tile, not the plain one
        got = path_under(m, pals, np.ones((AH, AW), np.uint8), "all ones")
        assert (got["cost_instance"], got["tiles_run"], got["tiles_all"]) == ("masked", 4, 4)
        plain(fresh, pals)
        assert path_under(fresh, pals, None, "no mask")["cost_instance"] == "plain"
        m.setMask(masks_for(AW, AH)["bernoulli"])
        other = _everything(m, pals)
        assert not np.array_equal(other["costs"], want["costs"]) and not np.array_equal(other["sums"][0], want["sums"][0])
        m.setMask(None)
        _assert_everything_equal(want, _everything(m, pals), "setMask(None) after a mask")
        m.setMask(masks_for(AW, AH)["cols3"])
        assert m.maskInfo()[0] == int(masks_for(AW, AH)["cols3"].sum())
        set_image(m, rgba, AW)  # a mask belongs to an image
        assert m.maskInfo() == (AW * AH, AW * AH, 0, 0)
        _assert_everything_equal(want, _everything(m, pals), "setImage drops the mask")
    finally:
        fresh.close()
        m.close()


# ---------------------------------------------------------------------------
# 4. The skip ran
# ---------------------------------------------------------------------------
def test_the_skip_ran(gpu):
    pals = pals_of(BK, 16, BP)
    rect, edges = rectangle(BW, BH, 130, 250, 17, 30), masks_for(BW, BH)["edges"]
    m = new_ctx(gpu)
    try:
        set_image(m, noise(BW, BH, BW + BH), BW)
        m.setMask(rect)
        plain(m, pals)
        assert m.maskInfo() == (120 * 13, 120 * 13, 1, 9)
        got = path_under(m, pals, rect, "skip")
        assert (got["cost"], got["cost_instance"], got["tiles_run"], got["tiles_all"]) == ("cost16w", "masked", 1, 9)
        m.setOption("mask_skip", 0)
        plain(m, pals)
        assert m.maskInfo()[2:] == (9, 9)
        got = path_under(m, pals, rect, "mask_skip 0")
        assert (got["cost_instance"], got["tiles_run"], got["tiles_all"]) == ("masked", 9, 9)
        m.setOption("mask_skip", 1)
        m.setOption("cost_rows", 8)  # 8 x 108 tiles: 3 x 5
        plain(m, pals)
        want = live_tiles(rect, BW, BH, 108, 8)
        assert m.maskInfo()[2:] == (len(want), 15) and len(want) == 4
        got = path_under(m, pals, rect, "8 x 108")
        assert (got["cost"], got["cost_instance"], got["tiles_run"], got["tiles_all"]) == ("cost_mfma", "masked", 4, 15)
        m.setOption("cost_rows", 16)
        m.setOption("cost_tw", 256)  # 16 x 256 tiles: 2 x 3, the rectangle inside tile (0, 1)
        plain(m, pals)
        assert m.maskInfo()[2:] == (len(live_tiles(rect, BW, BH, 256, 16)), 6) == (1, 6)
        got = path_under(m, pals, rect, "16 x 256")
        assert (got["cost_waves"], got["cost_instance"], got["tiles_run"], got["tiles_all"]) == (8, "masked", 1, 6)
        m.setOption("cost_tw", 128)
        m.setOption("pixel_err", 1)  # every tile stores its pixels' dE
        plain(m, pals)
        assert m.maskInfo()[2:] == (9, 9)
        got = path_under(m, pals, rect, "pixel_err 1")
        assert (got["cost_instance"], got["tiles_run"], got["tiles_all"]) == ("masked", 9, 9)
        m.setOption("pixel_err", 0)
        m.setOption("cost_variant", 1)  # the generic path
        plain(m, pals)
        assert m.maskInfo()[2:] == (0, 0)
        got = path_under(m, pals, rect, "generic")
        assert (got["cost"], got["cost_instance"], got["tiles_run"], got["tiles_all"]) == ("tiled_generic", "masked", 0, 0)
        m.setOption("cost_variant", 0)
        m.setMask(edges)
        plain(m, pals)
        assert m.maskInfo()[2:] == (5, 9)
        assert path_under(m, pals, edges, "edges")["tiles_run"] == 5
        m.setMask(None)
        plain(m, pals)
        assert m.maskInfo() == (BW * BH, BW * BH, 9, 9)
        got = path_under(m, pals, None, "no mask")
        assert (got["cost_instance"], got["tiles_run"], got["tiles_all"]) == ("plain", 9, 9)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 5. NaN outside the mask
# ---------------------------------------------------------------------------
def test_nan_outside_the_mask(gpu):
    """dE94 on A with the palettes 69 .. 76, which have several pixels whose dE is NaN
    (test_mask.py shows it on the oracle; which ones hangs on the Lab's last bits).  The mask is
    isfinite of the unmasked error images."""
    pals = pals_of(AK, 69, 8)
    f = o.design_filters(72, 45.0)
    rgba = noise(AW, AH)
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, AW)
    m = new_ctx(gpu, DE94, pixel_err=1)
    try:
        m.setImage(rgba.reshape(-1), lab.reshape(-1), AW, m.illum)
        costs0, _ = plain(m, pals)
        fin = np.all([np.isfinite(m.getPixelErrors(p)) for p in range(8)], axis=0)
        print(f"unmasked dE94 costs {costs0.tolist()}, pixels without a number {np.count_nonzero(~fin)}")
        assert np.count_nonzero(~fin) >= 1
        mask = fin.astype(np.uint8).reshape(AH, AW)
        m.setMask(mask)
        costs, used = plain(m, pals)
        assert np.all(np.isfinite(costs))
        check_cost(m, mask, costs, used, "dE94, finite pixels")
        m.setOption("pixel_err", 0)  # the skipping launch: the same bits
        np.testing.assert_array_equal(u64(plain(m, pals)[0]), u64(costs))
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 6. Sums and histogram
# ---------------------------------------------------------------------------
def _pixels(rgba, img_u8):
    """(integer pixels (n, 3), den, cell coordinates at 4 bits) of a k/255 image in that form."""
    by = np.rint(rgba[:, :3].astype(np.float64) * 255).astype(np.int64)
    if img_u8:
        return by, 255, coord_byte(by, 4)
    return q32(rgba[:, :3]), DEN32, coord_float(rgba[:, :3], 4)


def _check_sums_and_hist(m, pals, px, den, coords, mask, msg):
    Pn, K = pals.shape[0], pals.shape[1] // 4
    plain(m, pals)
    sums, d = m.clusterSums(Pn, K)
    assert d == den
    for p in range(Pn):
        np.testing.assert_array_equal(sums[p], masked_cluster_sums(m.getIndices32(p), px, K, mask), err_msg=f"{msg} p={p}")
    assert np.all(sums[..., 3].sum(1) == int(inside(mask).sum()))
    cells, d = m.colorHistogram(4)
    assert d == den
    np.testing.assert_array_equal(cells, masked_histogram(coords, px, 4, mask), err_msg=msg)
    return sums


@pytest.mark.parametrize("img_u8", [1, 0])
def test_sums_and_histogram_equal_numpy(gpu, img_u8):
    rgba = noise(AW, AH)
    px, den, coords = _pixels(rgba, img_u8)
    m = new_ctx(gpu, img_u8=img_u8)
    try:
        set_image(m, rgba, AW)
        pals = pals_of(AK, 16)
        for name, mask in masks_for(AW, AH, worst=AW * 20 + 7).items():
            m.setMask(mask)
            sums = _check_sums_and_hist(m, pals, px, den, coords, mask, f"img_u8 {img_u8} {name}")
            if name == "worst":  # colours without an in-mask pixel keep their bits in the update
                new = m.centroidsFromSums(sums, den, pals).reshape(AP, AK, 4)
                keep = sums[..., 3] == 0
                np.testing.assert_array_equal(u32(new[keep]), u32(pals.reshape(AP, AK, 4)[keep]))
                assert np.count_nonzero(~keep) == AP
        # the single-colour wave shortcut with masked-out pixels in the wave
        flat = np.zeros((AW * AH, 4), np.float32)
        flat[:, :3] = np.asarray([51, 102, 204], np.float32) / np.float32(255)
        set_image(m, flat, AW)
        mask = masks_for(AW, AH)["bernoulli"]
        m.setMask(mask)
        _check_sums_and_hist(m, pals, *_pixels(flat, img_u8), mask, f"img_u8 {img_u8} flat")
    finally:
        m.close()


@pytest.mark.parametrize("K", [300, 1024])
def test_sums_on_chunked_palettes(gpu, K):
    w = h = 64
    rgba = noise(w, h)
    m = new_ctx(gpu)
    try:
        set_image(m, rgba, w)
        mask = masks_for(w, h)["bernoulli"]
        m.setMask(mask)
        _check_sums_and_hist(m, pals_of(K, 3 * K + w, 1), *_pixels(rgba, 1), mask, f"K={K}")
    finally:
        m.close()


def test_refine_population_under_a_mask(gpu):
    """hq_refine_population is the hand-written loop of the masked pieces."""
    rgba, pals, mask = noise(AW, AH), pals_of(AK, 16), masks_for(AW, AH)["bernoulli"]
    m = new_ctx(gpu, pixel_err=1)
    try:
        set_image(m, rgba, AW)
        m.setMask(mask)
        got, costs, used, trace = m.refinePopulation(pals, 2, DELTA, keep_best=False, return_trace=True)
        cur = pals.copy()
        for step in range(3):
            c, u = plain(m, cur)
            np.testing.assert_array_equal(u64(c), u64(trace[step]))
            if step < 2:
                cur = m.centroidsFromSums(*m.clusterSums(AP, AK), cur)
        np.testing.assert_array_equal(u32(got), u32(cur))
        check_cost(m, mask, costs, used, "refined")
        assert np.all(trace[2] < trace[0])
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 7. Shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("de", [DE76, DE00], ids=["de76", "de2000"])
def test_shards_add_up(gpu, de):
    rgba, pals = noise(AW, AH), pals_of(AK, 16)
    ms = masks_for(AW, AH)
    lower = np.zeros((AH, AW), np.uint8)  # nothing in rows [0, 20)
    lower[20:] = ms["bernoulli"][20:]
    m = new_ctx(gpu, de)
    try:
        for name, mask in (("bernoulli", ms["bernoulli"]), ("cols3", ms["cols3"]), ("lower", lower)):
            set_image(m, rgba, AW)
            m.setMask(mask)
            whole = partial_of(m, pals)
            wsums, whist = m.clusterSums(AP, AK)[0], m.colorHistogram(4)[0]
            costs = plain(m, pals)[0]
            n_full = int(inside(mask).sum())
            parts, sums, hist = [], 0, 0
            for r0, r1 in ((0, 20), (20, AH)):
                set_image(m, rgba, AW, row_begin=r0, row_end=r1)
                m.setMask(mask)  # the FULL image's mask on every shard
                parts.append(partial_of(m, pals))
                assert m.maskInfo()[:2] == (n_full, int(inside(mask[r0:r1]).sum()))
                sums, hist = sums + m.clusterSums(AP, AK)[0], hist + m.colorHistogram(4)[0]
                if name == "lower" and r0 == 0:
                    assert np.all(parts[0][:, 0] == 0.0) and m.maskInfo()[2] == 0
            np.testing.assert_array_equal(sums, wsums, err_msg=name)
            np.testing.assert_array_equal(hist, whist, err_msg=name)
            for p in range(AP):
                s = parts[0][p, 0] + parts[1][p, 0]
                print(f"{name} p={p}: shards {s!r}, whole {whole[p, 0]!r}")
                assert abs(s - whole[p, 0]) <= 1e-6 * whole[p, 0]
                unused = int(np.count_nonzero(whole[p, 1:] == 0))
                assert abs(whole[p, 0] / n_full + DELTA * unused - costs[p]) <= 1e-12 * costs[p]
    finally:
        m.close()


def test_a_single_rank_communicator(gpu):
    rgba, pals, mask = noise(AW, AH), pals_of(AK, 16), masks_for(AW, AH)["bernoulli"]
    m, c = new_ctx(gpu), new_ctx(gpu)
    try:
        c.initComm(1, 0, hq.ImageManipulation.commUniqueId())
        for x in (m, c):
            set_image(x, rgba, AW)
            x.setMask(mask)
        a, b = plain(m, pals), plain(c, pals)
        np.testing.assert_array_equal(u64(a[0]), u64(b[0]))
        np.testing.assert_array_equal(a[1], b[1])
        assert c.maskInfo() == m.maskInfo()
    finally:
        m.close()
        c.close()


# ---------------------------------------------------------------------------
# 8. Search
# ---------------------------------------------------------------------------
SAMP = (0.5, 0.5, 0.5)


def _search(gpu, masks, runs=(30,), opts=None, lloyd=0, amp=None, given=None, probe=None, trace=False):
    """A search on A under masks[0]; masks[i] is set before run i (None: no mask)."""
    lib = hq.load()
    m = new_ctx(gpu, **(opts or {}))
    try:
        set_image(m, noise(AW, AH), AW)
        m.setMask(masks[0])
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
                    m.setMask(masks[min(i, len(masks) - 1)])
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


@pytest.mark.parametrize("kind", ["plain", "lloyd2", "ordered", "from"])
def test_search_forms_agree_and_runs_compose(gpu, kind):
    mask = masks_for(AW, AH)["bernoulli"]
    kw = {"plain": {}, "lloyd2": {"lloyd": 2}, "ordered": {"amp": SAMP},
          "from": {"given": np.clip(pals_of(AK, 16), 0.0, 1.0), "lloyd": 3}}[kind]

    def reproduces(m, best, err):
        m.setOption("pixel_err", 1)
        pal = best.reshape(1, -1)
        costs, used = (m.orderedPopulation(pal, SAMP, DELTA, return_used=True) if kind == "ordered" else plain(m, pal))
        check_cost(m, mask, [err], used, f"{kind}: the search's best error")
        assert abs(costs[0] - err) <= 1e-6 * err

    dev = _search(gpu, [mask], probe=reproduces, **kw)
    assert dev[2] == 30
    _same_search(dev, _search(gpu, [mask], opts={"sa_device": 0}, **kw), "host-driven")
    _same_search(dev, _search(gpu, [mask], runs=(10, 20), **kw), "10 + 20 iterations")
    _same_search(dev, _search(gpu, [mask], opts={"sa_graph": 1}, **kw), "sa_graph 1")
    unmasked = _search(gpu, [None], **kw)
    assert unmasked[1] != dev[1]  # another objective


def test_search_identities_and_a_mask_changed_between_runs(gpu):
    ms = masks_for(AW, AH)
    ones = _search(gpu, [ms["ones"]], runs=(1,) * 30, trace=True)
    none = _search(gpu, [None], runs=(1,) * 30, trace=True)
    np.testing.assert_array_equal(u32(ones[0]), u32(none[0]))
    assert ones[1:] == none[1:]  # the best error after every iteration
    seq = [ms["bernoulli"], ms["cols3"], None]
    dev = _search(gpu, seq, runs=(10, 10, 10))
    _same_search(dev, _search(gpu, seq, runs=(10, 10, 10), opts={"sa_device": 0}), "masks changed, host-driven")
    _same_search(dev, _search(gpu, seq, runs=(10, 10, 10), opts={"sa_graph": 1}), "masks changed, sa_graph 1")
    assert dev[1] != _search(gpu, [ms["bernoulli"]], runs=(10, 10, 10))[1]


# ---------------------------------------------------------------------------
# 9. The region steers the seed
# ---------------------------------------------------------------------------
def test_the_region_steers_the_seed(gpu):
    w, h, K, bits = 64, 32, 4, 5
    rgba, _, mask = two_tone_image(w, h)
    m = new_ctx(gpu)
    try:
        set_image(m, rgba, w)
        cells, den = m.colorHistogram(bits)
        whole, _ = m.medianCut(cells, bits, den, K)
        m.setMask(mask)
        cells, den = m.colorHistogram(bits)
        assert cells[:, 3].sum() == w * h // 2
        seeded, made = m.medianCut(cells, bits, den, K)
        assert made == K
        costs = plain(m, np.stack([seeded, whole]))[0]
        print(f"masked cost of the masked seed {costs[0]!r}, of the whole image's seed {costs[1]!r}")
        assert costs[0] < costs[1]
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 10. Refusals and arguments
# ---------------------------------------------------------------------------
def test_set_mask_arguments(gpu):
    lib = hq.load()
    m = new_ctx(gpu)
    try:
        ones = np.ones(AW * AH, np.uint8)
        assert lib.hq_set_mask(None, _lib.u8ptr(ones), AW, AH) == _lib.HQ_ERR_ARG
        assert lib.hq_set_mask(m.ctx, None, 0, 0) == _lib.HQ_OK  # no mask, no image: a fresh context's state
        assert lib.hq_set_mask(m.ctx, _lib.u8ptr(ones), AW, AH) == _lib.HQ_ERR_STATE
        assert m.maskInfo() == (0, 0, 0, 0)
        set_image(m, noise(AW, AH), AW)
        good = masks_for(AW, AH)["cols3"]
        m.setMask(good)
        n = int(good.sum())
        for bad in (lambda: lib.hq_set_mask(m.ctx, _lib.u8ptr(ones), AH, AW),
                    lambda: lib.hq_set_mask(m.ctx, _lib.u8ptr(ones), AW, AH - 1),
                    lambda: lib.hq_set_mask(m.ctx, _lib.u8ptr(np.zeros(AW * AH, np.uint8)), AW, AH)):
            assert bad() == _lib.HQ_ERR_ARG
            assert m.maskInfo()[:2] == (n, n)  # the mask in force stays
        for none in (None, None, None, None), (None, C.byref(C.c_int64()), None, None):
            assert lib.hq_mask_info(m.ctx, *none) == _lib.HQ_OK
        assert lib.hq_mask_info(None, None, None, None, None) == _lib.HQ_ERR_ARG
        # Python: bool and 2-D masks, any integer dtype; None clears
        pals = pals_of(AK, 16)
        want = plain(m, pals)[0]
        for form in (good.astype(bool), good.reshape(-1).astype(np.int64) * -3, (good * 255).astype(np.uint8)):
            m.setMask(form)
            np.testing.assert_array_equal(u64(plain(m, pals)[0]), u64(want))
        for wrong in (good.astype(np.float32), good[:-1], good.T, good.reshape(1, AH, AW)):
            with pytest.raises(ValueError):
                m.setMask(wrong)
        m.setMask(None)
        assert m.maskInfo()[:2] == (AW * AH, AW * AH)
    finally:
        m.close()


def test_refusals_leave_outputs_and_state_untouched(gpu):
    lib = hq.load()
    pals, mask = pals_of(AK, 16), masks_for(AW, AH)["bernoulli"]
    amp = np.asarray(SAMP, np.float32)
    m = new_ctx(gpu, pixel_err=1)
    try:
        set_image(m, noise(AW, AH), AW)
        m.setMask(mask)
        plain(m, pals)

        def state():
            return ([m.getIndices(p) for p in range(AP)] + [m.getPixelErrors(p) for p in range(AP)] +
                    [m.clusterSums(AP, AK)[0]])

        held, path = state(), m.lastPath()
        assert path["sequence"] == 1 and path["cost_instance"] == "masked"
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
        p2 = pals.copy()
        assert lib.hq_repair_population(m.ctx, _lib.fptr(p2), AP, AK, 1, DELTA, -1, 1, _lib.dptr(costs), _lib.iptr(used),
                                        None) == _lib.HQ_ERR_UNSUPPORTED
        assert np.all(err == -7) and np.all(worst == -7.0) and np.all(costs == -7.0) and np.all(used == -7)
        np.testing.assert_array_equal(u32(p2), u32(pals))
        for a, b in zip(held, state()):
            np.testing.assert_array_equal(a, b)
        assert m.lastPath() == path  # no refused call enqueued a pass
        m.setMask(None)  # without a mask both answer
        assert lib.hq_cluster_errors(m.ctx, AP, AK, _lib.i64ptr(err), _lib.fptr(worst)) == _lib.HQ_OK
    finally:
        m.close()


@pytest.mark.parametrize("sa_device", [1, 0])
def test_search_refusals(gpu, sa_device):
    lib = hq.load()
    mask = masks_for(AW, AH)["bernoulli"]
    m = new_ctx(gpu, sa_device=sa_device)
    try:
        set_image(m, noise(AW, AH), AW)
        sw = hq.SWASA(population=AP, imax=100, seed=9, t0=0.05)
        params, h, ran = sw.params(), C.c_void_p(), C.c_int(-1)
        m.setMask(mask)
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
            assert lib.hq_search_set_repair(h, 0, -1) == _lib.HQ_OK
            _lib.check(lib.hq_search_run(h, 3, C.byref(ran)), m.ctx)
            assert ran.value == 3
            m.setMask(None)
            assert lib.hq_search_set_repair(h, 2, -1) == _lib.HQ_OK  # a period set without a mask ...
            m.setMask(mask)
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


# ---------------------------------------------------------------------------
# 11. Python surface
# ---------------------------------------------------------------------------
def test_find_best_quantization_and_quantization_with_a_mask(gpu):
    w, h, K = 64, 32, 4
    rgba, _, mask = two_tone_image(w, h)
    m = new_ctx(gpu)
    try:
        sw = hq.SWASA(population=2, imax=100, seed=4)
        best = {}
        for name, kw in (("masked", dict(mask=mask)), ("bool2d", dict(mask=mask.astype(bool))), ("plain", {}),
                         ("seeded", dict(mask=mask, init="mediancut", lloydSteps=2, lloydEvery=3))):
            best[name] = np.asarray(m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum,
                                                           iterations=10, **kw), np.float32)
            if name == "plain":
                assert m.maskInfo()[:2] == (w * h, w * h)  # setImage dropped the mask
                continue
            assert m.maskInfo()[:2] == (w * h // 2, w * h // 2)
            m.setOption("pixel_err", 1)
            costs, used = plain(m, best[name].reshape(1, -1))
            check_cost(m, mask, [m.bestError], used, name, delta=sw.delta)
            m.setOption("pixel_err", 0)
        np.testing.assert_array_equal(u32(best["masked"]), u32(best["bool2d"]))
        assert not np.array_equal(best["masked"], best["plain"])
        assert m.seedError >= m.bestError
        for kw in (dict(repairEvery=2), dict(repairSteps=1)):
            with pytest.raises(ValueError):
                m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum, iterations=2, mask=mask, **kw)
    finally:
        m.close()
    image = np.stack([rgba[:, 0], rgba[:, 1], rgba[:, 2]])
    q, pal, err = hq.quantization(image, w, K, hq.SWASA(population=2, imax=100, seed=4), device=gpu, iterations=10,
                                  mask=mask)
    assert q.shape == image.shape and np.isfinite(err) and pal.shape == (4 * K,)

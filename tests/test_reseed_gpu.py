"""GPU tests of the repair entry points (libhq's additions): hq_cluster_errors,
hq_repair_population and hq_search_set_repair, through the C ABI.  The checker of the
statistics is numpy (reseed_ref.py) on the library's own index and error images and the
test's own pixel array; every statistics assertion is exact equality (the statistics are
integers, the worst pixel a key maximum).  The device-resident repair iteration is
checked bit for bit against the host-driven one, which runs the public calls.
"""

import ctypes as C
import os

import numpy as np
import pytest

import c_oracle
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from hybridquantization_amd import _lib
from lloyd_ref import bits
from reseed_ref import cluster_errors_ref, merge_ref, reseed_ref, tied_maxima
from test_lloyd_gpu import blob_image, lattice_image, palettes

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def new_ctx(gpu, de=hq.deltaETypes.CIE76):
    m = pr.Context(de, device=gpu)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    return m


@pytest.fixture()
def ip(gpu):
    m = new_ctx(gpu)
    yield m
    m.close()


def golden(name):
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    img = g["rgb_u8"].astype(np.float32) / np.float32(255)
    rgba = o.inline_rgba(img[:, 0].copy(), img[:, 1].copy(), img[:, 2].copy())
    pals = np.ascontiguousarray(g["palettes"], np.float32)
    return rgba, int(g["w"]), int(g["h"]), pals.reshape(len(pals), -1), g["lab"].astype(np.float32)


def raw_errors(m, P, K):
    err = np.full((P, K, 4), -7, np.int64)
    worst = np.full((P, K, 4), -7, np.float32)
    rc = hq.load().hq_cluster_errors(m.ctx, P, K, _lib.i64ptr(err), _lib.fptr(worst))
    return rc, err, worst


def check_errors(m, pals, rgba, r0=0, r1=None):
    """clusterErrors of the population just evaluated on m (rows [r0, r1) of the image)
    against numpy on getIndices32 and getPixelErrors; the counts against clusterSums'."""
    P, K = pals.shape[0], pals.shape[1] // 4
    w = m.w
    px = rgba.reshape(-1, 4)[r0 * w:(None if r1 is None else r1 * w), :3]
    err, worst = m.clusterErrors(P, K)
    for p in range(P):
        idx, e = m.getIndices32(p)[:len(px)], m.getPixelErrors(p)[:len(px)]
        want, want_rgb = cluster_errors_ref(idx, e, px, pals[p].reshape(K, 4), pos0=r0 * w)
        np.testing.assert_array_equal(err[p], want, err_msg=f"P={P} K={K} p={p}")
        np.testing.assert_array_equal(bits(worst[p]), bits(want_rgb), err_msg=f"P={P} K={K} p={p}")
    np.testing.assert_array_equal(err[..., 1], m.clusterSums(P, K)[0][..., 3])
    assert np.all(err[..., 1].sum(1) == len(px))
    return err, worst


# ---------------------------------------------------------------------------
# 1. Statistics against the numpy restatement
# ---------------------------------------------------------------------------
STAT_CASES = {
    # w, h, K, P, options, dE type
    "193x131_p5": (193, 131, 16, 5, {}, "CIE76"),
    "k1_p1": (97, 53, 1, 1, {}, "CIE76"),
    "k256_p4": (97, 53, 256, 4, {}, "CIE76"),
    "k300_chunks": (97, 53, 300, 2, {}, "CIE76"),
    "k600_lists0": (97, 53, 600, 2, {"lists16": 0}, "CIE76"),
    "k600_lists2": (97, 53, 600, 2, {"lists16": 2}, "CIE76"),
    "k20000_wide": (64, 48, 20000, 2, {}, "CIE76"),
    "grid0": (97, 53, 64, 3, {"grid": 0}, "CIE76"),
    "planar": (97, 53, 16, 5, {"img_u8": 0}, "CIE76"),
    "generic_cost": (97, 53, 16, 2, {"cost_variant": 1}, "CIE76"),
    "de2000": (97, 53, 16, 3, {}, "CIEDE2000"),
}


@pytest.mark.parametrize("name", ["case_64x48_k16", "case_97x53_k64"])
def test_stats_on_the_golden_cases(ip, name):
    """A workgroup's span is 1024 pixels at these sizes (the launcher's smallest: whole steps
    of 256 quads), so 64 x 48 takes 3 workgroups per palette group and 97 x 53 takes 6: the
    flush's merge across workgroups -- add, add, max -- decides every colour's entry."""
    rgba, w, h, pals, lab = golden(name)
    ip.setOption("pixel_err", 1)
    ip.setImage(rgba.reshape(-1), lab.reshape(-1), w, ip.illum)
    ip.computeQuantizationErrorPopulation(pals, 2.0)
    err, _ = check_errors(ip, pals, rgba)
    assert np.any(err[..., 3] > 1024)  # a worst pixel from beyond the first workgroup's span


@pytest.mark.parametrize("case", list(STAT_CASES))
def test_stats_equal_numpy(gpu, case):
    """Every index width and argmin path (u8; u16 through per-chunk grids and the native
    lists; u32), P = 5 (a palette group of 4 and one of 1), both image forms, the generic
    cost path's error image, dE76 and CIEDE2000."""
    w, h, K, P, opts, de = STAT_CASES[case]
    m = new_ctx(gpu, getattr(hq.deltaETypes, de))
    try:
        m.setOption("pixel_err", 1)
        for name, v in opts.items():
            m.setOption(name, v)
        rgba, _ = lattice_image(w, h, seed=K + w)
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        pals = palettes(P, K, seed=5 * K + P)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        check_errors(m, pals, rgba)
    finally:
        m.close()


def test_both_image_forms_give_equal_outputs(ip):
    """A k/255 image through the packed bytes (rebuilt to k/255 in fp32) and through the
    planar floats: the same statistics and the same worst pixels, bit for bit."""
    w, h, K, P = 97, 53, 16, 5
    rgba, _ = lattice_image(w, h, seed=31)
    pals = palettes(P, K, seed=77)
    # a colour equal to a pixel: that pixel is not movable in either form
    pals[0, :3] = rgba[1234, :3]
    got = {}
    ip.setOption("pixel_err", 1)
    for img_u8 in (1, 0):
        ip.setOption("img_u8", img_u8)
        ip.setImage(rgba.reshape(-1), None, w, ip.illum)
        ip.computeQuantizationErrorPopulation(pals, 2.0)
        got[img_u8] = check_errors(ip, pals, rgba)
    np.testing.assert_array_equal(got[1][0], got[0][0])
    np.testing.assert_array_equal(bits(got[1][1]), bits(got[0][1]))


# ---------------------------------------------------------------------------
# 2. The tie rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("img_u8", [1, 0])
@pytest.mark.parametrize("A,B,c", [((79, 222, 108), (69, 211, 65), (104, 164, 140)),
                                   ((201, 31, 77), (31, 116, 250), (34, 98, 103))])
def test_lowest_position_wins_a_tie(ip, A, B, c, img_u8):
    """Two flat colours (rows 0 .. 23 A, 24 .. 47 B) under the palette (c, c): every pixel
    goes to colour 0 and is movable, and the rows further than the filter's half-width from
    the boundary have one dE, bit for bit -- the largest one in the A rows or the B rows.
    The worst pixel is the first of them."""
    w, h = 64, 48
    by = np.zeros((h, w, 3), np.int64)
    by[:h // 2], by[h // 2:] = A, B
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.reshape(-1, 3).astype(np.float32) / np.float32(255)
    pal = np.zeros((1, 8), np.float32)
    pal[0, 0:3] = pal[0, 4:7] = np.asarray(c, np.float32) / np.float32(255)
    f = o.design_filters()
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    _, parts = c_oracle.eval_palette(rgba, lab, pal.reshape(2, 4), f, w, return_parts=True)
    assert tied_maxima(parts["idx"], parts["err"], rgba[:, :3], pal, 0) >= 100
    ip.setOption("pixel_err", 1)
    ip.setOption("img_u8", img_u8)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    ip.computeQuantizationErrorPopulation(pal, 2.0)
    err, worst = check_errors(ip, pal, rgba)
    e = ip.getPixelErrors(0)
    ties = tied_maxima(ip.getIndices32(0), e, rgba[:, :3], pal, 0)
    print(f"device: {ties} tied maxima, the first at {err[0, 0, 3]}")
    assert ties >= 100
    assert err[0, 0, 3] == int(np.argmax(e)) and err[0, 0, 1] == w * h
    assert err[0, 1].tolist() == [0, 0, 0, -1] and not worst[0, 1].any()  # the duplicate: nothing


# ---------------------------------------------------------------------------
# 3. Shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("de,blocks", [("CIE76", ((0, 16), (16, 48), (48, 53))),
                                       ("CIEDE2000", ((0, 20), (20, 25), (25, 53)))])
def test_shards_add_and_merge_to_the_whole_image(gpu, de, blocks):
    """Three row blocks of the 97 x 53 case, one of 5 rows: shorter than the halo of 10.
    The statistics are exact functions of the stored per-pixel dE, so the shards' give the
    whole image's exactly where the shards' dE are the whole image's bit for bit: that is
    the cost kernels' property (hq_cost.hip, tile_item_to_grid) -- CIEDE2000 in every
    sharding, dE76 where a block starts on a multiple of the tile's 16 rows, a pixel then
    sitting at the same row of its tile.  Within each shard, whatever its rows, the
    statistics equal the restatement on that shard's own error image (check_errors)."""
    rgba, w, h, pals, lab = golden("case_97x53_k64")
    P, K = pals.shape[0], pals.shape[1] // 4
    ip = new_ctx(gpu, getattr(hq.deltaETypes, de))
    try:
        ip.setOption("pixel_err", 1)
        ip.setImage(rgba.reshape(-1), lab.reshape(-1), w, ip.illum)
        ip.computeQuantizationErrorPopulation(pals, 2.0)
        whole = check_errors(ip, pals, rgba)
    finally:
        ip.close()
    parts = []
    part = np.zeros(P * (1 + K), np.float64)
    for r0, r1 in blocks:
        sh = new_ctx(gpu, getattr(hq.deltaETypes, de))
        try:
            sh.setOption("pixel_err", 1)
            sh.setImage(rgba.reshape(-1), lab.reshape(-1), w, sh.illum, row_begin=r0, row_end=r1)
            _lib.check(hq.load().hq_eval_population_partial(sh.ctx, _lib.fptr(pals), P, K, _lib.dptr(part)), sh.ctx)
            parts.append(check_errors(sh, pals, rgba, r0, r1))
        finally:
            sh.close()
    err, worst = merge_ref(parts)
    np.testing.assert_array_equal(err, whole[0])
    np.testing.assert_array_equal(bits(worst), bits(whole[1]))
    wins = [int(np.sum((e[..., 3] >= 0) & (e[..., 3] == whole[0][..., 3]))) for e, _ in parts]
    assert all(n > 0 for n in wins), wins  # every shard holds some cluster's worst pixel


# ---------------------------------------------------------------------------
# 4. Refusals
# ---------------------------------------------------------------------------
def test_state_refusals(ip):
    w, h, K, P = 64, 48, 8, 2
    rgba, _ = lattice_image(w, h, seed=2)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pals = palettes(P, K, seed=1)
    ip.setOption("pixel_err", 1)
    assert raw_errors(ip, P, K)[0] == _lib.HQ_ERR_STATE  # before any evaluation
    ip.setOption("pixel_err", 0)
    ip.computeQuantizationErrorPopulation(pals, 2.0)
    rc, err, worst = raw_errors(ip, P, K)
    assert rc == _lib.HQ_ERR_STATE and np.all(err == -7) and np.all(worst == -7)
    ip.setOption("pixel_err", 1)  # on now, but off at that evaluation
    assert raw_errors(ip, P, K)[0] == _lib.HQ_ERR_STATE
    ip.computeQuantizationErrorPopulation(pals, 2.0)
    assert raw_errors(ip, P + 1, K)[0] == _lib.HQ_ERR_STATE
    assert raw_errors(ip, P, K + 1)[0] == _lib.HQ_ERR_STATE
    assert raw_errors(ip, P, K)[0] == _lib.HQ_OK
    lib = hq.load()
    assert lib.hq_cluster_errors(ip.ctx, P, K, None, None) == _lib.HQ_ERR_ARG
    sw = hq.SWASA(population=P, imax=100, seed=3)
    params = sw.params()
    s = C.c_void_p()
    _lib.check(lib.hq_search_create(ip.ctx, C.byref(params), K, sw.seed, C.byref(s)), ip.ctx)
    try:
        ran = C.c_int()
        _lib.check(lib.hq_search_run(s, 2, C.byref(ran)), ip.ctx)
        rc, err, worst = raw_errors(ip, P, K)
        assert rc == _lib.HQ_ERR_STATE and np.all(err == -7) and np.all(worst == -7)
    finally:
        lib.hq_search_destroy(s)
    ip.computeQuantizationErrorPopulation(pals, 2.0)  # an evaluation makes them available again
    check_errors(ip, pals, rgba)
    ip.setOption("slice_ranks", 2)
    part = np.zeros(P * (1 + K), np.float64)
    _lib.check(lib.hq_eval_population_partial(ip.ctx, _lib.fptr(pals), P, K, _lib.dptr(part)), ip.ctx)
    assert raw_errors(ip, P, K)[0] == _lib.HQ_ERR_UNSUPPORTED


def test_nan_errors_are_unsupported(gpu):
    """dE94 on the 97 x 53 golden case: the fp32 restatement of the reference's unclamped dH
    (oracle.ciede94_f32) has NaN pixels there, and so has the device (a NaN cost).  An inf
    palette colour on a dE76 context gives the same.  The call after a refusal works."""
    rgba, w, h, pals, lab = golden("case_97x53_k64")
    P, K = pals.shape[0], pals.shape[1] // 4
    f = o.design_filters()
    nan_px = 0
    for p in range(P):
        _, parts = c_oracle.eval_palette(rgba, lab, pals[p].reshape(K, 4), f, w, return_parts=True)
        nan_px += int(np.isnan(o.ciede94_f32(lab, o.candidate_scielab(parts["idx"], pals[p].reshape(K, 4), f, w, h))).sum())
    assert nan_px >= 1
    m = new_ctx(gpu, hq.deltaETypes.CIE94)
    try:
        m.setOption("pixel_err", 1)
        m.setImage(rgba.reshape(-1), lab.reshape(-1), w, m.illum)
        costs = m.computeQuantizationErrorPopulation(pals, 2.0)
        assert np.isnan(costs).any()
        rc, err, worst = raw_errors(m, P, K)
        assert rc == _lib.HQ_ERR_UNSUPPORTED and np.all(err == -7) and np.all(worst == -7)
    finally:
        m.close()
    m = new_ctx(gpu)
    try:
        m.setOption("pixel_err", 1)
        m.setImage(rgba.reshape(-1), lab.reshape(-1), w, m.illum)
        # a palette whose inf colour takes pixels (its only colour): their dE is not a number
        bad = np.array([[np.inf, 0.5, 0.5, 0]], np.float32)
        assert not np.isfinite(m.computeQuantizationErrorPopulation(bad, 2.0)[0])
        rc, err, worst = raw_errors(m, 1, 1)
        assert rc == _lib.HQ_ERR_UNSUPPORTED and np.all(err == -7) and np.all(worst == -7)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        check_errors(m, pals, rgba)
        # an inf colour next to finite ones is never the nearest: every dE is a number, no refusal
        bad = pals.copy()
        bad[1, 4 * 3 + 1] = np.inf
        m.computeQuantizationErrorPopulation(bad, 2.0)
        err, _ = check_errors(m, bad, rgba)
        assert err[1, 3, 1] == 0
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 5. The evaluated population is undisturbed
# ---------------------------------------------------------------------------
def test_the_evaluated_population_is_undisturbed(ip):
    w, h, K, P = 97, 53, 16, 5
    rgba, _ = lattice_image(w, h, seed=8)
    pals = palettes(P, K, seed=12)
    ip.setOption("pixel_err", 1)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    costs = ip.computeQuantizationErrorPopulation(pals, 2.0)

    def state():
        return ([ip.getIndices(p) for p in range(P)], [ip.getPixelErrors(p) for p in range(P)], ip.clusterSums(P, K))

    before = state()
    a = ip.clusterErrors(P, K)
    after = state()
    b = ip.clusterErrors(P, K)  # and a second call gives the same
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(before[2][0], after[2][0])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
    np.testing.assert_array_equal(ip.computeQuantizationErrorPopulation(pals, 2.0), costs)


# ---------------------------------------------------------------------------
# 6. Polish
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs():
    return blob_image(96, 64, seed=11)


def five_plus_three(by):
    """5 sensible colours (means of a crude split of the blob image) and 3 copies."""
    order = np.argsort(by.sum(1), kind="stable")
    pal = np.zeros((8, 4), np.float32)
    for i, part in enumerate(np.array_split(order, 5)):
        pal[i, :3] = (by[part].mean(0) / 255).astype(np.float32)
    pal[5:] = pal[:3]
    return pal.reshape(1, -1)


def hand_repair(ip, pals, steps, delta, max_moves=-1):
    """The loop hq_repair_population runs, spelt out with the public calls."""
    P, K = pals.shape[0], pals.shape[1] // 4
    ip.setOption("pixel_err", 1)
    cur = pals.copy()
    costs, used = ip.computeQuantizationErrorPopulation(cur, delta, return_used=True)
    hist = [(cur.copy(), costs.copy(), used.copy())]
    stats = []
    for _ in range(steps):
        err, worst = ip.clusterErrors(P, K)
        stats.append((err, worst))
        cur, moved = ip.reseedUnused(err, worst, cur, max_moves)
        if not moved.any():
            hist.append(hist[-1])
            continue
        costs, used = ip.computeQuantizationErrorPopulation(cur, delta, return_used=True)
        hist.append((cur.copy(), costs.copy(), used.copy()))
    ip.setOption("pixel_err", 0)
    return hist, stats


def test_repair_brings_back_every_unused_colour(ip, blobs):
    rgba, by = blobs
    w, K = 96, 8
    assert len(np.unique(by, axis=0)) >= 8  # so 8 colours can all be used
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pals = five_plus_three(by)
    hist, stats = hand_repair(ip, pals, 1, 2.0)
    assert hist[0][2].sum() == 5
    pal, costs, used, trace = ip.repairPopulation(pals, 1, 2.0, keep_best=False, return_trace=True)
    assert used.sum() == 8
    assert costs[0] < trace[0, 0]
    print(f"cost {trace[0, 0]!r} -> {costs[0]!r}")
    np.testing.assert_array_equal(bits(pal), bits(hist[1][0]))
    np.testing.assert_array_equal(costs, hist[1][1])
    np.testing.assert_array_equal(used, hist[1][2])
    np.testing.assert_array_equal(trace, np.stack([hh[1] for hh in hist]))
    want, moved = reseed_ref(stats[0][0], stats[0][1], pals)
    assert moved[0] == 3
    np.testing.assert_array_equal(bits(pal), bits(want))
    f = o.design_filters()
    ref = c_oracle.eval_palette(rgba, ip.getLabRef().reshape(-1, 4), want.reshape(K, 4), f, w)
    assert abs(costs[0] - ref) <= 1e-5 * abs(ref), (costs[0], ref)
    # the caller's option is back, and a second step finds nothing to move: the trace repeats
    assert hq.load().hq_get_pixel_errors(ip.ctx, 0, _lib.fptr(np.zeros(w * 64, np.float32))) == _lib.HQ_ERR_STATE
    pal2, costs2, _, trace2 = ip.repairPopulation(pals, 3, 2.0, keep_best=False, return_trace=True)
    np.testing.assert_array_equal(bits(pal2), bits(pal))
    np.testing.assert_array_equal(trace2, np.stack([trace[0], trace[1], trace[1], trace[1]]))
    # max_moves = 1 per step: three steps bring the three back one at a time
    hist1, _ = hand_repair(ip, pals, 3, 2.0, max_moves=1)
    pal3, costs3, used3, trace3 = ip.repairPopulation(pals, 3, 2.0, max_moves=1, keep_best=False, return_trace=True)
    np.testing.assert_array_equal(bits(pal3), bits(hist1[-1][0]))
    np.testing.assert_array_equal(trace3, np.stack([hh[1] for hh in hist1]))
    assert [int(hh[2].sum()) for hh in hist1] == [5, 6, 7, 8]


def test_repair_keep_best_refuses_a_step_that_raises_the_cost(ip, blobs):
    """delta = -2 pays for every unused colour, so the repair raises the cost: keep_best 1
    returns the input, keep_best 0 the repaired palette."""
    rgba, by = blobs
    ip.setImage(rgba.reshape(-1), None, 96, ip.illum)
    pals = five_plus_three(by)
    pal0, costs0, used0, trace0 = ip.repairPopulation(pals, 1, -2.0, keep_best=False, return_trace=True)
    assert trace0[1, 0] > trace0[0, 0] and used0.sum() == 8
    pal1, costs1, used1, trace1 = ip.repairPopulation(pals, 1, -2.0, keep_best=True, return_trace=True)
    np.testing.assert_array_equal(trace1, trace0)
    np.testing.assert_array_equal(bits(pal1), bits(pals))
    assert costs1[0] == trace0[0, 0] and used1.sum() == 5


def test_repair_of_a_median_cut_with_fewer_cells_than_colours(ip):
    """An image of 5 colour cells (each cell a few nearby colours) at K = 8: the median cut
    makes 5 colours and 3 copies, one repair step uses all 8."""
    w, h, K = 96, 64, 8
    rng = np.random.default_rng(3)
    centres = np.array([[20, 20, 20], [200, 40, 40], [40, 200, 40], [40, 40, 200], [220, 220, 220]])
    by = centres[rng.integers(0, 5, w * h)] + rng.integers(0, 4, (w * h, 3))
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    cells, den = ip.colorHistogram(5)
    seed, made = ip.medianCut(cells, 5, den, K)
    assert made == 5
    pals = seed.reshape(1, -1)
    hist, stats = hand_repair(ip, pals, 1, 2.0)
    pal, costs, used, trace = ip.repairPopulation(pals, 1, 2.0, return_trace=True)
    assert hist[0][2].sum() == 5 and used.sum() == 8
    assert costs[0] < trace[0, 0]
    np.testing.assert_array_equal(bits(pal), bits(reseed_ref(stats[0][0], stats[0][1], pals)[0]))
    np.testing.assert_array_equal(costs, hist[1][1])


def test_repair_scope_refusals(ip):
    w, h, K, P = 64, 48, 8, 2
    rgba, _ = lattice_image(w, h, seed=2)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum, row_begin=8, row_end=40)
    pals = np.ascontiguousarray(palettes(P, K, seed=1))
    costs = np.zeros(P)
    lib = hq.load()
    assert lib.hq_repair_population(ip.ctx, _lib.fptr(pals), P, K, 2, 2.0, -1, 1, _lib.dptr(costs), None,
                                    None) == _lib.HQ_ERR_STATE
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    assert lib.hq_repair_population(ip.ctx, _lib.fptr(pals), P, K, -1, 2.0, -1, 1, _lib.dptr(costs), None,
                                    None) == _lib.HQ_ERR_ARG
    assert lib.hq_repair_population(ip.ctx, _lib.fptr(pals), P, K, 0, 2.0, -1, 1, _lib.dptr(costs), None,
                                    None) == _lib.HQ_OK
    np.testing.assert_array_equal(costs, ip.computeQuantizationErrorPopulation(pals, 2.0))


# ---------------------------------------------------------------------------
# 7. Search
# ---------------------------------------------------------------------------
class Search:
    """hq_search_* through ctypes."""

    def __init__(self, m, K, sw):
        self.m, self.K, self.lib = m, K, hq.load()
        params = sw.params()
        self.h = C.c_void_p()
        _lib.check(self.lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(self.h)), m.ctx)
        pr.check_search(m, self.h, params.population, K)  # device-resident exactly when sa_device is 1

    def set_repair(self, every, max_moves=-1):
        return self.lib.hq_search_set_repair(self.h, every, max_moves)

    def set_lloyd(self, every):
        return self.lib.hq_search_set_lloyd(self.h, every)

    def run(self, n):
        ran = C.c_int(-5)
        _lib.check(self.lib.hq_search_run(self.h, n, C.byref(ran)), self.m.ctx)
        return ran.value

    def best(self):
        best = np.zeros(4 * self.K, np.float32)
        err, it = C.c_double(), C.c_int()
        _lib.check(self.lib.hq_search_best(self.h, _lib.fptr(best), C.byref(err), C.byref(it)), self.m.ctx)
        return best, err.value, it.value

    def close(self):
        self.lib.hq_search_destroy(self.h)


def sw_for(P, seed, imax=40):
    return hq.SWASA(population=P, imax=imax, seed=seed, t0=0.05)


def run_search(m, K, P, seed, device, repair=None, lloyd=0, moves=-1, runs=(17, 1, 22)):
    """-> the trajectory ((best, err, iteration) after every hq_search_run call)."""
    m.setOption("sa_device", device)
    s = Search(m, K, sw_for(P, seed))
    try:
        if repair is not None:
            assert s.set_repair(repair, moves) == _lib.HQ_OK, hq.load().hq_last_error(m.ctx)
        if lloyd:
            assert s.set_lloyd(lloyd) == _lib.HQ_OK
        out = []
        for n in runs:
            assert s.run(n) == n
            out.append(s.best())
            pr.check_search(m, s.h, P, K, ran=True)  # captured exactly when sa_graph is 1
        return out
    finally:
        s.close()


def assert_same_trajectory(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[1] == y[1] and x[2] == y[2]
        np.testing.assert_array_equal(bits(x[0]), bits(y[0]))


@pytest.mark.parametrize("opts", [{}, {"sa_graph": 1}, {"img_u8": 0}], ids=["default", "sa_graph", "planar"])
@pytest.mark.parametrize("every", [1, 3, 10])
@pytest.mark.parametrize("K", [8, 16])
def test_device_search_matches_host_driven(gpu, blobs, K, every, opts):
    """40 iterations in runs of (17, 1, 22): with every = 3 iteration 18 is a whole run of one
    repair iteration.  The blob image leaves colours of a random palette unused, so the
    repairs move colours (the plain search ends elsewhere)."""
    m = new_ctx(gpu)
    try:
        for name, v in opts.items():
            m.setOption(name, v)
        m.setImage(blobs[0].reshape(-1), None, 96, m.illum)
        host = run_search(m, K, 3, 21, 0, repair=every)
        dev = run_search(m, K, 3, 21, 1, repair=every)
        assert_same_trajectory(dev, host)
        assert host[-1][2] == 40
        plain = run_search(m, K, 3, 21, 1)
        assert plain[-1][1] != dev[-1][1]
        if not opts:  # with a k-means move on top (first) and a limit on the moves
            assert_same_trajectory(run_search(m, K, 3, 21, 1, repair=every, lloyd=1, moves=2),
                                   run_search(m, K, 3, 21, 0, repair=every, lloyd=1, moves=2))
    finally:
        m.close()


@pytest.mark.parametrize("lloyd", [0, 1])
def test_host_driven_matches_the_public_calls(gpu, blobs, lloyd):
    """The host-driven search against hq_swasa_search_host_lloyd with a refine callback made
    of the public calls: with a k-means move on top the move comes first."""
    K, P, every, iters = 8, 3, 3, 24
    m = new_ctx(gpu)
    try:
        m.setImage(blobs[0].reshape(-1), None, 96, m.illum)
        host = run_search(m, K, P, 33, 0, repair=every, lloyd=every if lloyd else 0, runs=(iters,))[0]
        delta = sw_for(P, 33).delta

        def refine(pal):
            flat = pal.reshape(P, -1).copy()
            if lloyd:
                m.computeQuantizationErrorPopulation(flat, delta)
                sums, den = m.clusterSums(P, K)
                flat = m.centroidsFromSums(sums, den, flat)
            m.setOption("pixel_err", 1)
            m.computeQuantizationErrorPopulation(flat, delta)
            err, worst = m.clusterErrors(P, K)
            m.setOption("pixel_err", 0)
            return m.reseedUnused(err, worst, flat)[0]

        hb, he, _ = sw_for(P, 33).search_host(
            K, lambda ps: m.computeQuantizationErrorPopulation(ps.reshape(P, -1), delta), iterations=iters,
            refine=refine, every=every)
        assert host[2] == iters and host[1] == he
        np.testing.assert_array_equal(bits(host[0]), bits(hb))
    finally:
        m.close()


def test_every_zero_is_the_plain_search(gpu, blobs):
    m = new_ctx(gpu)
    try:
        m.setImage(blobs[0].reshape(-1), None, 96, m.illum)
        for device in (1, 0):
            assert_same_trajectory(run_search(m, 8, 3, 5, device), run_search(m, 8, 3, 5, device, repair=0))
        # switched off between runs: the rest is plain iterations
        m.setOption("sa_device", 1)
        got = {}
        for device in (1, 0):
            m.setOption("sa_device", device)
            s = Search(m, 8, sw_for(3, 5))
            try:
                assert s.set_repair(2) == _lib.HQ_OK
                assert s.run(10) == 10
                assert s.set_repair(0) == _lib.HQ_OK
                assert s.run(10) == 10
                got[device] = [s.best()]
            finally:
                s.close()
        assert_same_trajectory(got[1], got[0])
    finally:
        m.close()


def test_launch_counts_of_a_repair_run(gpu, blobs):
    m = new_ctx(gpu)
    lib = hq.load()
    try:
        m.setImage(blobs[0].reshape(-1), None, 96, m.illum)
        s = Search(m, 8, sw_for(3, 2))
        try:
            lib.hq_profile_enable(m.ctx, 1)
            lib.hq_profile_reset(m.ctx)
            assert s.set_repair(3) == _lib.HQ_OK
            assert s.run(10) == 10
            got = {}
            for name in ("errsum", "reseed", "assign", "grid", "cost", "sa_step", "lloyd"):
                n = C.c_int64()
                _lib.check(lib.hq_profile_get(m.ctx, name.encode(), None, C.byref(n)), m.ctx)
                got[name] = n.value
            assert got == {"errsum": 3, "reseed": 3, "assign": 13, "grid": 13, "cost": 13, "sa_step": 10, "lloyd": 0}
        finally:
            s.close()
    finally:
        m.close()


def test_search_refusals(gpu, blobs):
    K, P = 8, 2
    rgba = blobs[0]
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, 96, m.illum)
        s = Search(m, K, sw_for(P, 4))
        try:
            assert s.set_repair(-1) == _lib.HQ_ERR_ARG
            assert s.set_repair(2) == _lib.HQ_OK
        finally:
            s.close()
        s = Search(m, 600, sw_for(P, 4))  # device-resident, chunked palettes
        try:
            assert s.set_repair(1) == _lib.HQ_ERR_UNSUPPORTED
            assert b"sa_device" in hq.load().hq_last_error(m.ctx)
            assert s.set_repair(0) == _lib.HQ_OK
        finally:
            s.close()
        m.setOption("sa_device", 0)  # host-driven: every K
        s = Search(m, 600, sw_for(P, 4))
        try:
            assert s.set_repair(1) == _lib.HQ_OK
            assert s.run(2) == 2
        finally:
            s.close()
        for device in (1, 0):  # a rank count above 1 (the palette slice of two ranks)
            m.setOption("sa_device", device)
            s = Search(m, K, sw_for(P, 4))
            try:
                m.setOption("slice_ranks", 2)
                assert s.set_repair(1) == _lib.HQ_ERR_UNSUPPORTED
            finally:
                m.setOption("slice_ranks", 1)
                s.close()
        m.setOption("sa_device", 1)
        m.setOption("shard_solo", 1)  # a row-block shard
        m.setImage(rgba.reshape(-1), None, 96, m.illum, row_begin=8, row_end=40)
        s = Search(m, K, sw_for(P, 4))
        try:
            assert s.set_repair(3) == _lib.HQ_ERR_STATE
            assert s.set_repair(0) == _lib.HQ_OK
        finally:
            s.close()
    finally:
        m.close()
    m = new_ctx(gpu, hq.deltaETypes.CIE94)
    try:
        m.setImage(rgba.reshape(-1), None, 96, m.illum)
        for device in (1, 0):
            m.setOption("sa_device", device)
            s = Search(m, K, sw_for(P, 4))
            try:
                assert s.set_repair(1) == _lib.HQ_ERR_UNSUPPORTED
            finally:
                s.close()
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 8. Quality
# ---------------------------------------------------------------------------
def test_repair_search_is_no_worse_than_the_plain_search(gpu, blobs):
    """The blob image and settings of DESIGN.md section 11's table (P = 3, seed 17, 60
    iterations); DESIGN.md section 13 holds the costs measured."""
    m = new_ctx(gpu)
    try:
        def run(**kw):
            sw = hq.SWASA(population=3, imax=60, seed=17)
            best = m.findBestQuantization(blobs[0].reshape(-1), None, 96, 8, sw, None, None, m.illum, iterations=60, **kw)
            assert m.iterations == 60
            _, used = m.computeQuantizationErrorPopulation(np.asarray(best, np.float32).reshape(1, -1), sw.delta,
                                                           return_used=True)
            return m.bestError, int(used.sum())

        rows = {"plain": run(), "repair1": run(repairEvery=1), "lloyd1": run(lloydEvery=1),
                "lloyd1+repair1": run(lloydEvery=1, repairEvery=1), "mediancut": run(init="mediancut"),
                "mediancut+repair1": run(init="mediancut", repairEvery=1),
                "plain+repairSteps1": run(repairSteps=1)}
        for name, (cost, n_used) in rows.items():
            print(f"{name}: cost {cost!r}, {n_used} of 8 colours used")
        assert rows["repair1"][0] <= rows["plain"][0]
        assert rows["repair1"][1] == 8
    finally:
        m.close()

"""GPU tests of the k-means entry points (libhq's additions): hq_cluster_sums,
hq_centroids_from_sums, hq_refine_population and the search polish, through the
C ABI.  The checker is numpy on the library's own index image and the test's own
pixel array; every sums assertion is exact equality (the sums are integers).
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from hybridquantization_amd import _lib
from lloyd_ref import DEN32, bits, centroids_ref, cluster_sums_ref, q32

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ip(gpu):
    m = pr.Context(hq.deltaETypes.CIE76, device=gpu)
    assert m.getOpenCLAvailable()
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    assert m.halfSize == 10
    m.illum = sp.illuminant
    yield m
    m.close()


def make_ctx(gpu):
    m = pr.Context(hq.deltaETypes.CIE76, device=gpu)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    return m


def lattice_image(w, h, seed):
    """k/255 image -> (rgba inline float32, bytes (n, 3))."""
    R, G, B = o.synthetic_image(w, h, seed=seed)
    by = np.stack([np.rint(c.astype(np.float64) * 255).astype(np.int64) for c in (R, G, B)], 1)
    return o.inline_rgba(R, G, B), by


def float_image(w, h, seed):
    """Off-lattice floats in [0, 1] with exact 0, exact 1 and values below 2^-9 (ties of
    q = RN(v 2^32) and a denormal among them)."""
    rng = np.random.default_rng(seed)
    v = rng.random((w * h, 3)).astype(np.float32)
    special = np.array([0.0, 1.0, 2.0 ** -33, 3 * 2.0 ** -33, 2.0 ** -10, 1.7e-5, 1e-40, 2.0 ** -9,
                        np.nextafter(np.float32(1), np.float32(0))], np.float32)
    pos = rng.choice(w * h * 3, 4 * len(special), replace=False)
    v.reshape(-1)[pos] = np.tile(special, 4)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = v
    assert not np.all(np.rint(v.astype(np.float64) * 255) / 255 == v)
    return rgba, q32(v)


def palettes(P, K, seed):
    return np.stack([o.synthetic_palette(K, seed + p).reshape(-1) for p in range(P)])


def check_sums(m, pals, px, n_own, den_want, used=None):
    """clusterSums of the population just evaluated on m against numpy on getIndices32."""
    P, K = pals.shape[0], pals.shape[1] // 4
    sums, den = m.clusterSums(P, K)
    assert den == den_want
    for p in range(P):
        idx = m.getIndices32(p)[:n_own]
        np.testing.assert_array_equal(sums[p], cluster_sums_ref(idx, px, K), err_msg=f"P={P} K={K} p={p}")
    assert np.all(sums[..., 3].sum(1) == n_own)
    if used is not None:
        np.testing.assert_array_equal(sums[..., 3] > 0, used != 0)
    return sums


# ---------------------------------------------------------------------------
# Sums and counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "planar", "float"])
@pytest.mark.parametrize("w,h", [(10, 10), (64, 48), (97, 53), (301, 173)])
def test_sums_equal_numpy(ip, w, h, form):
    """K in {1, 2, 16, 256} x P in {1, 4, 5} (5: a group of four and one of one) on a k/255
    image in both forms (img_u8 1: bytes, den 255; img_u8 0: q(v), den 2^32) and on an
    off-lattice float image."""
    if form == "float":
        rgba, px = float_image(w, h, seed=w + h)
    else:
        rgba, by = lattice_image(w, h, seed=w)
        px = by if form == "packed" else q32(rgba[:, :3])
    ip.setOption("img_u8", 1 if form == "packed" else 0)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    for K in (1, 2, 16, 256):
        for P in (1, 4, 5):
            pals = palettes(P, K, seed=3 * K + P)
            _, used = ip.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
            check_sums(ip, pals, px, w * h, 255 if form == "packed" else DEN32, used)


@pytest.mark.parametrize("case", ["k600_lists0", "k600_lists2", "k4096_native", "k20000_wide", "k256_grid0"])
def test_sums_on_every_index_width_and_argmin_path(ip, case):
    w, h, K, opts = {"k600_lists0": (97, 53, 600, {"lists16": 0}), "k600_lists2": (97, 53, 600, {"lists16": 2}),
                     "k4096_native": (128, 128, 4096, {}), "k20000_wide": (64, 48, 20000, {}),
                     "k256_grid0": (97, 53, 256, {"grid": 0})}[case]
    for name, v in opts.items():
        ip.setOption(name, v)
    rgba, by = lattice_image(w, h, seed=K)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pals = palettes(2, K, seed=K)
    _, used = ip.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
    check_sums(ip, pals, by, w * h, 255, used)
    ip.setOption("img_u8", 0)  # the same index images, the planar pixels
    check_sums(ip, pals, q32(rgba[:, :3]), w * h, DEN32, used)


# ---------------------------------------------------------------------------
# Shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("img_u8", [1, 0])
def test_shard_sums_add_up_to_the_whole_image(gpu, ip, img_u8):
    """Row blocks with blocks shorter than the halo (10 rows) and a one-row block: owned
    rows only, and the blocks' sums add up exactly to the unsharded context's."""
    w, h, K, P = 301, 173, 16, 5
    rgba, by = lattice_image(w, h, seed=7)
    px = by if img_u8 else q32(rgba[:, :3])
    den_want = 255 if img_u8 else DEN32
    pals = palettes(P, K, seed=40)
    ip.setOption("img_u8", img_u8)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    ip.computeQuantizationErrorPopulation(pals, 2.0)
    whole = check_sums(ip, pals, px, w * h, den_want)
    total = np.zeros_like(whole)
    lib = hq.load()
    part = np.zeros(P * (1 + K), np.float64)
    for r0, r1 in ((0, 7), (7, 60), (60, 61), (61, 173)):
        sh = make_ctx(gpu)
        try:
            sh.setOption("img_u8", img_u8)
            sh.setImage(rgba.reshape(-1), None, w, sh.illum, row_begin=r0, row_end=r1)
            _lib.check(lib.hq_eval_population_partial(sh.ctx, _lib.fptr(np.ascontiguousarray(pals)), P, K,
                                                      _lib.dptr(part)), sh.ctx)
            total += check_sums(sh, pals, px[r0 * w:r1 * w], w * (r1 - r0), den_want)
        finally:
            sh.close()
    np.testing.assert_array_equal(total, whole)


# ---------------------------------------------------------------------------
# Accumulator width
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("img_u8", [1, 0])
def test_all_white_megapixel(ip, img_u8):
    """2^20 pixels on one colour: the smallest shape at which a narrow packed LDS field or
    a missed flush shows."""
    w = h = 1024
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = 1.0
    pal = np.array([[1, 1, 1, 0, 0, 0, 0, 0]], np.float32)  # white, black
    ip.setOption("img_u8", img_u8)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    ip.computeQuantizationErrorPopulation(pal, 2.0)
    sums, den = ip.clusterSums(1, 2)
    one = 255 * 2 ** 20 if img_u8 else 2 ** 52
    assert den == (255 if img_u8 else DEN32)
    np.testing.assert_array_equal(sums[0], np.array([[one, one, one, 2 ** 20], [0, 0, 0, 0]], np.int64))


def test_all_white_megapixel_many_palettes(ip):
    """The planar form keeps its count in 16 bits above a 48-bit sum, which holds for the
    2^15 pixels a workgroup may cover.  256 palettes (64 groups) leave few workgroups per
    group: 2^20 pixels would come to 2^16 per workgroup without that cap, and the count of
    an all-white span would carry out of its field."""
    w = h = 1024
    P = 256
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = 1.0
    pal = np.tile(np.array([[1, 1, 1, 0, 0, 0, 0, 0]], np.float32), (P, 1))
    ip.setOption("img_u8", 0)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    ip.computeQuantizationErrorPopulation(pal, 2.0)
    sums, den = ip.clusterSums(P, 2)
    assert den == DEN32
    want = np.array([[2 ** 52, 2 ** 52, 2 ** 52, 2 ** 20], [0, 0, 0, 0]], np.int64)
    np.testing.assert_array_equal(sums, np.broadcast_to(want, (P, 2, 4)))


# ---------------------------------------------------------------------------
# Update rule
# ---------------------------------------------------------------------------
def test_update_rule_keeps_unused_colours(ip):
    """A palette with an exact duplicate (index 2 of 1), a colour far from every pixel
    (3) and a non-finite colour (4): none gets a pixel, all three keep their bits."""
    w, h, K = 64, 48, 8
    rng = np.random.default_rng(5)
    by = rng.integers(102, 154, (w * h, 3))  # channels in [0.4, 0.6]
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    pal = np.zeros((2, K, 4), np.float32)
    for p in range(2):
        pal[p, :, :3] = 0.4 + 0.2 * rng.random((K, 3))
        pal[p, 0, :3] = 0.5
        pal[p, 2] = pal[p, 1]
        pal[p, 3, :3] = [0.0, 1.0, 0.0]
        pal[p, 4, :3] = [np.nan, 0.5, 0.5]
    pal = pal.reshape(2, -1)
    got = {}
    for img_u8 in (1, 0):
        ip.setOption("img_u8", img_u8)
        ip.setImage(rgba.reshape(-1), None, w, ip.illum)
        _, used = ip.computeQuantizationErrorPopulation(pal, 2.0, return_used=True)
        assert np.all(used[:, 2:5] == 0) and np.all(used[:, 0] == 1)
        sums = check_sums(ip, pal, by if img_u8 else q32(rgba[:, :3]), w * h, 255 if img_u8 else DEN32, used)
        den = 255 if img_u8 else DEN32
        new = ip.centroidsFromSums(sums, den, pal)
        np.testing.assert_array_equal(bits(new), bits(centroids_ref(sums, den, pal)))
        n4, p4 = new.reshape(2, K, 4), pal.reshape(2, K, 4)
        np.testing.assert_array_equal(bits(n4[:, 2:5]), bits(p4[:, 2:5]))
        assert np.any(bits(n4[:, 0, :3]) != bits(p4[:, 0, :3]))  # colour 0 (0.5 grey) moved
        got[img_u8] = new
    # the two units give the same centroids up to their roundings: each q(v) within 2^-33
    # of v, each float rounding within 2^-25 of a value in [0, 1] -> at most 2 2^-24 apart
    ok = ~np.isnan(got[1])
    assert np.max(np.abs(got[1][ok].astype(np.float64) - got[0][ok].astype(np.float64))) <= 2 * 2.0 ** -24


# ---------------------------------------------------------------------------
# hq_refine_population
# ---------------------------------------------------------------------------
def blob_image(w, h, seed):
    """A few Gaussian colour blobs rounded to bytes."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(40, 216, (5, 3))
    which = rng.integers(0, 5, w * h)
    by = np.clip(np.rint(centres[which] + 12.0 * rng.standard_normal((w * h, 3))), 0, 255).astype(np.int64)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    return rgba, by


def hand_loop(ip, pals, steps, delta):
    """The loop hq_refine_population runs, spelt out with the three public calls."""
    P, K = pals.shape[0], pals.shape[1] // 4
    cur = pals.copy()
    costs, used = ip.computeQuantizationErrorPopulation(cur, delta, return_used=True)
    hist = [(cur.copy(), costs.copy(), used.copy())]
    for _ in range(steps):
        sums, den = ip.clusterSums(P, K)
        cur = ip.centroidsFromSums(sums, den, cur)
        costs, used = ip.computeQuantizationErrorPopulation(cur, delta, return_used=True)
        hist.append((cur.copy(), costs.copy(), used.copy()))
    return hist


def rgb_distortion(rgba, pal):
    """Float64 sum of squared RGB distances under nearest assignment."""
    x = rgba[:, None, :3].astype(np.float64)
    c = pal.reshape(-1, 4)[None, :, :3].astype(np.float64)
    return float(((x - c) ** 2).sum(2).min(1).sum())


@pytest.fixture(scope="module")
def blobs():
    return blob_image(96, 64, seed=11)


def test_refine_equals_the_hand_written_loop(ip, blobs):
    rgba, _ = blobs
    w, K, P, steps = 96, 8, 3, 4
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pals = palettes(P, K, seed=90)
    hist = hand_loop(ip, pals, steps, 2.0)
    pal, costs, used, trace = ip.refinePopulation(pals, steps, 2.0, keep_best=False, return_trace=True)
    np.testing.assert_array_equal(bits(pal), bits(hist[-1][0]))
    np.testing.assert_array_equal(costs, hist[-1][1])
    np.testing.assert_array_equal(used, hist[-1][2])
    np.testing.assert_array_equal(trace, np.stack([hh[1] for hh in hist]))
    # steps = 0 is hq_eval_population
    pal0, costs0, used0, trace0 = ip.refinePopulation(pals, 0, 2.0, keep_best=False, return_trace=True)
    np.testing.assert_array_equal(bits(pal0), bits(pals))
    np.testing.assert_array_equal(costs0, hist[0][1])
    np.testing.assert_array_equal(used0, hist[0][2])
    np.testing.assert_array_equal(trace0, hist[0][1][None, :])
    # k-means does not raise the RGB distortion, up to the argmin's documented tie band
    # (near_d2, DESIGN.md section 2: 1e-6 relative in d2, inside which the reference
    # distance may prefer the lower index)
    for p in range(P):
        d = [rgb_distortion(rgba, hh[0][p]) for hh in hist]
        print(f"palette {p}: RGB distortion per step {d}")
        for a, b in zip(d, d[1:]):
            assert b <= a * (1 + 2e-6)
        assert d[-1] < d[0]


def test_refine_keep_best(ip, blobs):
    rgba, _ = blobs
    w, K, P, steps = 96, 8, 3, 4
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pals = palettes(P, K, seed=90)
    hist = hand_loop(ip, pals, steps, 2.0)
    pal, costs, used, trace = ip.refinePopulation(pals, steps, 2.0, keep_best=True, return_trace=True)
    np.testing.assert_array_equal(trace, np.stack([hh[1] for hh in hist]))
    for p in range(P):
        s = int(np.argmin(trace[:, p]))  # (the first of equal minima)
        assert costs[p] == trace[s, p] == trace[:, p].min()
        assert costs[p] <= trace[0, p]
        np.testing.assert_array_equal(bits(pal[p]), bits(hist[s][0][p]))
        np.testing.assert_array_equal(used[p], hist[s][2][p])


# ---------------------------------------------------------------------------
# Error paths (return codes only)
# ---------------------------------------------------------------------------
def raw_sums(m, P, K):
    sums = np.full((P, K, 4), -7, np.int64)
    den = C.c_int64(-7)
    rc = hq.load().hq_cluster_sums(m.ctx, P, K, _lib.i64ptr(sums), C.byref(den))
    return rc, sums, den.value


def test_cluster_sums_state_errors(ip):
    w, h, K, P = 64, 48, 8, 2
    rgba, _ = lattice_image(w, h, seed=2)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    assert raw_sums(ip, P, K)[0] == _lib.HQ_ERR_STATE  # before any evaluation
    pals = palettes(P, K, seed=1)
    ip.computeQuantizationErrorPopulation(pals, 2.0)
    assert raw_sums(ip, P + 1, K)[0] == _lib.HQ_ERR_STATE
    assert raw_sums(ip, P, K + 1)[0] == _lib.HQ_ERR_STATE
    assert raw_sums(ip, P, K)[0] == _lib.HQ_OK
    lib = hq.load()
    sw = hq.SWASA(population=P, imax=100, seed=3)
    params = sw.params()
    s = C.c_void_p()
    _lib.check(lib.hq_search_create(ip.ctx, C.byref(params), K, sw.seed, C.byref(s)), ip.ctx)
    try:
        ran = C.c_int()
        _lib.check(lib.hq_search_run(s, 2, C.byref(ran)), ip.ctx)
        assert ran.value == 2
        rc, sums, den = raw_sums(ip, P, K)
        assert rc == _lib.HQ_ERR_STATE and den == -7 and np.all(sums == -7)
    finally:
        lib.hq_search_destroy(s)
    ip.computeQuantizationErrorPopulation(pals, 2.0)  # an evaluation makes them available again
    assert raw_sums(ip, P, K)[0] == _lib.HQ_OK


@pytest.mark.parametrize("bad", [np.nan, 1.5])
def test_planar_pixel_out_of_range_is_unsupported(ip, bad):
    w = h = 16
    rgba, _ = float_image(w, h, seed=4)
    rgba[100, 1] = bad
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pals = palettes(2, 8, seed=6)
    ip.computeQuantizationErrorPopulation(pals, 2.0)
    rc, sums, den = raw_sums(ip, 2, 8)
    assert rc == _lib.HQ_ERR_UNSUPPORTED
    assert den == -7 and np.all(sums == -7)  # outputs untouched


def test_refine_on_a_shard_is_a_state_error(ip):
    w, h, K, P = 64, 48, 8, 2
    rgba, _ = lattice_image(w, h, seed=2)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum, row_begin=8, row_end=40)
    pals = np.ascontiguousarray(palettes(P, K, seed=1))
    costs = np.zeros(P)
    rc = hq.load().hq_refine_population(ip.ctx, _lib.fptr(pals), P, K, 2, 2.0, 1, _lib.dptr(costs), None, None)
    assert rc == _lib.HQ_ERR_STATE


# ---------------------------------------------------------------------------
# Search polish
# ---------------------------------------------------------------------------
def test_find_best_quantization_with_lloyd_steps(ip, blobs):
    rgba, _ = blobs
    w, K = 96, 8

    def run(lloyd):
        sw = hq.SWASA(population=3, imax=60, seed=17)
        best = ip.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, ip.illum, iterations=60,
                                       lloydSteps=lloyd)
        return np.asarray(best, np.float32), ip.bestError, sw.delta

    plain, plain_err, delta = run(0)
    polished, err, _ = run(3)
    assert ip.bestErrorSA == plain_err  # the search itself is untouched
    assert err <= ip.bestErrorSA
    again = ip.computeQuantizationErrorPopulation(polished.reshape(1, -1), delta)[0]
    assert again == err
    print(f"SA {plain_err!r} -> polished {err!r}")

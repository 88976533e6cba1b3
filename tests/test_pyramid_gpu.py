"""GPU tests of hq_search_population and of the coarse-to-fine search built on it
(hybridquantization_amd.pyramid.pyramidSearch, quantization(pyramid=...)): libhq's additions.
Small images (96 x 64 blobs, 64 x 64 noise), K <= 16 (one K = 300 case for the chunked
layout), tens of iterations.  Nothing here asserts a time.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import path_ref as pr
from hybridquantization_amd import _lib, pyramid
from test_lloyd_gpu import blob_image

pytestmark = pytest.mark.gpu

W, H = 96, 64
DELTA = 2.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dbits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def new_ctx(gpu):
    m = pr.Context(hq.deltaETypes.CIE76, device=gpu)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.illum, m.sp = sp.illuminant, sp
    return m


@pytest.fixture()
def ip(gpu):
    m = new_ctx(gpu)
    yield m
    m.close()


@pytest.fixture(scope="module")
def blobs():
    return blob_image(W, H, seed=11)[0]


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(7)
    rgba = np.zeros((64 * 64, 4), np.float32)
    rgba[:, :3] = rng.integers(0, 256, (64 * 64, 3)).astype(np.float32) / np.float32(255)
    return rgba


def random_population(P, K, seed):
    rng = np.random.default_rng(seed)
    pop = np.zeros((P, K, 4), np.float32)
    pop[:, :, :3] = rng.random((P, K, 3), dtype=np.float32)
    return pop.reshape(P, 4 * K)


class Search:
    """hq_search_* through ctypes, with the population accessor."""

    def __init__(self, m, K, P, seed=17, imax=40, population=None):
        self.m, self.K, self.P, self.lib = m, K, P, hq.load()
        sw = hq.SWASA(population=P, imax=imax, seed=seed, t0=0.05)
        params = sw.params()
        self.h = C.c_void_p()
        pop = None if population is None else _lib.fptr(population)
        _lib.check(self.lib.hq_search_create_from(m.ctx, C.byref(params), K, sw.seed, pop, C.byref(self.h)), m.ctx)

    def run(self, n):
        ran = C.c_int(-5)
        _lib.check(self.lib.hq_search_run(self.h, n, C.byref(ran)), self.m.ctx)
        assert ran.value == n
        return self

    def best(self):
        best = np.zeros(4 * self.K, np.float32)
        err = C.c_double()
        _lib.check(self.lib.hq_search_best(self.h, _lib.fptr(best), C.byref(err), None), self.m.ctx)
        return best, err.value

    def population(self):
        return self.m.searchPopulation(self.h, self.P, self.K)

    def close(self):
        self.lib.hq_search_destroy(self.h)


def searched(m, rgba, w, K, P, device, graph=0, runs=(17, 6), population=None):
    """A search on a fresh image -> [(population, errors, best error) after creation and every run]."""
    m.setOption("sa_device", device)
    m.setOption("sa_graph", graph)
    m.setImage(rgba.reshape(-1), None, w, m.illum)
    s = Search(m, K, P, population=population)
    try:
        info = m.searchInfo(s.h)
        assert info["device_resident"] == bool(device)
        out = [s.population() + (s.best()[1],)]
        for n in runs:
            s.run(n)
            out.append(s.population() + (s.best()[1],))
        if device:
            assert m.searchInfo(s.h)["graph"] == bool(graph)
        return out
    finally:
        s.close()


# ---------------------------------------------------------------------------
# hq_search_population
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", [1, 0])
def test_population_after_creation_is_the_given_one(ip, blobs, device):
    P, K = 4, 12
    pop = random_population(P, K, 3)
    (colors, errors, best), = searched(ip, blobs, W, K, P, device, runs=(), population=pop)
    assert colors.shape == (P, 4 * K) and errors.shape == (P,)
    assert {r.tobytes() for r in bits(colors)} == {r.tobytes() for r in bits(pop)}  # the same colours as a set
    np.testing.assert_array_equal(bits(colors), bits(pop))                          # ... and in the order given
    want = ip.computeQuantizationErrorPopulation(pop, DELTA)
    np.testing.assert_array_equal(dbits(errors), dbits(want))
    assert best == errors.min()
    # errors may be NULL
    s = Search(ip, K, P, population=pop)
    try:
        only = np.zeros((P, 4 * K), np.float32)
        _lib.check(s.lib.hq_search_population(s.h, _lib.fptr(only), None), ip.ctx)
        np.testing.assert_array_equal(bits(only), bits(pop))
        assert s.lib.hq_search_population(s.h, None, None) == _lib.HQ_ERR_ARG
        assert s.lib.hq_search_population(None, _lib.fptr(only), None) == _lib.HQ_ERR_ARG
    finally:
        s.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_device_resident_population_equals_host_driven(gpu, blobs, graph):
    P, K = 4, 12
    a, b = new_ctx(gpu), new_ctx(gpu)
    try:
        dev = searched(a, blobs, W, K, P, 1, graph)
        host = searched(b, blobs, W, K, P, 0)
        moved = False
        for (c1, e1, b1), (c0, e0, b0) in zip(dev, host):
            np.testing.assert_array_equal(bits(c1), bits(c0))
            np.testing.assert_array_equal(dbits(e1), dbits(e0))
            assert b1 == b0 and e1.min() >= b1  # the best member may have been replaced since
            moved |= not np.array_equal(bits(c1), bits(dev[0][0]))
        assert moved  # (the runs changed the population: the comparison is not of two copies of the start)
    finally:
        a.close()
        b.close()


def test_chunked_population_is_plain(gpu, noise):
    """K = 300: two chunks of 256 on the device; the population comes back as [P][4K]."""
    P, K = 2, 300
    a, b = new_ctx(gpu), new_ctx(gpu)
    try:
        pop = random_population(P, K, 9)
        dev = searched(a, noise, 64, K, P, 1, runs=(5,), population=pop)
        assert a.lastPath()["nch"] == 2
        host = searched(b, noise, 64, K, P, 0, runs=(5,), population=pop)
        np.testing.assert_array_equal(bits(dev[0][0]), bits(pop))
        for (c1, e1, b1), (c0, e0, b0) in zip(dev, host):
            assert c1.shape == (P, 4 * K)
            np.testing.assert_array_equal(bits(c1), bits(c0))
            np.testing.assert_array_equal(dbits(e1), dbits(e0))
            assert np.all(c1.reshape(P, K, 4)[:, :, 3] == 0)
        # every colour within [0, 1]: no padding colour, no stale memory, came back with it
        assert np.all((dev[-1][0] >= 0) & (dev[-1][0] <= 1))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("device", [1, 0])
def test_a_search_created_from_the_returned_population(ip, blobs, device):
    P, K = 4, 12
    _, (colors, errors, best) = searched(ip, blobs, W, K, P, device, runs=(23,))
    assert errors.min() >= best
    (again, errors2, best2), = searched(ip, blobs, W, K, P, device, runs=(), population=colors)
    np.testing.assert_array_equal(bits(again), bits(colors))
    np.testing.assert_array_equal(dbits(errors2), dbits(errors))
    assert best2 == errors.min()


# ---------------------------------------------------------------------------
# pyramidSearch
# ---------------------------------------------------------------------------
def plain(m, rgba, w, K, sw, iterations, **kw):
    best = m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, m.sp.Ofilters, m.sp.absOfilters, m.illum,
                                  iterations=iterations, **kw)
    return best, m.bestError


def coarse_to_fine(m, rgba, w, K, sw, levels, **kw):
    best = hq.pyramidSearch(m, rgba.reshape(-1), w, K, sw, 72, 45.0, hq.Whitepoint.D65, levels=levels, **kw)
    return best, m.bestError


def test_one_level_is_find_best_quantization(gpu, blobs):
    K, n = 12, 30
    sw = hq.SWASA(population=4, imax=n, seed=17, t0=0.05)
    a, b = new_ctx(gpu), new_ctx(gpu)
    try:
        want, want_err = plain(a, blobs, W, K, sw, n)
        got, got_err = coarse_to_fine(b, blobs, W, K, sw, ((1, n),))
        np.testing.assert_array_equal(bits(got), bits(want))
        assert got_err == want_err and b.iterations == a.iterations == n
        assert b.levelErrors == [got_err]
    finally:
        a.close()
        b.close()


def test_the_same_call_twice_gives_the_same_bits(gpu, blobs):
    K = 12
    sw = hq.SWASA(population=4, imax=60, seed=5)
    out = []
    for _ in range(2):
        m = new_ctx(gpu)
        try:
            best, err = coarse_to_fine(m, blobs, W, K, sw, ((4, 20), (2, 20), (1, 10)), lloydEvery=5)
            out.append((best, err, list(m.levelErrors), m.seedError))
        finally:
            m.close()
    np.testing.assert_array_equal(bits(out[0][0]), bits(out[1][0]))
    assert out[0][1:] == out[1][1:]
    assert len(out[0][2]) == 3 and out[0][2][-1] == out[0][1] <= out[0][3]


def test_a_coarse_search_beats_the_random_start_at_full_resolution(gpu, blobs):
    """Robust quality: 40 iterations at half resolution, none at full resolution.  The full-
    resolution cost of what the coarse search hands over lies strictly below the best cost the
    plain search of the same seed holds at its creation, its random start.

    The level's search is the hybrid one (lloydEvery = 1, the setting of the library's quality
    examples on this image: scripts/fixed_timing.py, scripts/weights_timing.py) at t0 = 0.05, as
    every short search of this suite runs.  What is under test is the hand-over, so the level
    has to get somewhere in its 40 iterations, and annealing alone does not, at either
    resolution: with imax = 40 the first steps move every channel of every colour by up to
    0.37, and 40 such iterations at FULL resolution only go from 21.5 to 14.0 where k-means
    palettes cost about 4.  Measured with annealing alone (MI355X, K = 12, P = 4, seed 17): the
    coarse level lowers its own cost from 30.5 to 21.8 and hands over a population that costs
    24.189 at full resolution, above the random start's 21.537 -- the blob image draws every
    pixel's blob independently, a 2 x 2 box mixes blobs, and one random palette's cost differs
    by up to 9 between the two resolutions, as much as those 40 iterations gain."""
    K = 12
    sw = hq.SWASA(population=4, imax=40, seed=17, t0=0.05)
    a, b = new_ctx(gpu), new_ctx(gpu)
    try:
        _, start = plain(a, blobs, W, K, sw, 0)  # creation only: the random population's best
        best, err = coarse_to_fine(b, blobs, W, K, sw, ((2, 40), (1, 0)), lloydEvery=1)
        print(f"random start {start:.5f}, coarse result at full resolution {err:.5f}, level errors {b.levelErrors}")
        assert err < start
        assert b.iterations == 0 and b.seedError == err and len(b.levelErrors) == 2 and b.levelErrors[1] == err
        np.testing.assert_array_equal(bits(b.seedColors), bits(best))
        fresh = new_ctx(gpu)
        try:
            fresh.setImage(blobs.reshape(-1), None, W, fresh.illum)
            assert fresh.computeQuantizationErrorPopulation(best.reshape(1, -1), sw.delta)[0] == err
        finally:
            fresh.close()
    finally:
        a.close()
        b.close()


def region_mask():
    m = np.zeros((H, W), np.uint8)
    m[10:50, 20:81] = 1
    m[3, 5] = 1  # a lone pixel: its block must survive the reduction
    return m


FIXED = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 1]], np.float32)
CASES = {
    "mask": dict(mask=region_mask()),
    "weights": dict(weights=(np.arange(H * W).reshape(H, W) % 7 * 40).astype(np.uint8)),
    "fixed": dict(fixed=FIXED),
    "mediancut": dict(init="mediancut"),
    "all": dict(mask=region_mask(), fixed=FIXED, init="mediancut", lloydEvery=3),
}


@pytest.mark.parametrize("case", list(CASES))
def test_mask_weights_fixed_and_seed_run_through_every_level(ip, gpu, blobs, case):
    K, kw = 12, CASES[case]
    sw = hq.SWASA(population=3, imax=30, seed=3)
    held = np.array([[0.25, 0.5, 0.75, 0.0]], np.float32)
    ip.setFixedColors(held)
    best, err = coarse_to_fine(ip, blobs, W, K, sw, ((4, 12), (2, 8), (1, 6)), **kw)
    assert best.shape == (4 * K,) and np.isfinite(err) and len(ip.levelErrors) == 3
    np.testing.assert_array_equal(ip.fixedColors(), held)  # the context's own fixed colours are back
    if "fixed" in kw:
        np.testing.assert_array_equal(bits(best.reshape(K, 4)[:3, :3]), bits(FIXED))
        np.testing.assert_array_equal(bits(ip.seedColors.reshape(K, 4)[:3, :3]), bits(FIXED))
    else:  # the colours the context held apply on every level, as they do to any search
        np.testing.assert_array_equal(bits(best[:3]), bits(held[0, :3]))
    assert err <= ip.seedError
    # the reported error: a fresh evaluation of the returned palette under the same mask or weights
    fresh = new_ctx(gpu)
    try:
        fresh.setImage(blobs.reshape(-1), None, W, fresh.illum)
        if "mask" in kw:
            fresh.setMask(kw["mask"])
        if "weights" in kw:
            fresh.setWeights(kw["weights"])
        assert fresh.computeQuantizationErrorPopulation(best.reshape(1, -1), sw.delta)[0] == err
    finally:
        fresh.close()
    # ip itself is left on the full-resolution image with the region in force
    assert (ip.w, ip.h) == (W, H)
    n_full = ip.maskInfo()[0]
    assert n_full == (int(np.count_nonzero(kw["mask"])) if "mask" in kw else
                      int(np.count_nonzero(kw["weights"])) if "weights" in kw else W * H)


class NoContext(hq.ImageManipulation):
    def __init__(self, *a, **k):
        raise AssertionError("a context was created")

    def __del__(self):
        pass


def test_bad_levels_and_small_levels_raise_before_any_context(ip, blobs, monkeypatch):
    monkeypatch.setattr(pyramid, "ImageManipulation", NoContext)
    monkeypatch.setattr(pyramid, "ScielabProcessor", NoContext)  # (would set ip's filters)
    sw = hq.SWASA(population=3, imax=30, seed=3)
    rgb = blobs.reshape(-1)
    for bad in ((), ((2, 5),), ((1, 5), (1, 5)), ((2, 5), (4, 5), (1, 5)), ((2, 5), (2, 5), (1, 5)), ((17, 5), (1, 5)),
                ((0, 5), (1, 5)), ((2, -1), (1, 5)), ((2.5, 5), (1, 5)), ((2,), (1,)), 7, ((4, 5), (2, 5))):
        with pytest.raises(ValueError):
            hq.pyramidSearch(ip, rgb, W, 8, sw, 72, 45.0, hq.Whitepoint.D65, levels=bad)
    # an 8 x 8 image: below the halfSize 10 of the filters designed at 72 dpi, and its 4 x 4 reduction
    # below the halfSize 5 of those designed at 36 dpi
    tiny = np.zeros(4 * 8 * 8, np.float32)
    for small in (((1, 5),), ((2, 5), (1, 5))):
        with pytest.raises(ValueError, match="halfSize"):
            hq.pyramidSearch(ip, tiny, 8, 8, sw, 72, 45.0, hq.Whitepoint.D65, levels=small)
    with pytest.raises(ValueError, match="no filters"):  # 1 dpi: less than one sample per degree
        hq.pyramidSearch(ip, rgb, W, 8, sw, 16, 45.0, hq.Whitepoint.D65, levels=((16, 5), (1, 5)))
    # the refusals findBestQuantization has, made before anything runs
    one = np.ones((H, W), np.uint8)
    for kw in (dict(mask=one, weights=one), dict(mask=one, repairEvery=2), dict(weights=one, repairEvery=2),
               dict(init="kmeans"), dict(fixed=np.zeros((9, 3)))):
        with pytest.raises(ValueError):
            hq.pyramidSearch(ip, rgb, W, 8, sw, 72, 45.0, hq.Whitepoint.D65, levels=((2, 5), (1, 5)), **kw)
    with pytest.raises(ValueError):
        hq.quantization(None, W, 8, sw, pyramid=((2, 5),))
    with pytest.raises(ValueError):
        hq.quantization(None, W, 8, sw, pyramid=((2, 5), (1, 5)), iterations=3)


def test_level_contexts_are_closed_on_every_way_out(ip, blobs, monkeypatch):
    made = []

    class Counted(hq.ImageManipulation):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(pyramid, "ImageManipulation", Counted)
    sw = hq.SWASA(population=3, imax=30, seed=3)
    coarse_to_fine(ip, blobs, W, 8, sw, ((4, 3), (2, 3), (1, 3)))
    assert len(made) == 2 and not any(m.openCLAvailable for m in made)
    # a failure inside a level (an init of the wrong shape): its context is closed all the same
    del made[:]
    with pytest.raises(ValueError):
        coarse_to_fine(ip, blobs, W, 8, sw, ((2, 3), (1, 3)), init=np.zeros(5, np.float32))
    assert len(made) == 1 and not made[0].openCLAvailable
    assert ip.openCLAvailable


def test_quantization_routes_through_the_pyramid(gpu, blobs):
    K = 8
    sw = hq.SWASA(population=3, imax=30, seed=3)
    image = blobs[:, :3].T.copy()
    q, best, err = hq.quantization(image, W, K, sw, device=gpu, pyramid=((2, 10), (1, 5)))
    assert q.shape == (3, W * H) and best.shape == (4 * K,) and np.isfinite(err) and err > 0
    pal = best.reshape(K, 4)[:, :3]
    assert all(any(np.array_equal(px, c) for c in pal) for px in q.T[::97])  # the rendering uses the palette
    q2, best2, err2 = hq.quantization(image, W, K, sw, device=gpu, pyramid=((2, 10), (1, 5)),
                                      mask=region_mask(), fixed=FIXED)
    np.testing.assert_array_equal(bits(best2.reshape(K, 4)[:3, :3]), bits(FIXED))
    assert q2.shape == (3, W * H) and np.isfinite(err2)

"""GPU tests of the seeding entry points (libhq's additions), through the C ABI and the
mirror: hq_color_histogram against numpy on the test's own pixels (exact equality: the
sums are integers), hq_search_create_from device-resident against host-driven bit for
bit, and findBestQuantization(init="mediancut") against the numpy median cut.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from hybridquantization_amd import _lib
from lloyd_ref import bits as fbits
from seed_ref import DEN32, coord_byte, coord_float, histogram_ref, median_cut_ref, q32
from test_lloyd_gpu import blob_image, float_image, lattice_image, palettes

pytestmark = pytest.mark.gpu

BITS = (2, 3, 4, 5, 6)
BLOB_SEED_COST = 4.4947951799986186  # the CPU oracle's cost of the blob image's 5-bit median cut at K = 8


def make_ctx(gpu):
    m = pr.Context(hq.deltaETypes.CIE76, device=gpu)
    assert m.getOpenCLAvailable()
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    return m


@pytest.fixture()
def ip(gpu):
    m = make_ctx(gpu)
    yield m
    m.close()


def raw_hist(m, bits, ncells=None):
    """hq_color_histogram through ctypes -> (rc, cells, den); the outputs start at -7."""
    n = (1 << (3 * bits)) if ncells is None else ncells
    cells = np.full((n, 4), -7, np.int64)
    den = C.c_int64(-7)
    rc = hq.load().hq_color_histogram(m.ctx, bits, _lib.i64ptr(cells), C.byref(den))
    return rc, cells, den.value


def check_hist(m, coords_of, px, n_own, den_want):
    """Every bits: the histogram equals numpy's, its counts add to the owned pixels, and a
    second call gives identical bytes."""
    out = {}
    for bits in BITS:
        cells, den = m.colorHistogram(bits)
        assert den == den_want
        np.testing.assert_array_equal(cells, histogram_ref(coords_of(bits), px, bits), err_msg=f"bits={bits}")
        assert int(cells[:, 3].sum()) == n_own
        again, den2 = m.colorHistogram(bits)
        assert den2 == den and again.tobytes() == cells.tobytes()
        out[bits] = cells
    return out


# ---------------------------------------------------------------------------
# Histogram
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "planar", "float"])
@pytest.mark.parametrize("w,h", [(10, 10), (97, 53), (301, 173)])
def test_histogram_equals_numpy(ip, w, h, form):
    """A k/255 image packed (bytes, den 255), the same image with img_u8 0 (q(v), den 2^32, the
    cells of the packed form: the reference coordinates are the bytes' shifts in both), and
    an off-lattice float image with exact 0, exact 1, values below 2^-9 and a denormal."""
    if form == "float":
        rgba, px = float_image(w, h, seed=w + h)
        coords_of = lambda b: coord_float(rgba[:, :3], b)  # noqa: E731
    else:
        rgba, by = lattice_image(w, h, seed=w)
        px = by if form == "packed" else q32(rgba[:, :3])
        coords_of = lambda b: coord_byte(by, b)  # noqa: E731
    ip.setOption("img_u8", 1 if form == "packed" else 0)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    check_hist(ip, coords_of, px, w * h, 255 if form == "packed" else DEN32)


@pytest.mark.parametrize("img_u8", [1, 0])
def test_single_colour_image(ip, img_u8):
    """256 x 256 pixels of one colour: every wave takes the uniform-wave path, the worst case
    of same-address atomics otherwise.  One cell, exact."""
    w = h = 256
    by = np.tile(np.array([[128, 64, 200]], np.int64), (w * h, 1))
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    ip.setOption("img_u8", img_u8)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    px = by if img_u8 else q32(rgba[:, :3])
    got = check_hist(ip, lambda b: coord_byte(by, b), px, w * h, 255 if img_u8 else DEN32)
    for bits, cells in got.items():
        on = np.flatnonzero(cells[:, 3])
        assert len(on) == 1 and on[0] == ((128 >> (8 - bits)) << (2 * bits)) | ((64 >> (8 - bits)) << bits) | (
            200 >> (8 - bits))
        np.testing.assert_array_equal(cells[on[0]], np.append(px[0] * (w * h), w * h))


@pytest.mark.parametrize("img_u8", [1, 0])
def test_runs_of_uniform_steps(ip, img_u8):
    """2048 x 2048, the smallest square at which a workgroup's span holds more than one step
    of 256 quads on 256 CUs, so a wave keeps its sums across steps: one colour up to a pixel
    that is neither a step's nor a quad's first, another after it (a run that goes on, a run
    that ends on a mixed step, a run of the other cell)."""
    w = h = 2048
    n1 = w * 1029 + 522
    by = np.empty((w * h, 3), np.int64)
    by[:n1] = [128, 64, 200]
    by[n1:] = [7, 255, 0]
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    ip.setOption("img_u8", img_u8)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    px = by if img_u8 else q32(rgba[:, :3])
    for bits in (2, 5):
        cells, den = ip.colorHistogram(bits)
        assert den == (255 if img_u8 else DEN32)
        want = np.zeros_like(cells)
        for lo, hi in ((0, n1), (n1, w * h)):
            c = coord_byte(by[lo], bits)
            want[(c[0] << (2 * bits)) | (c[1] << bits) | c[2]] += np.append(px[lo] * (hi - lo), hi - lo)
        np.testing.assert_array_equal(cells, want)


@pytest.mark.parametrize("img_u8", [1, 0])
def test_two_colour_checkerboard(ip, img_u8):
    """Width 37, no multiple of 4: a thread's quad of 4 pixels straddles cells and rows."""
    w, h = 37, 29
    y, x = np.divmod(np.arange(w * h), w)
    two = np.array([[250, 3, 77], [12, 130, 255]], np.int64)
    by = two[(x + y) % 2]
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    ip.setOption("img_u8", img_u8)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    got = check_hist(ip, lambda b: coord_byte(by, b), by if img_u8 else q32(rgba[:, :3]), w * h,
                     255 if img_u8 else DEN32)
    assert all(np.count_nonzero(c[:, 3]) == 2 for c in got.values())


@pytest.mark.parametrize("img_u8", [1, 0])
def test_shard_histograms_add_up_to_the_whole_image(gpu, ip, img_u8):
    """Three row blocks of unequal heights, one shorter than the halo (10 rows): owned rows
    only, the same den, and the blocks' histograms add up exactly to the whole image's."""
    w, h = 301, 173
    rgba, by = lattice_image(w, h, seed=7)
    px = by if img_u8 else q32(rgba[:, :3])
    den_want = 255 if img_u8 else DEN32
    ip.setOption("img_u8", img_u8)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    whole = {b: ip.colorHistogram(b) for b in (2, 5, 6)}
    total = {b: np.zeros_like(whole[b][0]) for b in whole}
    for r0, r1 in ((0, 7), (7, 100), (100, 173)):
        sh = make_ctx(gpu)
        try:
            sh.setOption("img_u8", img_u8)
            sh.setImage(rgba.reshape(-1), None, w, sh.illum, row_begin=r0, row_end=r1)
            for b in whole:
                cells, den = sh.colorHistogram(b)
                assert den == den_want == whole[b][1]
                own = slice(r0 * w, r1 * w)
                np.testing.assert_array_equal(cells, histogram_ref(coord_byte(by[own], b), px[own], b))
                total[b] += cells
        finally:
            sh.close()
    for b in whole:
        np.testing.assert_array_equal(total[b], whole[b][0])
        np.testing.assert_array_equal(whole[b][0], histogram_ref(coord_byte(by, b), px, b))


def test_histogram_errors(gpu, ip):
    assert raw_hist(ip, 5)[0] == _lib.HQ_ERR_STATE  # no image
    w = h = 16
    rgba, _ = float_image(w, h, seed=4)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    assert raw_hist(ip, 5)[0] == _lib.HQ_OK
    for bits in (1, 7, 0, -2):
        rc, cells, den = raw_hist(ip, bits, ncells=1 << 21)
        assert rc == _lib.HQ_ERR_ARG and den == -7 and np.all(cells == -7)
    rgba[100, 1] = np.nan
    rgba[37, 2] = 1.5
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    for bits in BITS:
        rc, cells, den = raw_hist(ip, bits)
        assert rc == _lib.HQ_ERR_UNSUPPORTED
        assert den == -7 and np.all(cells == -7)  # outputs untouched


def test_histogram_leaves_the_evaluated_population_alone(ip):
    """A call between hq_eval_population and hq_cluster_sums: the sums, the index images and
    the next evaluation are what they are without it."""
    w, h, K, P = 97, 53, 16, 3
    rgba, _ = lattice_image(w, h, seed=3)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pals = palettes(P, K, seed=21)
    costs, used = ip.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
    sums, den = ip.clusterSums(P, K)
    idx = [ip.getIndices(p) for p in range(P)]
    ip.computeQuantizationErrorPopulation(pals, 2.0)
    for bits in (2, 5):
        ip.colorHistogram(bits)
    sums2, den2 = ip.clusterSums(P, K)
    assert den2 == den
    np.testing.assert_array_equal(sums2, sums)
    for p in range(P):
        np.testing.assert_array_equal(ip.getIndices(p), idx[p])
    costs2, used2 = ip.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
    np.testing.assert_array_equal(costs2, costs)
    np.testing.assert_array_equal(used2, used)


# ---------------------------------------------------------------------------
# A search that starts from a given population
# ---------------------------------------------------------------------------
class Search:
    """hq_search_* through ctypes; population None is hq_search_create."""

    def __init__(self, m, K, sw, population, create_from=True):
        self.m, self.K, self.lib = m, K, hq.load()
        params = sw.params()
        self.h = C.c_void_p()
        if create_from:
            pop = None if population is None else _lib.fptr(np.ascontiguousarray(population, np.float32))
            rc = self.lib.hq_search_create_from(m.ctx, C.byref(params), K, sw.seed, pop, C.byref(self.h))
        else:
            rc = self.lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(self.h))
        _lib.check(rc, m.ctx)
        pr.check_search(m, self.h, params.population, K)  # device-resident exactly when sa_device is 1

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


def seeded_population(m, P, K, bits=5):
    """Member 0: the median cut of the image on m; member 1: cyclic copies of its first 5
    colours (duplicates); the others random."""
    cells, den = m.colorHistogram(bits)
    cut, _ = m.medianCut(cells, bits, den, K)
    pop = np.stack([cut] + [o.synthetic_palette(K, 70 + p).reshape(-1) for p in range(1, P)])
    if P > 1:
        pop[1] = cut.reshape(K, 4)[np.arange(K) % min(K, 5)].reshape(-1)
    return np.ascontiguousarray(pop, np.float32)


def run_from(m, K, sw, pop, device, runs, every=0, create_from=True):
    """-> the best (colours, error, iteration) at creation and after each run."""
    m.setOption("sa_device", device)
    s = Search(m, K, sw, pop, create_from)
    try:
        if every:
            assert s.lib.hq_search_set_lloyd(s.h, every) == _lib.HQ_OK, m._lib.hq_last_error(m.ctx)
        out = [s.best()]
        for n in runs:
            assert s.run(n) == n
            out.append(s.best())
            pr.check_search(m, s.h, sw.params().population, K, ran=True)  # captured exactly when sa_graph is 1
        return out
    finally:
        s.close()


def assert_same_runs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[2] == y[2] and x[1] == y[1]
        np.testing.assert_array_equal(fbits(x[0]), fbits(y[0]))


SEEDED = [
    # K, P, w, h, every, options
    (16, 3, 64, 48, 0, {}),
    (600, 3, 97, 53, 0, {}),  # the chunked device search: 3 chunks of 256, the third padded
    (16, 3, 64, 48, 2, {}),
    (16, 3, 64, 48, 0, {"sa_graph": 1}),
]


@pytest.mark.parametrize("K,P,w,h,every,opts", SEEDED,
                         ids=[f"K{c[0]}-P{c[1]}-e{c[4]}-{'_'.join(f'{k}{v}' for k, v in c[5].items()) or 'default'}"
                              for c in SEEDED])
def test_seeded_device_search_matches_host_driven(ip, K, P, w, h, every, opts):
    """40 iterations in two hq_search_run calls from the same given population: the best
    palette, the best error and the iteration count at creation and after each run."""
    for name, v in opts.items():
        ip.setOption(name, v)
    rgba, _ = lattice_image(w, h, seed=9)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pop = seeded_population(ip, P, K)
    mk = lambda: hq.SWASA(population=P, imax=100, seed=5 + P, t0=0.05)  # noqa: E731
    host = run_from(ip, K, mk(), pop, 0, (17, 23), every)
    dev = run_from(ip, K, mk(), pop, 1, (17, 23), every)
    assert [x[2] for x in dev] == [0, 17, 40]
    assert_same_runs(dev, host)
    plain = run_from(ip, K, mk(), None, 1, (17, 23), every)
    assert plain[0][1] != dev[0][1]  # the given population took part


@pytest.mark.parametrize("K,w,h", [(16, 64, 48), (600, 97, 53)])
def test_seeded_with_the_draws_is_hq_search_create(ip, K, w, h):
    """The population the draws would give: the trajectory of hq_search_create on the device
    path, the best after each of three runs equal."""
    P, seed = 3, 23
    rgba, _ = lattice_image(w, h, seed=9)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    osw = o.Swasa(o.SwasaParams(population=P, imax=100, t0=0.05), seed)
    draws = np.stack([osw.generate_random_colors(K).reshape(-1) for _ in range(P)])
    mk = lambda: hq.SWASA(population=P, imax=100, seed=seed, t0=0.05)  # noqa: E731
    plain = run_from(ip, K, mk(), None, 1, (5, 1, 14), create_from=False)
    assert_same_runs(run_from(ip, K, mk(), draws, 1, (5, 1, 14)), plain)
    assert_same_runs(run_from(ip, K, mk(), None, 1, (5, 1, 14)), plain)  # NULL is hq_search_create itself
    assert_same_runs(run_from(ip, K, mk(), draws, 0, (5, 1, 14)), plain)


@pytest.mark.parametrize("device", [1, 0])
def test_creation_records_the_first_best_member(ip, device):
    """Before any run hq_search_best returns argmin_first's member of the given population
    (.w stored as 0) and its error is hq_eval_population's cost of it."""
    w, h, K, P = 64, 48, 16, 4
    rgba, _ = lattice_image(w, h, seed=9)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pop = seeded_population(ip, P, K)
    pop = pop[[2, 0, 3, 0]]  # the best member twice: the first of equal minima is member 1
    costs = ip.computeQuantizationErrorPopulation(pop, 2.0)
    m = o.argmin_first(list(costs))
    assert m == 1
    given = pop.copy()
    given[:, 3::4] = 5.0
    best, err, it = run_from(ip, K, hq.SWASA(population=P, imax=100, seed=3), given, device, ())[0]
    assert it == 0 and err == costs[m]
    np.testing.assert_array_equal(fbits(best), fbits(pop[m]))
    # a channel outside [0, 1] or not finite is refused
    for bad in (np.nan, -0.1, 1.5):
        wrong = pop.copy()
        wrong[2, 4 * 7 + 1] = bad
        params = hq.SWASA(population=P, imax=100, seed=3).params()
        handle = C.c_void_p()
        rc = hq.load().hq_search_create_from(ip.ctx, C.byref(params), K, 3, _lib.fptr(wrong), C.byref(handle))
        assert rc == _lib.HQ_ERR_ARG and not handle.value


# ---------------------------------------------------------------------------
# findBestQuantization(init=...)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs():
    return blob_image(96, 64, seed=11)


def search(ip, rgba, **kw):
    sw = hq.SWASA(population=3, imax=60, seed=17)
    best = ip.findBestQuantization(rgba.reshape(-1), None, 96, 8, sw, None, None, ip.illum, iterations=60, **kw)
    return np.asarray(best, np.float32), ip.bestError


def test_init_mediancut_starts_from_the_median_cut(ip, blobs):
    rgba, by = blobs
    want, made = median_cut_ref(histogram_ref(coord_byte(by, 5), by, 5), 5, 255, 8)
    assert made == 8
    best, err = search(ip, rgba, init="mediancut")
    np.testing.assert_array_equal(fbits(ip.seedColors), fbits(want))
    cells, den = ip.colorHistogram(5)
    np.testing.assert_array_equal(fbits(ip.medianCut(cells, 5, den, 8)[0]), fbits(want))
    print(f"seedError {ip.seedError!r} (CPU oracle {BLOB_SEED_COST!r}), after 60 iterations {err!r}")
    assert abs(ip.seedError - BLOB_SEED_COST) <= 1e-4 * BLOB_SEED_COST
    assert err <= ip.seedError
    assert ip.computeQuantizationErrorPopulation(best.reshape(1, -1), 2.0)[0] == err
    # the palette as an array, (4K,) and (P, 4K): the same search
    for arr in (want, np.tile(want, (3, 1))):
        b2, e2 = search(ip, rgba, init=arr)
        assert e2 == err and ip.seedError == ip.computeQuantizationErrorPopulation(want.reshape(1, -1), 2.0)[0]
        np.testing.assert_array_equal(fbits(b2), fbits(best))
    # other histogram resolutions: another start
    _, _ = search(ip, rgba, init="mediancut", initBits=3)
    want3, _ = median_cut_ref(histogram_ref(coord_byte(by, 3), by, 3), 3, 255, 8)
    np.testing.assert_array_equal(fbits(ip.seedColors), fbits(want3))


def test_quality_on_the_blob_image(ip, blobs):
    """At the settings of the k-means tests (K = 8, P = 3, seed 17, 60 iterations): the seed
    alone, before an iteration has run, costs less than the plain search's best after 60.
    k-means lowers RGB distortion, not necessarily the S-CIELAB cost: the hybrid figures are
    reported, not asserted against each other."""
    rgba, _ = blobs
    _, plain = search(ip, rgba)
    _, seeded = search(ip, rgba, init="mediancut")
    seed_err = ip.seedError
    _, every1 = search(ip, rgba, init="mediancut", lloydEvery=1)
    assert ip.seedError == seed_err
    _, steps3 = search(ip, rgba, init="mediancut", lloydSteps=3)
    print(f"plain {plain!r}  seed {seed_err!r}  seeded {seeded!r}  seeded + lloydEvery=1 {every1!r}  "
          f"seeded + lloydSteps=3 {steps3!r}")
    assert seed_err < plain
    for e in (seeded, every1, steps3):
        assert e <= seed_err

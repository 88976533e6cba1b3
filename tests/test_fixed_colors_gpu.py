"""GPU tests of the fixed palette colours (libhq's addition): hq_set_fixed_colors through the
device-resident search (sa_step's select, the k-means and repair kernels' skips, the chunk
padding), the host-driven search, the creation's overwrite and latch, the two polishes and the
Python surface.  The device-resident search is checked bit for bit against the host-driven
one, which runs the public calls; the polishes against a step-by-step restatement through the
public calls.  Nothing here asserts a time.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from hybridquantization_amd import _lib
from test_lloyd_gpu import blob_image

pytestmark = pytest.mark.gpu

BLACK_WHITE_MAGENTA = np.array([[0, 0, 0, 0], [1, 1, 1, 0], [1, 0, 1, 0]], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def new_ctx(gpu, de=hq.deltaETypes.CIE76):
    m = pr.Context(de, device=gpu)
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
    return blob_image(96, 64, seed=11)[0]


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(7)
    rgba = np.zeros((64 * 64, 4), np.float32)
    rgba[:, :3] = rng.integers(0, 256, (64 * 64, 3)).astype(np.float32) / np.float32(255)
    return rgba


class Search:
    """hq_search_* through ctypes."""

    def __init__(self, m, K, P, seed=17, imax=40, population=None):
        self.m, self.K, self.lib = m, K, hq.load()
        sw = hq.SWASA(population=P, imax=imax, seed=seed, t0=0.05)
        params = sw.params()
        self.h = C.c_void_p()
        pop = None if population is None else _lib.fptr(population)
        self.rc = self.lib.hq_search_create_from(m.ctx, C.byref(params), K, sw.seed, pop, C.byref(self.h))

    def run(self, n):
        ran = C.c_int(-5)
        _lib.check(self.lib.hq_search_run(self.h, n, C.byref(ran)), self.m.ctx)
        return ran.value

    def best(self):
        best = np.zeros(4 * self.K, np.float32)
        err, it = C.c_double(), C.c_int()
        _lib.check(self.lib.hq_search_best(self.h, _lib.fptr(best), C.byref(err), C.byref(it)), self.m.ctx)
        return best.reshape(self.K, 4), err.value, it.value

    def close(self):
        self.lib.hq_search_destroy(self.h)


def run_search(m, K, P, device, lloyd=0, repair=0, moves=-1, ordered=None, runs=(17, 1, 22), imax=40, population=None,
               after_create=None, resident=None):
    """A search on m under the fixed colours m holds -> (best (K, 4), error, iteration) after every run."""
    m.setOption("sa_device", device)
    s = Search(m, K, P, imax=imax, population=population)
    assert s.rc == _lib.HQ_OK, hq.load().hq_last_error(m.ctx)
    try:
        info = m.searchInfo(s.h)
        assert info["device_resident"] == bool(device)
        if resident is not None:
            assert info == {"device_resident": True, "nch": resident, "graph": False}
        if after_create is not None:
            after_create()
        if ordered is not None:
            _lib.check(s.lib.hq_search_set_ordered(s.h, _lib.fptr(np.full(3, ordered, np.float32))), m.ctx)
        if lloyd:
            _lib.check(s.lib.hq_search_set_lloyd(s.h, lloyd), m.ctx)
        if repair:
            _lib.check(s.lib.hq_search_set_repair(s.h, repair, moves), m.ctx)
        out = [s.best()]
        for n in runs:
            assert s.run(n) == n
            out.append(s.best())
        if device:
            assert m.searchInfo(s.h)["graph"] == bool(m.options.get("sa_graph", 0))
        return out
    finally:
        s.close()


def assert_same_trajectory(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[1] == y[1] and x[2] == y[2], (x[1:], y[1:])
        np.testing.assert_array_equal(bits(x[0]), bits(y[0]))


def assert_fixed_throughout(traj, fixed):
    for best, _, _ in traj:
        np.testing.assert_array_equal(bits(best[:len(fixed)]), bits(fixed))


# ---------------------------------------------------------------------------
# 4. Device-resident equals host-driven
# ---------------------------------------------------------------------------
MODES = {
    "plain": dict(),
    "lloyd2": dict(lloyd=2),
    "repair3_all": dict(repair=3, moves=-1),
    "repair3_one": dict(repair=3, moves=1),
    "lloyd2_repair2": dict(lloyd=2, repair=2),
    "ordered": dict(ordered=0.2),
    "de2000": dict(),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_device_search_matches_host_driven(gpu, blobs, mode):
    """K = 8 with black, white and magenta fixed; 40 iterations in runs of (17, 1, 22).  Magenta
    is no pixel's nearest colour, so it stays unused and keeps paying delta: the repair moves must
    pass it over (it is colour 2, before every free colour) and the k-means move must leave it."""
    K, P = 8, 3
    m = new_ctx(gpu, hq.deltaETypes.CIEDE2000 if mode == "de2000" else hq.deltaETypes.CIE76)
    try:
        m.setImage(blobs.reshape(-1), None, 96, m.illum)
        m.setFixedColors(BLACK_WHITE_MAGENTA[:, :3])
        kw = MODES[mode]
        host = run_search(m, K, P, 0, **kw)
        dev = run_search(m, K, P, 1, **kw)
        assert_same_trajectory(dev, host)
        assert host[-1][2] == 40
        assert_fixed_throughout(dev, BLACK_WHITE_MAGENTA)
        assert dev[-1][1] < dev[0][1]  # (the free colours moved)
        best, err, _ = dev[-1]
        if mode == "ordered":
            costs, used = m.orderedPopulation(best.reshape(1, -1), 0.2, 2.0, return_used=True)
        else:
            costs, used = m.computeQuantizationErrorPopulation(best.reshape(1, -1), 2.0, return_used=True)
        print(f"{mode}: best error {err!r}, used {used[0].tolist()}")
        assert used[0, 2] == 0
        assert costs[0] == err
    finally:
        m.close()


def test_captured_run_matches_the_stream(gpu, blobs):
    """sa_graph 1 against 0 with both moves on: the captured launches' arguments carry n."""
    K, P = 8, 3
    m = new_ctx(gpu)
    try:
        m.setImage(blobs.reshape(-1), None, 96, m.illum)
        m.setFixedColors(BLACK_WHITE_MAGENTA)
        stream = run_search(m, K, P, 1, lloyd=2, repair=3)
        m.setOption("sa_graph", 1)
        graph = run_search(m, K, P, 1, lloyd=2, repair=3)
        assert_same_trajectory(graph, stream)
        assert_fixed_throughout(graph, BLACK_WHITE_MAGENTA)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 5. Chunked palettes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 260])
def test_chunked_device_search_matches_host_driven(gpu, noise, n):
    """K = 300 in two chunks of 256: n = 260 crosses the chunk boundary (the test is on the
    global colour index), and with colour 0 fixed the second chunk's padding is the member's
    colour 0 itself, as pack_chunks pads the host-driven form."""
    K, P = 300, 2
    rng = np.random.default_rng(n)
    fixed = np.zeros((n, 4), np.float32)
    fixed[:, :3] = rng.integers(0, 256, (n, 3)).astype(np.float32) / np.float32(255)
    m = new_ctx(gpu)
    try:
        m.setImage(noise.reshape(-1), None, 64, m.illum)
        m.setFixedColors(fixed)
        host = run_search(m, K, P, 0, runs=(12,))
        dev = run_search(m, K, P, 1, runs=(12,), resident=2)
        assert_same_trajectory(dev, host)
        assert dev[-1][2] == 12 and dev[-1][1] < dev[0][1]
        assert_fixed_throughout(dev, fixed)
        assert np.any(bits(dev[-1][0][n:]) != bits(dev[0][0][n:]))
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 6. Creation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", [1, 0])
def test_creation_overwrites_the_first_colours(ip, blobs, device):
    K, n = 8, 3
    ip.setImage(blobs.reshape(-1), None, 96, ip.illum)
    free = run_search(ip, K, 1, device, runs=())[0]
    ip.setFixedColors(BLACK_WHITE_MAGENTA)
    got = run_search(ip, K, 1, device, runs=())[0]
    np.testing.assert_array_equal(bits(got[0][n:]), bits(free[0][n:]))  # hq_search_create's draws
    np.testing.assert_array_equal(bits(got[0][:n]), bits(BLACK_WHITE_MAGENTA))
    assert got[1] == ip.computeQuantizationErrorPopulation(got[0].reshape(1, -1), 2.0)[0]
    # a given population: its first n colours are overwritten, the others are its own
    pop = np.ascontiguousarray(o.synthetic_palette(K, 3).reshape(1, -1), np.float32)
    given = run_search(ip, K, 1, device, runs=(), population=pop)[0]
    np.testing.assert_array_equal(bits(given[0][n:]), bits(pop.reshape(K, 4)[n:]))
    np.testing.assert_array_equal(bits(given[0][:n]), bits(BLACK_WHITE_MAGENTA))


@pytest.mark.parametrize("device", [1, 0])
def test_a_search_keeps_the_colours_it_was_created_with(ip, blobs, device):
    K, P = 8, 3
    ip.setImage(blobs.reshape(-1), None, 96, ip.illum)
    ip.setFixedColors(BLACK_WHITE_MAGENTA)
    kept = run_search(ip, K, P, device, lloyd=2, repair=3, runs=(20,))
    cleared = run_search(ip, K, P, device, lloyd=2, repair=3, runs=(20,), after_create=lambda: ip.setFixedColors(None))
    assert ip.fixedColors().shape == (0, 4)
    ip.setFixedColors(BLACK_WHITE_MAGENTA)
    changed = run_search(ip, K, P, device, lloyd=2, repair=3, runs=(20,),
                         after_create=lambda: ip.setFixedColors([[0.5, 0.5, 0.5]] * 5))
    assert_same_trajectory(cleared, kept)
    assert_same_trajectory(changed, kept)
    assert_fixed_throughout(cleared, BLACK_WHITE_MAGENTA)


# ---------------------------------------------------------------------------
# 7. Polishes
# ---------------------------------------------------------------------------
def start_palettes(rgba):
    """Two palettes of 8: colour 0 magenta (no pixel's nearest), five crude means of the image and
    two copies of colours 1 and 2 (unused: an equal colour at a lower index wins)."""
    px = rgba[:, :3]
    order = np.argsort(px.sum(1), kind="stable")
    pals = np.zeros((2, 8, 4), np.float32)
    for p in range(2):
        pals[p, 0, :3] = (1, 0, 1)
        for i, part in enumerate(np.array_split(order, 5 + p)[:5]):
            pals[p, 1 + i, :3] = px[part].mean(0)
        pals[p, 6:] = pals[p, 1:3]
    return np.ascontiguousarray(pals.reshape(2, -1))


def hand_refine(ip, pals, steps, delta, n):
    P, K = pals.shape[0], pals.shape[1] // 4
    cur = pals.copy()
    costs, used = ip.computeQuantizationErrorPopulation(cur, delta, return_used=True)
    trace = [costs.copy()]
    for _ in range(steps):
        sums, den = ip.clusterSums(P, K)
        nxt = ip.centroidsFromSums(sums, den, cur)
        nxt.reshape(P, K, 4)[:, :n] = cur.reshape(P, K, 4)[:, :n]  # the first n colours put back
        cur = nxt
        costs, used = ip.computeQuantizationErrorPopulation(cur, delta, return_used=True)
        trace.append(costs.copy())
    return cur, costs, used, np.stack(trace)


def hand_repair(ip, pals, steps, delta, n):
    P, K = pals.shape[0], pals.shape[1] // 4
    ip.setOption("pixel_err", 1)
    cur = pals.copy()
    costs, used = ip.computeQuantizationErrorPopulation(cur, delta, return_used=True)
    trace, moves = [costs.copy()], []
    for _ in range(steps):
        if moves and not moves[-1].any():  # the polish stops on a step that moved no colour
            trace.append(trace[-1])
            continue
        err, worst = ip.clusterErrors(P, K)
        cur, moved = ip.reseedUnused(err, worst, cur, -1, nfixed=n)
        moves.append(moved)
        if moved.any():
            costs, used = ip.computeQuantizationErrorPopulation(cur, delta, return_used=True)
        trace.append(costs.copy())
    ip.setOption("pixel_err", 0)
    return cur, costs, used, np.stack(trace), moves


@pytest.mark.parametrize("under", ["nothing", "mask", "weights"])
def test_refine_polish_equals_the_public_calls(ip, blobs, under):
    """The context's fixed VALUES are not used by a polish, only their count: the palettes' own
    first three colours (magenta among them, which has no pixels, and two that have) come back
    with their bits."""
    n = 3
    ip.setFixedColors(BLACK_WHITE_MAGENTA)
    ip.setImage(blobs.reshape(-1), None, 96, ip.illum)
    rng = np.random.default_rng(5)
    if under == "mask":
        ip.setMask(rng.integers(0, 2, (64, 96)))
    if under == "weights":
        ip.setWeights(rng.integers(0, 256, (64, 96)))
    pals = start_palettes(blobs)
    np.testing.assert_array_equal(ip.fixedColors(), BLACK_WHITE_MAGENTA)  # (setImage, setMask and setWeights keep them)
    want = hand_refine(ip, pals, 3, 2.0, n)
    pal, costs, used, trace = ip.refinePopulation(pals, 3, 2.0, keep_best=False, return_trace=True)
    np.testing.assert_array_equal(bits(pal), bits(want[0]))
    np.testing.assert_array_equal(costs, want[1])
    np.testing.assert_array_equal(used, want[2])
    np.testing.assert_array_equal(trace, want[3])
    np.testing.assert_array_equal(bits(pal.reshape(2, 8, 4)[:, :n]), bits(pals.reshape(2, 8, 4)[:, :n]))
    assert np.all(used[:, 1:3] == 1) and np.all(used[:, 0] == 0)  # fixed colours with pixels did not move either
    assert np.any(bits(pal.reshape(2, 8, 4)[:, n:6]) != bits(pals.reshape(2, 8, 4)[:, n:6]))
    best = ip.refinePopulation(pals, 3, 2.0, keep_best=True)[0]
    np.testing.assert_array_equal(bits(best.reshape(2, 8, 4)[:, :n]), bits(pals.reshape(2, 8, 4)[:, :n]))
    # without the state the same call moves them
    ip.setFixedColors(None)
    free = ip.refinePopulation(pals, 3, 2.0, keep_best=False)[0]
    assert np.any(bits(free.reshape(2, 8, 4)[:, 1:n]) != bits(pals.reshape(2, 8, 4)[:, 1:n]))
    if under != "nothing":  # the repair polish stays refused there, as without fixed colours
        ip.setFixedColors(BLACK_WHITE_MAGENTA)
        c = np.zeros(2)
        rc = hq.load().hq_repair_population(ip.ctx, _lib.fptr(pals.copy()), 2, 8, 2, 2.0, -1, 0, _lib.dptr(c), None, None)
        assert rc == _lib.HQ_ERR_UNSUPPORTED


def test_repair_polish_equals_the_public_calls(ip, blobs):
    """Unused: colour 0 (magenta, fixed) and the copies 6 and 7 (free).  Step 1 moves the two
    free ones onto the first two donors, magenta takes no donor; step 2 moves nothing and ends
    the loop, as without fixed colours, though an unused colour is left."""
    n = 3
    ip.setImage(blobs.reshape(-1), None, 96, ip.illum)
    pals = start_palettes(blobs)
    ip.setFixedColors(BLACK_WHITE_MAGENTA)
    want = hand_repair(ip, pals, 2, 2.0, n)
    assert [mv.tolist() for mv in want[4]] == [[2, 2], [0, 0]]
    pal, costs, used, trace = ip.repairPopulation(pals, 2, 2.0, keep_best=False, return_trace=True)
    np.testing.assert_array_equal(bits(pal), bits(want[0]))
    np.testing.assert_array_equal(costs, want[1])
    np.testing.assert_array_equal(used, want[2])
    np.testing.assert_array_equal(trace, want[3])
    assert used.sum(1).tolist() == [7, 7] and np.all(used[:, 0] == 0)
    np.testing.assert_array_equal(bits(pal.reshape(2, 8, 4)[:, :n]), bits(pals.reshape(2, 8, 4)[:, :n]))
    best = ip.repairPopulation(pals, 2, 2.0, keep_best=True)[0]
    np.testing.assert_array_equal(bits(best), bits(pal))
    # without the state magenta is the first receiver
    ip.setFixedColors(None)
    free, _, used_free = ip.repairPopulation(pals, 2, 2.0, keep_best=False)
    assert used_free.sum(1).tolist() == [8, 8]
    for p in range(2):
        assert np.any(bits(free.reshape(2, 8, 4)[p, 0]) != bits(pals.reshape(2, 8, 4)[p, 0]))


def test_more_fixed_colours_than_the_palette_has(ip, blobs):
    K, P = 8, 2
    ip.setImage(blobs.reshape(-1), None, 96, ip.illum)
    ip.setFixedColors(np.full((9, 3), 0.5))
    lib = hq.load()
    pals = start_palettes(blobs)
    c = np.zeros(P)
    for steps in (0, 2):
        assert lib.hq_refine_population(ip.ctx, _lib.fptr(pals), P, K, steps, 2.0, 0, _lib.dptr(c), None,
                                        None) == _lib.HQ_ERR_ARG
        assert lib.hq_repair_population(ip.ctx, _lib.fptr(pals), P, K, steps, 2.0, -1, 0, _lib.dptr(c), None,
                                        None) == _lib.HQ_ERR_ARG
    for device in (1, 0):
        ip.setOption("sa_device", device)
        s = Search(ip, K, P)
        assert s.rc == _lib.HQ_ERR_ARG and not s.h
    ip.setFixedColors(np.full((8, 3), 0.5))  # n = K: everything fixed, nothing to search, no error
    s = Search(ip, K, P)
    assert s.rc == _lib.HQ_OK
    s.close()
    # hq_set_fixed_colors' own refusals leave the colours in force
    for bad, nn in ((np.zeros((1, 4), np.float32), -1), (np.zeros((16385, 4), np.float32), 16385),
                    (np.array([[0, 1.5, 0, 0]], np.float32), 1), (np.array([[np.nan, 0, 0, 0]], np.float32), 1)):
        assert lib.hq_set_fixed_colors(ip.ctx, _lib.fptr(bad), nn) == _lib.HQ_ERR_ARG
        assert ip.fixedColors().shape == (8, 4)
    w = np.array([[0.25, 0.5, 0.75, 9.0]], np.float32)  # .w is ignored and stored as 0
    assert lib.hq_set_fixed_colors(ip.ctx, _lib.fptr(w), 1) == _lib.HQ_OK
    np.testing.assert_array_equal(ip.fixedColors(), [[0.25, 0.5, 0.75, 0.0]])


# ---------------------------------------------------------------------------
# 8. Nothing set is the library as it was
# ---------------------------------------------------------------------------
def test_set_and_cleared_is_a_fresh_context(gpu, blobs):
    K, P = 8, 3
    res = []
    for touched in (True, False):
        m = new_ctx(gpu)
        try:
            m.setImage(blobs.reshape(-1), None, 96, m.illum)
            if touched:
                m.setFixedColors(BLACK_WHITE_MAGENTA)
                m.setFixedColors(None)
            assert m.fixedColors().shape == (0, 4)
            pals = start_palettes(blobs)
            res.append((run_search(m, K, P, 1), run_search(m, K, P, 1, lloyd=2), run_search(m, K, P, 0, lloyd=2),
                        m.refinePopulation(pals, 3, 2.0, keep_best=False, return_trace=True)))
        finally:
            m.close()
    for i in range(3):
        assert_same_trajectory(res[0][i], res[1][i])
    for a, b in zip(res[0][3], res[1][3]):
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


# ---------------------------------------------------------------------------
# 9. Rank blocks and a single-rank communicator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["comm", "blocks"])
def test_sharded_layouts_equal_the_plain_context(gpu, layout):
    """The geometry of test_gpu.py's communicator and rank-block tests (80 x 72, where the plain
    search is the single context's bit for bit): a single-rank RCCL communicator with row blocks,
    and this context's counters as block 5 of 8."""
    K, P, w = 8, 3, 80
    R, G, B = o.synthetic_image(w, 72, seed=13)
    rgba = o.inline_rgba(R, G, B).reshape(-1)
    res = []
    for sharded in (False, True):
        m = new_ctx(gpu)
        try:
            m.setImage(rgba, None, w, m.illum)
            if sharded and layout == "comm":
                m.initComm(1, 0, hq.ImageManipulation.commUniqueId())
            if sharded and layout == "blocks":
                m.setOption("fold_blocks", 8)
                m.setOption("fold_block", 5)
            m.setFixedColors(BLACK_WHITE_MAGENTA)
            res.append(run_search(m, K, P, 1, runs=(10,), imax=25))
        finally:
            m.close()
    assert_same_trajectory(res[1], res[0])
    assert_fixed_throughout(res[1], BLACK_WHITE_MAGENTA)
    assert res[1][-1][2] == 10


# ---------------------------------------------------------------------------
# 10. The Python surface
# ---------------------------------------------------------------------------
def test_find_best_quantization_under_fixed_colours(ip, blobs):
    K = 8
    F = BLACK_WHITE_MAGENTA[:, :3]
    before = np.array([[0.25, 0.5, 0.75, 0.0]], np.float32)
    ip.setFixedColors(before)
    sw = hq.SWASA(population=3, imax=40, seed=17, t0=0.05)
    best = ip.sp.bestColors(blobs.reshape(-1), None, 96, K, sw, iterations=12, fixed=F, init="mediancut", lloydEvery=2,
                            lloydSteps=2, repairSteps=1)
    np.testing.assert_array_equal(bits(best.reshape(K, 4)[:3]), bits(BLACK_WHITE_MAGENTA))
    np.testing.assert_array_equal(bits(ip.seedColors.reshape(K, 4)[:3]), bits(BLACK_WHITE_MAGENTA))
    assert ip.bestError <= ip.bestErrorSA <= ip.seedError
    np.testing.assert_array_equal(ip.fixedColors(), before)
    # the cut is one of K - n colours
    cells, den = ip.colorHistogram(5)
    np.testing.assert_array_equal(bits(ip.seedColors[12:]), bits(ip.medianCut(cells, 5, den, K - 3)[0]))
    # n = K: no cut, nothing moves
    all_fixed = np.linspace(0, 1, 3 * K, dtype=np.float32).reshape(K, 3)
    best = ip.sp.bestColors(blobs.reshape(-1), None, 96, K, sw, iterations=3, fixed=all_fixed, init="mediancut")
    np.testing.assert_array_equal(bits(best.reshape(K, 4)[:, :3]), bits(all_fixed))
    # the dithered search goes through hq_swasa_search_host_fixed
    best = ip.sp.bestColors(blobs.reshape(-1), None, 96, K, sw, iterations=4, fixed=F, dither=1.0, ditherSearch=True)
    np.testing.assert_array_equal(bits(best.reshape(K, 4)[:3]), bits(BLACK_WHITE_MAGENTA))
    np.testing.assert_array_equal(ip.fixedColors(), before)
    # a ValueError from inside the call, after the state was set: the previous state is back
    with pytest.raises(ValueError):
        ip.sp.bestColors(blobs.reshape(-1), None, 96, K, sw, iterations=3, fixed=F, mask=np.ones((64, 96), np.uint8),
                         weights=np.ones((64, 96), np.uint8))
    np.testing.assert_array_equal(ip.fixedColors(), before)


def test_bad_fixed_colours_raise_before_anything_runs(gpu):
    m = new_ctx(gpu)  # no image: anything that ran would fail otherwise
    try:
        m.openCLFiltersReady = False
        sw = hq.SWASA(population=3, imax=40, seed=17)
        for bad in (np.zeros((2, 5)), np.zeros(7), [[0.0, 0.0, 1.5]], [[0.0, np.nan, 0.0]], np.zeros((9, 3))):
            with pytest.raises(ValueError):
                m.findBestQuantization(None, None, 96, 8, sw, None, None, None, fixed=bad)
            with pytest.raises(ValueError):
                hq.quantization(None, 96, 8, sw, device=gpu, fixed=bad)
            assert not m.openCLFiltersReady and m.fixedColors().shape == (0, 4)
        for bad in (np.zeros((2, 5)), [[0.0, 0.0, 1.5]]):
            with pytest.raises(ValueError):
                m.setFixedColors(bad)
    finally:
        m.close()

"""GPU tests of the search under the dot-diffused cost (hq_search_set_dot), after
test_ordered_gpu.py's section 6: the 48 x 40 noise image, K = 8, 30 iterations.  Device-resident,
captured ("sa_graph" 1), host-driven and split runs, and both forms of the rendering ("dot_tile" 0
and 1), agree bit for bit; strength 0 is the plain search; the best error is hq_dot_population's of
the best colours within 1e-6 relative (the bar of the folded accept step under the ordered cost);
the matrix is the search's own; the refusals; the Python surface.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import path_ref as pr
from dot_ref import random_classes
from hybridquantization_amd import _lib
from test_dither_gpu import new_ctx, noise, pals_of
from test_dot_gpu import matrix_of

pytestmark = pytest.mark.gpu

SW, SH, SK, S = 48, 40, 8, 1.0
PERM4 = random_classes(4, 44)
TILED = {"dot_tile": 1, "dot_tile_shape": 1}   # 16 x 16 tiles: 3 x 3 of them, the last row partial
CHAIN = {"dot_tile": 0}


def set_dot(h, cls, strength):
    mat = None if cls is None else matrix_of(cls)
    return hq.load().hq_search_set_dot(h, None if mat is None else C.byref(mat), strength)


def _search(gpu, Pn, strength, cls=None, runs=(30,), opts=None, probe=None, between=None, K=SK):
    """A search on the 48 x 40 noise image: hq_search_set_dot(cls, strength) (None: not called)
    before the first run, then the runs (between(m, h) after each but the last) -> (best colours,
    best error, iteration)."""
    lib = hq.load()
    m = new_ctx(gpu, **(opts or {}))
    try:
        m.setImage(noise(SW, SH, 11).reshape(-1), None, SW, m.illum)
        sw = hq.SWASA(population=Pn, imax=100, seed=9, t0=0.05)
        params, h = sw.params(), C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(h)), m.ctx)
        pr.check_search(m, h, Pn, K)  # device-resident exactly when sa_device is 1
        try:
            if strength is not None:
                _lib.check(set_dot(h, cls, strength), m.ctx)
            for i, n in enumerate(runs):
                ran = C.c_int()
                _lib.check(lib.hq_search_run(h, n, C.byref(ran)), m.ctx)
                assert ran.value == n
                if between and i + 1 < len(runs):
                    between(m, h)
            pr.check_search(m, h, Pn, K, ran=True)  # ... and captured exactly when sa_graph is 1
            best, err, it = np.zeros(4 * K, np.float32), C.c_double(), C.c_int()
            _lib.check(lib.hq_search_best(h, _lib.fptr(best), C.byref(err), C.byref(it)), m.ctx)
            if probe:
                probe(m, h, best, err.value)
            return best, err.value, it.value
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()


def _same_search(a, b, msg):
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32), err_msg=msg)
    assert a[1] == b[1] and a[2] == b[2], (msg, a[1:], b[1:])


@pytest.mark.parametrize("Pn", [3, 5])
def test_search_forms_agree_and_runs_compose(gpu, Pn):
    forms = []

    def reproduces(want_form):
        def probe(m, h, best, err):
            forms.append(m.dotForm()[0])
            assert forms[-1] == want_form  # (the search's own passes took this form)
            cost = m.dotPopulation(best.reshape(1, -1), S, 2.0)[0]
            print(f"P={Pn}: best_error {err!r}, hq_dot_population of the best colours {cost!r}")
            assert abs(cost - err) <= 1e-6 * err
        return probe

    dev = _search(gpu, Pn, S, opts=TILED, probe=reproduces(2))
    assert dev[2] == 30
    _same_search(dev, _search(gpu, Pn, S, opts=CHAIN, probe=reproduces(1)), "the chain")
    _same_search(dev, _search(gpu, Pn, S, opts={"sa_graph": 1, **TILED}), "sa_graph 1, tiled")
    _same_search(dev, _search(gpu, Pn, S, opts={"sa_graph": 1, **CHAIN}), "sa_graph 1, the chain")
    _same_search(dev, _search(gpu, Pn, S, opts={"sa_device": 0, **TILED}), "host-driven, tiled")
    _same_search(dev, _search(gpu, Pn, S, opts={"sa_device": 0, **CHAIN}), "host-driven, the chain")
    _same_search(dev, _search(gpu, Pn, S, runs=(10, 20), opts=TILED), "10 + 20 iterations")
    _same_search(dev, _search(gpu, Pn, S), "auto")
    plain = _search(gpu, Pn, None)
    assert not np.array_equal(plain[0], dev[0]) and plain[1] != dev[1]  # another objective, another search
    _same_search(plain, _search(gpu, Pn, 0.0), "strength 0")
    _same_search(plain, _search(gpu, Pn, 0.0, opts={"sa_device": 0}), "strength 0, host-driven")
    assert forms == [2, 1]


def test_the_matrix_is_the_searchs_own(gpu):
    """Another matrix gives another search; a hq_dot_population call under another matrix between
    two runs changes nothing in the search, and the getters answer for that call until the next run."""
    knuth = _search(gpu, 3, S, runs=(10, 20), opts=TILED)
    other = _search(gpu, 3, S, PERM4, runs=(10, 20), opts=TILED)
    assert not np.array_equal(knuth[0], other[0]) and knuth[1] != other[1]
    pals = pals_of(SK, 5)

    def foreign_call(m, h):
        costs = m.dotPopulation(pals, 0.5, 2.0, classes=PERM4)
        idx = [m.getIndices(p) for p in range(3)]
        fresh = new_ctx(gpu, **TILED)
        try:
            fresh.setImage(noise(SW, SH, 11).reshape(-1), None, SW, fresh.illum)
            np.testing.assert_array_equal(fresh.dotPopulation(pals, 0.5, 2.0, classes=PERM4), costs)
            for p in range(3):
                np.testing.assert_array_equal(fresh.getIndices(p), idx[p])  # (the live search did not reach it)
        finally:
            fresh.close()

    for opts in (TILED, CHAIN, {"sa_device": 0, **TILED}):
        _same_search(knuth, _search(gpu, 3, S, runs=(10, 20), opts=opts, between=foreign_call), f"{opts}")


@pytest.mark.parametrize("sa_device", [1, 0])
def test_search_refusals(gpu, sa_device):
    lib = hq.load()
    amp = np.asarray((0.5, 0.5, 0.5), np.float32)

    def exclusions(m, h, best, err):
        for setter in (lambda e: lib.hq_search_set_lloyd(h, e), lambda e: lib.hq_search_set_repair(h, e, -1)):
            assert setter(2) == _lib.HQ_OK
            assert set_dot(h, None, 1.0) == _lib.HQ_ERR_UNSUPPORTED
            assert set_dot(h, None, 0.0) == _lib.HQ_OK  # (off: nothing to refuse)
            assert setter(0) == _lib.HQ_OK
        # an ordered cost in force, and the converse: one rendering per search
        assert lib.hq_search_set_ordered(h, _lib.fptr(amp)) == _lib.HQ_OK
        assert set_dot(h, None, 1.0) == _lib.HQ_ERR_UNSUPPORTED
        assert lib.hq_search_set_ordered(h, None) == _lib.HQ_OK
        assert set_dot(h, None, 1.0) == _lib.HQ_OK
        assert lib.hq_search_set_ordered(h, _lib.fptr(amp)) == _lib.HQ_ERR_UNSUPPORTED
        assert lib.hq_search_set_ordered(h, None) == _lib.HQ_OK  # (zeros: nothing to refuse)
        # once it is on, a period is refused (0 is no period)
        assert lib.hq_search_set_lloyd(h, 2) == _lib.HQ_ERR_UNSUPPORTED
        assert lib.hq_search_set_repair(h, 2, -1) == _lib.HQ_ERR_UNSUPPORTED
        assert lib.hq_search_set_lloyd(h, 0) == _lib.HQ_OK and lib.hq_search_set_repair(h, 0, -1) == _lib.HQ_OK
        for bad in (-0.1, 1.5, float("nan")):
            assert set_dot(h, None, bad) == _lib.HQ_ERR_ARG
        illegal = matrix_of(PERM4)
        illegal.cls[0] = illegal.cls[1]
        assert lib.hq_search_set_dot(h, C.byref(illegal), 1.0) == _lib.HQ_ERR_ARG
        assert lib.hq_search_set_dot(None, None, 1.0) == _lib.HQ_ERR_ARG
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            assert set_dot(h, None, 0.5) == _lib.HQ_ERR_UNSUPPORTED
            m.setOption(name, 0 if name == "palette_split" else 1)
        ran = C.c_int()  # after the refusals the search still runs, under the cost last accepted
        assert lib.hq_search_run(h, 2, C.byref(ran)) == _lib.HQ_OK and ran.value == 2
        assert m.dotForm()[0] != 0 and m.lastPath()["argmin"] == "dot"

    _search(gpu, 3, None, runs=(2,), opts={"sa_device": sa_device}, probe=exclusions)


@pytest.mark.parametrize("sa_device", [1, 0])
def test_search_refuses_a_sharded_context(gpu, sa_device):
    """hq_dot_population's answer for a row-block shard, HQ_ERR_STATE in whole_image_only's words:
    from hq_search_set_dot, and from every hq_search_run of a search that has the cost on already
    (the scope is asked again at each run), which then runs nothing.  Back on the whole image the
    search goes on.  A communicator of more than one rank, the third condition of that row, needs
    more than one GPU and is not run here."""
    lib = hq.load()
    text = "sharded context: the whole image is needed for hq_dither_population (error diffusion)"
    rgba = noise(SW, SH, 11)

    def shard(m):
        m.setImage(rgba.reshape(-1), None, SW, m.illum, row_begin=8, row_end=24)

    def whole(m):
        m.setImage(rgba.reshape(-1), None, SW, m.illum)

    def probe(m, h, best, err):
        ran = C.c_int(-5)
        # 1. the cost is off: the call on a shard is refused and leaves the search plain
        shard(m)
        assert set_dot(h, None, 1.0) == _lib.HQ_ERR_STATE
        assert lib.hq_last_error(m.ctx).decode() == text
        whole(m)
        assert lib.hq_search_run(h, 2, C.byref(ran)) == _lib.HQ_OK and ran.value == 2
        assert m.lastPath()["argmin"] != "dot"
        # 2. the cost is on: a run on a shard is refused before anything is enqueued
        assert set_dot(h, None, 1.0) == _lib.HQ_OK
        assert lib.hq_search_run(h, 2, C.byref(ran)) == _lib.HQ_OK and ran.value == 2
        before = np.zeros(4 * SK, np.float32), C.c_double(), C.c_int()
        _lib.check(lib.hq_search_best(h, _lib.fptr(before[0]), C.byref(before[1]), C.byref(before[2])), m.ctx)
        shard(m)
        ran.value = -5
        assert lib.hq_search_run(h, 2, C.byref(ran)) == _lib.HQ_ERR_STATE and ran.value == 0
        assert lib.hq_last_error(m.ctx).decode() == text
        assert set_dot(h, PERM4, 0.5) == _lib.HQ_ERR_STATE  # (another matrix or strength: the same answer)
        after = np.zeros(4 * SK, np.float32), C.c_double(), C.c_int()
        _lib.check(lib.hq_search_best(h, _lib.fptr(after[0]), C.byref(after[1]), C.byref(after[2])), m.ctx)
        np.testing.assert_array_equal(before[0].view(np.uint32), after[0].view(np.uint32))
        assert before[1].value == after[1].value and before[2].value == after[2].value
        # 3. back on the whole image it runs again, under the dot-diffused cost
        whole(m)
        assert lib.hq_search_run(h, 2, C.byref(ran)) == _lib.HQ_OK and ran.value == 2
        assert m.lastPath()["argmin"] == "dot"
        _lib.check(lib.hq_search_best(h, None, None, C.byref(after[2])), m.ctx)
        assert after[2].value == before[2].value + 2

    _search(gpu, 3, None, runs=(2,), opts={"sa_device": sa_device}, probe=probe)


def test_search_refuses_an_image_outside_the_unit_range(gpu):
    lib = hq.load()
    m = new_ctx(gpu)
    try:
        rgba = noise(SW, SH, 11).copy()
        rgba[7, 1] = 1.25
        m.setImage(rgba.reshape(-1), None, SW, m.illum)
        sw = hq.SWASA(population=3, imax=100, seed=9)
        params, h = sw.params(), C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), SK, sw.seed, C.byref(h)), m.ctx)
        try:
            assert set_dot(h, None, 1.0) == _lib.HQ_ERR_UNSUPPORTED
            ran = C.c_int()
            assert lib.hq_search_run(h, 2, C.byref(ran)) == _lib.HQ_OK and ran.value == 2
            assert m.lastPath()["argmin"] != "dot"  # (still the plain search)
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()


def test_search_refuses_more_than_256_colours(gpu):
    lib = hq.load()
    m = new_ctx(gpu, sa_device=0)
    try:
        m.setImage(noise(SW, SH, 11).reshape(-1), None, SW, m.illum)
        sw = hq.SWASA(population=2, imax=100, seed=9)
        params, h = sw.params(), C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), 257, sw.seed, C.byref(h)), m.ctx)
        try:
            assert set_dot(h, None, 1.0) == _lib.HQ_ERR_UNSUPPORTED
            assert set_dot(h, None, 0.0) == _lib.HQ_OK
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()


def _find(m, rgba, w, K, **kw):
    sw = hq.SWASA(population=2, imax=100, seed=4)
    best = m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum, iterations=10, **kw)
    return np.asarray(best, np.float32), sw


def test_find_best_quantization_with_a_device_dot_search(gpu):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    found = {}
    for form in (0, 1):
        m = new_ctx(gpu, dot_tile=form, dot_tile_shape=1)
        try:
            best, sw = _find(m, rgba, w, K, dot=1.0, dotSearch="device")
            assert m.iterations == 10
            assert m.bestError == m.bestErrorDot == m.dotPopulation(best.reshape(1, -1), 1.0, sw.delta)[0]
            assert m.dotForm()[0] == 1 + form
            found[form] = best
            if form:
                plain, _ = _find(m, rgba, w, K, dot=1.0)
                assert not np.array_equal(plain, best)  # (the search did run under the other cost)
                with pytest.raises(ValueError):
                    _find(m, rgba, w, K, dotSearch="device")
                with pytest.raises(ValueError):
                    _find(m, rgba, w, K, dot=1.0, dotSearch="device", lloydEvery=2)
                with pytest.raises(ValueError):
                    _find(m, rgba, w, K, dot=1.0, dotSearch="host")
        finally:
            m.close()
    np.testing.assert_array_equal(found[0].view(np.uint32), found[1].view(np.uint32))


def test_quantization_passes_the_device_dot_search_through(gpu):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    image = np.stack([rgba[:, 0], rgba[:, 1], rgba[:, 2]])
    sw = hq.SWASA(population=2, imax=100, seed=4)
    _, best0, err0 = hq.quantization(image, w, K, sw, device=gpu, iterations=10, dot=1.0)
    q1, best1, err1 = hq.quantization(image, w, K, sw, device=gpu, iterations=10, dot=1.0, dotSearch="device")
    assert not np.array_equal(best0, best1)
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        want = m.quantizeDotDiffused(best1, 1.0).reshape(-1, 4)[:, :3].T
        assert err1 == m.dotPopulation(np.asarray(best1, np.float32).reshape(1, -1), 1.0, sw.delta)[0]
    finally:
        m.close()
    np.testing.assert_array_equal(q1, want)

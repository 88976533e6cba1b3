"""GPU tests of the hybrid search (hq_search_set_lloyd: a k-means move inside the SWASA
loop, libhq's addition).  The device-resident form -- assign-only pass, sums kernel,
lloyd_update_kernel, evaluation, no host round trip -- is checked bit for bit against
the host-driven form, which runs the public triple (hq_eval_population, hq_cluster_sums,
hq_centroids_from_sums) per hybrid iteration and is itself checked against a numpy
restatement on the oracle's loop.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from hybridquantization_amd import _lib
from lloyd_ref import bits, centroids_ref, cluster_sums_ref
from test_lloyd_gpu import blob_image, float_image, lattice_image

pytestmark = pytest.mark.gpu

W, H = 96, 64


def single_colour_image(w, h):
    by = np.tile(np.array([[128, 64, 200]], np.int64), (w * h, 1))
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    return rgba, by


@pytest.fixture(scope="module")
def images():
    return {"lattice": lattice_image(W, H, seed=9)[0], "float": float_image(W, H, seed=12)[0],
            "single": single_colour_image(W, H)[0]}


def new_ctx(gpu, de=hq.deltaETypes.CIE76):
    m = pr.Context(de, device=gpu)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    return m


class Search:
    """hq_search_* through ctypes."""

    def __init__(self, m, K, sw):
        self.m, self.K, self.lib = m, K, hq.load()
        params = sw.params()
        self.h = C.c_void_p()
        _lib.check(self.lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(self.h)), m.ctx)
        pr.check_search(m, self.h, params.population, K)  # device-resident exactly when sa_device is 1

    def set_lloyd(self, every):
        return self.lib.hq_search_set_lloyd(self.h, every)

    def run(self, n, check=True):
        ran = C.c_int(-5)
        rc = self.lib.hq_search_run(self.h, n, C.byref(ran))
        if check:
            _lib.check(rc, self.m.ctx)
        return rc, ran.value

    def best(self):
        best = np.zeros(4 * self.K, np.float32)
        err, it = C.c_double(), C.c_int()
        _lib.check(self.lib.hq_search_best(self.h, _lib.fptr(best), C.byref(err), C.byref(it)), self.m.ctx)
        return best, err.value, it.value

    def close(self):
        self.lib.hq_search_destroy(self.h)


def run_plan(m, K, P, seed, plan, device, imax=50):
    """plan: (every or None, iterations) per hq_search_run call -> (best, err, iteration, ran total)."""
    m.setOption("sa_device", device)
    s = Search(m, K, hq.SWASA(population=P, imax=imax, seed=seed, t0=0.05))
    try:
        total = 0
        for every, n in plan:
            if every is not None:
                assert s.set_lloyd(every) == _lib.HQ_OK, m._lib.hq_last_error(m.ctx)
            total += s.run(n)[1]
            pr.check_search(m, s.h, P, K, ran=True)  # captured exactly when sa_graph is 1
        return s.best() + (total,)
    finally:
        s.close()


def assert_same(a, b):
    assert a[2] == b[2] and a[3] == b[3]
    assert a[1] == b[1]
    np.testing.assert_array_equal(bits(a[0]), bits(b[0]))


# ---------------------------------------------------------------------------
# Device-resident equals host-driven
# ---------------------------------------------------------------------------
CASES = [
    # K, P, every, image, options, dE type
    (8, 3, 1, "lattice", {}, "CIE76"),
    (1, 1, 3, "lattice", {}, "CIE76"),
    (37, 5, 3, "float", {}, "CIE76"),          # P = 5: a centroid palette group of 4 + 1; den 2^32
    (256, 4, 1, "lattice", {}, "CIE76"),
    (256, 64, 3, "lattice", {}, "CIE76"),      # kSaMaxP
    (37, 64, 1, "float", {}, "CIE76"),
    (8, 1, 1, "float", {}, "CIE76"),
    (8, 3, 3, "lattice", {"img_u8": 0}, "CIE76"),  # a k/255 image through the planar sums
    (8, 5, 1, "single", {}, "CIE76"),          # the sums kernel's uniform-wave path; one colour moves
    (37, 3, 3, "single", {"img_u8": 0}, "CIE76"),
    (37, 3, 3, "lattice", {"grid": 0}, "CIE76"),
    (8, 3, 3, "float", {"cost_variant": 1}, "CIE76"),
    (8, 5, 3, "lattice", {"sa_graph": 1}, "CIE76"),
    (37, 4, 1, "float", {"sa_graph": 1}, "CIE76"),
    (8, 3, 1, "lattice", {}, "CIEDE2000"),
]


@pytest.mark.parametrize("K,P,every,image,opts,de", CASES,
                         ids=[f"K{c[0]}-P{c[1]}-e{c[2]}-{c[3]}-{'_'.join(f'{k}{v}' for k, v in c[4].items()) or 'default'}"
                              f"-{c[5]}" for c in CASES])
def test_device_search_matches_host_driven(gpu, images, K, P, every, image, opts, de):
    """Runs of (17, 1, 40) to imax = 50: with every = 3 iteration 18 is a whole run of one
    hybrid iteration, with every = 1 every run starts and ends on one."""
    m = new_ctx(gpu, getattr(hq.deltaETypes, de))
    try:
        for name, v in opts.items():
            m.setOption(name, v)
        m.setImage(images[image].reshape(-1), None, W, m.illum)
        plan = [(every, 17), (None, 1), (None, 40)]
        host = run_plan(m, K, P, 5 + P, plan, device=0)
        dev = run_plan(m, K, P, 5 + P, plan, device=1)
        assert host[2] == host[3] == 50
        assert_same(dev, host)
        plain = run_plan(m, K, P, 5 + P, [(None, 17), (None, 1), (None, 40)], device=1)
        assert plain[1] != dev[1]  # the k-means moves took part
        if image == "single":  # one colour takes every pixel and becomes it; the cost is then 0
            px = images[image][0, :3]
            assert np.any(np.all(dev[0].reshape(K, 4)[:, :3] == px, axis=1))
    finally:
        m.close()


# ---------------------------------------------------------------------------
# Host-driven equals a Python restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 5])
def test_host_driven_matches_numpy_restatement(gpu, every):
    w, h, K, P, imax, seed = 64, 48, 8, 3, 40, 23
    rgba, by = lattice_image(w, h, seed=3)
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        calls = [0]

        def oracle_eval(ps):
            n = calls[0]
            calls[0] += 1
            if n > 0 and n % every == 0:
                m.computeQuantizationErrorPopulation(ps, 2.0)  # the argmin of the candidates
                for p, pal in enumerate(ps):
                    sums = cluster_sums_ref(m.getIndices32(p), by, K)
                    pal[...] = centroids_ref(sums[None], 255, pal.reshape(1, -1)).reshape(K, 4)
            return list(m.computeQuantizationErrorPopulation(ps, 2.0))

        osw = o.Swasa(o.SwasaParams(population=P, imax=imax), seed)
        ob, oe = o.find_best_quantization(oracle_eval, K, osw)
        m.setOption("sa_device", 0)
        s = Search(m, K, hq.SWASA(population=P, imax=imax, seed=seed))
        try:
            assert s.set_lloyd(every) == _lib.HQ_OK
            assert s.run(imax)[1] == imax
            best, err, it = s.best()
        finally:
            s.close()
        assert it == imax and err == oe
        np.testing.assert_array_equal(bits(best.reshape(K, 4)), bits(ob))
    finally:
        m.close()


# ---------------------------------------------------------------------------
# `every` switched during a search
# ---------------------------------------------------------------------------
def test_every_switched_between_runs(gpu, images):
    K, P = 8, 3
    m = new_ctx(gpu)
    try:
        m.setImage(images["lattice"].reshape(-1), None, W, m.illum)
        plan = [(3, 10), (0, 10), (2, 5)]
        host = run_plan(m, K, P, 11, plan, device=0)
        dev = run_plan(m, K, P, 11, plan, device=1)
        assert_same(dev, host)
        # the tail of plain iterations is not that of a search that went on refining
        on = run_plan(m, K, P, 11, [(3, 10), (None, 10), (2, 5)], device=1)
        assert on[1] != dev[1] or not np.array_equal(on[0], dev[0])
        # never calling the setter is every = 0
        assert_same(run_plan(m, K, P, 11, [(None, 10), (None, 15)], device=1),
                    run_plan(m, K, P, 11, [(0, 10), (0, 15)], device=1))
        assert_same(run_plan(m, K, P, 11, [(None, 25)], device=0), run_plan(m, K, P, 11, [(0, 25)], device=0))
    finally:
        m.close()


# ---------------------------------------------------------------------------
# Launch counts
# ---------------------------------------------------------------------------
def test_launch_counts_of_a_hybrid_run(gpu, images):
    m = new_ctx(gpu)
    lib = hq.load()
    try:
        m.setImage(images["lattice"].reshape(-1), None, W, m.illum)
        s = Search(m, 8, hq.SWASA(population=3, imax=50, seed=2, t0=0.05))
        try:
            lib.hq_profile_enable(m.ctx, 1)
            lib.hq_profile_reset(m.ctx)
            assert s.set_lloyd(3) == _lib.HQ_OK
            assert s.run(10)[1] == 10
            got = {}
            for name in ("lloyd", "centroid", "assign", "grid", "cost", "sa_step"):
                ms, n = C.c_double(), C.c_int64()
                _lib.check(lib.hq_profile_get(m.ctx, name.encode(), C.byref(ms), C.byref(n)), m.ctx)
                got[name] = n.value
                assert ms.value > 0, name
            assert got == {"lloyd": 3, "centroid": 3, "assign": 13, "grid": 13, "cost": 10, "sa_step": 10}
            # a second run reuses the event slots: plain iterations there count nothing extra
            lib.hq_profile_reset(m.ctx)
            assert s.set_lloyd(0) == _lib.HQ_OK
            assert s.run(10)[1] == 10
            for name, want in (("lloyd", 0), ("centroid", 0), ("assign", 10)):
                n = C.c_int64()
                _lib.check(lib.hq_profile_get(m.ctx, name.encode(), None, C.byref(n)), m.ctx)
                assert n.value == want, name
        finally:
            s.close()
    finally:
        m.close()


# ---------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------
def test_device_search_of_chunked_palettes_is_refused_host_driven_runs(gpu):
    w, h, K, P = 64, 48, 600, 2
    rgba, _ = lattice_image(w, h, seed=5)
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        sw = hq.SWASA(population=P, imax=20, seed=4, t0=0.05)
        s = Search(m, K, sw)  # device-resident, chunked
        try:
            assert s.set_lloyd(1) == _lib.HQ_ERR_UNSUPPORTED
            assert b"sa_device" in hq.load().hq_last_error(m.ctx)
            assert s.set_lloyd(0) == _lib.HQ_OK
            assert s.run(2)[1] == 2
        finally:
            s.close()
        m.setOption("sa_device", 0)
        s = Search(m, K, sw)
        try:
            assert s.set_lloyd(1) == _lib.HQ_OK
            assert s.run(3)[1] == 3
            best, err, it = s.best()
        finally:
            s.close()

        def refine(pal):  # the hand-written k-means move: the three public calls
            flat = pal.reshape(P, -1)
            m.computeQuantizationErrorPopulation(flat, sw.delta)
            sums, den = m.clusterSums(P, K)
            return m.centroidsFromSums(sums, den, flat)

        hb, he, _ = hq.SWASA(population=P, imax=20, seed=4, t0=0.05).search_host(
            K, lambda ps: m.computeQuantizationErrorPopulation(ps.reshape(P, -1), sw.delta), iterations=3,
            refine=refine, every=1)
        assert it == 3 and err == he
        np.testing.assert_array_equal(bits(best), bits(hb))
    finally:
        m.close()


def test_scope_and_argument_refusals(gpu, images):
    K, P = 8, 2
    m = new_ctx(gpu)
    try:
        m.setImage(images["lattice"].reshape(-1), None, W, m.illum)
        s = Search(m, K, hq.SWASA(population=P, imax=50, seed=4))
        try:
            assert s.set_lloyd(-1) == _lib.HQ_ERR_ARG
            assert s.set_lloyd(2) == _lib.HQ_OK
            assert s.run(4)[1] == 4
            # hq_cluster_sums after a hybrid run: still a state error
            sums = np.zeros((P, K, 4), np.int64)
            den = C.c_int64()
            assert hq.load().hq_cluster_sums(m.ctx, P, K, _lib.i64ptr(sums), C.byref(den)) == _lib.HQ_ERR_STATE
        finally:
            s.close()
        # a row-block shard (searched alone under shard_solo)
        m.setOption("shard_solo", 1)
        m.setImage(images["lattice"].reshape(-1), None, W, m.illum, row_begin=8, row_end=40)
        s = Search(m, K, hq.SWASA(population=P, imax=50, seed=4))
        try:
            assert s.set_lloyd(3) == _lib.HQ_ERR_STATE
            assert s.set_lloyd(0) == _lib.HQ_OK
        finally:
            s.close()
    finally:
        m.close()


@pytest.mark.parametrize("device", [1, 0])
@pytest.mark.parametrize("bad", [np.nan, 1.5])
def test_planar_pixel_out_of_range_refuses_the_run(gpu, bad, device):
    w = h = 16
    rgba, _ = float_image(w, h, seed=4)
    rgba[100, 1] = bad
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        m.setOption("sa_device", device)
        s = Search(m, 8, hq.SWASA(population=2, imax=50, seed=4))
        try:
            assert s.set_lloyd(3) == _lib.HQ_OK
            assert s.run(2)[1] == 2  # no hybrid iteration in it
            before = s.best()
            for _ in range(2):  # (the second call takes the remembered verdict)
                rc, ran = s.run(5, check=False)
                assert rc == _lib.HQ_ERR_UNSUPPORTED and ran == 0
            after = s.best()
            assert after[2] == before[2] == 2
            np.testing.assert_array_equal(bits(after[0]), bits(before[0]))
            assert s.set_lloyd(0) == _lib.HQ_OK  # the plain search goes on
            assert s.run(5)[1] == 5
        finally:
            s.close()
    finally:
        m.close()


# ---------------------------------------------------------------------------
# Quality
# ---------------------------------------------------------------------------
def test_hybrid_search_beats_the_plain_search(gpu):
    """The blob image and settings of DESIGN.md section 11's table.  The CPU oracle's loop gives
    13.37 plain, 6.14 with a k-means move on every 10th iteration and 3.62 on every one."""
    rgba, _ = blob_image(96, 64, seed=11)
    m = new_ctx(gpu)
    try:
        def run(every):
            sw = hq.SWASA(population=3, imax=60, seed=17)
            m.findBestQuantization(rgba.reshape(-1), None, 96, 8, sw, None, None, m.illum, iterations=60,
                                   lloydEvery=every)
            assert m.iterations == 60
            return m.bestError

        plain, e10, e1 = run(0), run(10), run(1)
        print(f"best cost after 60 iterations: plain {plain!r}, lloydEvery=10 {e10!r}, lloydEvery=1 {e1!r}")
        assert e10 < plain
        assert e1 < plain
    finally:
        m.close()

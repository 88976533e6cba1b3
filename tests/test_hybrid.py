"""CPU checks of the hybrid search (a k-means move inside the SWASA loop, libhq's
addition): the host driver's policy through hq_swasa_search_host_lloyd against
the oracle's loop, and the update arithmetic the device kernel shares with
hq_centroids_from_sums.  No GPU needed."""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
from hybridquantization_amd import _lib
from lloyd_ref import DEN32, bits, centroids_ref


def cost(pal):
    """A cheap deterministic cost of one palette."""
    pal = np.asarray(pal, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    return float(np.sum((pal - 0.3) ** 2) + 0.01 * np.sum(np.sin(pal * 17)))


def snap(pal):
    """A cheap deterministic refine: every channel to the nearest multiple of 1/8,
    in place (exact in float32)."""
    v = pal[..., :3]
    v[...] = np.rint(v * np.float32(8)) / np.float32(8)


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("every", [1, 3, 7])
def test_host_policy_matches_the_oracle_loop(P, every):
    """oracle.find_best_quantization keeps whatever its evaluator leaves in the candidate
    arrays, so an evaluator that snaps them in place on its calls n > 0 with n % every == 0
    (call 0 is the initial population, call n iteration n) states the semantics on its own."""
    K, imax = 5, 45
    sw = hq.SWASA(population=P, imax=imax, seed=31 + P, t0=0.05, iTc=7)
    iters = imax + 9  # past imax: the driver stops there
    best, err, trace = sw.search_host(K, lambda ps: [cost(p) for p in ps], iterations=iters, refine=snap,
                                      every=every)
    calls = [0]

    def oracle_eval(ps):
        n = calls[0]
        calls[0] += 1
        if n > 0 and n % every == 0:
            for p in ps:
                snap(p)
        return [cost(p) for p in ps]

    osw = o.Swasa(o.SwasaParams(population=P, imax=imax, t0=0.05, iTc=7), 31 + P)
    tr = []
    ob, oe = o.find_best_quantization(oracle_eval, K, osw, trace=tr)
    assert calls[0] == imax + 1
    np.testing.assert_array_equal(trace[:imax], np.array([[t[3]] + t[1] for t in tr]))
    assert np.all(trace[imax:] == 0)  # nothing ran past imax
    np.testing.assert_array_equal(bits(best.reshape(K, 4)), bits(ob))
    assert err == oe
    # the refine took part: the plain search ends elsewhere
    plain = hq.SWASA(population=P, imax=imax, seed=31 + P, t0=0.05, iTc=7).search_host(
        K, lambda ps: [cost(p) for p in ps], iterations=iters)
    assert not np.array_equal(plain[2], trace)


def raw_search(sw, K, iters, refine, every, eval_rc=0):
    """hq_swasa_search_host_lloyd through ctypes -> (rc, best, err, trace)."""
    lib = hq.load()
    params = sw.params()
    P = sw.population

    def _ev(user, pal, P_, K_, costs):
        arr = np.ctypeslib.as_array(pal, shape=(P_ * K_ * 4,)).reshape(P_, K_, 4)
        for i in range(P_):
            costs[i] = cost(arr[i])
        return eval_rc

    best = np.zeros(4 * K, np.float32)
    err = C.c_double()
    trace = np.zeros(iters * (1 + P), np.float64)
    rc = lib.hq_swasa_search_host_lloyd(C.byref(params), K, sw.seed, iters, _lib.EVAL_FN(_ev), refine, every, None,
                                        _lib.fptr(best), C.byref(err), _lib.dptr(trace))
    return rc, best, err.value, trace.reshape(iters, 1 + P)


def test_every_zero_and_null_refine_are_the_plain_search():
    K, iters = 6, 40
    mk = lambda: hq.SWASA(population=3, imax=60, seed=8, t0=0.05, iTc=7)  # noqa: E731
    pb, pe, pt = mk().search_host(K, lambda ps: [cost(p) for p in ps], iterations=iters)

    def _snap(user, pal, P, KK):
        snap(np.ctypeslib.as_array(pal, shape=(P * KK * 4,)).reshape(P, KK, 4))
        return 0

    for refine, every in ((_lib.REFINE_FN(_snap), 0), (_lib.REFINE_FN(), 2), (_lib.REFINE_FN(), 0)):
        rc, b, e, t = raw_search(mk(), K, iters, refine, every)
        assert rc == _lib.HQ_OK
        np.testing.assert_array_equal(bits(b), bits(pb))
        np.testing.assert_array_equal(t, pt)
        assert e == pe
    assert raw_search(mk(), K, iters, _lib.REFINE_FN(_snap), -1)[0] == _lib.HQ_ERR_ARG


def test_a_failing_refine_returns_its_code():
    seen = []

    def _bad(user, pal, P, KK):
        seen.append(1)
        return 0 if len(seen) < 3 else 37

    rc, _, _, trace = raw_search(hq.SWASA(population=2, imax=60, seed=8), 4, 20, _lib.REFINE_FN(_bad), 2)
    assert rc == 37 and len(seen) == 3  # iterations 2 and 4 refined, 6 failed


def test_search_host_propagates_refine_errors():
    def bad(pal):
        raise ValueError("boom")

    with pytest.raises(ValueError):
        hq.SWASA(population=2, imax=10, seed=1).search_host(4, lambda ps: [cost(p) for p in ps], refine=bad, every=1)


def test_shared_update_arithmetic_on_its_edge_cases():
    """lloyd_mean (hq_lloyd.h) is what hq_centroids_from_sums computes with on the host and
    lloyd_update_kernel on the device: count 0 with NaN colour bits, a sum above 2^53,
    count 1, for both den."""
    n = 1 << 30
    for den in (255, DEN32):
        top = 255 if den == 255 else DEN32
        sums = np.array([[[0, 0, 0, 0],                                   # count 0: keeps its bits
                          [17, 99, 5, 0],                                 # sums without a count: ignored
                          [top, 0, top // 3, 1],                          # count 1
                          [(1 << 53) + 1, 3 * (1 << 54) + 7, n * top - 12345, n],  # sums above 2^53
                          [1, top - 1, 12345, 7]]], np.int64)
        if den == 255:
            sums[0, 3, :3] = [(1 << 36) + 1, 255 * n, 255 * n - 1]       # (a byte sum stays below 2^38)
        pal = np.full((1, 5 * 4), 0.25, np.float32)
        pal[0, 0:4] = [np.nan, np.inf, -0.0, 5.0]
        pal.view(np.uint32)[0, 0] = 0x7FC12345  # a NaN with a payload
        pal[0, 4:8] = [0.1, 0.2, 0.3, 0.7]
        got = hq.ImageManipulation.centroidsFromSums(sums, den, pal)
        np.testing.assert_array_equal(bits(got), bits(centroids_ref(sums, den, pal)))
        np.testing.assert_array_equal(bits(got[0, :8]), bits(pal[0, :8]))
        np.testing.assert_array_equal(got[0, 8:12], np.array([1.0, 0.0, np.float32(top // 3 / top), 0.0], np.float32))

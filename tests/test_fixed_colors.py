"""CPU tests of the fixed palette colours (libhq's addition): the repair rule under fixed
colours against a numpy restatement written here, and the host driver's semantics through
hq_swasa_search_host_fixed with Python evaluators -- the draws do not shift, the evaluator
never sees a palette without the fixed colours' bits, and the driver puts them back after a
refine callback.  Every comparison is bit for bit.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
from hybridquantization_amd import _lib


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------
# 1. hq_reseed_unused_fixed against a numpy restatement
# ---------------------------------------------------------------------------
def reseed_fixed_ref(err, worst, pals, max_moves, nfixed):
    """hq.h's rule: per palette the receivers are the colours k >= nfixed with count 0, ascending;
    the donors the colours with count > 0 and a worst pixel ([3] >= 0), by sum descending and the
    lower index first on a tie; receiver i takes donor i's worst pixel, .w = 0."""
    P, K = err.shape[:2]
    out = pals.reshape(P, K, 4).copy()
    moved = np.zeros(P, np.int32)
    for p in range(P):
        donors = [k for k in range(K) if err[p, k, 1] > 0 and err[p, k, 3] >= 0]
        donors.sort(key=lambda k: (-int(err[p, k, 0]), k))
        receivers = [k for k in range(nfixed, K) if err[p, k, 1] == 0]
        n = min(len(donors), len(receivers))
        if max_moves >= 0:
            n = min(n, max_moves)
        for r, d in zip(receivers[:n], donors[:n]):
            out[p, r, :3] = worst[p, d, :3]
            out[p, r, 3] = 0.0
        moved[p] = n
    return out.reshape(P, -1), moved


def random_stats(rng, P, K, unused, flat=False):
    """Integer statistics in hq_cluster_errors' layout: `unused[p]` = the colours of palette p with
    count 0; flat: every donor has the same sum (the tie rule decides the whole order)."""
    err = np.zeros((P, K, 4), np.int64)
    worst = np.zeros((P, K, 4), np.float32)
    for p in range(P):
        for k in range(K):
            if k in unused[p]:
                err[p, k] = (0, 0, 0, -1)
                continue
            movable = rng.random() < 0.85
            err[p, k] = (7 if flat else rng.integers(0, 4) * 1000, rng.integers(1, 50),
                         0x3f000000 if movable else 0, rng.integers(0, 6000) if movable else -1)
            if movable:
                worst[p, k, :3] = rng.integers(0, 256, 3).astype(np.float32) / np.float32(255)
    pals = rng.random((P, 4 * K)).astype(np.float32)
    pals[:, 3::4] = 0.0
    return err, worst, pals


def raw_reseed_fixed(err, worst, pals, max_moves, nfixed):
    P, K = err.shape[:2]
    out = pals.copy()
    moved = np.full(P, -7, np.int32)
    rc = hq.load().hq_reseed_unused_fixed(_lib.i64ptr(err), _lib.fptr(worst), P, K, max_moves, nfixed, _lib.fptr(out),
                                          moved.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, out, moved


UNUSED = {
    # some fixed colours with count 0; palette 0: more receivers than donors, palette 1 the reverse
    "mixed": [{0, 2, 3, 5, 6, 7, 8, 9, 10, 11}, {1, 6}, {0, 4, 5, 9, 11}],
    "fixed_only": [{0, 1, 2}, {0, 4}, {3}],
    "none": [set(), set(), set()],
}


@pytest.mark.parametrize("flat", [False, True], ids=["sums", "equal_sums"])
@pytest.mark.parametrize("which", list(UNUSED))
def test_reseed_fixed_equals_the_restatement(which, flat):
    P, K = 3, 12
    rng = np.random.default_rng(len(which) + 10 * flat)
    err, worst, pals = random_stats(rng, P, K, UNUSED[which], flat)
    for nfixed in (0, 1, 5, 12):
        for mm in (-1, 0, 2):
            rc, got, moved = raw_reseed_fixed(err, worst, pals, mm, nfixed)
            want, want_moved = reseed_fixed_ref(err, worst, pals, mm, nfixed)
            assert rc == _lib.HQ_OK
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"nfixed={nfixed} max_moves={mm}")
            np.testing.assert_array_equal(moved, want_moved)
            np.testing.assert_array_equal(bits(got.reshape(P, K, 4)[:, :nfixed]),
                                          bits(pals.reshape(P, K, 4)[:, :nfixed]))
            if nfixed == 0:  # hq_reseed_unused itself, and the Python surface's default
                old, old_moved = hq.ImageManipulation.reseedUnused(err, worst, pals, mm)
                np.testing.assert_array_equal(bits(old), bits(got))
                np.testing.assert_array_equal(old_moved, moved)
            else:
                via, via_moved = hq.ImageManipulation.reseedUnused(err, worst, pals, mm, nfixed=nfixed)
                np.testing.assert_array_equal(bits(via), bits(got))
                np.testing.assert_array_equal(via_moved, moved)
    if which == "mixed" and not flat:  # the cases the list above promises
        _, m0 = reseed_fixed_ref(err, worst, pals, -1, 5)
        donors = [(err[p, :, 1] > 0) & (err[p, :, 3] >= 0) for p in range(P)]
        assert m0[0] == donors[0].sum() < len([k for k in UNUSED[which][0] if k >= 5])
        assert m0[1] == 1 < donors[1].sum()


def test_reseed_fixed_refuses_a_bad_count():
    rng = np.random.default_rng(2)
    err, worst, pals = random_stats(rng, 3, 12, UNUSED["mixed"])
    for nfixed in (-1, 13):
        rc, got, moved = raw_reseed_fixed(err, worst, pals, -1, nfixed)
        assert rc == _lib.HQ_ERR_ARG
        np.testing.assert_array_equal(bits(got), bits(pals))
        assert np.all(moved == -7)


# ---------------------------------------------------------------------------
# 2. / 3. The host driver
# ---------------------------------------------------------------------------
K, P = 6, 4
TARGETS = (np.arange(K * 3, dtype=np.float64).reshape(K, 3) * 0.05 + 0.02) % 1.0


def free_cost(pals):
    """Depends on colours 2 .. 5 only: squared distances to six targets (no delta, no counts)."""
    d = pals[:, 2:, :3].astype(np.float64) - TARGETS[2:]
    return (d * d).sum((1, 2))


def seeing_cost(pals):
    d = pals[:, :, :3].astype(np.float64) - TARGETS
    return (d * d).sum((1, 2))


def raw_search(fn_name, cost, population, fixed, nfixed, iters=60, every=0, refine=None, seed=5, imax=60, seen=None,
               convergence=True):
    """hq_swasa_search_host_fixed or _from through ctypes -> (best (K, 4), error, trace)."""
    lib = hq.load()
    params = hq.SWASA(population=P, imax=imax, seed=seed, convergence=convergence).params()

    def _cb(user, pal, PP, KK, costs):
        arr = np.ctypeslib.as_array(pal, shape=(PP * KK * 4,)).reshape(PP, KK, 4).copy()
        if seen is not None:
            seen.append(arr)
        for i, v in enumerate(cost(arr)):
            costs[i] = float(v)
        return 0

    def _rf(user, pal, PP, KK):
        refine(np.ctypeslib.as_array(pal, shape=(PP * KK * 4,)).reshape(PP, KK, 4))
        return 0

    cb = _lib.EVAL_FN(_cb)
    rf = _lib.REFINE_FN(_rf) if refine is not None else _lib.REFINE_FN()
    best = np.zeros(4 * K, np.float32)
    err = C.c_double()
    trace = np.zeros(iters * (1 + P), np.float64)
    pop = None if population is None else _lib.fptr(population)
    if fn_name == "fixed":
        fx = None if fixed is None else _lib.fptr(fixed)
        rc = lib.hq_swasa_search_host_fixed(C.byref(params), K, seed, iters, cb, rf, every, pop, fx, nfixed, None,
                                            _lib.fptr(best), C.byref(err), _lib.dptr(trace))
    else:
        rc = lib.hq_swasa_search_host_from(C.byref(params), K, seed, iters, cb, rf, every, pop, None,
                                           _lib.fptr(best), C.byref(err), _lib.dptr(trace))
    assert rc == _lib.HQ_OK
    return best.reshape(K, 4), err.value, trace.reshape(iters, 1 + P)


def start_population():
    rng = np.random.default_rng(41)
    pop = rng.random((P, K, 4)).astype(np.float32)
    pop[..., 3] = 0.0
    pop[:, :2] = pop[0, :2]  # every member starts with the same two first colours
    return np.ascontiguousarray(pop.reshape(P, -1))


@pytest.mark.parametrize("given", ["values", "as_they_stand"])
def test_the_draws_do_not_shift(given):
    """The cost does not look at colours 0 and 1, so fixing them must leave the whole search
    where it was: the same trace and the same free colours, which they are only when every
    draw of the fixed colours is still made and thrown away."""
    pop = start_population()
    fx = np.ascontiguousarray(pop.reshape(P, K, 4)[0, :2])
    seen = []
    b1, e1, t1 = raw_search("fixed", free_cost, pop, fx if given == "values" else None, 2, seen=seen)
    b0, e0, t0 = raw_search("from", free_cost, pop, None, 0)
    np.testing.assert_array_equal(t1, t0)
    assert e1 == e0
    np.testing.assert_array_equal(bits(b1[2:]), bits(b0[2:]))
    assert np.any(bits(b0[:2]) != bits(fx))       # the free search moved them
    assert len(np.unique(t0[:, 1:])) > P and np.any(np.diff(t0[:, 0]) < 0)   # a search that went somewhere
    assert len(seen) == 61
    for arr in seen:
        np.testing.assert_array_equal(bits(arr[:, :2]), bits(np.broadcast_to(fx, (P, 2, 4))))
    np.testing.assert_array_equal(bits(b1[:2]), bits(fx))
    # through the Python surface: SWASA.search_host(fixed=...)
    sw = hq.SWASA(population=P, imax=60, seed=5)
    best, err, trace = sw.search_host(K, free_cost, iterations=60, initial=pop, fixed=fx[:, :3])
    np.testing.assert_array_equal(trace, t1)
    np.testing.assert_array_equal(bits(best.reshape(K, 4)), bits(b1))


def test_fixed_values_overwrite_the_population_and_the_draws():
    """fixed_colors given: written over the first colours of a given population and of the
    random one, whose free colours stay hq_swasa_search_host's draws."""
    fx = np.array([[0, 0, 0, 9], [1, 0.5, 0.25, 9]], np.float32)
    want = fx.copy()
    want[:, 3] = 0.0
    for pop in (start_population(), None):
        seen, seen0 = [], []
        raw_search("fixed", free_cost, pop, fx, 2, iters=1, seen=seen)
        raw_search("from", free_cost, pop, None, 0, iters=1, seen=seen0)
        np.testing.assert_array_equal(bits(seen[0][:, :2]), bits(np.broadcast_to(want, (P, 2, 4))))
        np.testing.assert_array_equal(bits(seen[0][:, 2:]), bits(seen0[0][:, 2:]))
        np.testing.assert_array_equal(bits(seen[1][:, :2]), bits(np.broadcast_to(want, (P, 2, 4))))


def test_the_driver_puts_the_fixed_colours_back_after_refine():
    """A refine callback that adds 0.01 to every channel, fixed ones included, every third
    iteration: the evaluator still sees the fixed bits every time, and the search is the one
    whose refine leaves the first two colours alone."""
    pop = start_population()
    fx = np.ascontiguousarray(pop.reshape(P, K, 4)[0, :2])

    def bump_all(arr):
        arr[..., :3] += np.float32(0.01)

    def bump_free(arr):
        arr[:, 2:, :3] += np.float32(0.01)

    seen = []
    b1, e1, t1 = raw_search("fixed", free_cost, pop, fx, 2, every=3, refine=bump_all, seen=seen)
    b0, e0, t0 = raw_search("from", free_cost, pop, None, 0, every=3, refine=bump_free)
    np.testing.assert_array_equal(t1, t0)
    np.testing.assert_array_equal(bits(b1[2:]), bits(b0[2:]))
    for arr in seen:
        np.testing.assert_array_equal(bits(arr[:, :2]), bits(np.broadcast_to(fx, (P, 2, 4))))
    _, _, plain = raw_search("from", free_cost, pop, None, 0)
    assert not np.array_equal(plain, t1)  # (the refine did something)


def test_nfixed_zero_and_nfixed_k():
    pop = start_population()
    b1, e1, t1 = raw_search("fixed", seeing_cost, pop, None, 0)
    b0, e0, t0 = raw_search("from", seeing_cost, pop, None, 0)
    np.testing.assert_array_equal(t1, t0)
    np.testing.assert_array_equal(bits(b1), bits(b0))
    assert e1 == e0
    # every colour fixed: a member's candidates are the member, so its error never changes
    # (with the convergence copies off: after one, a member's error is the copied member's)
    _, eK, tK = raw_search("fixed", seeing_cost, pop, None, K, convergence=False)
    first = seeing_cost(pop.reshape(P, K, 4))
    np.testing.assert_array_equal(tK[:, 1:], np.broadcast_to(first, (60, P)))
    assert eK == first.min() and np.all(tK[:, 0] == eK)


def test_refusals():
    lib = hq.load()
    pop = start_population()
    params = hq.SWASA(population=P, imax=60, seed=5).params()
    cb = _lib.EVAL_FN(lambda *a: 0)
    best = np.zeros(4 * K, np.float32)
    for fx, n in ((None, -1), (None, K + 1), (np.array([[0, 2, 0, 0]], np.float32), 1),
                  (np.array([[0, np.nan, 0, 0]], np.float32), 1)):
        rc = lib.hq_swasa_search_host_fixed(C.byref(params), K, 5, 3, cb, _lib.REFINE_FN(), 0, _lib.fptr(pop),
                                            None if fx is None else _lib.fptr(fx), n, None, _lib.fptr(best), None, None)
        assert rc == _lib.HQ_ERR_ARG, (fx, n)
    sw = hq.SWASA(population=P, imax=60, seed=5)
    for bad in (np.zeros((2, 5)), np.zeros(7), [[0, 0, 1.5]], [[0, np.nan, 0]], np.zeros((K + 1, 3))):
        with pytest.raises(ValueError):
            sw.search_host(K, lambda p: 1 / 0, iterations=3, fixed=bad)

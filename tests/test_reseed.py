"""CPU tests of hq_reseed_unused (libhq's addition: the repair rule, host code only)
against the numpy restatement of reseed_ref.py, bit for bit, through ctypes."""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
from hybridquantization_amd import _lib
from lloyd_ref import bits
from reseed_ref import reseed_ref


def raw_reseed(err, worst, pal, max_moves, with_moved=True):
    """hq_reseed_unused through ctypes -> (rc, palettes, moved)."""
    err = np.ascontiguousarray(err, np.int64)
    P, K = err.shape[:2]
    worst = np.ascontiguousarray(worst, np.float32)
    out = np.ascontiguousarray(pal, np.float32).reshape(P, 4 * K).copy()
    moved = np.full(P, -7, np.int32)
    rc = hq.load().hq_reseed_unused(_lib.i64ptr(err), _lib.fptr(worst), P, K, int(max_moves), _lib.fptr(out),
                                    moved.ctypes.data_as(C.POINTER(C.c_int)) if with_moved else None)
    return rc, out, moved


def random_stats(P, K, seed, unused=0.4, unmovable=0.2, ties=False):
    """Statistics in hq_cluster_errors' layout: a share of colours without pixels, a share of
    the others without a movable pixel; `ties`: the sums drawn from three values."""
    rng = np.random.default_rng(seed)
    err = np.zeros((P, K, 4), np.int64)
    worst = np.zeros((P, K, 4), np.float32)
    count = rng.integers(1, 1000, (P, K)) * (rng.random((P, K)) >= unused)
    has = (count > 0) & (rng.random((P, K)) >= unmovable)
    err[..., 0] = np.where(count > 0, rng.integers(0, 3, (P, K)) * 5 if ties else rng.integers(0, 2 ** 50, (P, K)), 0)
    err[..., 1] = count
    err[..., 2] = np.where(has, rng.integers(0, 0x49800000, (P, K)), 0)
    err[..., 3] = np.where(has, rng.integers(0, 2 ** 32 - 1, (P, K)), -1)
    worst[..., :3] = np.where(has[..., None], rng.random((P, K, 3)).astype(np.float32), 0)
    pal = rng.random((P, K, 4)).astype(np.float32)
    pal[..., 3] = 0
    return err, worst, pal.reshape(P, 4 * K)


def check(err, worst, pal, max_moves):
    rc, out, moved = raw_reseed(err, worst, pal, max_moves)
    assert rc == _lib.HQ_OK
    want, want_moved = reseed_ref(err, worst, pal, max_moves)
    np.testing.assert_array_equal(bits(out), bits(want))
    np.testing.assert_array_equal(moved, want_moved)
    return out, moved


@pytest.mark.parametrize("K", [1, 2, 8, 300])
@pytest.mark.parametrize("P", [1, 5])
def test_random_stats_equal_numpy(P, K):
    for seed, ties in ((1, False), (2, True)):
        err, worst, pal = random_stats(P, K, seed=100 * K + 10 * P + seed, ties=ties)
        for max_moves in (-1, 0, 1, 3):
            _, moved = check(err, worst, pal, max_moves)
            if max_moves >= 0:
                assert np.all(moved <= max_moves)
    # the wrapper gives the same
    got, moved = hq.ImageManipulation.reseedUnused(err, worst, pal, 3)
    np.testing.assert_array_equal(bits(got), bits(reseed_ref(err, worst, pal, 3)[0]))
    np.testing.assert_array_equal(moved, reseed_ref(err, worst, pal, 3)[1])


def stats(rows):
    """One palette from (sum, count, position or -1) per colour; colour k's worst pixel is (k, k + 0.5, -k)."""
    K = len(rows)
    err = np.zeros((1, K, 4), np.int64)
    worst = np.zeros((1, K, 4), np.float32)
    for k, (s, n, pos) in enumerate(rows):
        err[0, k] = (s, n, 0x40000000 if pos >= 0 else 0, pos)
        if pos >= 0:
            worst[0, k, :3] = (k, k + 0.5, -k)
    pal = np.full((1, 4 * K), 0.25, np.float32)
    pal[0, 3::4] = 0
    return err, worst, pal


def colour(out, k):
    return tuple(out[0, 4 * k:4 * k + 3])


def test_equal_sums_the_lower_index_gives_first():
    err, worst, pal = stats([(0, 0, -1), (40, 2, 5), (0, 0, -1), (40, 9, 3), (40, 1, 8), (0, 0, -1)])
    out, moved = check(err, worst, pal, -1)
    assert moved[0] == 3
    assert colour(out, 0) == (1, 1.5, -1) and colour(out, 2) == (3, 3.5, -3) and colour(out, 5) == (4, 4.5, -4)
    for k in (1, 3, 4):  # the donors themselves do not move
        assert colour(out, k) == (0.25, 0.25, 0.25)


def test_more_receivers_than_donors_and_the_reverse():
    err, worst, pal = stats([(0, 0, -1), (0, 0, -1), (0, 0, -1), (7, 1, 2)])
    out, moved = check(err, worst, pal, -1)
    assert moved[0] == 1 and colour(out, 0) == (3, 3.5, -3)
    assert colour(out, 1) == colour(out, 2) == (0.25, 0.25, 0.25)
    err, worst, pal = stats([(5, 1, 0), (9, 1, 1), (0, 0, -1), (7, 1, 2)])
    out, moved = check(err, worst, pal, -1)
    assert moved[0] == 1 and colour(out, 2) == (1, 1.5, -1)


def test_a_donor_without_a_movable_pixel_is_skipped():
    err, worst, pal = stats([(99, 50, -1), (0, 0, -1), (3, 1, 4), (0, 0, -1)])
    out, moved = check(err, worst, pal, -1)
    assert moved[0] == 1 and colour(out, 1) == (2, 2.5, -2) and colour(out, 3) == (0.25, 0.25, 0.25)


@pytest.mark.parametrize("max_moves,want", [(0, 0), (1, 1), (-1, 2), (-5, 2), (7, 2)])
def test_max_moves(max_moves, want):
    err, worst, pal = stats([(0, 0, -1), (4, 1, 0), (0, 0, -1), (6, 1, 1), (5, 1, 2)])
    out, moved = check(err, worst, pal, max_moves)
    assert moved[0] == want
    assert colour(out, 0) == ((3, 3.5, -3) if want >= 1 else (0.25, 0.25, 0.25))
    assert colour(out, 2) == ((4, 4.5, -4) if want >= 2 else (0.25, 0.25, 0.25))


def test_no_receiver_leaves_the_bits():
    err, worst, pal = random_stats(3, 8, seed=9, unused=0.0)
    pal[1, 5] = np.float32(-0.0)
    pal[2, 3] = 7.0  # .w of an untouched colour is not rewritten
    rc, out, moved = raw_reseed(err, worst, pal, -1, with_moved=False)  # (moved may be NULL)
    assert rc == _lib.HQ_OK
    np.testing.assert_array_equal(bits(out), bits(pal))
    assert np.all(check(err, worst, pal, -1)[1] == 0)


def test_refusals():
    err, worst, pal = random_stats(2, 8, seed=4)
    lib = hq.load()
    for field in (0, 1):  # a negative sum, a negative count
        bad = err.copy()
        bad[1, 6, field] = -1
        rc, out, moved = raw_reseed(bad, worst, pal, -1)
        assert rc == _lib.HQ_ERR_ARG
        np.testing.assert_array_equal(bits(out), bits(pal))  # untouched, palette 0 included
        assert np.all(moved == -7)
    e, w, p = _lib.i64ptr(err), _lib.fptr(np.ascontiguousarray(worst)), _lib.fptr(pal.copy())
    assert lib.hq_reseed_unused(e, w, 0, 8, -1, p, None) == _lib.HQ_ERR_ARG
    assert lib.hq_reseed_unused(e, w, 2, 0, -1, p, None) == _lib.HQ_ERR_ARG
    assert lib.hq_reseed_unused(None, w, 2, 8, -1, p, None) == _lib.HQ_ERR_ARG
    assert lib.hq_reseed_unused(e, None, 2, 8, -1, p, None) == _lib.HQ_ERR_ARG
    assert lib.hq_reseed_unused(e, w, 2, 8, -1, None, None) == _lib.HQ_ERR_ARG

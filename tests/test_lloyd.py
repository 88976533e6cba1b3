"""CPU check of hq_centroids_from_sums (the k-means update, libhq's addition):
bit for bit against the numpy formulas of include/hq.h.  No GPU needed."""

import numpy as np

import hybridquantization_amd as hq
from hybridquantization_amd import _lib
from lloyd_ref import DEN32, bits, centroids_ref


def random_case(den, seed, P=3, K=37):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 5000, (P, K))
    cnt[rng.random((P, K)) < 0.3] = 0
    top = 255 if den == 255 else DEN32
    sums = np.zeros((P, K, 4), np.int64)
    for ch in range(3):
        sums[..., ch] = (rng.random((P, K)) * cnt * top).astype(np.int64)
    sums[..., 3] = cnt
    pal = rng.random((P, 4 * K)).astype(np.float32)
    return sums, pal


def test_update_matches_numpy_bitwise_for_both_units():
    for den in (255, DEN32):
        for seed in range(3):
            sums, pal = random_case(den, seed)
            got = hq.ImageManipulation.centroidsFromSums(sums, den, pal)
            np.testing.assert_array_equal(bits(got), bits(centroids_ref(sums, den, pal)))
            # colours without pixels keep every bit (.w included), the others get .w = 0
            has = sums[..., 3] > 0
            g4, p4 = got.reshape(3, -1, 4), pal.reshape(3, -1, 4)
            np.testing.assert_array_equal(bits(g4[~has]), bits(p4[~has]))
            assert np.all(bits(g4[has][:, 3]) == 0) and np.any(p4[has][:, 3] != 0)


def test_sums_above_2_53_round_as_the_double_conversion():
    """2^30 pixels of value ~1: channel sums near 2^62, where int64 -> double rounds."""
    n = 1 << 30
    sums = np.array([[[n * DEN32 - 12345, (1 << 53) + 1, (1 << 61) + 3, n],
                      [(1 << 62) - 1, 3 * (1 << 54) + 7, 12345678901234567, n - 1]]], np.int64)
    assert np.any(sums[..., :3].astype(np.float64).astype(np.int64) != sums[..., :3])  # the rounding happens
    pal = np.full((1, 8), 0.25, np.float32)
    got = hq.ImageManipulation.centroidsFromSums(sums, DEN32, pal)
    np.testing.assert_array_equal(bits(got), bits(centroids_ref(sums, DEN32, pal)))
    s255 = np.array([[[255 * n, (1 << 36) + 1, 17, n], [0, 1, 2, 3]]], np.int64)
    got = hq.ImageManipulation.centroidsFromSums(s255, 255, pal)
    np.testing.assert_array_equal(bits(got), bits(centroids_ref(s255, 255, pal)))
    assert got[0, 0] == 1.0 and got[0, 3] == 0.0


def test_count_zero_keeps_bits_nan_included():
    pal = np.zeros((1, 12), np.float32)
    pal[0, 0:4] = [0.1, 0.2, 0.3, 0.7]
    pal[0, 4:8] = [np.nan, np.inf, -0.0, 5.0]
    pal.view(np.uint32)[0, 4] = 0x7FC12345  # a NaN with a payload
    pal[0, 8:12] = [0.9, 0.8, 0.7, 0.6]
    sums = np.zeros((1, 3, 4), np.int64)
    sums[0, 1, :3] = 99  # sums without a count are ignored
    sums[0, 2] = [255 * 4, 0, 510, 4]
    got = hq.ImageManipulation.centroidsFromSums(sums, 255, pal)
    np.testing.assert_array_equal(bits(got[0, :8]), bits(pal[0, :8]))
    np.testing.assert_array_equal(got[0, 8:], np.array([1.0, 0.0, 0.5, 0.0], np.float32))


def test_bad_den_and_arguments_refused():
    lib = hq.load()
    sums = np.ones((1, 2, 4), np.int64)
    pal = np.full(8, 0.5, np.float32)
    before = pal.copy()
    for den in (0, 1, 256, -255, 1 << 31, (1 << 32) + 1):
        assert lib.hq_centroids_from_sums(_lib.i64ptr(sums), den, 1, 2, _lib.fptr(pal)) == _lib.HQ_ERR_ARG
    assert lib.hq_centroids_from_sums(_lib.i64ptr(sums), 255, 0, 2, _lib.fptr(pal)) == _lib.HQ_ERR_ARG
    assert lib.hq_centroids_from_sums(None, 255, 1, 2, _lib.fptr(pal)) == _lib.HQ_ERR_ARG
    np.testing.assert_array_equal(pal, before)
    assert lib.hq_centroids_from_sums(_lib.i64ptr(sums), 255, 1, 2, _lib.fptr(pal)) == _lib.HQ_OK

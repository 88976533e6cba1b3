"""The pixel weights' numpy restatements (weights_ref.py) against brute force, the k-means
update and the median cut on weighted sums, and the zeros-and-ones identity of the
restatements themselves.  No GPU."""

import numpy as np
import pytest

import hybridquantization_amd as hq
from lloyd_ref import DEN32, bits as fbits, centroids_ref, cluster_sums_ref, q32
from mask_ref import live_tiles_brute, masked_cluster_sums, masked_histogram, masked_sum
from seed_ref import coord_byte, coord_float, histogram_ref, median_cut_ref
from weights_ref import (LIMIT, as_int64, live_tile_count, nonzero, weight_maps, weight_sum, weighted_cluster_sums,
                         weighted_cost, weighted_histogram, weighted_sum)

SHAPES = [(97, 53), (300, 40), (5, 1), (1, 5), (2, 3), (64, 64)]
TILES = [(128, 16), (108, 8), (256, 16)]


def _data(w, h, K=16, seed=3):
    rng = np.random.default_rng(seed + w + h)
    err = rng.random(w * h).astype(np.float32) * 30
    idx = rng.integers(0, K, w * h)
    px = rng.integers(0, 256, (w * h, 3))
    return err, idx, px


@pytest.mark.parametrize("w,h", SHAPES)
def test_the_maps_are_what_the_tests_say(w, h):
    ms = weight_maps(w, h)
    assert set(ms) == {"hgrad", "vgrad", "noise", "corners", "all255", "zeros_ones"}
    for name, m in ms.items():
        assert m.dtype == np.uint8 and m.shape == (h, w) and m.any(), name
    assert set(np.unique(ms["zeros_ones"])) <= {0, 1} and np.all(ms["all255"] == 255)
    if w >= 64:
        assert ms["hgrad"][0, 0] == 0 and ms["hgrad"][0, -1] == 255 and ms["vgrad"].min() == 0
        assert ms["vgrad"].max() == 255 and nonzero(ms["corners"]) == 4
        for g in (ms["hgrad"], ms["vgrad"]):  # non-uniform within every run of 4 pixels of a row
            runs = np.lib.stride_tricks.sliding_window_view(g, 4, axis=1)
            assert np.all(runs.max(-1) > runs.min(-1))
        assert np.all(ms["noise"][h // 4:3 * h // 4, w // 4:3 * w // 4] == 0) and ms["noise"].max() > 200


@pytest.mark.parametrize("w,h", SHAPES)
def test_weighted_cost_sums_and_histogram_against_brute_force(w, h):
    err, idx, px = _data(w, h)
    for name, m in weight_maps(w, h).items():
        e = err.copy()
        zero = np.flatnonzero(m.reshape(-1) == 0)
        if len(zero):
            e[zero[0]] = np.nan  # (a NaN under weight 0 stays out)
        wt = [int(v) for v in m.reshape(-1)]
        s, W, n = 0.0, 0, 0
        sums = [[0] * 4 for _ in range(16)]
        cells = [[0] * 4 for _ in range(1 << 9)]
        for i in range(w * h):
            W += wt[i]
            if wt[i] == 0:
                continue
            n += 1
            s += float(e[i]) * wt[i]
            c = ((int(px[i, 0]) >> 5) << 6) | ((int(px[i, 1]) >> 5) << 3) | (int(px[i, 2]) >> 5)
            for ch in range(3):
                sums[idx[i]][ch] += wt[i] * int(px[i, ch])
                cells[c][ch] += wt[i] * int(px[i, ch])
            sums[idx[i]][3] += wt[i]
            cells[c][3] += wt[i]
        assert weight_sum(m) == W and nonzero(m) == n, name
        got = weighted_sum(e, m)
        assert np.isfinite(got) and abs(got - s) <= 1e-12 * abs(s), name
        assert abs(weighted_cost(e, m, W, 3, 2.0) - (s / W + 6.0)) <= 1e-12 * (s / W + 6.0)
        assert weighted_cluster_sums(idx, px, 16, m).tolist() == sums, name
        assert weighted_histogram(coord_byte(px, 3), px, 3, m).tolist() == cells, name
        for tw, th in TILES:
            for r0, r1 in ((0, h),) + (((0, 20), (20, h), (21, 37)) if h > 37 else ()):
                for de in (False, True):
                    want = len(live_tiles_brute(m, w, h, tw, th, r0, r1, de))
                    assert live_tile_count(m, w, h, tw, th, r0, r1, de) == want, (name, tw, th, r0, r1, de)
    e = err.copy()
    e[0] = np.nan
    assert np.isnan(weighted_sum(e, np.ones((h, w), np.uint8)))  # ... and under weight 1 it does not


@pytest.mark.parametrize("w,h", SHAPES)
def test_zeros_and_ones_restate_the_mask_and_a_uniform_map_scales(w, h):
    err, idx, px = _data(w, h)
    zo = weight_maps(w, h)["zeros_ones"]
    assert weighted_sum(err, zo) == masked_sum(err, zo)
    np.testing.assert_array_equal(as_int64(weighted_cluster_sums(idx, px, 16, zo)), masked_cluster_sums(idx, px, 16, zo))
    np.testing.assert_array_equal(as_int64(weighted_histogram(coord_byte(px, 4), px, 4, zo)),
                                  masked_histogram(coord_byte(px, 4), px, 4, zo))
    for c in (2, 255):
        uni = np.full((h, w), c, np.uint8)
        np.testing.assert_array_equal(as_int64(weighted_cluster_sums(idx, px, 16, uni)), c * cluster_sums_ref(idx, px, 16))
        np.testing.assert_array_equal(as_int64(weighted_histogram(coord_byte(px, 4), px, 4, uni)),
                                      c * histogram_ref(coord_byte(px, 4), px, 4))
        total = float(err.astype(np.float64).sum())
        assert abs(weighted_cost(err, uni, c * w * h, 0, 2.0) - total / (w * h)) <= 1e-12 * total / (w * h)


def test_planar_sums_need_python_ints_and_the_limit_is_where_int64_ends():
    """One colour, every pixel white (q = 2^32): the weighted sum is 2^32 times the weight sum,
    below 2^63 exactly while the weight sum is below 2^31."""
    n = 1000
    px = np.full((n, 3), DEN32, np.int64)
    idx = np.zeros(n, np.int64)
    for c in (254, 255):
        s = weighted_cluster_sums(idx, px, 1, np.full(n, c, np.uint8))
        assert s[0].tolist() == [DEN32 * c * n] * 3 + [c * n]
    assert DEN32 * (LIMIT - 1) < 1 << 63 <= DEN32 * LIMIT
    assert 2904 * 2900 * 254 < LIMIT <= 2904 * 2900 * 255 and 2904 * 2900 >= 1 << 23
    assert 260 * 260 * 255 * 255 > 1 << 32 and (1 << 16) * 255 * 255 < 1 << 32


def _mean_py(s, n, den):
    """The weighted mean by hq_centroids_from_sums' rule, from Python ints: int -> double (round
    to nearest even, as the C conversion), one product or exact scaling, one division, one
    rounding to float."""
    s, n = np.float64(float(int(s))), np.float64(float(int(n)))
    return np.float32(s / (np.float64(255.0) * n)) if den == 255 else np.float32(np.ldexp(s, -32) / n)


@pytest.mark.parametrize("den", [255, DEN32])
def test_centroids_from_weighted_sums(den):
    w, h, K = 97, 53, 16
    rng = np.random.default_rng(11)
    idx = rng.integers(0, K - 1, w * h)  # (colour K - 1 has no pixel: it keeps its bits)
    by = rng.integers(0, 256, (w * h, 3))
    px = by if den == 255 else q32(by.astype(np.float32) / np.float32(255))
    pal = rng.random((2, 4 * K)).astype(np.float32)
    for name, m in weight_maps(w, h).items():
        sums = as_int64(np.stack([weighted_cluster_sums(idx, px, K, m), weighted_cluster_sums((idx + 1) % (K - 1), px, K, m)]))
        got = hq.ImageManipulation.centroidsFromSums(sums, den, pal)
        np.testing.assert_array_equal(fbits(got), fbits(centroids_ref(sums, den, pal)), err_msg=name)
        g = got.reshape(2, K, 4)
        for p in range(2):
            for k in range(K):
                if sums[p, k, 3] == 0:
                    np.testing.assert_array_equal(fbits(g[p, k]), fbits(pal[p].reshape(K, 4)[k]))
                    continue
                for ch in range(3):
                    assert fbits(g[p, k, ch]) == fbits(_mean_py(sums[p, k, ch], sums[p, k, 3], den)), (name, p, k, ch)
                assert g[p, k, 3] == 0
    # sums above 2^53 (the planar form near its limit): the int -> double conversion rounds
    big = np.asarray([[[DEN32 * (LIMIT - 1) - 12345, (1 << 62) + 3, (1 << 53) + 1, LIMIT - 1]]], np.int64)
    if den == DEN32:
        got = hq.ImageManipulation.centroidsFromSums(big, den, np.zeros((1, 4), np.float32))
        for ch in range(3):
            assert fbits(got[0, ch]) == fbits(_mean_py(big[0, 0, ch], big[0, 0, 3], den))
    # a uniform map moves nothing in the packed form: c s, 255 c n, s and 255 n are exact doubles
    # (below 2^53), so (c s) / (255 c n) and s / (255 n) are one real quotient, rounded once
    if den == 255:
        plain = np.stack([cluster_sums_ref(idx, px, K), cluster_sums_ref((idx + 1) % (K - 1), px, K)])
        want = hq.ImageManipulation.centroidsFromSums(plain, den, pal)
        for c in (3, 255):
            got = hq.ImageManipulation.centroidsFromSums(c * plain, den, pal)
            np.testing.assert_array_equal(fbits(got), fbits(want), err_msg=f"uniform {c}")


@pytest.mark.parametrize("img_u8", [1, 0])
def test_median_cut_of_a_weighted_histogram(img_u8):
    w, h, K, nbits = 64, 32, 8, 5
    rng = np.random.default_rng(5)
    by = rng.integers(0, 256, (w * h, 3))
    f = by.astype(np.float32) / np.float32(255)
    px, den, coords = (by, 255, coord_byte(by, nbits)) if img_u8 else (q32(f), DEN32, coord_float(f, nbits))
    seeds = {}
    for name, m in weight_maps(w, h).items():
        cells = as_int64(weighted_histogram(coords, px, nbits, m))
        got, made = hq.ImageManipulation.medianCut(cells, nbits, den, K)
        want, wmade = median_cut_ref(cells, nbits, den, K)
        assert made == wmade, name
        np.testing.assert_array_equal(fbits(got), fbits(want), err_msg=name)
        seeds[name] = got
    assert not np.array_equal(seeds["hgrad"], seeds["all255"])  # the seed follows the weights

"""The pixel mask's numpy restatements (mask_ref.py) against brute force, and the
seed inequality of test_mask_gpu.py established with the oracle.  No GPU."""

import numpy as np
import pytest

import c_oracle
import oracle as o
from lloyd_ref import cluster_sums_ref
from mask_ref import (inside, live_tiles, live_tiles_brute, masked_cluster_sums, masked_cost, masked_histogram,
                      masked_sum, masks_for, rectangle, tile_grid, two_tone_image)
from seed_ref import coord_byte, histogram_ref, median_cut_ref

SHAPES = [(97, 53), (300, 40), (5, 1), (1, 5), (2, 3), (64, 64)]
TILES = [(128, 16), (108, 8), (256, 16)]


def _data(w, h, K=16, seed=3):
    rng = np.random.default_rng(seed + w + h)
    err = rng.random(w * h).astype(np.float32) * 30
    idx = rng.integers(0, K, w * h)
    px = rng.integers(0, 256, (w * h, 3))
    return err, idx, px


@pytest.mark.parametrize("w,h", SHAPES)
def test_live_tiles_against_brute_force(w, h):
    for name, m in masks_for(w, h, worst=(w * h) // 2).items():
        for tw, th in TILES:
            for de in (False, True):
                assert live_tiles(m, w, h, tw, th, de2000=de) == live_tiles_brute(m, w, h, tw, th, de2000=de), name
                if h > 24:  # a shard whose dE2000 grid starts above r0, and one row of it
                    for r0, r1 in ((21, 37), (21, 22), (0, 20), (20, h)):
                        got = live_tiles(m, w, h, tw, th, r0, r1, de)
                        assert got == live_tiles_brute(m, w, h, tw, th, r0, r1, de), (name, r0, r1)
                        assert all(0 <= t < np.prod(tile_grid(w, r0, r1, tw, th, de)[1:]) for t in got)


def test_live_tiles_of_the_rectangle_and_the_edges():
    w, h = 300, 40
    rect = rectangle(w, h, 130, 250, 17, 30)
    assert live_tiles(rect, w, h, 128, 16) == [4]  # one of nine
    assert tile_grid(w, 0, h, 128, 16)[1:] == (3, 3) and tile_grid(w, 0, h, 108, 8)[1:] == (3, 5)
    assert live_tiles(rect, w, h, 108, 8) == [7, 8, 10, 11]  # columns 108 .. 323, rows 16 .. 31
    assert live_tiles(masks_for(w, h)["edges"], w, h, 128, 16) == [2, 5, 6, 7, 8]
    empty = np.zeros((h, w), np.uint8)
    empty[30] = 1
    assert live_tiles(empty, w, h, 128, 16, 0, 20) == []


@pytest.mark.parametrize("w,h", SHAPES)
def test_masked_cost_sums_and_histogram_against_brute_force(w, h):
    err, idx, px = _data(w, h)
    err[0] = np.nan  # (left out by the masks that leave pixel 0 out)
    for name, m in masks_for(w, h, worst=w * h - 1).items():
        f = inside(m)
        s, sums, cells = 0.0, np.zeros((16, 4), np.int64), np.zeros((1 << 9, 4), np.int64)
        for i in range(w * h):
            if not f[i]:
                continue
            s += float(err[i])
            sums[idx[i], :3] += px[i]
            sums[idx[i], 3] += 1
            c = ((px[i, 0] >> 5) << 6) | ((px[i, 1] >> 5) << 3) | (px[i, 2] >> 5)
            cells[c, :3] += px[i]
            cells[c, 3] += 1
        got = masked_sum(err, m)
        assert (np.isnan(s) and np.isnan(got)) or abs(got - s) <= 1e-12 * abs(s), name
        if not f[0]:
            assert np.isfinite(got), name
        n = int(f.sum())
        want = s / n + 2.0 * 3
        c = masked_cost(err, m, n, 3, 2.0)
        assert (np.isnan(want) and np.isnan(c)) or abs(c - want) <= 1e-12 * abs(want)
        np.testing.assert_array_equal(masked_cluster_sums(idx, px, 16, m), sums, err_msg=name)
        np.testing.assert_array_equal(masked_histogram(coord_byte(px, 3), px, 3, m), cells, err_msg=name)


@pytest.mark.parametrize("w,h", SHAPES)
def test_all_ones_is_unmasked_and_disjoint_masks_add_up(w, h):
    err, idx, px = _data(w, h)
    ms = masks_for(w, h)
    total = float(err.astype(np.float64).sum())
    assert masked_sum(err, ms["ones"]) == total
    assert masked_cost(err, ms["ones"], w * h, 2, 2.0) == total / (w * h) + 4.0
    np.testing.assert_array_equal(masked_cluster_sums(idx, px, 16, ms["ones"]), cluster_sums_ref(idx, px, 16))
    np.testing.assert_array_equal(masked_histogram(coord_byte(px, 4), px, 4, ms["ones"]),
                                  histogram_ref(coord_byte(px, 4), px, 4))
    for name in ("bernoulli", "cols3", "values"):
        a, b = ms[name], (ms[name] == 0).astype(np.uint8)
        assert abs(masked_sum(err, a) + masked_sum(err, b) - total) <= 1e-12 * total
        np.testing.assert_array_equal(masked_cluster_sums(idx, px, 16, a) + masked_cluster_sums(idx, px, 16, b),
                                      cluster_sums_ref(idx, px, 16))
        np.testing.assert_array_equal(masked_histogram(coord_byte(px, 4), px, 4, a) +
                                      masked_histogram(coord_byte(px, 4), px, 4, b),
                                      histogram_ref(coord_byte(px, 4), px, 4))


def test_values_1_7_255_mean_the_same():
    m = masks_for(97, 53)["values"]
    assert set(np.unique(m)) == {0, 1, 7, 255}
    err, _, _ = _data(97, 53)
    assert masked_sum(err, m) == masked_sum(err, (m != 0).astype(np.uint8))


def test_de94_has_a_pixel_without_a_number_on_the_oracle():
    """test_mask_gpu.py's NaN case: dE94 of the synthetic palettes 69 .. 76 on the 97 x 53 noise
    image is NaN for several pixels (the reference's fp32 dE94, CL:210-226), so the mask of the
    finite pixels excludes something.  Which pixels are NaN hangs on the Lab's last bits, where
    the device and the oracle differ (test_pixel_errors_de94_vs_oracle): eight palettes with a
    handful of such pixels on the oracle, so that the device has at least one."""
    w, h, K = 97, 53, 16
    R, G, B = o.synthetic_image(w, h, 5)
    rgba = o.inline_rgba(R, G, B).reshape(-1, 4)
    f = o.design_filters(72, 45.0)
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    nan = np.zeros(w * h, bool)
    for seed in range(69, 77):
        pal = o.synthetic_palette(K, seed).reshape(K, 4)
        idx, _ = c_oracle.assign(rgba, pal)
        nan |= np.isnan(o.ciede94_f32(lab, o.candidate_scielab(idx, pal, f, w, h)))
    print(f"pixels without a number for one of the palettes: {int(nan.sum())}")
    assert 4 <= int(nan.sum()) < w * h // 100


def test_the_region_steers_the_seed_on_the_oracle():
    """The inequality test_mask_gpu.py asserts on the device, established here with the oracle and
    seed_ref.py: the median cut of the masked histogram (the blue half) has a strictly lower
    masked cost than the median cut of the whole image's."""
    w, h, K, bits = 64, 32, 4, 5
    rgba, by, mask = two_tone_image(w, h)
    f = o.design_filters(72, 45.0)
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    costs = {}
    for name, m in (("masked", mask), ("whole", np.ones((h, w), np.uint8))):
        pal, made = median_cut_ref(masked_histogram(coord_byte(by, bits), by, bits, m), bits, 255, K)
        assert made == K
        _, parts = c_oracle.eval_palette(rgba, lab, pal.reshape(K, 4), f, w, return_parts=True)
        costs[name] = masked_cost(parts["err"], mask, int(inside(mask).sum()), 0, 2.0)
    print(f"masked cost of the masked seed {costs['masked']!r}, of the whole image's seed {costs['whole']!r}")
    assert costs["masked"] < costs["whole"]

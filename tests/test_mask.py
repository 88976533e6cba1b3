"""The pixel mask's numpy restatements (mask_ref.py) against brute force, and the
seed inequality of test_mask_gpu.py established with the oracle.  No GPU."""

import numpy as np
import pytest

import c_oracle
import oracle as o
from lloyd_ref import cluster_sums_ref
from mask_ref import (inside, live_tiles, live_tiles_brute, masked_cluster_sums, masked_cost, masked_histogram,
                      masked_sum, masks_for, rectangle, tile_grid, tile_masks, tile_weight_maps, two_tone_image)
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


# The launch geometries of test_mask_matrix_gpu.py (test_every_fast_instance_is_reached's sizes):
# name -> (w, h, tile width, tile height, tile columns, tile rows)
GEOMETRIES = {"16x128": (301, 93, 128, 16, 3, 6), "8x108": (301, 93, 108, 8, 3, 12),
              "16x256": (535, 45, 256, 16, 3, 3), "chunked-16x128": (300, 45, 128, 16, 3, 3)}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_tile_masks_cut_the_grid(name):
    """Conditions of test_mask_matrix_gpu.py's inputs: on every launch geometry the masks make
    the skip run and the live list be decoded with more than one tile column."""
    w, h, tw, th, tx, ty = GEOMETRIES[name]
    assert tile_grid(w, 0, h, tw, th)[1:] == (tx, ty) and tx >= 3 and ty >= 3
    ms, maps = tile_masks(w, h, tw, th), tile_weight_maps(w, h, tw, th)
    assert list(ms) == ["ones", "edges", "one_tile", "checker_corners", "seams", "bernoulli"]
    assert list(maps) == list(ms) + ["ramp"]
    for k, m in ms.items():
        assert m.dtype == np.uint8 and m.shape == (h, w) and set(np.unique(m)) <= {0, 1}
        assert live_tiles(m, w, h, tw, th) == live_tiles_brute(m, w, h, tw, th), k
        assert set(np.unique(maps[k])) <= {0, 1, 7, 128, 255} and np.array_equal(maps[k] != 0, m != 0), k
        assert m.sum() < 100 or set(np.unique(maps[k])) >= {1, 7, 128, 255}, k  # (every value, given the pixels)
    every = list(range(tx * ty))
    assert live_tiles(ms["ones"], w, h, tw, th) == every
    assert live_tiles(ms["one_tile"], w, h, tw, th) == [tx + 1] and ms["one_tile"].sum() == tw * th
    assert 0 < len(live_tiles(ms["checker_corners"], w, h, tw, th)) < tx * ty
    assert live_tiles(ms["checker_corners"], w, h, tw, th) == [t for t in every if (t % tx + t // tx) % 2]
    assert len(live_tiles(ms["edges"], w, h, tw, th)) == tx + ty - 1
    assert ms["edges"].sum() == w + h - 1 and ms["edges"][:, w - 1].all() and ms["edges"][h - 1].all()
    assert live_tiles(ms["seams"], w, h, tw, th) == every
    cols = sorted({x for k in range(1, tx) for x in (k * tw - 1, k * tw)})
    rows = sorted({y for j in range(1, ty) for y in (j * th - 1, j * th)})
    want = np.zeros((h, w), bool)
    want[:, cols] = want[rows] = True
    assert np.array_equal(ms["seams"] != 0, want)
    assert 0.45 < ms["bernoulli"].mean() < 0.55 and live_tiles(ms["bernoulli"], w, h, tw, th) == every
    ramp = maps["ramp"].astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(ramp, (xx + yy) % 256) and (ramp == 0).any() and ramp.max() == 255
    assert live_tiles(maps["ramp"], w, h, tw, th) == every
    other = tile_masks(w + 1, h, tw, th)["bernoulli"]  # seeded from (w, h, tw, th)
    assert not np.array_equal(other[:, :w], ms["bernoulli"])


@pytest.mark.parametrize("de2000", [False, True])
def test_tile_masks_of_a_shard(de2000):
    """The grid of the rows [r0, r1): from r0, or for dE2000 from the image's tile row."""
    w, h, tw, th, r0, r1 = 301, 93, 128, 16, 37, 92
    g0, tx, ty = tile_grid(w, r0, r1, tw, th, de2000)
    assert (g0, tx, ty) == ((32, 3, 4) if de2000 else (37, 3, 4))
    for k, m in tile_masks(w, h, tw, th, r0, r1, de2000).items():
        assert live_tiles(m, w, h, tw, th, r0, r1, de2000) == live_tiles_brute(m, w, h, tw, th, r0, r1, de2000), k
    ms = tile_masks(w, h, tw, th, r0, r1, de2000)
    assert live_tiles(ms["one_tile"], w, h, tw, th, r0, r1, de2000) == [tx + 1]
    assert len(live_tiles(ms["edges"], w, h, tw, th, r0, r1, de2000)) == tx + ty - 1
    assert not ms["edges"][:r0].any() and not ms["edges"][r1:].any() and ms["edges"][r1 - 1].all()
    first = g0 + th  # the first inner boundary's two rows
    assert ms["seams"][first - 1:first + 1].all() and not ms["seams"][first + 1, 5]


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


@pytest.mark.parametrize("w,h,K,P", [(301, 93, 64, 2), (535, 45, 64, 2), (300, 45, 300, 1)])
def test_de94_share_without_a_number_on_the_matrix_images(w, h, K, P):
    """test_mask_matrix_gpu.py takes the pixels whose dE94 is NaN out of every mask and asserts that
    they are less than 1% of the image.  The oracle's share on its images and palettes
    (test_dispatch_gpu's _image and _pals, restated) at half-width 10 is held to a tenth of that:
    which pixels are NaN hangs on the Lab's last bits, where the device differs.  The same
    over every half-width of its matrix (7 .. 24) and every K of CHUNKS (300 .. 8192), run once:
    5 to 21 pixels of 27993, 24075 and 13500, at most 8.9e-4."""
    R, G, B = (np.ascontiguousarray(np.round(x * 255) / np.float32(255), np.float32) for x in o.synthetic_image(w, h, seed=w + h))
    rgba = o.inline_rgba(R, G, B).reshape(-1, 4)
    f = o.design_filters(72, 45.0)
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    nan = np.zeros(w * h, bool)
    for p in range(P):
        pal = o.synthetic_palette(K, 70 + 3 * K + p).astype(np.float32).reshape(K, 4)
        idx, _ = c_oracle.assign(rgba, pal)
        nan |= np.isnan(o.ciede94_f32(lab, o.candidate_scielab(idx, pal, f, w, h)))
    print(f"{w} x {h}, K = {K}: {int(nan.sum())} of {w * h} pixels without a number")
    assert int(nan.sum()) < w * h // 1000


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

"""numpy restatements of the pixel weights (hq_set_weights) as include/hq.h states them,
nothing of libhq's: the weighted cost, the weighted cluster sums and histogram, the
live-tile count and the weight maps the tests use.  Sums that int64 or float64 could not
prove (w q(v) up to 255 2^32 per pixel, totals up to 2^63) are Python ints in object arrays."""

import numpy as np

from mask_ref import live_tiles

LIMIT = 1 << 31  # the planar form's sums are safe while the owned weights sum to less


def weights_flat(weights):
    """The weights as Python-int-safe int64 (h w,); bytes 0 .. 255."""
    w = np.asarray(weights).reshape(-1).astype(np.int64)
    assert w.min() >= 0 and w.max() <= 255
    return w


def weight_sum(weights):
    return int(weights_flat(weights).sum())


def nonzero(weights):
    return int(np.count_nonzero(weights_flat(weights)))


def weighted_sum(err, weights):
    """float64 sum of w dE over the pixels of non-zero weight: a select, so a NaN under weight
    0 does not reach it.  Each product is exact in float64 (24 bits by 8)."""
    w = weights_flat(weights)
    e = np.asarray(err, np.float64).reshape(-1)
    m = w != 0
    return float((e[m] * w[m].astype(np.float64)).sum())


def weighted_cost(err, weights, w_full, unused, delta):
    """costs[p] = (sum of w dE over the owned pixels with w > 0) / W + delta #unused, W the
    weight sum of the FULL image (err and weights may be a shard's rows)."""
    return weighted_sum(err, weights) / float(w_full) + float(delta) * int(unused)


def weighted_cluster_sums(idx, px, K, weights):
    """(K, 4) object array of Python ints: (sum w R, sum w G, sum w B, sum w) of integer pixels
    px (n, 3) under the index image idx (n,), over the pixels of non-zero weight."""
    w = weights_flat(weights)
    idx = np.asarray(idx).reshape(-1).astype(np.int64)
    px = np.asarray(px, np.int64)
    out = np.zeros((K, 4), object)
    m = np.flatnonzero(w)
    wo = w[m].astype(object)
    for ch in range(3):
        np.add.at(out[:, ch], idx[m], px[m, ch].astype(object) * wo)
    np.add.at(out[:, 3], idx[m], wo)
    return out


def weighted_histogram(coords, px, bits, weights):
    """(2^(3 bits), 4) object array of Python ints, the cells weighted the same way."""
    coords = np.asarray(coords, np.int64)
    cell = (coords[:, 0] << (2 * bits)) | (coords[:, 1] << bits) | coords[:, 2]
    return weighted_cluster_sums(cell, px, 1 << (3 * bits), weights)


def as_int64(a):
    """An object array of Python ints as int64, asserting that every entry fits (< 2^63)."""
    a = np.asarray(a, object)
    assert all(0 <= int(v) < (1 << 63) for v in a.reshape(-1))
    return a.astype(np.int64)


def live_tile_count(weights, w, h, tw, th, r0=0, r1=None, de2000=False):
    """Tiles of the fast cost launch that hold an owned pixel of non-zero weight."""
    return len(live_tiles(np.asarray(weights).reshape(h, w), w, h, tw, th, r0, r1, de2000))


def weight_maps(w, h):
    """The tests' weight maps of an (h, w) image, name -> uint8 (h, w).  The horizontal
    gradient is the ramp 0 .. 255 over the columns (w <= 300: no four consecutive pixels
    alike); the vertical one the ramp over the rows with the column's two low bits XORed in, so
    that it too differs within every quad of four consecutive pixels and still spans 0 .. 255."""
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(4321 + 7 * w + h)
    hgrad = xx * 255 // max(w - 1, 1)
    vgrad = (yy * 255 // max(h - 1, 1)) ^ (xx & 3)
    noise = rng.integers(0, 256, (h, w))
    noise[h // 4:max(h // 4 + 1, 3 * h // 4), w // 4:max(w // 4 + 1, 3 * w // 4)] = 0
    corners = np.zeros((h, w), np.int64)
    corners[0, 0], corners[0, w - 1], corners[h - 1, 0], corners[h - 1, w - 1] = 1, 7, 255, 128
    out = {
        "hgrad": hgrad,
        "vgrad": vgrad,
        "noise": noise,
        "corners": corners,
        "all255": np.full((h, w), 255),
        "zeros_ones": (rng.random((h, w)) < 0.5).astype(np.int64),
    }
    for k in out:  # (tiny images: never all zero)
        out[k] = np.ascontiguousarray(out[k], np.uint8)
        if not out[k].any():
            out[k][h - 1, w - 1] = 3
    return out

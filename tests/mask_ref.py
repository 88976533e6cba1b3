"""numpy restatements of the pixel mask (hq_set_mask) as include/hq.h states it,
nothing of libhq's: the masked cost, the masked cluster sums and histogram (the
unmasked restatements of lloyd_ref.py and seed_ref.py over the in-mask pixels),
the live-tile list of the fast cost launch and the masks the tests use."""

import numpy as np

from lloyd_ref import cluster_sums_ref
from seed_ref import histogram_ref


def inside(mask):
    """Flat bool array: non-zero = the pixel counts (1, 7 and 255 mean the same)."""
    return np.asarray(mask).reshape(-1) != 0


def masked_sum(err, mask):
    """float64 sum of the per-pixel dE over the in-mask pixels: a select, so a masked-out
    NaN does not reach it."""
    return float(np.asarray(err, np.float64).reshape(-1)[inside(mask)].sum())


def masked_cost(err, mask, n_full, unused, delta):
    """costs[p] = (sum over in-mask pixels of dE) / N + delta #unused, N the in-mask pixels
    of the FULL image (err and mask may be a shard's rows)."""
    return masked_sum(err, mask) / float(n_full) + float(delta) * int(unused)


def masked_cluster_sums(idx, px, K, mask):
    m = inside(mask)
    return cluster_sums_ref(np.asarray(idx).reshape(-1)[m], np.asarray(px)[m], K)


def masked_histogram(coords, px, bits, mask):
    m = inside(mask)
    return histogram_ref(np.asarray(coords)[m], np.asarray(px)[m], bits)


def tile_grid(w, r0, r1, tw, th, de2000=False):
    """(grid_row0, tiles_x, tiles_y) of the fast cost launch over rows [r0, r1): tiles of
    tw x th from row r0, or for dE2000 from the image's tile row that holds r0."""
    g0 = r0 // th * th if de2000 else r0
    return g0, -(-w // tw), -(-(r1 - g0) // th)


def live_tiles(mask, w, h, tw, th, r0=0, r1=None, de2000=False):
    """Ascending numbers ty tiles_x + tx of the tiles that hold an in-mask pixel of the owned
    rows [r0, r1) of the (h, w) mask."""
    r1 = h if r1 is None else r1
    g0, tx, ty = tile_grid(w, r0, r1, tw, th, de2000)
    m = inside(mask).reshape(h, w)
    out = []
    for j in range(ty):
        y0, y1 = max(g0 + j * th, r0), min(g0 + (j + 1) * th, r1)
        for i in range(tx):
            if m[y0:y1, i * tw:(i + 1) * tw].any():
                out.append(j * tx + i)
    return out


def live_tiles_brute(mask, w, h, tw, th, r0=0, r1=None, de2000=False):
    """The same pixel by pixel."""
    r1 = h if r1 is None else r1
    g0, tx, _ = tile_grid(w, r0, r1, tw, th, de2000)
    m = inside(mask).reshape(h, w)
    s = set()
    for y in range(r0, r1):
        for x in range(w):
            if m[y, x]:
                s.add((y - g0) // th * tx + x // tw)
    return sorted(s)


def masks_for(w, h, worst=None):
    """The tests' masks of an (h, w) image, name -> uint8 (h, w); worst: the position of the
    single-pixel mask (the pixel whose dE is largest for palette 0)."""
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(1234 + 7 * w + h)
    out = {
        "ones": np.ones((h, w), np.uint8),
        "bernoulli": (rng.random((h, w)) < 0.5).astype(np.uint8),
        "cols3": (xx % 3 == 0).astype(np.uint8),
        "edges": ((xx == w - 1) | (yy == h - 1)).astype(np.uint8),
        "values": np.where(rng.random((h, w)) < 0.5, 0, rng.choice(np.array([1, 7, 255], np.uint8), (h, w))).astype(np.uint8),
    }
    for k in ("bernoulli", "values"):  # (tiny images: never empty)
        if not out[k].any():
            out[k][0, 0] = 1 if k == "bernoulli" else 7
    if worst is not None:
        one = np.zeros((h, w), np.uint8)
        one.reshape(-1)[int(worst)] = 1
        out["worst"] = one
    return out


def tile_masks(w, h, tw, th, r0=0, r1=None, de2000=False):
    """Masks cut along the tile grid of one fast cost launch (tiles of tw x th over the rows
    [r0, r1), tile_grid's), name -> uint8 (h, w) of the full image; at least 2 x 2 tiles.  They
    make the live-tile list differ wherever a tile width, a tile height or tiles_x is wrong:
    edges: column w - 1 and row r1 - 1 only, the partial last tile column and row;
    one_tile: every pixel of the interior tile (1, 1) and nothing else;
    checker_corners: the four corner pixels of every tile with tx + ty odd;
    seams: the two pixel columns and the two rows at every inner tile boundary."""
    r1 = h if r1 is None else r1
    g0, tx, ty = tile_grid(w, r0, r1, tw, th, de2000)
    assert tx >= 2 and ty >= 2, (w, h, tw, th, r0, r1)
    xs = [(i * tw, min((i + 1) * tw, w)) for i in range(tx)]
    ys = [(max(g0 + j * th, r0), min(g0 + (j + 1) * th, r1)) for j in range(ty)]
    own = np.zeros((h, w), bool)
    own[r0:r1] = True
    edges, one, checker, seams = (np.zeros((h, w), bool) for _ in range(4))
    edges[:, w - 1] = edges[r1 - 1] = True
    one[ys[1][0]:ys[1][1], xs[1][0]:xs[1][1]] = True
    for j, (y0, y1) in enumerate(ys):
        for i, (x0, x1) in enumerate(xs):
            if (i + j) % 2:
                checker[np.ix_((y0, y1 - 1), (x0, x1 - 1))] = True
    for x0, _ in xs[1:]:
        seams[:, x0 - 1:x0 + 1] = True
    for y0, _ in ys[1:]:
        seams[y0 - 1:y0 + 1] = True
    rng = np.random.default_rng([w, h, tw, th])
    out = {"ones": np.ones((h, w), bool), "edges": edges & own, "one_tile": one, "checker_corners": checker,
           "seams": seams & own, "bernoulli": rng.random((h, w)) < 0.5}
    return {k: np.ascontiguousarray(v, np.uint8) for k, v in out.items()}


TILE_WEIGHTS = np.array([1, 7, 128, 255], np.uint8)


def tile_weight_maps(w, h, tw, th, r0=0, r1=None, de2000=False):
    """tile_masks' supports with weights drawn from {1, 7, 128, 255}, and ramp: (x + y) % 256,
    which has zeros -> name -> uint8 (h, w)."""
    rng = np.random.default_rng([w, h, tw, th, 1])
    out = {k: np.where(m != 0, rng.choice(TILE_WEIGHTS, (h, w)), 0).astype(np.uint8)
           for k, m in tile_masks(w, h, tw, th, r0, r1, de2000).items()}
    yy, xx = np.mgrid[0:h, 0:w]
    out["ramp"] = ((xx + yy) % 256).astype(np.uint8)
    return out


def two_tone_image(w=64, h=32):
    """A k/255 image whose left half is shades of blue and right half shades of red, and the
    mask of the left half -> (rgba (n, 4) float32, bytes (n, 3) int64, mask uint8 (h, w))."""
    yy, xx = np.mgrid[0:h, 0:w]
    left = xx < w // 2
    strong = 40 + 6 * (xx % (w // 2)) + (yy % 8)         # 40 .. 233
    weak = 5 + 2 * (yy % 16)                             # 5 .. 35
    by = np.stack([np.where(left, weak, strong), weak // 2 + 3, np.where(left, strong, weak)], -1).reshape(-1, 3)
    by = by.astype(np.int64)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)  # (the fp32 quotient: the lattice the library detects)
    return rgba, by, left.astype(np.uint8)


def rectangle(w, h, x0, x1, y0, y1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m

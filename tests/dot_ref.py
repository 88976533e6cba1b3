"""numpy restatement of hq_dot_population's index images, written from include/hq.h's text:
Knuth's dot diffusion in the argmin's space, every operation one fp32 operation rounded to
nearest (numpy float32 arithmetic: no fma), the argmin oracle.assign (which takes the device's
v_sqrt_f32 once the gpu fixture has installed it).  Nothing of libhq's is used here.

A class matrix of side n in {4, 8, 16}, a permutation of 0 .. n n - 1, tiled over the image,
gives pixel (x, y) the class cls[y mod n, x mod n].  The 8 neighbours weigh 2 (orthogonal) or 1
(diagonal).  Pixels are taken in ascending class:

    W(p)   = the summed weights of p's in-image neighbours of higher class
    a(q)   = +0, then a = a + (float(wt(p, q)) * e(p)) / float(W(p)) over q's in-image
             neighbours p of lower class, in ascending class of p
    v      = min(max(pix(q) + s * a(q), 0), 1)
    idx(q) = the first minimum over k of ref_dist(v, pal[k])
    e(q)   = v - pal[idx]

dot() takes a class at a time, all its pixels at once, gathering; dot_scatter() is the
definition pixel by pixel, each finished pixel adding its shares into a(.) of its neighbours.
"""

import numpy as np

import oracle as o

f32 = np.float32

# (dx, dy, weight) of the eight neighbours
NEIGHBOURS = ((-1, -1, 1), (0, -1, 2), (1, -1, 1), (-1, 0, 2), (1, 0, 2), (-1, 1, 1), (0, 1, 2), (1, 1, 1))

# Knuth's 8 x 8 class matrix, row by row (hq.h: HQ_DOT_KNUTH8)
KNUTH8 = np.array([[34, 48, 40, 32, 29, 15, 23, 31],
                   [42, 58, 56, 53, 21, 5, 7, 10],
                   [50, 62, 61, 45, 13, 1, 2, 18],
                   [38, 46, 54, 37, 25, 17, 9, 26],
                   [28, 14, 22, 30, 35, 49, 41, 33],
                   [20, 4, 6, 11, 43, 59, 57, 52],
                   [12, 0, 3, 19, 51, 63, 60, 44],
                   [24, 16, 8, 27, 39, 47, 55, 36]], np.int32)


def legal(n, cls):
    """hq.h's rule: side 4, 8 or 16, and the first n n entries a permutation of 0 .. n n - 1."""
    if n not in (4, 8, 16):
        return False
    c = [int(v) for v in np.asarray(cls).reshape(-1)[:n * n]]
    return len(c) == n * n and sorted(c) == list(range(n * n))


def barons(cls):
    """Cells whose 8 neighbours on the torus all have a lower class."""
    c = np.asarray(cls)
    n = c.shape[0]
    count = 0
    for y in range(n):
        for x in range(n):
            count += all(c[(y + dy) % n, (x + dx) % n] < c[y, x] for dx, dy, _ in NEIGHBOURS)
    return count


def random_classes(n, seed):
    """A random permutation as an (n, n) class matrix."""
    return np.random.default_rng(seed).permutation(n * n).astype(np.int32).reshape(n, n)


def class_image(cls, w, h):
    c = np.asarray(cls, np.int32)
    n = c.shape[0]
    return c[np.arange(h)[:, None] % n, np.arange(w)[None, :] % n]


def weight_sums(ci):
    """W(p) for every pixel of the class image ci (h, w), as int."""
    h, w = ci.shape
    big = np.full((h + 2, w + 2), -1, np.int64)  # outside the image: never higher
    big[1:-1, 1:-1] = ci
    W = np.zeros((h, w), np.int64)
    for dx, dy, wt in NEIGHBOURS:
        W += wt * (big[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] > ci)
    return W


def _prepare(rgb3, palette4, w, h, s, classes):
    cls = KNUTH8 if classes is None else np.asarray(classes, np.int32)
    assert legal(cls.shape[0], cls) and cls.shape[0] == cls.shape[1]
    px = np.ascontiguousarray(np.asarray(rgb3, f32)[:, :3]).reshape(h, w, 3)
    pal = np.ascontiguousarray(np.asarray(palette4, f32).reshape(-1, 4))
    return cls, px, pal, f32(s)


def _finish(idx, K):
    used = np.zeros(K, np.int32)
    used[np.unique(idx)] = 1
    return idx.reshape(-1), used


def dot(rgb3, palette4, w, h, s, classes=None):
    """-> (idx int32 [w h], used int32 [K]), a class at a time, gathering."""
    cls, px, pal, s = _prepare(rgb3, palette4, w, h, s, classes)
    n = cls.shape[0]
    ci = class_image(cls, w, h)
    W = weight_sums(ci).astype(f32)
    err = np.zeros((h, w, 3), f32)
    idx = np.zeros((h, w), np.int32)
    cells = {int(cls[cy, cx]): (cx, cy) for cy in range(n) for cx in range(n)}
    for k in range(n * n):
        cx, cy = cells[k]
        if cx >= w or cy >= h:
            continue  # a class without a pixel
        Y, X = np.meshgrid(np.arange(cy, h, n), np.arange(cx, w, n), indexing="ij")
        # the cell's neighbours of lower class, in ascending class (taken on the torus)
        lower = sorted((int(cls[(cy + dy) % n, (cx + dx) % n]), dx, dy, wt) for dx, dy, wt in NEIGHBOURS
                       if cls[(cy + dy) % n, (cx + dx) % n] < k)
        a = np.zeros(Y.shape + (3,), f32)
        for _, dx, dy, wt in lower:
            PX, PY = X + dx, Y + dy
            ok = (PX >= 0) & (PX < w) & (PY >= 0) & (PY < h)
            sx, sy = np.where(ok, PX, 0), np.where(ok, PY, 0)
            div = np.where(ok, W[sy, sx], f32(1))  # (q is a higher neighbour of p: W(p) >= wt)
            share = (f32(wt) * err[sy, sx]) / div[..., None]
            a = np.where(ok[..., None], a + share, a)
        v = np.minimum(np.maximum(px[Y, X] + s * a, f32(0)), f32(1))
        kk = o.assign(v.reshape(-1, 3), pal)[0].reshape(Y.shape)
        idx[Y, X] = kk
        err[Y, X] = v - pal[kk, :3]
    return _finish(idx, len(pal))


def dot_scatter(rgb3, palette4, w, h, s, classes=None):
    """The definition pixel by pixel: pixels in ascending class (within a class in raster
    order), each finished pixel adding its shares to a(.) of its higher neighbours."""
    cls, px, pal, s = _prepare(rgb3, palette4, w, h, s, classes)
    ci = class_image(cls, w, h)
    a = np.zeros((h, w, 3), f32)
    idx = np.zeros((h, w), np.int32)
    order = sorted((int(ci[y, x]), y, x) for y in range(h) for x in range(w))
    for _, y, x in order:
        v = np.minimum(np.maximum(px[y, x] + s * a[y, x], f32(0)), f32(1))
        k = int(o.assign(v[None, :], pal)[0][0])
        idx[y, x] = k
        e = v - pal[k, :3]
        to = [(x + dx, y + dy, wt) for dx, dy, wt in NEIGHBOURS
              if 0 <= x + dx < w and 0 <= y + dy < h and ci[y + dy, x + dx] > ci[y, x]]
        if not to:
            continue  # a baron, or an edge's: the error is dropped
        W = f32(sum(wt for _, _, wt in to))
        for qx, qy, wt in to:
            a[qy, qx] = a[qy, qx] + (f32(wt) * e) / W
    return _finish(idx, len(pal))

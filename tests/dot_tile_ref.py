"""numpy restatements for dot diffusion's tiled form, written from include/hq.h's text: the
reach of a class matrix in four directions (hq_dot_reach2), its levels (hq_dot_levels) and the
rendering restricted to a window (dot_ref's scatter form with whole-image classes and W(p)).
Nothing of libhq's is used here.
"""

import numpy as np

import oracle as o
from dot_ref import NEIGHBOURS, _prepare, class_image, weight_sums

f32 = np.float32


def reach2(cls):
    """(above, below, left, right): in ascending class, for a cell c and each neighbour p of
    lower class at offset (dx, dy) on the torus,
        above[c] = max(above[c], above[p] - dy)    below[c] = max(below[c], below[p] + dy)
        left[c]  = max(left[c],  left[p] - dx)     right[c] = max(right[c], right[p] + dx)
    all from 0; the result is the maximum over the cells."""
    c = np.asarray(cls)
    n = c.shape[0]
    ext = np.zeros((n, n, 4), np.int64)
    for k in range(n * n):
        cy, cx = (int(v[0]) for v in np.where(c == k))
        for dx, dy, _ in NEIGHBOURS:
            py, px = (cy + dy) % n, (cx + dx) % n
            if c[py, px] < k:
                shifted = ext[py, px] + np.array([-dy, dy, -dx, dx])
                ext[cy, cx] = np.maximum(ext[cy, cx], shifted)
    return tuple(int(v) for v in ext.reshape(-1, 4).max(axis=0))


def levels(cls):
    """(level (n, n), depth): level 0 for a cell without a neighbour of lower class on the
    torus, else 1 + the largest level among those neighbours; depth = 1 + the largest level."""
    c = np.asarray(cls)
    n = c.shape[0]
    lv = np.zeros((n, n), np.int32)
    for k in range(n * n):
        cy, cx = (int(v[0]) for v in np.where(c == k))
        below = [lv[(cy + dy) % n, (cx + dx) % n] for dx, dy, _ in NEIGHBOURS if c[(cy + dy) % n, (cx + dx) % n] < k]
        lv[cy, cx] = 1 + max(below) if below else 0
    return lv, int(lv.max()) + 1


def row_major(n=16):
    return np.arange(n * n, dtype=np.int32).reshape(n, n)


def column_major(n=16):
    return row_major(n).T.copy()


def dot_window(rgb3, palette4, w, h, s, classes, x0, y0, x1, y1):
    """The scatter form over the window [x0, x1) x [y0, y1) of the image alone: the classes
    and W(p) are the whole image's, a pixel outside the window neither gives nor takes.
    -> idx int32 (y1 - y0, x1 - x0)."""
    cls, px, pal, s = _prepare(rgb3, palette4, w, h, s, classes)
    ci = class_image(cls, w, h)
    W = weight_sums(ci)
    a = np.zeros((h, w, 3), f32)
    idx = np.zeros((h, w), np.int32)
    order = sorted((int(ci[y, x]), y, x) for y in range(y0, y1) for x in range(x0, x1))
    for _, y, x in order:
        v = np.minimum(np.maximum(px[y, x] + s * a[y, x], f32(0)), f32(1))
        k = int(o.assign(v[None, :], pal)[0][0])
        idx[y, x] = k
        e = v - pal[k, :3]
        if W[y, x] == 0:
            continue
        for dx, dy, wt in NEIGHBOURS:
            qx, qy = x + dx, y + dy
            if x0 <= qx < x1 and y0 <= qy < y1 and ci[qy, qx] > ci[y, x]:
                a[qy, qx] = a[qy, qx] + (f32(wt) * e) / f32(W[y, x])
    return idx[y0:y1, x0:x1]


def tiled(rgb3, palette4, w, h, s, classes, tw, th, reach):
    """Every tw x th tile rendered from its own window -- the tile extended by the reach
    (above, below, left, right), clipped to the image -- and only the tile's pixels kept."""
    above, below, left, right = reach
    out = np.zeros((h, w), np.int32)
    for ty in range(0, h, th):
        for tx in range(0, w, tw):
            x0, y0 = max(tx - left, 0), max(ty - above, 0)
            x1, y1 = min(tx + tw + right, w), min(ty + th + below, h)
            win = dot_window(rgb3, palette4, w, h, s, classes, x0, y0, x1, y1)
            ex, ey = min(tx + tw, w), min(ty + th, h)
            out[ty:ey, tx:ex] = win[ty - y0:ey - y0, tx - x0:ex - x0]
    return out.reshape(-1)

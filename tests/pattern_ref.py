"""numpy restatement of hq_pattern_population's index images (include/hq.h): pattern dithering in
the argmin's space, every operation one fp32 operation rounded to nearest (numpy float32
arithmetic: no fma), the distance and its first-minimum rule ordered_ref.py's (oracle.assign).

    Y_k = ((0.299f R_k) + (0.587f G_k)) + (0.114f B_k);  rank: the colours' order by (Y_k, k)
    e = 0;  for i < n:  v = min(max(pix + e strength, 0), 1);  k_i = argmin(v);  e = e + (pix - pal[k_i])
    s = the k_i sorted by rank;  m = map[(y mod mh) mw + (x mod mw)]
    r = min((int)((m + 0.5f) (float)n), n - 1);  idx(x, y) = s_r
"""

import numpy as np

import oracle as o
from ordered_ref import bayer

f32 = np.float32


def luminance_order(palette4):
    """-> (rank int64 [K], color int64 [K]): colour k's position by (Y, k), and its inverse."""
    pal = np.asarray(palette4, f32).reshape(-1, 4)
    y = ((f32(0.299) * pal[:, 0]) + (f32(0.587) * pal[:, 1])) + (f32(0.114) * pal[:, 2])
    assert y.dtype == f32
    color = np.lexsort((np.arange(len(pal)), y))
    rank = np.empty_like(color)
    rank[color] = np.arange(len(pal))
    return rank, color


def pattern(rgb3, palette4, w, h, n, strength, tmap=None, y0=0):
    """-> (idx int32 [w h], used int32 [K]) of the rows y0 .. y0 + h - 1 (rgb3 holds those rows)."""
    tmap = bayer(4) if tmap is None else np.asarray(tmap, f32)
    pal = np.ascontiguousarray(np.asarray(palette4, f32).reshape(-1, 4))
    pix = np.ascontiguousarray(np.asarray(rgb3, f32)[:, :3])
    rank, color = luminance_order(pal)
    e = np.zeros_like(pix)
    ranks = np.empty((n, len(pix)), np.int64)
    for i in range(n):
        v = np.minimum(np.maximum(pix + e * f32(strength), f32(0)), f32(1))
        k = o.assign(v, pal)[0]
        e = e + (pix - pal[k, :3])
        ranks[i] = rank[k]
    assert e.dtype == f32
    mh, mw = tmap.shape
    m = tmap[(np.arange(h) + y0)[:, None] % mh, np.arange(w)[None, :] % mw].reshape(-1)
    r = np.minimum(((m + f32(0.5)) * f32(n)).astype(np.int64), n - 1)
    idx = color[np.sort(ranks, axis=0)[r, np.arange(len(pix))]].astype(np.int32)
    used = np.zeros(len(pal), np.int32)
    used[np.unique(idx)] = 1
    return idx, used

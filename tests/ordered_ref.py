"""numpy restatement of hq_ordered_population's index images (include/hq.h):
ordered (threshold-map) dithering in the argmin's space, every operation one fp32 operation
rounded to nearest (numpy float32 arithmetic: no fma), the argmin oracle.assign (which takes
the device's v_sqrt_f32 once the gpu fixture has installed it).

    m   = map[(y mod mh) * mw + (x mod mw)]      x, y: the position in the full image
    t_c = amp[c] * m
    v_c = min(max(pix_c + t_c, 0), 1)
    idx(x, y) = the first minimum over k of ref_dist(v, pal[k])

bayer(L) is hq_bayer_map by its integer rule.
"""

import numpy as np

import oracle as o

f32 = np.float32


def bayer_rank(L):
    """B(x, y) of the Bayer map of side 2**L, int64 [n, n] (row y, column x)."""
    n = 1 << L
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    B = np.zeros((n, n), np.int64)
    for i in range(L):
        B |= (((x ^ y) >> i) & 1) << (2 * (L - 1 - i) + 1)
        B |= ((y >> i) & 1) << (2 * (L - 1 - i))
    return B


def bayer(L):
    """float32 [n, n]: (B + 0.5) / n**2 - 0.5, in fp32 operations (each exact)."""
    n = 1 << L
    return (bayer_rank(L).astype(f32) + f32(0.5)) * (f32(1) / f32(n * n)) - f32(0.5)


def amp3(amp):
    a = np.asarray(amp, f32).reshape(-1)
    return np.repeat(a, 3) if a.size == 1 else a


def ordered_values(rgb3, w, h, amp, tmap=None, y0=0):
    """The values the argmin reads, float32 [h w, 3], of the rows y0 .. y0 + h - 1 (rgb3 holds
    those rows only; y0: the full-image row of its first)."""
    tmap = bayer(4) if tmap is None else np.asarray(tmap, f32)
    mh, mw = tmap.shape
    px = np.ascontiguousarray(np.asarray(rgb3, f32)[:, :3]).reshape(h, w, 3)
    m = tmap[(np.arange(h) + y0)[:, None] % mh, np.arange(w)[None, :] % mw]
    t = amp3(amp)[None, None, :] * m[:, :, None]
    v = np.minimum(np.maximum(px + t, f32(0)), f32(1))
    assert v.dtype == f32
    return v.reshape(-1, 3)


def ordered(rgb3, palette4, w, h, amp, tmap=None, y0=0):
    """-> (idx int32 [w h], used int32 [K])."""
    pal = np.ascontiguousarray(np.asarray(palette4, f32).reshape(-1, 4))
    idx = o.assign(ordered_values(rgb3, w, h, amp, tmap, y0), pal)[0].astype(np.int32)
    used = np.zeros(len(pal), np.int32)
    used[np.unique(idx)] = 1
    return idx.reshape(-1), used

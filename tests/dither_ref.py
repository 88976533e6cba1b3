"""numpy restatement of hq_dither_population's index images (include/hq.h):
raster Floyd-Steinberg error diffusion in the argmin's space, every operation one fp32
operation rounded to nearest (numpy float32 arithmetic: no fma), the argmin oracle.assign
(which takes the device's v_sqrt_f32 once the gpu fixture has installed it).

    a = 7 e(x-1, y)   b = 3 e(x+1, y-1)   c = 5 e(x, y-1)   d = e(x-1, y-1)
    t = ((a + b) + (c + d)) * 0.0625
    v = min(max(pix + s * t, 0), 1)
    idx(x, y) = the first minimum over k of ref_dist(v, pal[k])
    e(x, y) = v - pal[idx]

dither() goes by the wavefronts t = x + 2 y, vectorised per wavefront; dither_raster() is
the definition's own order, pixel by pixel, for checking the former on tiny images.
"""

import numpy as np

import oracle as o

f32 = np.float32


def _value(pix, el, eur, eu, eul, s):
    a = f32(7) * el
    b = f32(3) * eur
    c = f32(5) * eu
    t = ((a + b) + (c + eul)) * f32(0.0625)
    m = s * t
    return np.minimum(np.maximum(pix + m, f32(0)), f32(1))


def _prepare(rgb3, palette4, w, h, s):
    px = np.ascontiguousarray(np.asarray(rgb3, f32)[:, :3]).reshape(h, w, 3)
    pal = np.ascontiguousarray(np.asarray(palette4, f32).reshape(-1, 4))
    err = np.zeros((h + 1, w + 2, 3), f32)  # e(x, y) at [y + 1, x + 1]; zero outside the image
    return px, pal, err, f32(s)


def _finish(idx, K):
    used = np.zeros(K, np.int32)
    used[np.unique(idx)] = 1
    return idx.reshape(-1), used


def dither(rgb3, palette4, w, h, s):
    """-> (idx int32 [w h], used int32 [K]) by wavefronts."""
    px, pal, err, s = _prepare(rgb3, palette4, w, h, s)
    idx = np.zeros((h, w), np.int32)
    for t in range(w + 2 * (h - 1)):
        ys = np.arange(max(0, (t - w + 2) // 2), min(h - 1, t // 2) + 1)
        xs = t - 2 * ys
        v = _value(px[ys, xs], err[ys + 1, xs], err[ys, xs + 2], err[ys, xs + 1], err[ys, xs], s)
        k = o.assign(v, pal)[0]
        idx[ys, xs] = k
        err[ys + 1, xs + 1] = v - pal[k, :3]
    return _finish(idx, len(pal))


def dither_raster(rgb3, palette4, w, h, s):
    """The same in raster order, one pixel at a time."""
    px, pal, err, s = _prepare(rgb3, palette4, w, h, s)
    idx = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            v = _value(px[y, x], err[y + 1, x], err[y, x + 2], err[y, x + 1], err[y, x], s)
            k = int(o.assign(v[None, :], pal)[0][0])
            idx[y, x] = k
            err[y + 1, x + 1] = v - pal[k, :3]
    return _finish(idx, len(pal))


def ramp_image(w, h):
    """The RGB ramp of the issue's table: R along x, G along y, B along the diagonal, k/255."""
    x = np.arange(w)[None, :].repeat(h, 0)
    y = np.arange(h)[:, None].repeat(w, 1)
    by = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1)
    rgba = np.zeros((w * h, 4), f32)
    rgba[:, :3] = by.reshape(-1, 3).astype(f32) / f32(255)
    return rgba


def cube_corners():
    """The eight corners of the RGB cube as a palette [8, 4]."""
    pal = np.zeros((8, 4), f32)
    for k in range(8):
        pal[k, :3] = [(k >> 2) & 1, (k >> 1) & 1, k & 1]
    return pal

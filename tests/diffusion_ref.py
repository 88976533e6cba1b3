"""numpy restatement of hq_diffuse_population's index images (include/hq.h):
raster error diffusion under a diffusion kernel in scatter notation -- w[dy][dx + 2] / div is
the share pixel (x, y) sends to (x + dx, y + dy) -- in the argmin's space, every operation one
fp32 operation rounded to nearest (numpy float32 arithmetic: no fma), the argmin oracle.assign
(which takes the device's v_sqrt_f32 once the gpu fixture has installed it).

    acc = the products float(w[dy][dx+2]) * e(x-dx, y-dy) of the non-zero taps, added one at a
          time in the order dy = 0 (dx = 1, 2), dy = 1 (dx = -2 .. 2), dy = 2 (dx = -2 .. 2);
          acc starts as the first product
    t   = acc / float(div)
    v   = min(max(pix + s * t, 0), 1)
    idx(x, y) = the first minimum over k of ref_dist(v, pal[k])
    e(x, y) = v - pal[idx]

diffuse_raster() is the definition's own order, pixel by pixel; diffuse() goes by the wavefronts
t = x + S y of the tap set's slope S (classify), vectorised per wavefront.  Also here: the
preset table, the legality rule and the (R, S) classification, restated from hq.h.
"""

import numpy as np

import oracle as o

f32 = np.float32

# name: (rows dy = 0 .. 2 of the weights at dx = -2 .. 2, div); hq.h's enum order
PRESETS = {
    "floyd_steinberg": ([[0, 0, 0, 7, 0], [0, 3, 5, 1, 0], [0, 0, 0, 0, 0]], 16),
    "jarvis": ([[0, 0, 0, 7, 5], [3, 5, 7, 5, 3], [1, 3, 5, 3, 1]], 48),
    "stucki": ([[0, 0, 0, 8, 4], [2, 4, 8, 4, 2], [1, 2, 4, 2, 1]], 42),
    "burkes": ([[0, 0, 0, 8, 4], [2, 4, 8, 4, 2], [0, 0, 0, 0, 0]], 32),
    "sierra3": ([[0, 0, 0, 5, 3], [2, 4, 5, 4, 2], [0, 2, 3, 2, 0]], 32),
    "sierra2": ([[0, 0, 0, 4, 3], [1, 2, 3, 2, 1], [0, 0, 0, 0, 0]], 16),
    "sierra_lite": ([[0, 0, 0, 2, 0], [0, 1, 1, 0, 0], [0, 0, 0, 0, 0]], 4),
    "atkinson": ([[0, 0, 0, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]], 8),
}
# the instance of each: (R, S)
PRESET_CLASS = {"floyd_steinberg": (1, 2), "jarvis": (2, 3), "stucki": (2, 3), "burkes": (1, 3),
                "sierra3": (2, 3), "sierra2": (1, 3), "sierra_lite": (1, 2), "atkinson": (2, 2)}
# the twelve positions that may hold a weight, in the summation order: (dy, dx)
POSITIONS = [(0, 1), (0, 2)] + [(dy, dx) for dy in (1, 2) for dx in range(-2, 3)]


def preset(name):
    w, div = PRESETS[name]
    return np.array(w, np.int64), div


def single_tap(dy, dx):
    """The tap set with weight 1 at (dy, dx) alone, div 1."""
    w = np.zeros((3, 5), np.int64)
    w[dy, dx + 2] = 1
    return w, 1


def legal(w, div):
    """hq.h's rule: every weight >= 0; row 0 holds weights at dx = 1, 2 only; div >= 1; a non-zero
    weight; sum w <= div."""
    w = np.asarray(w, dtype=object)
    if w.shape != (3, 5) or any(int(v) < 0 for v in w.reshape(-1)) or any(int(v) != 0 for v in w[0, :3]):
        return False
    total = sum(int(v) for v in w.reshape(-1))
    return int(div) >= 1 and 1 <= total <= int(div)


def classify(w):
    """(R, S): R the highest dy that holds a weight, at least 1; S = max(a, 1) + 1, a the
    largest -dx among row 1's weights."""
    w = np.asarray(w)
    R = 2 if np.any(w[2] != 0) else 1
    a = max([-dx for dx in range(-2, 3) if w[1, dx + 2] != 0] + [0])
    return R, max(a, 1) + 1


def _taps(w):
    """The non-zero taps in the summation order: [(float32 weight, dy, dx)]."""
    w = np.asarray(w)
    return [(f32(int(w[dy, dx + 2])), dy, dx) for dy, dx in POSITIONS if w[dy, dx + 2] != 0]


def _value(pix, err, ys, xs, taps, div, s):
    """err holds e(x, y) at [y + 2, x + 2], zero outside the image."""
    acc = None
    for wt, dy, dx in taps:
        prod = wt * err[ys + 2 - dy, xs + 2 - dx]
        acc = prod if acc is None else acc + prod
    t = acc / f32(div)
    m = s * t
    return np.minimum(np.maximum(pix + m, f32(0)), f32(1))


def _prepare(rgb3, palette4, w, h, s):
    px = np.ascontiguousarray(np.asarray(rgb3, f32)[:, :3]).reshape(h, w, 3)
    pal = np.ascontiguousarray(np.asarray(palette4, f32).reshape(-1, 4))
    err = np.zeros((h + 2, w + 4, 3), f32)
    return px, pal, err, f32(s)


def _finish(idx, K):
    used = np.zeros(K, np.int32)
    used[np.unique(idx)] = 1
    return idx.reshape(-1), used


def diffuse_raster(rgb3, palette4, w, h, s, taps, div):
    """-> (idx int32 [w h], used int32 [K]) in raster order, one pixel at a time."""
    px, pal, err, s = _prepare(rgb3, palette4, w, h, s)
    tp = _taps(taps)
    idx = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            ys, xs = np.array([y]), np.array([x])
            v = _value(px[ys, xs], err, ys, xs, tp, div, s)
            k = int(o.assign(v, pal)[0][0])
            idx[y, x] = k
            err[y + 2, x + 2] = v[0] - pal[k, :3]
    return _finish(idx, len(pal))


def wavefronts(w, h, S):
    """The pixels of an image in the order of the wavefronts t = x + S y: [(ys, xs)]."""
    out = []
    for t in range(w + S * (h - 1)):
        ys = np.arange(max(0, -((w - 1 - t) // S)), min(h - 1, t // S) + 1)
        out.append((ys, t - S * ys))
    return out


def diffuse(rgb3, palette4, w, h, s, taps, div, slope=None):
    """The same by wavefronts of slope S (classify's unless given), vectorised per wavefront."""
    px, pal, err, s = _prepare(rgb3, palette4, w, h, s)
    tp = _taps(taps)
    S = classify(taps)[1] if slope is None else slope
    idx = np.zeros((h, w), np.int32)
    for ys, xs in wavefronts(w, h, S):
        v = _value(px[ys, xs], err, ys, xs, tp, div, s)
        k = o.assign(v, pal)[0]
        idx[ys, xs] = k
        err[ys + 2, xs + 2] = v - pal[k, :3]
    return _finish(idx, len(pal))

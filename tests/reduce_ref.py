"""numpy restatement of the image pyramid's arithmetic (include/hq.h, "an image pyramid on
the device"): hq_reduced_size, hq_reduce_weights and the two forms of hq_set_image_reduced.
Written from the header's text, block by block in plain loops; no GPU and no libhq here.
"""

import numpy as np


def reduced_size(w, h, f):
    return -(-int(w) // int(f)), -(-int(h) // int(f))


def blocks(w, h, f):
    """(X, Y, x0, x1, y0, y1) of every output pixel: source columns [x0, x1), rows [y0, y1)."""
    rw, rh = reduced_size(w, h, f)
    for Y in range(rh):
        for X in range(rw):
            yield X, Y, X * f, min(X * f + f, w), Y * f, min(Y * f + f, h)


def reduce_weights(src, w, h, f, is_mask):
    """hq_reduce_weights: floor((2 S + n) / (2 n)) of each block's bytes (a mask's non-zero
    bytes count as 255), raised to 1 when any byte of the block is non-zero."""
    m = np.asarray(src).reshape(h, w).astype(np.int64)
    rw, rh = reduced_size(w, h, f)
    out = np.zeros((rh, rw), np.uint8)
    for X, Y, x0, x1, y0, y1 in blocks(w, h, f):
        b = m[y0:y1, x0:x1]
        v = np.where(b != 0, 255, 0) if is_mask else b
        n = b.size
        r = (2 * int(v.sum()) + n) // (2 * n)
        out[Y, X] = max(r, 1) if np.any(b != 0) else r
    return out


def reduce_bytes(by, w, h, f):
    """The packed form on the bytes themselves: by (h w, 3) integers 0 .. 255 -> (rh rw, 3)
    bytes, per channel floor((2 s + n) / (2 n))."""
    m = np.asarray(by).reshape(h, w, 3).astype(np.int64)
    rw, rh = reduced_size(w, h, f)
    out = np.zeros((rh, rw, 3), np.int64)
    for X, Y, x0, x1, y0, y1 in blocks(w, h, f):
        b = m[y0:y1, x0:x1].reshape(-1, 3)
        n = b.shape[0]
        out[Y, X] = (2 * b.sum(axis=0) + n) // (2 * n)
    return out.reshape(-1, 3)


def unit(by):
    """k/255 as a float division makes it: what the library's planes hold for byte k."""
    return np.asarray(by).astype(np.float32) / np.float32(255)


def reduce_u8(rgba, w, h, f):
    """hq_set_image_reduced of an image whose channels are all k/255: inline RGBA (h w, 4)
    float32 -> the reduced inline RGBA (rh rw, 4), .w = 0."""
    rgba = np.asarray(rgba, np.float32).reshape(-1, 4)
    by = np.rint(rgba[:, :3].astype(np.float64) * 255).astype(np.int64)
    assert np.array_equal(unit(by), rgba[:, :3]), "not a k/255 image"
    red = reduce_bytes(by, w, h, f)
    out = np.zeros((red.shape[0], 4), np.float32)
    out[:, :3] = unit(red)
    return out


def reduce_planar(rgba, w, h, f):
    """hq_set_image_reduced of any other image: per channel the fp32 sum of the block in raster
    order, starting from its first pixel, then one fp32 division by float32(n)."""
    m = np.asarray(rgba, np.float32).reshape(h, w, 4)
    rw, rh = reduced_size(w, h, f)
    out = np.zeros((rh, rw, 4), np.float32)
    for X, Y, x0, x1, y0, y1 in blocks(w, h, f):
        b = m[y0:y1, x0:x1, :3].reshape(-1, 3)  # rows outer, columns inner
        acc = b[0].copy()
        for px in b[1:]:
            acc = (acc + px).astype(np.float32)  # float32 + float32: one rounding each
        out[Y, X, :3] = acc / np.float32(b.shape[0])
    return out.reshape(-1, 4)

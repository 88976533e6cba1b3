"""numpy restatements of the seeding entry points (hq_color_histogram,
hq_median_cut), written from the rule as include/hq.h states it, nothing of
libhq's.  The histogram works on the test's own pixel array; the median cut is
integer arithmetic (int64 sums, Python ints for the priority) until the final
means."""

import numpy as np

DEN32 = 1 << 32


def q32(v):
    """The planar form's integer per channel value: RN(v 2^32), ties to even."""
    return np.rint(np.asarray(v, np.float32).astype(np.float64) * 2 ** 32).astype(np.int64)


def coord_float(v, bits):
    """Cell coordinate of float32 channel values in [0, 1]: min(floor(v 2^bits), 2^bits - 1),
    the product in float32 (a power-of-two scaling: exact)."""
    v = np.asarray(v, np.float32)
    x = np.floor(v * np.float32(1 << bits)).astype(np.int64)
    return np.minimum(x, (1 << bits) - 1)


def coord_byte(b, bits):
    """The same for the bytes of a k/255 image."""
    return np.asarray(b, np.int64) >> (8 - bits)


def histogram_ref(coords, px, bits):
    """(2^(3 bits), 4) int64 cells = (sum R, sum G, sum B, count) of integer pixels px (n, 3)
    with cell coordinates coords (n, 3).  bincount adds in float64: exact below 2^53."""
    coords = np.asarray(coords, np.int64)
    px = np.asarray(px, np.int64)
    n = 1 << (3 * bits)
    cell = (coords[:, 0] << (2 * bits)) | (coords[:, 1] << bits) | coords[:, 2]
    out = np.zeros((n, 4), np.int64)
    for ch in range(3):
        assert int(px[:, ch].sum()) <= 2 ** 53
        out[:, ch] = np.bincount(cell, weights=px[:, ch], minlength=n).astype(np.int64)
    out[:, 3] = np.bincount(cell, minlength=n)
    return out


def mean_ref(s, n, den):
    """lloyd_mean (hq_centroids_from_sums' rule): int -> double conversions, one fp64 product
    and one fp64 division, one rounding to float."""
    s, n = np.float64(int(s)), np.float64(int(n))
    return np.float32(s / (np.float64(255.0) * n)) if den == 255 else np.float32(np.ldexp(s, -32) / n)


class _Box:
    def __init__(self, members, xyz, cnt):
        self.members = members  # indices into the non-empty cells
        x = xyz[members]
        self.lo = x.min(0)
        self.hi = x.max(0)
        self.count = int(cnt[members].sum())  # (int64: the totals stay below 2^48)

    def priority(self):
        e = [int(h) - int(l) for l, h in zip(self.lo, self.hi)]
        return self.count * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2])


def median_cut_ref(cells, bits, den, K):
    """-> (palette float32[4K], made)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 4)
    assert cells.shape[0] == 1 << (3 * bits) and K >= 1
    ne = np.flatnonzero(cells[:, 3] > 0)
    mask = (1 << bits) - 1
    xyz = np.stack([ne >> (2 * bits), (ne >> bits) & mask, ne & mask], 1)
    cnt = cells[ne, 3]
    boxes = [_Box(np.arange(len(ne)), xyz, cnt)]
    while len(boxes) < K:
        prio = [b.priority() for b in boxes]
        best = max(prio)
        if best == 0:
            break
        i = prio.index(best)  # the lowest index among equal priorities
        b = boxes[i]
        ext = [int(h) - int(l) for l, h in zip(b.lo, b.hi)]
        axis = ext.index(max(ext))  # R, then G, then B among equal extents
        lo, hi = int(b.lo[axis]), int(b.hi[axis])
        m = np.zeros(hi + 1, np.int64)
        np.add.at(m, xyz[b.members, axis], cnt[b.members])  # (int64 adds: exact)
        acc, t = 0, hi
        for x in range(lo, hi + 1):
            acc += int(m[x])
            if 2 * acc >= b.count:
                t = x
                break
        t = min(t, hi - 1)
        low = b.members[xyz[b.members, axis] <= t]
        up = b.members[xyz[b.members, axis] > t]
        boxes[i] = _Box(low, xyz, cnt)
        boxes.append(_Box(up, xyz, cnt))
    made = len(boxes)
    pal = np.zeros((K, 4), np.float32)
    for i, b in enumerate(boxes):
        for ch in range(3):
            s = int(cells[ne[b.members], ch].sum())  # (int64, as the library's)
            pal[i, ch] = mean_ref(s, b.count, den)
    for i in range(made, K):
        pal[i] = pal[i % made]
    return pal.reshape(-1), made

"""numpy checkers of the k-means entry points (hq_cluster_sums,
hq_centroids_from_sums): the formulas of include/hq.h, nothing of libhq's."""

import numpy as np

DEN32 = 1 << 32


def q32(v):
    """The planar form's integer per channel value: RN(v 2^32), ties to even."""
    return np.rint(np.asarray(v, np.float32).astype(np.float64) * 2 ** 32).astype(np.int64)


def cluster_sums_ref(idx, px, K):
    """(K, 4) int64 (sum R, sum G, sum B, count) of integer pixels px (n, 3) under the
    index image idx (n,).  bincount adds in float64: exact while a total stays below 2^53."""
    idx = np.asarray(idx).astype(np.int64)
    px = np.asarray(px, np.int64)
    out = np.zeros((K, 4), np.int64)
    for ch in range(3):
        assert int(px[:, ch].sum()) <= 2 ** 53
        out[:, ch] = np.bincount(idx, weights=px[:, ch], minlength=K).astype(np.int64)
    out[:, 3] = np.bincount(idx, minlength=K)
    return out


def centroids_ref(sums, den, pal):
    """hq_centroids_from_sums in numpy: (P, K, 4) int64 sums, (P, 4K) float32 palettes."""
    sums = np.asarray(sums, np.int64)
    P, K = sums.shape[:2]
    out = np.ascontiguousarray(pal, np.float32).reshape(P, K, 4).copy()
    cnt = sums[..., 3]
    has = cnt > 0
    n = np.where(has, cnt, 1).astype(np.float64)
    for ch in range(3):
        s = sums[..., ch].astype(np.float64)  # (rounds above 2^53, as the C conversion does)
        mean = s / (255.0 * n) if den == 255 else np.ldexp(s, -32) / n
        out[..., ch] = np.where(has, mean.astype(np.float32), out[..., ch])
    out[..., 3] = np.where(has, np.float32(0), out[..., 3])
    return out.reshape(P, 4 * K)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)

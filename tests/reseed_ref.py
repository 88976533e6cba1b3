"""numpy restatements of the repair entry points (hq_cluster_errors,
hq_reseed_unused), written from the rules as include/hq.h states them, nothing
of libhq's.  The statistics work on the library's own index and error images
and the test's own pixel array; everything is integer arithmetic."""

import numpy as np

SCALE = 1 << 20
TOP = 0xFFFFFFFF


def ebits(e):
    return np.ascontiguousarray(e, np.float32).view(np.uint32)


def cluster_errors_ref(idx, e, px, pal, pos0=0):
    """(err (K, 4) int64, worst (K, 4) float32) of one palette pal (K, 4) under the index
    image idx (n,), the error image e (n,) float32 and the pixels px (n, 3) float32 as the
    argmin saw them; pixel i has position pos0 + i in the full image."""
    idx = np.asarray(idx).astype(np.int64)
    e = np.ascontiguousarray(e, np.float32)
    px = np.ascontiguousarray(px, np.float32)
    pal = np.ascontiguousarray(pal, np.float32).reshape(-1, 4)
    K, n = pal.shape[0], idx.shape[0]
    with np.errstate(invalid="ignore"):
        good = np.isfinite(e) & ~np.signbit(e) & (e < np.float32(SCALE))
    v = np.zeros(n, np.int64)
    v[good] = np.rint(e[good].astype(np.float64) * SCALE).astype(np.int64)  # exact product, half to even
    assert int(v.sum()) < 2 ** 53  # bincount adds in float64
    err = np.zeros((K, 4), np.int64)
    err[:, 0] = np.bincount(idx, weights=v, minlength=K).astype(np.int64)
    err[:, 1] = np.bincount(idx, minlength=K)
    err[:, 3] = -1
    with np.errstate(invalid="ignore"):
        movable = good & np.any(px != pal[idx, :3], axis=1)
    pos = pos0 + np.arange(n, dtype=np.int64)
    key = (ebits(e).astype(np.uint64) << np.uint64(32)) | (TOP - pos).astype(np.uint64)
    best = np.zeros(K, np.uint64)
    np.maximum.at(best, idx[movable], key[movable])
    worst = np.zeros((K, 4), np.float32)
    for k in np.nonzero(best)[0]:
        at = TOP - int(best[k] & np.uint64(TOP))
        err[k, 2] = int(best[k] >> np.uint64(32))
        err[k, 3] = at
        worst[k, :3] = px[at - pos0]
    return err, worst


def tied_maxima(idx, e, px, pal, k):
    """How many movable pixels of cluster k share its largest dE."""
    idx = np.asarray(idx).astype(np.int64)
    pal = np.ascontiguousarray(pal, np.float32).reshape(-1, 4)
    sel = (idx == k) & np.any(np.ascontiguousarray(px, np.float32) != pal[idx, :3], axis=1)
    return int((ebits(e)[sel] == ebits(e)[sel].max()).sum()) if sel.any() else 0


def merge_ref(parts):
    """Shards' (err, worst) -> the whole image's: sums and counts add, the larger [2]
    wins, then the lower [3], worst follows the winner."""
    err, worst = parts[0][0].copy(), parts[0][1].copy()
    for e2, w2 in parts[1:]:
        err[..., :2] += e2[..., :2]
        has1, has2 = err[..., 3] >= 0, e2[..., 3] >= 0
        wins = has2 & (~has1 | (e2[..., 2] > err[..., 2]) | ((e2[..., 2] == err[..., 2]) & (e2[..., 3] < err[..., 3])))
        err[..., 2:] = np.where(wins[..., None], e2[..., 2:], err[..., 2:])
        worst = np.where(wins[..., None], w2, worst)
    return err, worst


def reseed_ref(err, worst, pal, max_moves=-1):
    """hq_reseed_unused: err (P, K, 4) int64, worst (P, K, 4), palettes (P, 4K) ->
    (new palettes (P, 4K), moved (P,))."""
    err = np.asarray(err, np.int64)
    P, K = err.shape[:2]
    worst = np.ascontiguousarray(worst, np.float32).reshape(P, K, 4)
    out = np.ascontiguousarray(pal, np.float32).reshape(P, K, 4).copy()
    moved = np.zeros(P, np.int32)
    for p in range(P):
        receivers = [k for k in range(K) if err[p, k, 1] == 0]
        donors = sorted((k for k in range(K) if err[p, k, 1] > 0 and err[p, k, 3] >= 0),
                        key=lambda k: (-int(err[p, k, 0]), k))
        m = min(len(receivers), len(donors))
        if max_moves >= 0:
            m = min(m, max_moves)
        for r, d in zip(receivers[:m], donors[:m]):
            out[p, r, :3] = worst[p, d, :3]
            out[p, r, 3] = 0
        moved[p] = m
    return out.reshape(P, 4 * K), moved

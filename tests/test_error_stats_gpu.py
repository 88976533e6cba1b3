"""GPU tests of hq_error_stats (libhq's addition): every output against hq.h's rule restated in numpy
on hq_get_pixel_errors of the same evaluation -- exact integers and one pixel's bits, so array_equal
throughout -- under no map, a mask and weights, across workgroups, on a shard; the non-finite count;
the tie on the maximum; the identities and the refusals."""
import numpy as np
import pytest

from hybridquantization_amd import _lib
from test_grad_gpu import FILTERS, context, noise_rgba, palettes

pytestmark = pytest.mark.gpu
K, FILL = 16, -7


def reference(e, nbins, top, wt, pos0=0):
    """hq.h's rule on one palette's error image e (the owned pixels) under the int64 weights wt (0: not
    counted) -> (hist, nonfinite, max_de, max_pixel)."""
    ok = np.isfinite(e) & (e >= 0)
    good, bad = (wt > 0) & ok, (wt > 0) & ~ok
    t = e[good].astype(np.float32) * np.float32(np.float32(nbins) / np.float32(top))
    b = np.where(t >= np.float32(nbins), nbins - 1, t.astype(np.int64))
    hist = np.zeros(nbins, np.int64)
    np.add.at(hist, b, wt[good])
    at = np.flatnonzero(good)
    mx = e[at].max() if at.size else np.float32(0)
    return hist, wt[bad].sum(), mx, pos0 + at[e[at] == mx][0] if at.size else -1


def evaluated(gpu, filt, rgba, w, lab=None, rows=(0, None)):
    m = context(gpu, filt)
    m.setOption("pixel_err", 1)
    m.setImage(rgba.reshape(-1), lab, w, filt.illum, *rows)
    return m


def check(m, P, nbins, top, wt, n_own, pos0=0):
    """errorStats against the reference on the same evaluation's error images -> the device's outputs."""
    got = m.errorStats(P, nbins, top)
    for p in range(P):
        want = reference(m.getPixelErrors(p)[:n_own], nbins, top, wt, pos0)
        for g, w_ in zip(got, want):
            assert np.array_equal(g[p], w_), (p, g[p], w_)
    return got


def int_map(w, h, kind):
    a = np.arange(w * h)
    return {"none": np.ones(w * h), "mask": a % 3 > 0, "weights": a % 200 + 1, "w01": a % 3 > 0}[kind].astype(np.int64)


# (filters, w, h, P, nbins, top, map, span, shard rows): 5 x 3 is less than a workgroup and no whole quad row
# (below the designed filters' half-width 10, which hq_set_image refuses: the one-tap filters there);
# 70-wide planes start palettes 1 and 2 off 16 bytes; span 1024 makes 4690 pixels five workgroups; top 4
# fills the overflow bin; 4096 bins are the most
CASES = [("one_tap", 5, 3, 1, 1, 50.0, "none", 0, None), ("designed", 70, 67, 3, 7, 50.0, "none", 1024, None),
         ("designed", 70, 67, 3, 256, 4.0, "mask", 0, None), ("designed", 64, 48, 2, 1024, 50.0, "weights", 0, None),
         ("designed", 64, 48, 2, 4096, 50.0, "w01", 0, None), ("designed", 64, 48, 1, 256, 50.0, "none", 0, (16, 32))]


@pytest.mark.parametrize("name,w,h,P,nbins,top,kind,span,rows", CASES)
def test_error_stats(gpu, name, w, h, P, nbins, top, kind, span, rows):
    filt, rgba, pals, wt = FILTERS[name](), noise_rgba(w, h, 3), palettes(P, K, 33), int_map(w, h, kind)
    m = evaluated(gpu, filt, rgba, w)
    try:
        if kind != "none":
            (m.setMask if kind == "mask" else m.setWeights)(wt.astype(np.uint8))
        m.setOption("errstats_span", span)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        if span:
            assert -(-w * h // span) > 1, "the case's condition: more than one workgroup flushes"
        got = check(m, P, nbins, top, wt, w * h)
        assert all(got[0][p].sum() + got[1][p] == wt.sum() for p in range(P))
        if top < 50.0:
            assert all(reference(m.getPixelErrors(p), nbins, top, wt)[0][-1] > 0 for p in range(P)), "overflow bin"
        if kind == "w01":  # the same map as a mask: the same bytes
            m.setMask(wt.astype(np.uint8))
            m.computeQuantizationErrorPopulation(pals, 2.0)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, m.errorStats(P, nbins, top)))
        if rows:  # the shard against the whole image's rows, at the full image's pixel indices
            want = reference(m.getPixelErrors(0)[rows[0] * w:rows[1] * w], nbins, top, wt[rows[0] * w:rows[1] * w],
                             rows[0] * w)
            s = evaluated(gpu, filt, rgba, w, rows=rows)
            try:
                part = np.zeros((P, 1 + K))
                _lib.check(s._lib.hq_eval_population_partial(s.ctx, _lib.fptr(pals), P, K, _lib.dptr(part)), s.ctx)
                n_own = (rows[1] - rows[0]) * w
                shard = check(s, P, nbins, top, wt[:n_own], n_own, rows[0] * w)
                assert all(np.array_equal(g[0], w_) for g, w_ in zip(shard, want))
            finally:
                s.close()
    finally:
        m.close()


def test_nonfinite_pixels(gpu):
    """A caller's LabRef with NaN at 5 pixels, 2 of them of weight 0: the weighted count of the other 3."""
    filt, w, h, P = FILTERS["designed"](), 64, 48, 2
    rgba, pals, wt, nan_at = noise_rgba(w, h, 3), palettes(P, K, 33), int_map(w, h, "weights"), [0, 77, 1000, 2049, 3071]
    wt[[77, 2049]] = 0
    m = evaluated(gpu, filt, rgba, w)
    try:
        lab = m.getLabRef().reshape(-1, 4)
        lab[nan_at, :3] = np.nan
        m.setImage(rgba.reshape(-1), lab.reshape(-1), w, filt.illum)
        m.setWeights(wt.astype(np.uint8))
        m.computeQuantizationErrorPopulation(pals, 2.0)
        assert np.array_equal(np.flatnonzero(np.isnan(m.getPixelErrors(0))), nan_at)
        hist, nonfinite, _, _ = check(m, P, 256, 50.0, wt, w * h)
        assert all(nonfinite[p] == wt[[0, 1000, 3071]].sum() and hist[p].sum() + nonfinite[p] == wt.sum() for p in range(P))
    finally:
        m.close()


def test_tie_on_the_maximum(gpu):
    """A pointwise cost on a tiled 8 x 8 block: the maximum occurs many times, the lowest index is reported;
    with that one masked out, the next."""
    filt, w, h = FILTERS["one_tap"](), 64, 48
    rgba = np.tile(noise_rgba(8, 8, 3).reshape(8, 8, 4), (h // 8, w // 8, 1))
    pals = palettes(1, K, 33)
    m = evaluated(gpu, filt, rgba, w)
    try:
        m.computeQuantizationErrorPopulation(pals, 2.0)
        e = m.getPixelErrors(0)
        at = np.flatnonzero(e == e.max())
        assert at.size > 1, "the case's condition: a tie"
        assert check(m, 1, 256, 50.0, np.ones(w * h, np.int64), w * h)[3][0] == at[0]
        wt = np.ones(w * h, np.int64)
        wt[at[0]] = 0
        m.setMask(wt.astype(np.uint8))
        m.computeQuantizationErrorPopulation(pals, 2.0)
        assert check(m, 1, 256, 50.0, wt, w * h)[3][0] == at[1]
    finally:
        m.close()


def raw(m, P, nbins, top):
    """hq_error_stats through ctypes -> (rc, outputs); the outputs start at FILL."""
    out = [np.full((P, max(nbins, 1)), FILL, np.int64), np.full(P, FILL, np.int64), np.full(P, FILL, np.float32),
           np.full(P, FILL, np.int64)]
    return m._lib.hq_error_stats(m.ctx, P, nbins, top, _lib.i64ptr(out[0]), _lib.i64ptr(out[1]), _lib.fptr(out[2]),
                                 _lib.i64ptr(out[3])), out


def _alone(m, pals):
    want = [a[1:2] for a in raw(m, 3, 256, 50.0)[1]]
    return (m.computeQuantizationErrorPopulation(pals[1:2], 2.0), ((1, 256, 50.0), _lib.HQ_OK, want))[1]


def _dot(m, pals):
    plain = m.getPixelErrors(0)
    m.dotPopulation(pals, 1.0, 2.0)
    assert not np.array_equal(m.getPixelErrors(0), plain)
    ref = [reference(m.getPixelErrors(p), 256, 50.0, np.ones(plain.size, np.int64)) for p in range(3)]
    return (3, 256, 50.0), _lib.HQ_OK, [np.stack([r[i] for r in ref]) for i in range(4)]


# name: (what comes before the call -> its arguments, the status, the outputs or None: still at FILL)
IDENTITIES_AND_REFUSALS = {
    "twice": lambda m, pals: ((3, 256, 50.0), _lib.HQ_OK, raw(m, 3, 256, 50.0)[1]),
    "alone": _alone,
    "after_dot": _dot,
    "pixel_err_off": lambda m, pals: (m.setOption("pixel_err", 0), ((3, 256, 50.0), _lib.HQ_ERR_STATE, None))[1],
    "other_P": lambda m, pals: ((2, 256, 50.0), _lib.HQ_ERR_STATE, None),
    "nbins_0": lambda m, pals: ((3, 0, 50.0), _lib.HQ_ERR_ARG, None),
    "nbins_4097": lambda m, pals: ((3, 4097, 50.0), _lib.HQ_ERR_ARG, None),
    "top_0": lambda m, pals: ((3, 256, 0.0), _lib.HQ_ERR_ARG, None),
    "top_nan": lambda m, pals: ((3, 256, float("nan")), _lib.HQ_ERR_ARG, None),
    "slice": lambda m, pals: (m.setOption("slice_ranks", 2), ((3, 256, 50.0), _lib.HQ_ERR_UNSUPPORTED, None))[1],
}


@pytest.mark.parametrize("name", IDENTITIES_AND_REFUSALS)
def test_identities_and_refusals(gpu, name):
    filt, w, h, pals = FILTERS["designed"](), 64, 48, palettes(3, K, 33)
    m = evaluated(gpu, filt, noise_rgba(w, h, 3), w)
    try:
        m.computeQuantizationErrorPopulation(pals, 2.0)
        args, status, want = IDENTITIES_AND_REFUSALS[name](m, pals)
        rc, got = raw(m, *args)
        assert rc == status
        for i, g in enumerate(got):
            assert g.tobytes() == (np.full_like(g, FILL) if want is None else np.asarray(want[i], g.dtype)).tobytes()
    finally:
        m.close()

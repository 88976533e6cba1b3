"""GPU tests of hq_cost_gradient and hq_descend_population (libhq's additions): the device's
gradient against the float64 statement of tests/grad_ref.py, measured by the fp32 statement's own
error; its exact properties; its refusals; the descent polish."""
import numpy as np
import pytest

import grad_ref as gr
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from hybridquantization_amd import _lib
from test_lloyd_gpu import blob_image

pytestmark = pytest.mark.gpu

FILTERS = {
    "one_tap": gr.one_tap_filters,                   # the adjoint is a scale: g and the sums alone
    "designed": lambda: o.design_filters(72, 45.0),  # half 10: the tiled form
    "long": lambda: o.design_filters(300, 50.0),     # half 51: the plain pair
    "asym": gr.asym_filters,                         # 5 asymmetric caller taps
}
# (filters, w, h, K, P, palette seed): W = H = halfSize; 70 x 67 = 3 x 3 tiles of 32 x 32 and 3 x 5 of
# 32 x 16, no multiple of either; 64 x 48.  The seeds: chosen on the CPU so that every pixel's float64
# E is at least 0.1 under the oracle's assignment (the test asserts 0.05 under the device's).
CASES = [("one_tap", 64, 48, 16, 1, 33), ("one_tap", 70, 67, 2, 3, 19), ("designed", 10, 10, 2, 1, 19),
         ("designed", 70, 67, 256, 3, 276), ("designed", 64, 48, 16, 3, 33), ("long", 51, 51, 16, 1, 33),
         ("long", 70, 67, 2, 1, 19), ("asym", 2, 2, 2, 3, 19), ("asym", 70, 67, 16, 1, 33),
         ("asym", 64, 48, 256, 1, 273)]


def context(gpu, filt, de=hq.deltaETypes.CIE76):
    m = pr.Context(de, device=gpu)
    assert m.getOpenCLAvailable()
    _lib.check(m._lib.hq_set_filters(m.ctx, filt.k1.shape[0], _lib.fptr(filt.k1), _lib.fptr(filt.k2),
                                     _lib.fptr(filt.k3), _lib.fptr(filt.absk3)), m.ctx)
    m._filters, m.openCLFiltersReady, m.illum = (filt.k1, filt.k2, filt.k3, filt.absk3), True, filt.illum
    return m


def noise_rgba(w, h, seed):
    return o.inline_rgba(*o.synthetic_image(w, h, seed=seed))


def palettes(P, K, seed):
    """Random palettes whose colour 0 has a channel at 0, at 1 and below 0.04045, and whose last
    colour duplicates an earlier one -- the copy at the higher index is never assigned: unused."""
    rng = np.random.default_rng(seed)
    pal = np.zeros((P, K, 4), np.float32)
    pal[..., :3] = rng.random((P, K, 3))
    pal[:, 0, :3] = (0.0, 1.0, 0.02)
    pal[:, K - 1] = pal[:, min(1, K - 2)]
    return pal.reshape(P, -1)


def raw_gradient(m, P, K, fill=-7.0):
    out = np.full((P, K, 4), fill)
    return m._lib.hq_cost_gradient(m.ctx, P, K, _lib.dptr(out)), out


def rel_err(g, g64):
    return np.abs(g - g64).max() / np.abs(g64).max()


def check_against_reference(m, filt, pals, w, h, K, forms, label):
    """Every palette's device gradient, in each form, within 4 x the fp32 statement's own error."""
    lab = m.getLabRef().reshape(-1, 4)
    for p in range(pals.shape[0]):
        idx = m.getIndices(p)
        g64, n64, E = gr.gradient(idx, pals[p].reshape(K, 4), filt, w, h, lab, filt.illum)
        g32 = gr.gradient(idx, pals[p].reshape(K, 4), filt, w, h, lab, filt.illum, np.float32)[0]
        assert E.min() >= 0.05, "the case's condition: no pixel measures rounding noise"
        bar = 4 * rel_err(g32, g64)
        for form in forms:
            m.setOption("grad_tiled", form)
            grad, counts = m.costGradient(pals.shape[0], K)
            print(f"{label} p={p} form={form}: device {rel_err(grad[p], g64):.3e}, fp32 {bar / 4:.3e}, "
                  f"ratio {rel_err(grad[p], g64) / (bar / 4):.2f}")
            assert np.array_equal(counts[p], np.bincount(idx, minlength=K))
            assert not grad[p][counts[p] == 0].any() and (counts[p] == 0).any()
            assert rel_err(grad[p], g64) <= bar


@pytest.mark.parametrize("name,w,h,K,P,seed", CASES)
def test_gradient(gpu, name, w, h, K, P, seed):
    filt = FILTERS[name]()
    m = context(gpu, filt)
    try:
        m.setImage(noise_rgba(w, h, 3).reshape(-1), None, w, filt.illum)
        pals = palettes(P, K, seed)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        forms = (0, 1) if filt.half <= 24 else (-1,)  # plain pair and tiled form; above 24 the plain pair
        check_against_reference(m, filt, pals, w, h, K, forms, f"{name} {w}x{h} K={K} P={P}")
        m.setOption("grad_tiled", -1)
        rc1, a = raw_gradient(m, P, K)
        rc2, b = raw_gradient(m, P, K)
        assert rc1 == rc2 == _lib.HQ_OK and a.tobytes() == b.tobytes()  # two calls: identical bits
        if P > 1:  # a palette alone and inside the population: identical bits
            m.computeQuantizationErrorPopulation(pals[1:2], 2.0)
            rc, alone = raw_gradient(m, 1, K)
            assert rc == _lib.HQ_OK and alone[0].tobytes() == a[1].tobytes()
    finally:
        m.close()


def test_gradient_follows_a_rendering(gpu):
    """After hq_dot_population the gradient is that of the dot-diffused index images."""
    filt, w, h, K = FILTERS["designed"](), 64, 48, 16
    m = context(gpu, filt)
    try:
        m.setImage(noise_rgba(w, h, 3).reshape(-1), None, w, filt.illum)
        pals = palettes(1, K, 5)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        plain = m.getIndices(0)
        m.dotPopulation(pals, 1.0, 2.0)
        assert not np.array_equal(m.getIndices(0), plain)
        lab, idx = m.getLabRef().reshape(-1, 4), m.getIndices(0)
        g64, n64, _ = gr.gradient(idx, pals[0].reshape(K, 4), filt, w, h, lab, filt.illum)
        g32 = gr.gradient(idx, pals[0].reshape(K, 4), filt, w, h, lab, filt.illum, np.float32)[0]
        grad, counts = m.costGradient(1, K)
        assert np.array_equal(counts[0], n64) and rel_err(grad[0], g64) <= 4 * rel_err(g32, g64)
    finally:
        m.close()


def _k300(m, w):
    m.computeQuantizationErrorPopulation(palettes(1, 300, 1), 2.0)
    return 300


REFUSALS = {
    # name: (dE type, what puts the context into the refused state -> K of the call, the status)
    "k_above_256": (hq.deltaETypes.CIE76, _k300, _lib.HQ_ERR_UNSUPPORTED),
    "de94": (hq.deltaETypes.CIE94, None, _lib.HQ_ERR_UNSUPPORTED),
    "de2000": (hq.deltaETypes.CIEDE2000, None, _lib.HQ_ERR_UNSUPPORTED),
    "shard": (hq.deltaETypes.CIE76, lambda m, w: m.setImage(noise_rgba(w, 48, 3).reshape(-1), None, w, m.illum, 16, 32),
              _lib.HQ_ERR_UNSUPPORTED),
    "slice": (hq.deltaETypes.CIE76, lambda m, w: m.setOption("slice_ranks", 2), _lib.HQ_ERR_UNSUPPORTED),
    "palette_split": (hq.deltaETypes.CIE76, lambda m, w: m.setOption("palette_split", 1), _lib.HQ_ERR_UNSUPPORTED),
    "mask": (hq.deltaETypes.CIE76, lambda m, w: m.setMask((np.arange(w * 48) % 3 > 0).astype(np.uint8)), _lib.HQ_ERR_UNSUPPORTED),
    "weights": (hq.deltaETypes.CIE76, lambda m, w: m.setWeights((np.arange(w * 48) % 200 + 1).astype(np.uint8)), _lib.HQ_ERR_UNSUPPORTED),
    "other_p": (hq.deltaETypes.CIE76, lambda m, w: -1, _lib.HQ_ERR_STATE),
    "new_image": (hq.deltaETypes.CIE76, lambda m, w: m.setImage(noise_rgba(w, 48, 4).reshape(-1), None, w, m.illum),
                  _lib.HQ_ERR_STATE),
}


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_write_nothing(gpu, name):
    """(A communicator of more than one rank needs two devices: tests/test_dist_gpu.py's ground.)"""
    de, act, status = REFUSALS[name]
    filt, w, K = FILTERS["designed"](), 64, 16
    m = context(gpu, filt, de)
    try:
        m.setImage(noise_rgba(w, 48, 3).reshape(-1), None, w, filt.illum)
        m.computeQuantizationErrorPopulation(palettes(2, K, 1), 2.0)
        r = act(m, w) if act else None
        P, K = (3, K) if r == -1 else (1, r) if type(r) is int else (2, K)
        rc, out = raw_gradient(m, P, K)
        assert rc == status and (out == -7.0).all()
        cost = np.zeros(P)
        pal = palettes(P, K, 2)
        if status == _lib.HQ_ERR_UNSUPPORTED and name not in ("shard", "slice"):  # (those: hq_refine_population's own)
            assert m._lib.hq_descend_population(m.ctx, _lib.fptr(pal), P, K, 1, 1e-4, 2.0, _lib.dptr(cost), None,
                                                None) == _lib.HQ_ERR_UNSUPPORTED
    finally:
        m.close()


def test_nothing_evaluated_is_a_state_error(gpu):
    m = context(gpu, FILTERS["designed"]())
    try:
        m.setImage(noise_rgba(64, 48, 3).reshape(-1), None, 64, m.illum)
        rc, out = raw_gradient(m, 1, 16)
        assert rc == _lib.HQ_ERR_STATE and (out == -7.0).all()
    finally:
        m.close()


def test_descend_population(gpu):
    """Three random palettes of K = 8 on the blob image, 8 steps: every cost falls, the returned
    palettes evaluate to the returned costs, fixed colours keep their bits, 0 steps is the evaluation."""
    filt, (rgba, _), K, P = FILTERS["designed"](), blob_image(96, 64, seed=11), 8, 3
    m = context(gpu, filt)
    try:
        m.setImage(rgba.reshape(-1), None, 96, filt.illum)
        pals = np.stack([o.synthetic_palette(K, 40 + p).reshape(-1) for p in range(P)])
        c0, u0 = m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
        pz, cz, uz = m.descendPopulation(pals, 0)
        assert pz.tobytes() == pals.tobytes() and cz.tobytes() == c0.tobytes() and np.array_equal(uz, u0)
        out, costs, used, trace = m.descendPopulation(pals, 8, return_trace=True)
        print("descent: input", c0.tolist(), "-> 8 steps", costs.tolist())
        assert (costs <= c0).all() and (costs < c0).all()
        assert (np.diff(trace, axis=0) <= 0).all() and np.array_equal(trace[0], c0) and np.array_equal(trace[-1], costs)
        c1, u1 = m.computeQuantizationErrorPopulation(out, 2.0, return_used=True)
        assert c1.tobytes() == costs.tobytes() and np.array_equal(u1, used)
        m.setFixedColors(pals[0].reshape(K, 4)[:2])
        start = pals.copy()
        start.reshape(P, K, 4)[:, :2] = pals[0].reshape(K, 4)[:2]
        fixed, fcosts, _ = m.descendPopulation(start, 4)
        assert fixed.reshape(P, K, 4)[:, :2].tobytes() == start.reshape(P, K, 4)[:, :2].tobytes()
        assert (fcosts <= m.computeQuantizationErrorPopulation(start, 2.0)).all()
    finally:
        m.close()

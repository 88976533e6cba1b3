"""The numpy statement of the cost's palette gradient (tests/grad_ref.py) against central
differences of its own float64 cost with the index image held fixed: what makes it a reference."""
import numpy as np
import pytest

import grad_ref as gr
import oracle as o

CASES = {
    # name: (filters, w, h, K)
    "designed": (o.design_filters, 40, 29, 6),
    "designed_w_h_half": (o.design_filters, None, None, 4),  # W = H = halfSize: both folds hit every pixel
    "asymmetric": (gr.asym_filters, 13, 9, 5),
    "asymmetric_w_h_half": (gr.asym_filters, 2, 2, 3),
    "one_tap": (gr.one_tap_filters, 7, 5, 4),
}


@pytest.mark.parametrize("name", CASES)
def test_gradient_matches_central_differences(name):
    make, w, h, K = CASES[name]
    filt = make()
    w, h = (filt.half, filt.half) if w is None else (w, h)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, K - 1, w * h)  # colour K - 1 is unused
    pal = np.zeros((K, 4), np.float32)
    pal[:, :3] = rng.random((K, 3))
    pal[0, :3] = (0.0, 1.0, 0.02)  # a channel at 0, at 1 and on srgb_lin's linear branch
    labref = np.stack([100 * rng.random(w * h), 80 * rng.random(w * h) - 40, 80 * rng.random(w * h) - 40], 1)
    grad, counts, E = gr.gradient(idx, pal, filt, w, h, labref, filt.illum)
    assert E.min() > 0.05 and counts[K - 1] == 0 and not grad[K - 1].any()
    eps = 1e-6
    fd = np.zeros((K, 3))
    for k in range(K):
        for ch in range(3):
            c = []
            for s in (eps, -eps):
                p = pal.astype(np.float64)
                p[k, ch] += s
                c.append(gr.cost_terms(idx, p, filt, w, h, labref, filt.illum)[0])
            fd[k, ch] = (c[0] - c[1]) / (2 * eps)
    assert np.abs(grad - fd).max() <= 1e-6 * np.abs(fd).max(), (grad, fd)


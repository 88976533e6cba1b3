"""The palette gradient of the S-CIELAB cost (hq_cost_gradient; include/hq.h) stated
in numpy, in float64 or in fp32 (``dt``): the forward blur, the pointwise term g, the adjoint blur
in gather form, the per-colour sums and the chain rule.  Inputs: the index image, the palette
[K, 4], an oracle.Filters, the image size, LabRef [N, >= 3] and the illuminant."""
import numpy as np

import oracle as o


F = np.float32
RGB2OPP, OPP2XYZ = np.asarray(o.RGB2OPPM, F), np.asarray(o.OPP2XYZM, F)
T0, LO, OFF, DIV, GAMMA = F(0.04045), F(12.92), F(0.055), F(1.055), F(2.4)  # srgb_lin, CL:85-87


def _c(v, dt):
    """v in dt: the device's fp32 constants and tables widen exactly; a float64 palette (a
    difference quotient's) stays what it is."""
    return np.asarray(v).astype(dt)


def fwd_matrix(k, n, dt):
    """(H f)(x) = sum_t k[t] f(reflect(x + t)), CL:256-263."""
    h = len(k) // 2
    m = np.zeros((n, n), dt)
    for x in range(n):
        for t in range(-h, h + 1):
            j = x + t
            j = -j - 1 if j < 0 else 2 * n - j - 1 if j >= n else j
            m[x, j] += k[t + h]
    return m


def adj_matrix(k, n, dt):
    """(H^T g)(y) = sum_t k[t] (g~(y - t) + g~(-y - 1 - t) + g~(2 n - y - 1 - t)), g~ zero outside."""
    h = len(k) // 2
    m = np.zeros((n, n), dt)
    for y in range(n):
        for t in range(-h, h + 1):
            for s in (y - t, -y - 1 - t, 2 * n - y - 1 - t):
                if 0 <= s < n:
                    m[y, s] += k[t + h]
    return m


def _pairs(filt, ch, dt):
    """(vertical taps, horizontal taps) of channel ch's separable filters."""
    k1, k2 = _c(filt.k1[:, ch], dt), _c(filt.k2[:, ch], dt)
    return [(k1, k1), (k2, k2)] + ([(_c(filt.absk3, dt), _c(filt.k3, dt))] if ch == 0 else [])


def cost_terms(idx, pal4, filt, w, h, labref, illum, dt=np.float64):
    """-> (C, E [h, w], t = XYZ / illuminant [h, w, 3], D = Lab - LabRef [h, w, 3]) with idx fixed."""
    rgb = _c(pal4, dt).reshape(-1, 4)[:, :3]
    with np.errstate(invalid="ignore"):
        lin = np.where(rgb <= _c(T0, dt), rgb / _c(LO, dt),
                       ((rgb + _c(OFF, dt)) / _c(DIV, dt)) ** _c(GAMMA, dt))
    opp = (lin @ _c(RGB2OPP, dt).T)[np.asarray(idx, np.int64)].reshape(h, w, 3)
    B = np.zeros((h, w, 3), dt)
    for ch in range(3):
        for kv, kh in _pairs(filt, ch, dt):
            B[..., ch] += fwd_matrix(kv, h, dt) @ (opp[..., ch] @ fwd_matrix(kh, w, dt).T)
    t = (B @ _c(OPP2XYZ, dt).T) / _c(illum, dt)
    f = np.where(t > _c(o.LABDELTA3, dt), np.cbrt(t), (_c(o.KAPPA, dt) * t + dt(16)) / dt(116))
    lab = np.stack([dt(116) * f[..., 1] - dt(16), dt(500) * (f[..., 0] - f[..., 1]),
                    dt(200) * (f[..., 1] - f[..., 2])], -1)
    D = lab - _c(labref, dt).reshape(h, w, -1)[..., :3]
    E = np.sqrt((D * D).sum(-1))
    return E.mean(dtype=dt), E, t, D


def gradient(idx, pal4, filt, w, h, labref, illum, dt=np.float64):
    """-> (grad [K, 3], counts [K], E [h, w])."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    K = np.asarray(pal4).reshape(-1, 4).shape[0]
    _, E, t, D = cost_terms(idx, pal4, filt, w, h, labref, illum, dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        U = np.where(E[..., None] > 0, D / E[..., None], dt(0))
        slope = np.where(t > _c(o.LABDELTA3, dt), dt(1) / (dt(3) * np.cbrt(t) ** 2), _c(o.KAPPA, dt) / dt(116))
    df = np.stack([dt(500) * U[..., 1], dt(116) * U[..., 0] - dt(500) * U[..., 1] + dt(200) * U[..., 2],
                   dt(-200) * U[..., 2]], -1)
    g = (df * slope / _c(illum, dt)) @ _c(OPP2XYZ, dt)
    a = np.zeros((h, w, 3), dt)
    for ch in range(3):
        for kv, kh in _pairs(filt, ch, dt):  # the vertical pass's transpose first
            a[..., ch] += (adj_matrix(kv, h, dt) @ g[..., ch]) @ adj_matrix(kh, w, dt).T
    S = np.zeros((K, 3), dt)
    np.add.at(S, idx, a.reshape(-1, 3))
    counts = np.bincount(idx, minlength=K)
    rgb = _c(pal4, dt).reshape(-1, 4)[:, :3]
    with np.errstate(invalid="ignore"):
        dlin = np.where(rgb <= _c(T0, dt), dt(1) / _c(LO, dt),
                        _c(GAMMA, dt) / _c(DIV, dt) * ((rgb + _c(OFF, dt)) / _c(DIV, dt)) ** (_c(GAMMA, dt) - dt(1)))
    grad = (S @ _c(RGB2OPP, dt)) * dlin / dt(w * h)
    grad[counts == 0] = 0
    return grad, counts, E


def taps_filters(k1, k2, k3, illum=o.D65):
    """An oracle.Filters of caller-given taps: k1, k2 [T, 3] per channel, k3 [T]."""
    T = len(k3)
    p1, p2 = np.zeros((T, 4), np.float32), np.zeros((T, 4), np.float32)
    p1[:, :3], p2[:, :3] = k1, k2
    k3 = np.asarray(k3, np.float32)
    return o.Filters(k1=p1, k2=p2, k3=k3, absk3=np.abs(k3), half=T // 2, illum=np.asarray(illum, np.float32),
                     ofilters=None)


def asym_filters():
    """An asymmetric 5-tap caller set: the fold-back and the |k3| / k3 order are visible in it."""
    k1 = np.array([[.05, .2, .1], [.3, .1, .25], [.4, .45, .3], [.15, .2, .3], [.1, .05, .05]], np.float32)
    k2 = np.array([[.3, .0, .1], [.1, .3, .05], [.2, .4, .5], [.05, .2, .3], [.3, .1, .05]], np.float32)
    return taps_filters(k1, k2, np.array([.2, -.3, .35, .1, -.15], np.float32))


def one_tap_filters():
    """One tap per filter: the blur and its adjoint are a per-channel scale."""
    return taps_filters(np.array([[.8, .7, .9]], np.float32), np.array([[.5, .6, .3]], np.float32),
                        np.array([-.4], np.float32))

"""hq_kmeanspp_seed's rule (include/hq.h) restated in numpy and Python integers, the inputs the
GPU test runs it on, and what can be checked without a device: the restatement never meets an
ambiguous prefix on those inputs, and the entry point exists and refuses a null context.
"""

import ctypes as C
import functools
import itertools

import numpy as np

import hybridquantization_amd as hq
from hybridquantization_amd import _lib

M64 = (1 << 64) - 1


def word(seed, p, r):
    z = (seed + (p << 32) + r + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def q_float(v, scale):
    """RN(clamp(v, 0, 1) scale): the fp32 product, ties to even."""
    return np.rint(np.clip(np.asarray(v, np.float32), 0, 1) * np.float32(scale)).astype(np.int64)


def seed_ref(q, w, P, K, seed, fixed_q=()):
    """q int64 (N, 3), w int64 (N,) -> pixels int64 (P, K) (-1: a fixed colour) and whether every
    draw was unambiguous: prefix[x - 1] <= t < prefix[x] with w D > 0 at x."""
    n = len(fixed_q)
    pixels, sharp = np.full((P, K), -1, np.int64), True
    dist = lambda c: ((q - np.asarray(c, np.int64)) ** 2).sum(axis=1)  # noqa: E731
    for p in range(P):
        D = None
        for c in fixed_q:
            D = dist(c) if D is None else np.minimum(D, dist(c))
        for r in range(n, K):
            wd = w * (1 if D is None else D)
            if int(wd.sum()) == 0:
                wd = w.copy()
            prefix = np.cumsum(wd)
            t = (word(seed, p, r) * int(prefix[-1])) >> 64
            x = int(np.searchsorted(prefix, t, side="right"))
            sharp &= bool(prefix[x] > t and (x == 0 or prefix[x - 1] <= t) and wd[x] > 0)
            pixels[p, r] = x
            D = dist(q[x]) if D is None else np.minimum(D, dist(q[x]))
    return pixels, sharp


# ---- the inputs: (w, h, form, variant, K, P), shared with test_kmeanspp_gpu.py ----
FIXED = np.array([[0.25, 0.5, 0.75], [1.0, 0.0, 0.1]], np.float32)
CASES = [c for c in itertools.product(((70, 67), (2, 2)), ("packed", "planar"), ("plain",), (2, 16, 256), (1, 3))] + \
        [c for c in itertools.product(((70, 67),), ("packed", "planar"), ("mask", "weights", "few", "fixed"), (16,), (3,))]
SEED = 0xC0FFEE12345


@functools.lru_cache(maxsize=None)
def inputs(shape, form, variant):
    """-> rgba float32 (N, 4), q int64 (N, 3), w int64 (N,), map uint8 (N,) or None.  packed: a k/255
    image (q: the bytes); planar: floats off that lattice with exact 0 and 1 (q: RN(v 4095)); few:
    5 distinct colours; mask: holes, and the first and last rows out; weights: 0 .. 255 with zeros."""
    n = shape[0] * shape[1]
    rng = np.random.default_rng(n + len(form))
    by = rng.integers(0, 256, (n, 3))
    if variant == "few":
        by = by[:5][rng.integers(0, 5, n)]
    rgba = np.zeros((n, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    if form == "planar":
        rgba[:, :3] = np.float32(0.999) * rgba[:, :3] if variant == "few" else rng.random((n, 3), np.float32)
        rgba[0, 0], rgba[n - 1, 2] = 0.0, 1.0
    q = by.astype(np.int64) if form == "packed" else q_float(rgba[:, :3], 4095)
    m = None
    if variant == "mask":
        m = (rng.random(n) < 0.6).astype(np.uint8) * 200
        m[:shape[0]] = m[-shape[0]:] = 0
    if variant == "weights":
        m = rng.integers(0, 256, n).astype(np.uint8) * (rng.random(n) < 0.7)
    w = np.ones(n, np.int64) if m is None else (m != 0).astype(np.int64) if variant == "mask" else m.astype(np.int64)
    return rgba, q, w, m


@functools.lru_cache(maxsize=None)
def expected(shape, form, variant, K, P):
    """The restatement on a case -> (pixels, sharp); computed once, read by every test."""
    _, q, w, _ = inputs(shape, form, variant)
    fixed_q = tuple(map(tuple, q_float(FIXED, 255 if form == "packed" else 4095))) if variant == "fixed" else ()
    return seed_ref(q, w, P, K, SEED, fixed_q)


def test_restatement_is_never_ambiguous():
    assert all(expected(*c)[1] for c in CASES)
    few = expected((70, 67), "packed", "few", 16, 3)[0]  # 5 colours at K = 16: the T = 0 branch was taken
    assert len({tuple(inputs((70, 67), "packed", "few")[1][x]) for x in few[0]}) == 5


def test_entry_point_refuses_a_null_context():
    out = np.full(8, -7, np.float32)
    assert hq.load().hq_kmeanspp_seed(None, 1, 2, 0, _lib.fptr(out), None) == _lib.HQ_ERR_ARG
    assert np.all(out == -7)
    assert word(0, 0, 0) == 0xE220A8397B1DCDAF  # SplitMix64's first output from state 0

"""GPU tests of pattern dithering (libhq's addition): hq_pattern_population[_partial] through the C ABI
and its Python surface.  Index images and used flags bit for bit against the numpy restatement
(pattern_ref.py), costs within 1e-6 relative of the oracle's cost of those indices (hq.h's bar for every
path); n = 1 and strength 0 are the plain evaluation bit for bit."""

import ctypes as C

import numpy as np
import pytest

import c_oracle
import hybridquantization_amd as hq
import oracle as o
from hybridquantization_amd import _lib
from pattern_ref import pattern
from reuse_walk import custom_map
from test_grad_gpu import FILTERS, context, noise_rgba
from test_pattern import TIES

pytestmark = pytest.mark.gpu
P = 3


def palettes(K, seed=40):
    """P palettes of K colours; from K = 5 on, palette 1 opens with TIES: a duplicated colour, two
    colours of one Y, and two colours at one distance from a black pixel."""
    pals = np.stack([o.synthetic_palette(K, seed + p).reshape(K, 4) for p in range(P)]).astype(np.float32)
    if K >= 5:
        pals[1, :5] = TIES
    return pals.reshape(P, -1)


def image(w, h):
    rgba = noise_rgba(w, h, 3).reshape(-1, 4).copy()
    rgba[0, :3], rgba[-1, :3] = 0.0, 1.0  # black: equidistant from TIES' first two colours
    return rgba


_REF = {}


def ref_of(filt, w, h, K, n, s, tmap):
    """The restatement's (idx, used) per palette and the oracle's cost of them: once per case."""
    key = (filt, w, h, K, n, s, tmap)
    if key not in _REF:
        f, rgba, pals = FILTERS[filt](), image(w, h), palettes(K)
        lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
        per = []
        for p in range(P):
            pal = pals[p].reshape(K, 4)
            idx, used = pattern(rgba, pal, w, h, n, s, custom_map() if tmap else None)
            err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
            per.append((idx, used, o.average_array(err) + o.compute_penalty(used, 2.0)))
        _REF[key] = (f, rgba, pals, per)
    return _REF[key]


def ctx_of(gpu, f, rgba, w, img_u8=1, rows=(0, None), **opts):
    m = context(gpu, f)
    for name, v in dict(img_u8=img_u8, **opts).items():
        m.setOption(name, v)
    m.setImage(rgba.reshape(-1), None, w, f.illum, *rows)
    return m


# (filters, w, h, K, n, strength, img_u8, custom map): 70 x 67 is no multiple of a block's 1024 pixels and
# takes five; 5 x 3 is less than a wave (below the designed half-width 10: the one-tap filters).  n K is
# kept small where the image is large: the restatement runs n argmins of K colours in numpy.
CASES = [("designed", 70, 67, 1, 16, 1.0, 1, 0), ("designed", 70, 67, 2, 64, 1.0, 1, 0),
         ("designed", 70, 67, 2, 2, 0.5, 0, 1), ("designed", 70, 67, 5, 16, 1.0, 1, 1),
         ("designed", 70, 67, 5, 64, 0.5, 0, 0), ("designed", 70, 67, 5, 2, 1.0, 0, 0),
         ("designed", 70, 67, 16, 16, 1.0, 0, 0), ("designed", 70, 67, 16, 16, 0.5, 1, 1),
         ("designed", 70, 67, 16, 1, 1.0, 1, 1), ("designed", 70, 67, 16, 64, 0.0, 1, 0),
         ("designed", 70, 67, 255, 2, 1.0, 1, 0), ("designed", 70, 67, 256, 2, 0.5, 0, 1),
         ("designed", 70, 67, 256, 1, 0.0, 1, 0), ("one_tap", 5, 3, 256, 16, 1.0, 1, 1),
         ("one_tap", 5, 3, 255, 64, 0.5, 0, 0), ("one_tap", 5, 3, 5, 16, 1.0, 0, 1),
         ("one_tap", 5, 3, 16, 2, 0.5, 1, 0), ("one_tap", 5, 3, 1, 64, 1.0, 0, 0),
         ("one_tap", 5, 3, 2, 1, 1.0, 1, 1), ("one_tap", 5, 3, 16, 64, 1.0, 1, 1)]


@pytest.mark.parametrize("filt,w,h,K,n,s,img_u8,tmap", CASES)
def test_indices_used_and_costs_against_the_restatement(gpu, filt, w, h, K, n, s, img_u8, tmap):
    f, rgba, pals, per = ref_of(filt, w, h, K, n, s, tmap)
    m = ctx_of(gpu, f, rgba, w, img_u8)
    try:
        if tmap:
            m.setDitherMap(custom_map())
        costs, used = m.patternPopulation(pals, n, s, 2.0, return_used=True)
        assert m.lastPath()["pixels"] == ("u8" if img_u8 else "planar")
        for p, (idx, want_used, want) in enumerate(per):
            np.testing.assert_array_equal(m.getIndices(p), idx.astype(np.uint8), err_msg=f"p={p}")
            np.testing.assert_array_equal(used[p], want_used, err_msg=f"p={p}")
            print(f"p={p}: cost {costs[p]!r}, oracle {want!r}, rel {abs(costs[p] - want) / want:.2e}")
            assert abs(costs[p] - want) <= 1e-6 * abs(want), p
        # a palette alone is the palette inside the population, and a second call the first
        alone = m.patternPopulation(pals[1:2], n, s, 2.0)
        np.testing.assert_array_equal(m.getIndices(0), per[1][0].astype(np.uint8))
        assert alone[0] == costs[1] and np.array_equal(m.patternPopulation(pals, n, s, 2.0), costs)
    finally:
        m.close()


@pytest.mark.parametrize("n,s,img_u8", [(1, 1.0, 1), (1, 0.5, 0), (16, 0.0, 1), (16, 0.0, 0)])
def test_identities_with_the_plain_evaluation(gpu, n, s, img_u8):
    f, rgba, pals = FILTERS["designed"](), image(70, 67), palettes(16)
    m = ctx_of(gpu, f, rgba, 70, img_u8, pixel_err=1)
    try:
        got = []
        for call in (lambda: m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True),
                     lambda: m.patternPopulation(pals, n, s, 2.0, return_used=True)):
            costs, used = call()
            got.append([costs, used] + [m.getIndices(p) for p in range(P)] + [m.getPixelErrors(p) for p in range(P)])
        for a, b in zip(*got):
            np.testing.assert_array_equal(a, b)
    finally:
        m.close()


def test_shards_equal_the_whole_images_rows_and_add_up(gpu):
    w, h, K, n = 64, 48, 16, 16
    f, rgba, pals, per = ref_of("designed", w, h, K, n, 1.0, 0)
    m = ctx_of(gpu, f, rgba, w)
    try:
        whole, parts = m.patternPopulationPartial(pals, n, 1.0), []
        for r0, r1 in ((0, 20), (20, h)):  # (the second shard's extended rows start at row 10)
            m.setImage(rgba.reshape(-1), None, w, f.illum, r0, r1)
            parts.append(m.patternPopulationPartial(pals, n, 1.0))
            for p in range(P):
                np.testing.assert_array_equal(m.getIndices(p)[:(r1 - r0) * w], per[p][0][r0 * w:r1 * w].astype(np.uint8))
        for p in range(P):
            np.testing.assert_array_equal(whole[p, 1:] != 0, per[p][1] != 0)
            np.testing.assert_array_equal((parts[0][p, 1:] != 0) | (parts[1][p, 1:] != 0), whole[p, 1:] != 0)
            s = parts[0][p, 0] + parts[1][p, 0]
            print(f"p={p}: shards {s!r}, whole {whole[p, 0]!r}")
            assert abs(s - whole[p, 0]) <= 1e-6 * whole[p, 0]
    finally:
        m.close()


def test_refusals_path_and_profile(gpu):
    lib = hq.load()
    w, h, K = 64, 48, 8
    f, rgba, pals = FILTERS["designed"](), image(w, h), palettes(K)
    m = ctx_of(gpu, f, rgba, w)
    try:
        def refused(status, pl=pals, n=16, s=1.0):
            costs, used = np.full(P, -7.0), np.full((P, pl.shape[1] // 4), -7, np.int32)
            seq = m.lastPath()["sequence"]
            rc = lib.hq_pattern_population(m.ctx, _lib.fptr(pl), P, pl.shape[1] // 4, n, s, 2.0, _lib.dptr(costs),
                                           _lib.iptr(used))
            assert rc == status, (rc, n, s)
            assert np.all(costs == -7.0) and np.all(used == -7) and m.lastPath()["sequence"] == seq

        m.computeQuantizationErrorPopulation(pals, 2.0)
        held = m.getIndices(1)
        for n in (0, -1, 3, 24, 128):
            refused(_lib.HQ_ERR_ARG, n=n)
        for s in (-0.001, 1.001, float("nan"), float("inf")):
            refused(_lib.HQ_ERR_ARG, s=s)
        refused(_lib.HQ_ERR_UNSUPPORTED, palettes(257))
        bad = pals.copy()
        bad[2, 5] = 1.001
        refused(_lib.HQ_ERR_ARG, bad)           # inherited: a palette channel outside [0, 1]
        m.setOption("slice_ranks", 2)
        refused(_lib.HQ_ERR_UNSUPPORTED)        # inherited: a palette slice
        m.setOption("slice_ranks", 1)
        np.testing.assert_array_equal(m.getIndices(1), held)
        # one "pattern" launch per pass, nothing under grid and assign
        lib.hq_profile_enable(m.ctx, 1)
        lib.hq_profile_reset(m.ctx)
        m.patternPopulation(pals, 16, 1.0)
        m.patternPopulation(pals, 2, 0.5)
        path, got = m.lastPath(), {}
        assert (path["argmin"], path["pass"], path["grid"], path["ordered"]) == ("pattern", "full", "none", 0)
        for name in ("pattern", "assign", "grid", "cost", "finalize"):
            ms, cnt = C.c_double(), C.c_int64()
            _lib.check(lib.hq_profile_get(m.ctx, name.encode(), C.byref(ms), C.byref(cnt)), m.ctx)
            got[name] = cnt.value
        assert got == {"pattern": 2, "assign": 0, "grid": 0, "cost": 2, "finalize": 2}
        # the Python renderings: the gathered palette, and findBestQuantization's final evaluation
        out = m.quantizePattern(pals[0], 16, 1.0)
        table = pals[0].reshape(K, 4)
        np.testing.assert_array_equal(out.reshape(-1, 4)[:, :3], table[m.getIndices(0)][:, :3])
        assert m.patternError == m.patternPopulation(pals[:1], 16, 1.0, 0.0)[0]
        sw = hq.SWASA(population=2, imax=100, seed=4)
        best = m.findBestQuantization(rgba.reshape(-1), None, w, 4, sw, None, None, f.illum, iterations=5, pattern=16)
        assert m.bestErrorPattern == m.patternPopulation(np.asarray(best, np.float32).reshape(1, -1), 16, 1.0, sw.delta)[0]
        with pytest.raises(ValueError):
            m.findBestQuantization(rgba.reshape(-1), None, w, 4, sw, None, None, f.illum, iterations=5, pattern=3)
    finally:
        m.close()

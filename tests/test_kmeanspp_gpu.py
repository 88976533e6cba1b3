"""GPU tests of hq_kmeanspp_seed through the C ABI and the binding: the drawn pixels equal the
numpy / Python-integer restatement of the rule (test_kmeanspp.py) exactly and the palettes bit
for bit, on every case of its list with the streaming kernel's span forced small and at its
default; then determinism, the population rule, the search start and the refusals.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
from hybridquantization_amd import _lib
from lloyd_ref import bits as fbits
from test_kmeanspp import CASES, FIXED, SEED, expected, inputs
from test_lloyd_gpu import blob_image
from test_seed_gpu import make_ctx, run_from

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ip(gpu):
    """A context with one-tap filters (half-width 0), so that a 2 x 2 image is accepted."""
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=gpu)
    one = np.ones(1, np.float32)
    m.updateOpenCLFilters([[one, one, one]] * 3, one)
    yield m
    m.close()


def set_case(m, shape, form, variant):
    rgba, _, w, mp = inputs(shape, form, variant)
    m.setImage(rgba.reshape(-1), None, shape[0], None)
    if variant == "mask":
        m.setMask(mp)
    if variant == "weights":
        m.setWeights(mp)
    m.setFixedColors(FIXED if variant == "fixed" else None)
    return rgba, w


def raw_seed(m, P, K, seed=SEED):
    """hq_kmeanspp_seed through ctypes -> (rc, palettes, pixels); the outputs start at -7."""
    pal = np.full((max(P, 1), 4 * max(min(K, 1 << 15), 1)), -7, np.float32)
    pix = np.full((pal.shape[0], pal.shape[1] // 4), -7, np.int64)
    rc = hq.load().hq_kmeanspp_seed(m.ctx, P, K, seed, _lib.fptr(pal), _lib.i64ptr(pix))
    return rc, pal, pix


@pytest.mark.parametrize("span", [1, 0], ids=["span1024", "auto"])
@pytest.mark.parametrize("shape,form,variant,K,P", CASES,
                         ids=[f"{c[0][0]}x{c[0][1]}-{c[1]}-{c[2]}-K{c[3]}-P{c[4]}" for c in CASES])
def test_seed_equals_the_restatement(ip, shape, form, variant, K, P, span):
    """span 1: spans of 1024 pixels, 5 partials at 70 x 67, so the pick crosses span boundaries;
    0: the default, one span.  2 x 2 at K > 4 and the 5-colour image take the T = 0 branch."""
    rgba, w = set_case(ip, shape, form, variant)
    ip.setOption("kmpp_span", span)
    pal, pix = ip.kmeansppSeed(P, K, SEED)
    want, _ = expected(shape, form, variant, K, P)
    np.testing.assert_array_equal(pix, want)
    colours = np.where(want[..., None] >= 0, rgba[want], 0)  # (the chosen pixel's colour, .w = 0)
    if variant == "fixed":
        colours[:, :2, :3] = FIXED
    np.testing.assert_array_equal(fbits(pal), fbits(colours.reshape(P, -1)))
    assert np.all(w[pix[pix >= 0]] > 0)  # every chosen pixel counts: in-mask, of non-zero weight


@pytest.mark.parametrize("form", ["packed", "planar"])
def test_two_calls_and_single_palettes_agree(ip, form):
    """The same call twice gives identical bits, and palette p of a population is the palette
    P = 1 draws under seed + (p << 32): the words depend on that sum alone."""
    set_case(ip, (70, 67), form, "weights")
    pal, pix = ip.kmeansppSeed(3, 16, SEED)
    again = ip.kmeansppSeed(3, 16, SEED)
    assert again[0].tobytes() == pal.tobytes() and again[1].tobytes() == pix.tobytes()
    for p in range(3):
        one, one_pix = ip.kmeansppSeed(1, 16, SEED + (p << 32))
        assert one.tobytes() == pal[p].tobytes() and one_pix.tobytes() == pix[p].tobytes()


def test_search_from_kmeanspp_is_create_from_on_the_seeded_population(gpu):
    """findBestQuantization(init="kmeans++") is hq_search_create_from on kmeansppSeed's
    population under the search's seed: the same best colours and error after 20 iterations."""
    m = make_ctx(gpu)
    try:
        rgba, _ = blob_image(96, 64, seed=11)
        sw = hq.SWASA(population=3, imax=60, seed=17)
        best = m.findBestQuantization(rgba.reshape(-1), None, 96, 8, sw, None, None, m.illum, iterations=20,
                                      init="kmeans++")
        err = m.bestError
        pop, pix = m.kmeansppSeed(3, 8, 17)
        assert len({tuple(row) for row in pix}) == 3  # three different starts
        _, (colours, want, it) = run_from(m, 8, hq.SWASA(population=3, imax=60, seed=17), pop, 1, (20,))
        assert it == 20 and want == err
        np.testing.assert_array_equal(fbits(np.asarray(best, np.float32)), fbits(colours))
    finally:
        m.close()


def test_refusals_write_nothing(ip):
    def refused(status, P=2, K=4):
        rc, pal, pix = raw_seed(ip, P, K)
        assert rc == status, ip._lib.hq_last_error(ip.ctx)
        assert np.all(pal == -7) and np.all(pix == -7)

    refused(_lib.HQ_ERR_STATE)  # no image
    rgba, _, _, _ = inputs((70, 67), "packed", "plain")
    ip.setImage(rgba.reshape(-1), None, 70, None, row_begin=0, row_end=30)
    refused(_lib.HQ_ERR_STATE)  # a row-block shard
    ip.setImage(rgba.reshape(-1), None, 70, None)
    for name, on, off in (("slice_ranks", 2, 1), ("palette_split", 1, 0), ("assign_space", 1, 0)):
        ip.setOption(name, on)
        refused(_lib.HQ_ERR_UNSUPPORTED)
        ip.setOption(name, off)
    for P, K in ((2, 16385), (2, 0), (0, 4)):
        refused(_lib.HQ_ERR_ARG, P, K)
    ip.setFixedColors(FIXED)
    refused(_lib.HQ_ERR_ARG, 2, 1)  # K - nfixed < 0
    ip.setFixedColors(None)
    # an all-zero mask never reaches the call: hq_set_mask refuses it and the state in force stays
    zeros = np.zeros(70 * 67, np.uint8)
    assert hq.load().hq_set_mask(ip.ctx, _lib.u8ptr(zeros), 70, 67) == _lib.HQ_ERR_ARG
    rc, pal, pix = raw_seed(ip, 2, 4)
    assert rc == _lib.HQ_OK and np.all(pix >= 0) and not np.any(pal == -7)
    assert hq.load().hq_kmeanspp_seed(ip.ctx, 2, 4, SEED, None, None) == _lib.HQ_ERR_ARG

"""GPU tests of dot diffusion's tiled form (hq_dot_tile.hip; option "dot_tile" 1): one launch
whose workgroups each render a tile from the window its matrix's reach gives.  The index images
and used flags are checked bit for bit against the numpy restatement (dot_ref.py), the costs
against the oracle's at test_dot_gpu.py's bar (1e-5), and both forms against each other.  The
tile is the smallest shape, 16 x 16 (option "dot_tile_shape" 1), so that small images cross tile
borders; hq_dot_form says which form ran.
"""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
from dot_ref import KNUTH8, dot, random_classes
from dot_tile_ref import column_major, levels, row_major
from hybridquantization_amd import _lib
from test_dither_gpu import _assert_same, new_ctx, noise, pals_of
from test_dot_gpu import PERM4, PERM4B, PERM16, _both, _filters, case_ref, check_against_ref, raw_dot
from test_fast_path_gpu import _ctx as filter_ctx

pytestmark = pytest.mark.gpu

PERM8 = random_classes(8, 2)  # its left reach of 10 exceeds its side
TILED = dict(dot_tile=1, dot_tile_shape=1)
TW = TH = 16
MATRICES = {"knuth8": None, "perm4": PERM4, "perm4b": PERM4B, "perm8_2": PERM8, "perm16": PERM16}
DEPTH = {name: levels(KNUTH8 if cls is None else cls)[1] for name, cls in MATRICES.items()}

# (w, h): smaller than every matrix; exactly one tile; one tile and a pixel each way; 2 x 2 tiles
# and a remainder of one column and two rows -- narrower than any left reach (2 at least) and
# shorter than any reach upwards (4 at least); a single row and a single column over three tiles;
# 97 x 53, 7 x 4 tiles with remainders.
SHAPES = [(3, 2), (16, 16), (17, 17), (33, 34), (40, 1), (1, 40), (97, 53)]
BIG_K = {(17, 17), (33, 34), (97, 53)}  # where K = 255 and 256 run as well


def assert_tiled(m, name, shape=(TW, TH)):
    assert m.dotForm() == (2, shape[0], shape[1], DEPTH[name])


@pytest.mark.parametrize("w,h", SHAPES)
def test_indices_used_and_costs_against_the_restatement(gpu, w, h):
    """Knuth's matrix at every K (1 lane per pixel up to K = 6, 4 lanes from 16 on: K = 255
    leaves the lanes unequal shares), the other matrices at K = 2 and 16 and the 16 x 16 one at
    255 too; P = 1 and 3; strengths 1 and 0.5; both image forms."""
    plan = [("knuth8", K) for K in (1, 2, 6, 16) + ((255, 256) if (w, h) in BIG_K else ())]
    plan += [(name, K) for name in ("perm4", "perm4b", "perm8_2", "perm16") for K in (2, 16)]
    if (w, h) == (33, 34):
        plan.append(("perm16", 255))
    for img_u8 in (1, 0):
        m = filter_ctx(gpu, _filters(w, h), img_u8=img_u8, **TILED)
        try:
            first = True
            for name, K in plan:
                for s in (1.0, 0.5):
                    ref = case_ref(w, h, K, s, name, MATRICES[name])
                    if first:
                        m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
                        first = False
                    for Pn in (1, 3):
                        check_against_ref(m, ref, Pn, s, MATRICES[name],
                                          f"tiled {w}x{h} {name} K={K} P={Pn} s={s} img_u8={img_u8}")
                        assert_tiled(m, name)
        finally:
            m.close()


@pytest.mark.parametrize("w,h", [(3, 2), (17, 17), (33, 34), (40, 1), (1, 40)])
def test_the_chain_against_the_restatement_at_the_edge_shapes(gpu, w, h):
    """"dot_tile" 0: with auto as the default the whole-image cases of test_dot_gpu.py may take the
    tiled kernel, so the chain keeps its own comparison with the restatement at the shapes where
    its launch arithmetic can go wrong: smaller than the matrix, a tile and a pixel, odd sizes, a
    single row and a single column."""
    plan = [("knuth8", K) for K in (1, 6, 16)] + [("perm4", 16), ("perm16", 16)]
    m = filter_ctx(gpu, _filters(w, h), dot_tile=0)
    try:
        first = True
        for name, K in plan:
            for s in (1.0, 0.5):
                ref = case_ref(w, h, K, s, name, MATRICES[name])
                if first:
                    m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
                    first = False
                check_against_ref(m, ref, 3, s, MATRICES[name], f"chain {w}x{h} {name} K={K} s={s}")
                assert m.dotForm() == (1, 0, 0, DEPTH[name])
    finally:
        m.close()


def test_auto_stays_inside_the_measured_region(gpu):
    """Option "dot_tile" -1: the tiled kernel with a 32 x 32 or 64 x 32 tile, never the 16 x 16
    one (it lost a measured case), and the chain for an image of more than 2^20 pixels."""
    K = 6
    pals = pals_of(K, 7)
    m = new_ctx(gpu)
    try:
        m.setImage(noise(97, 53).reshape(-1), None, 97, m.illum)
        want = {0: (2, 64, 32, 15), 1: (1, 0, 0, 15), 2: (2, 32, 32, 15), 3: (2, 64, 32, 15)}
        for shape, form in want.items():
            m.setOption("dot_tile_shape", shape)
            m.dotPopulation(pals, 1.0)
            assert m.dotForm() == form, shape
        m.setOption("dot_tile_shape", 0)
        w, h = 2048, 513  # (2^20 pixels and one row: K P is small, the pixel bound alone decides)
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        m.dotPopulation(pals[:1], 1.0)
        assert m.dotForm() == (1, 0, 0, 15)
        m.setOption("dot_tile", 1)
        m.dotPopulation(pals[:1], 1.0)
        assert m.dotForm() == (2, 64, 32, 15)
    finally:
        m.close()


def test_ties_across_lanes(gpu):
    """Half the image is the grey 0.5 and the palette holds 0.25 and 0.75 grey, each twice, at
    indices that fall to different lanes (K = 16: 4 lanes): every rank distance of such a pixel
    ties exactly, between the duplicates and between the two greys, so near_d2's re-resolution
    runs across the lanes and the lowest index has to win."""
    w, h, K = 37, 21, 16
    rgba = noise(w, h, 3).copy()
    rgba[::2, :3] = 0.5
    pals = np.zeros((3, K, 4), np.float32)
    pals[:, :, :3] = (np.arange(K, dtype=np.float32) / K * 0.1)[None, :, None]  # (dark: further from the grey)
    for p in range(3):
        pals[p, [1 + p, 6, 11], :3] = 0.25   # lanes 1 + p, 2 and 3
        pals[p, [5, 8 + p, 14], :3] = 0.75   # lanes 1, p and 2
    pals = pals.reshape(3, -1)
    m = new_ctx(gpu, **TILED)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        for cls in (None, PERM4):
            _, used = m.dotPopulation(pals, 1.0, 2.0, classes=cls, return_used=True)
            assert m.dotForm()[0] == 2
            for p in range(3):
                idx, want_used = dot(rgba, pals[p].reshape(K, 4), w, h, 1.0, cls)
                assert np.count_nonzero(idx == 1 + p) > 0  # (a tie was there to resolve)
                np.testing.assert_array_equal(m.getIndices(p), idx.astype(np.uint8), err_msg=f"p={p}")
                np.testing.assert_array_equal(used[p], want_used)
    finally:
        m.close()


def _call(m, pals, s, cls):
    costs, used = m.dotPopulation(pals, s, 2.0, classes=cls, return_used=True)
    n = pals.shape[0]
    return costs, used, [m.getIndices(p) for p in range(n)], [m.getPixelErrors(p) for p in range(n)]


@pytest.mark.parametrize("shape", [0, 1, 2, 3])
def test_the_forms_agree_under_every_tile_shape(gpu, shape):
    """"dot_tile" 0 and 1 alternately on one context: identical costs (as doubles), used flags,
    index images and per-pixel errors; every tile shape, and 0 = the largest that fits."""
    w, h, K = 97, 53, 16
    tile = {0: (64, 32), 1: (16, 16), 2: (32, 32), 3: (64, 32)}[shape]
    m = new_ctx(gpu, pixel_err=1, dot_tile_shape=shape)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        pals = pals_of(K, 16)
        for name in ("knuth8", "perm16", "perm8_2"):
            for s in (1.0, 0.5):
                got = []
                for form in (0, 1, 0, 1):
                    m.setOption("dot_tile", form)
                    got.append(_call(m, pals, s, MATRICES[name]))
                    if form:
                        assert_tiled(m, name, tile)
                    else:
                        assert m.dotForm() == (1, 0, 0, DEPTH[name])
                for other in got[1:]:
                    _assert_same(got[0], other, f"{name} s={s} shape {shape}")
    finally:
        m.close()


def test_strength_zero_is_the_plain_evaluation(gpu):
    w, h, K = 97, 53, 16
    m = new_ctx(gpu, pixel_err=1, **TILED)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        for cls in (None, PERM16):
            plain, dotted = _both(m, pals_of(K, 16), 0.0, cls)
            assert m.dotForm()[0] == 2
            assert np.isfinite(plain[0]).all()
            _assert_same(plain, dotted)
    finally:
        m.close()


def test_dot_form_reports_the_form_taken(gpu):
    w, h, K = 37, 40, 6
    rgba, pals = noise(w, h, 9), pals_of(K, 7)
    m = new_ctx(gpu, dot_apron=5)
    try:
        assert m.dotForm() == (0, 0, 0, 0)  # no dot pass yet
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        assert m.dotForm() == (0, 0, 0, 0)
        m.setOption("dot_tile", 1)
        m.setOption("dot_tile_shape", 1)
        m.dotPopulation(pals, 1.0)
        assert m.dotForm() == (2, 16, 16, 15)
        # not eligible: the row-major and column-major 16 x 16 matrices reach 255 pixels sideways or upwards
        for cls in (row_major(), column_major()):
            want = [dot(rgba, pals[p].reshape(K, 4), w, h, 1.0, cls)[0] for p in range(3)]
            m.dotPopulation(pals, 1.0, classes=cls)
            assert m.dotForm() == (1, 0, 0, 256)
            for p in range(3):
                np.testing.assert_array_equal(m.getIndices(p), want[p].astype(np.uint8))
        m.dotPopulation(pals, 1.0)
        assert m.dotForm() == (2, 16, 16, 15)
        # a refused call (an illegal matrix, a strength outside [0, 1]) leaves the answer
        bad = KNUTH8.copy()
        bad[0, 0] = bad[0, 1]
        assert raw_dot(m, pals, 1.0, bad)[0] == _lib.HQ_ERR_ARG
        assert raw_dot(m, pals, 1.5)[0] == _lib.HQ_ERR_ARG
        assert m.dotForm() == (2, 16, 16, 15)
        m.setOption("dot_tile", 0)
        m.dotPopulation(pals, 1.0)
        assert m.dotForm() == (1, 0, 0, 15)
        # a row-block shard keeps the chain whatever the option says
        m.setOption("dot_tile", 1)
        m.setImage(rgba.reshape(-1), None, w, m.illum, row_begin=8, row_end=24)
        m.dotPopulationPartial(pals, 1.0)
        assert m.dotForm() == (1, 0, 0, 15)
        for name, bad in (("dot_tile", -2), ("dot_tile", 2), ("dot_tile_shape", -1), ("dot_tile_shape", 4)):
            with pytest.raises(Exception):
                m.setOption(name, bad)
        assert hq.load().hq_dot_form(None, None, None, None, None) == _lib.HQ_ERR_ARG
        assert hq.load().hq_dot_form(m.ctx, None, None, None, None) == _lib.HQ_OK
    finally:
        m.close()


def test_last_path_and_profile_are_the_chains(gpu):
    w, h, K = 97, 53, 16
    lib = hq.load()
    m = new_ctx(gpu, dot_tile_shape=1)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        pals = pals_of(K, 16)
        keys = set(m.lastPath())
        lib.hq_profile_enable(m.ctx, 1)
        m.dotPopulation(pals, 1.0)  # (so that both forms below follow a dot pass: previous_pass)

        def counts():
            got = {}
            for name in ("dot", "dither", "assign", "grid", "cost", "finalize"):
                ms, n = C.c_double(), C.c_int64()
                _lib.check(lib.hq_profile_get(m.ctx, name.encode(), C.byref(ms), C.byref(n)), m.ctx)
                got[name] = n.value
                assert (ms.value > 0) == (n.value > 0)
            return got

        seen = {}
        for form in (0, 1):
            m.setOption("dot_tile", form)
            lib.hq_profile_reset(m.ctx)
            m.dotPopulation(pals, 1.0)
            assert m.dotForm()[0] == 1 + form
            path = m.lastPath()
            assert set(path) == keys  # no key beyond the ones lastPath() had
            assert path["argmin"] == "dot" and path["pass"] == "dither" and path["grid"] == "none"
            path.pop("sequence")
            seen[form] = (path, counts())
        assert seen[0] == seen[1]
        assert seen[1][1] == {"dot": 1, "dither": 0, "assign": 0, "grid": 0, "cost": 1, "finalize": 1}
    finally:
        m.close()


def test_mask_and_weights_compose_and_leave_the_indices(gpu):
    """The rendering does not read the mask; the cost does: under a mask and under weights the
    tiled form's indices are the unmasked ones and its costs the chain's, as doubles."""
    w, h, K = 97, 53, 16
    m = new_ctx(gpu, dot_tile_shape=1)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        pals = pals_of(K, 16)
        m.setOption("dot_tile", 1)
        base_costs, _ = m.dotPopulation(pals, 1.0, 2.0, return_used=True)
        base = [m.getIndices(p) for p in range(3)]
        rng = np.random.default_rng(8)
        block = np.zeros((h, w), np.uint8)
        block[5:40, 20:70] = 1  # (crosses tile borders both ways)
        masks = [("mask", block, m.setMask), ("mask", (rng.random((h, w)) < 0.5).astype(np.uint8), m.setMask),
                 ("weights", rng.integers(0, 256, (h, w)).astype(np.uint8), m.setWeights)]
        for kind, arr, setter in masks:
            setter(arr)
            got = {}
            for form in (0, 1):
                m.setOption("dot_tile", form)
                costs, used = m.dotPopulation(pals, 1.0, 2.0, return_used=True)
                assert m.dotForm()[0] == 1 + form
                got[form] = (costs, used)
                for p in range(3):
                    np.testing.assert_array_equal(m.getIndices(p), base[p], err_msg=f"{kind} form {form} p={p}")
            np.testing.assert_array_equal(got[0][0], got[1][0])
            np.testing.assert_array_equal(got[0][1], got[1][1])
            if np.count_nonzero(arr) < arr.size:
                assert not np.array_equal(got[1][0], base_costs)  # (the cost did read it)
            setter(None)
    finally:
        m.close()

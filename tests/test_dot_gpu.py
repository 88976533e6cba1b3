"""GPU tests of dot diffusion (libhq's addition): hq_dot_population through the C ABI and its
Python surface.  The index images and used flags are checked bit for bit against the numpy
restatement (dot_ref.py), the costs against the oracle's cost of those indices at
test_dither_gpu.py's bar (1e-5); strength 0 is the plain evaluation bit for bit.  The shapes
are chosen for the launch arithmetic: one launch per class, and none for a class without a
pixel in an image smaller than the tile.
"""

import ctypes as C

import numpy as np
import pytest

import c_oracle
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from dither_ref import cube_corners, ramp_image
from dot_ref import KNUTH8, dot, random_classes
from hybridquantization_amd import _lib
from test_dither_gpu import _assert_same, _search16, _sums_and_errors, new_ctx, noise, pals_of
from test_fast_path import caller_filters
from test_fast_path_gpu import _ctx as filter_ctx
from test_lloyd_gpu import blob_image
from test_mask_gpu import sweep_masks
from test_weights_gpu import sweep_maps

pytestmark = pytest.mark.gpu

DE76 = hq.deltaETypes.CIE76
PMAX = 5
PERM4, PERM4B, PERM16 = random_classes(4, 44), random_classes(4, 45), random_classes(16, 46)


def matrix_of(cls):
    m = _lib.hq_dot_classes()
    c = np.asarray(cls)
    m.n = c.shape[0]
    for i, v in enumerate(c.reshape(-1)):
        m.cls[i] = int(v)
    return m


def raw_dot(m, pals, strength, cls=None, delta=2.0, Pn=None, K=None, costs_ptr=True):
    """hq_dot_population with sentinel outputs -> (status, costs, used); cls: None (NULL), an
    array or an hq_dot_classes."""
    Pn = pals.shape[0] if Pn is None else Pn
    K = pals.shape[1] // 4 if K is None else K
    costs = np.full(max(Pn, 1), -7.0, np.float64)
    used = np.full((max(Pn, 1), max(K, 1)), -7, np.int32)
    mat = None if cls is None else cls if isinstance(cls, _lib.hq_dot_classes) else matrix_of(cls)
    rc = hq.load().hq_dot_population(m.ctx, _lib.fptr(pals) if pals is not None else None, Pn, K,
                                     None if mat is None else C.byref(mat), strength, delta,
                                     _lib.dptr(costs) if costs_ptr else None, _lib.iptr(used))
    return rc, costs, used


# ---------------------------------------------------------------------------
# 1. Indices, used flags and costs against the restatement
# ---------------------------------------------------------------------------
# (w, h): smaller than the tile (most classes have no pixel, so no launch); one tile and one
# pixel more each way; two tiles side by side; no multiple of the tile; a single row and column;
# more than one workgroup per class needs 256 n^2 pixels -- 97 x 53 under the 4 x 4 matrix.
SHAPES = [(1, 1), (3, 2), (5, 7), (8, 8), (9, 9), (16, 8), (13, 11), (1, 17), (17, 1), (37, 21), (97, 53)]
_REF = {}


def _filters(w, h):
    """The designed 72 dpi / 45 cm set (half-width 10) where the image holds it, else a
    caller-supplied set of half-width 0, as test_dither_gpu.py's small cases."""
    return o.design_filters(72, 45.0) if min(w, h) >= 10 else caller_filters("asymmetric", 0)


def case_ref(w, h, K, s, mname, cls):
    """Image, oracle LabRef, PMAX palettes and per palette the restatement's indices, used
    flags and the oracle's cost of them; computed once per case, read-only."""
    key = (w, h, K, s, mname)
    if key not in _REF:
        base = (w, h)
        if base not in _REF:
            f = _filters(w, h)
            rgba = noise(w, h, seed=5 if (w, h) == (97, 53) else w + h)
            lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
            _REF[base] = dict(f=f, rgba=rgba, lab=lab)
        b = _REF[base]
        pals = pals_of(K, 16 if (w, h) == (97, 53) else 3 * K + w, PMAX)
        per = []
        for p in range(PMAX):
            pal = pals[p].reshape(K, 4)
            idx, used = dot(b["rgba"], pal, w, h, s, cls)
            err = o.ciede76(b["lab"], o.candidate_scielab(idx, pal, b["f"], w, h))
            per.append(dict(idx=idx, used=used, cost=o.average_array(err) + o.compute_penalty(used, 2.0)))
        _REF[key] = dict(b, pals=pals, per=per)
    return _REF[key]


def check_against_ref(m, ref, Pn, s, cls, msg):
    costs, used = m.dotPopulation(ref["pals"][:Pn], s, 2.0, classes=cls, return_used=True)
    for p in range(Pn):
        r = ref["per"][p]
        np.testing.assert_array_equal(m.getIndices(p), r["idx"].astype(np.uint8), err_msg=f"{msg} p={p}")
        np.testing.assert_array_equal(used[p], r["used"], err_msg=f"{msg} p={p}")
        print(f"{msg} p={p}: cost {costs[p]!r}, oracle {r['cost']!r}")
        assert abs(costs[p] - r["cost"]) <= 1e-5 * abs(r["cost"]), f"{msg} p={p}"


@pytest.mark.parametrize("w,h", SHAPES)
def test_indices_used_and_costs_against_the_restatement(gpu, w, h):
    """Both image forms (the packed bytes of a k/255 image, and the planar floats: the kernel
    reads the planar floats either way); Knuth's matrix at every K and P, the 4 x 4 permutation
    at K = 2 and 16 and P = 1 and 3; strengths 0.5 and 1."""
    plan = [("knuth8", None, K, Pn) for K in (1, 2, 6, 16) + ((256,) if (w, h) == (37, 21) else ())
            for Pn in (1, 3, 5)]
    plan += [("perm4", PERM4, K, Pn) for K in (2, 16) for Pn in (1, 3)]
    for img_u8 in (1, 0):
        m = filter_ctx(gpu, _filters(w, h), img_u8=img_u8)
        try:
            first = True
            for mname, cls, K, Pn in plan:
                for s in (1.0, 0.5):
                    ref = case_ref(w, h, K, s, mname, cls)
                    if first:
                        m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
                        first = False
                    check_against_ref(m, ref, Pn, s, cls, f"{w}x{h} {mname} K={K} P={Pn} s={s} img_u8={img_u8}")
        finally:
            m.close()


def test_a_16x16_matrix_runs_256_launches(gpu):
    """(20, 35): wider than the tile by 4 and taller by 3, so 256 launches of 1 to 6 pixels."""
    w, h = 20, 35
    m = filter_ctx(gpu, _filters(w, h))
    try:
        for K in (6, 16):
            for s in (1.0, 0.5):
                ref = case_ref(w, h, K, s, "perm16", PERM16)
                m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
                check_against_ref(m, ref, 3, s, PERM16, f"20x35 perm16 K={K} s={s}")
    finally:
        m.close()


def test_two_matrices_alternately_on_one_context(gpu):
    """The tables on the device are those of the matrix of the call: Knuth's, two 4 x 4
    permutations and the 16 x 16 one in turn, each twice in a row and again later."""
    w, h, K = 37, 21, 6
    m = filter_ctx(gpu, _filters(w, h))
    try:
        ref0 = case_ref(w, h, K, 1.0, "knuth8", None)
        m.setImage(ref0["rgba"].reshape(-1), ref0["lab"].reshape(-1), w, m.illum)
        seq = [("perm4", PERM4), ("knuth8", None), ("knuth8", KNUTH8), ("perm4b", PERM4B), ("perm4", PERM4),
               ("perm4", PERM4), ("perm16", PERM16), ("perm4b", PERM4B), ("knuth8", None)]
        for i, (mname, cls) in enumerate(seq):
            ref = case_ref(w, h, K, 1.0, "knuth8" if cls is KNUTH8 else mname, cls)
            check_against_ref(m, ref, 3, 1.0, cls, f"call {i} {mname}")
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 2. Strength 0, NULL, the path, the state
# ---------------------------------------------------------------------------
def _both(m, pals, s, cls=None):
    """(plain, dot-diffused at s): costs, used, indices and per-pixel dE of each."""
    out = []
    for call in (lambda: m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True),
                 lambda: m.dotPopulation(pals, s, 2.0, classes=cls, return_used=True)):
        costs, used = call()
        n = pals.shape[0]
        out.append((costs, used, [m.getIndices(p) for p in range(n)], [m.getPixelErrors(p) for p in range(n)]))
    return out


@pytest.mark.parametrize("cost_variant", [0, 1])
def test_strength_zero_is_the_plain_evaluation(gpu, cost_variant):
    w, h, K = 97, 53, 16
    m = new_ctx(gpu, DE76, pixel_err=1, cost_variant=cost_variant)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        for cls in (None, PERM4):
            plain, dotted = _both(m, pals_of(K, 16), 0.0, cls)
            assert np.isfinite(plain[0]).all()
            _assert_same(plain, dotted, f"cost_variant {cost_variant}")
    finally:
        m.close()


def test_null_classes_is_the_preset_passed_explicitly(gpu):
    w, h, K = 37, 21, 6
    m = new_ctx(gpu, pixel_err=1)
    try:
        m.setImage(noise(w, h, w + h).reshape(-1), None, w, m.illum)
        pals = pals_of(K, 7)
        preset = _lib.hq_dot_classes()
        assert hq.load().hq_dot_preset(0, C.byref(preset)) == _lib.HQ_OK
        got = []
        for cls in (None, preset, PERM4):
            rc, costs, used = raw_dot(m, pals, 1.0, cls)
            assert rc == _lib.HQ_OK
            got.append((costs, used, [m.getIndices(p) for p in range(3)], [m.getPixelErrors(p) for p in range(3)]))
        _assert_same(got[0], got[1], "NULL against the preset")
        assert any(not np.array_equal(a, b) for a, b in zip(got[0][2], got[2][2]))  # (another matrix is another image)
    finally:
        m.close()


@pytest.mark.parametrize("cost_variant", [0, 1])
def test_last_path_names_the_dot_kernel_and_the_cost_path(gpu, cost_variant):
    w, h, K = 97, 53, 16
    m = new_ctx(gpu, cost_variant=cost_variant)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        keys = set(m.lastPath())
        m.dotPopulation(pals_of(K, 16), 1.0)
        trim_ok, taps_fit = pr.filter_properties(m)
        want = pr.expected(m.options, m.deltaEType, m.halfSize, K, 3, trim_ok=trim_ok, taps_fit=taps_fit,
                           kind="dither", w=w, h=h)
        want["argmin"] = "dot"  # the model's rendering pass, with this kernel in the argmin's place
        got = m.lastPath()
        pr.assert_path(got, want, f"cost_variant {cost_variant}")
        assert got["cost"] == ("cost16w" if cost_variant == 0 else "tiled_generic")
        assert got["diffuse_rows"] == got["diffuse_slope"] == 0 and got["grid"] == "none"
        assert set(got) == keys  # no key beyond the ones lastPath() had
    finally:
        m.close()


def test_state_after_a_dot_diffused_call(gpu):
    """The getters answer for the rendering; clusterSums and clusterErrors give HQ_ERR_STATE
    until the next plain evaluation."""
    w, h, K = 97, 53, 16
    m = new_ctx(gpu, pixel_err=1)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        pals = pals_of(K, 16)
        before = _both(m, pals, 1.0)
        ref = case_ref(w, h, K, 1.0, "knuth8", None)
        for p in range(3):
            np.testing.assert_array_equal(before[1][2][p], ref["per"][p]["idx"].astype(np.uint8))
            np.testing.assert_array_equal(m.getIndices32(p), before[1][2][p].astype(np.uint32))
            assert before[1][3][p].shape == (w * h,) and np.isfinite(before[1][3][p]).all()
            # the stored per-pixel errors are this rendering's: their mean is its cost without the penalty
            mean = float(np.mean(before[1][3][p].astype(np.float64)))
            unused = int(np.count_nonzero(before[1][1][p] == 0))
            assert abs(before[1][0][p] - 2.0 * unused - mean) <= 1e-5 * mean
        assert list(_sums_and_errors(m, 3, K)[:2]) == [_lib.HQ_ERR_STATE, _lib.HQ_ERR_STATE]
        m.computeQuantizationErrorPopulation(pals, 2.0)
        s1 = _sums_and_errors(m, 3, K)
        assert s1[:2] == (_lib.HQ_OK, _lib.HQ_OK)
        again = _both(m, pals, 1.0)
        _assert_same(before[0], again[0], "the plain evaluation, before and after dot-diffused calls")
        _assert_same(before[1], again[1], "two identical dot-diffused calls")
    finally:
        m.close()


def _dot_eval(m, pals):
    return m.dotPopulation(pals, 0.75, 2.0, return_used=True)


def test_under_a_mask_and_under_weights(gpu):
    """test_mask_gpu.py's and test_weights_gpu.py's sweeps with this rendering as the
    evaluation: under every mask and weight map the indices, used flags and stored errors keep
    the unmasked call's bits and the cost is the masked or weighted cost of them."""
    w, h, K = 97, 53, 16
    m = new_ctx(gpu, pixel_err=1)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        sweep_masks(m, pals_of(K, 16), w, h, "dot", evaluate=_dot_eval)
        sweep_maps(m, pals_of(K, 16), w, h, "dot", evaluate=_dot_eval)
    finally:
        m.close()


def test_a_live_search_does_not_see_a_dot_diffused_call(gpu):
    """Two runs of a device search with and without a call between them: one trajectory."""
    w, h, K = 97, 53, 16
    lib = hq.load()
    out = []
    for between in (False, True):
        m = new_ctx(gpu)
        try:
            m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
            sw = hq.SWASA(population=3, imax=100, seed=9, t0=0.05)
            params, hd = sw.params(), C.c_void_p()
            _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(hd)), m.ctx)
            try:
                ran = C.c_int()
                _lib.check(lib.hq_search_run(hd, 8, C.byref(ran)), m.ctx)
                if between:
                    m.dotPopulation(pals_of(K, 16), 1.0)
                _lib.check(lib.hq_search_run(hd, 8, C.byref(ran)), m.ctx)
                best, err = np.zeros(4 * K, np.float32), C.c_double()
                _lib.check(lib.hq_search_best(hd, _lib.fptr(best), C.byref(err), None), m.ctx)
                out.append((ran.value, best, err.value))
            finally:
                lib.hq_search_destroy(hd)
        finally:
            m.close()
    assert out[0][0] == out[1][0] == 8 and out[0][2] == out[1][2]
    np.testing.assert_array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
    # and a search made after a dot-diffused call is the search without one
    first = []
    for dotted_first in (False, True):
        m = new_ctx(gpu)
        try:
            m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
            if dotted_first:
                m.dotPopulation(pals_of(K, 16), 1.0)
            first.append(_search16(m, K))
        finally:
            m.close()
    assert first[0][2] == first[1][2]
    np.testing.assert_array_equal(first[0][1].view(np.uint32), first[1][1].view(np.uint32))


# ---------------------------------------------------------------------------
# 3. Refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_outputs_state_and_path_untouched(gpu):
    w, h, K = 64, 48, 8
    rgba = noise(w, h, 2)
    pals = pals_of(K, 1)
    m = new_ctx(gpu)
    try:
        def refused(status, pl=pals, s=1.0, cls=None, **kw):
            path = m.lastPath()
            rc, costs, used = raw_dot(m, pl, s, cls, **kw)
            assert rc == status, (rc, hq.load().hq_last_error(m.ctx))
            assert np.all(costs == -7.0) and np.all(used == -7)
            assert m.lastPath() == path

        refused(_lib.HQ_ERR_STATE)  # no image set
        m.setImage(rgba.reshape(-1), None, w, m.illum, row_begin=8, row_end=40)
        refused(_lib.HQ_ERR_STATE)  # a row-block shard
        m.setOption("pixel_err", 1)
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        plain = _both(m, pals, 1.0)[0]

        def state():
            return [m.getIndices(p) for p in range(3)] + [m.getPixelErrors(p) for p in range(3)]

        m.computeQuantizationErrorPopulation(pals, 2.0)
        held = state()
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            refused(_lib.HQ_ERR_UNSUPPORTED)
            m.setOption(name, 0 if name == "palette_split" else 1)
        refused(_lib.HQ_ERR_UNSUPPORTED, pals_of(257, 1))  # K > 256
        refused(_lib.HQ_ERR_UNSUPPORTED, np.zeros((65536, 4), np.float32))  # P > 65535, K = 1
        refused(_lib.HQ_ERR_ARG, Pn=0)
        refused(_lib.HQ_ERR_ARG, K=0)
        refused(_lib.HQ_ERR_ARG, None, Pn=3, K=K)
        assert raw_dot(m, pals, 1.0, costs_ptr=False)[0] == _lib.HQ_ERR_ARG
        for s in (-0.001, 1.001, float("nan"), float("inf")):
            refused(_lib.HQ_ERR_ARG, s=s)
        for ch, v in ((0, np.nan), (5, np.inf), (2, -0.001), (4 * K * 2 + 1, 1.001)):
            bad = pals.copy()
            bad.reshape(-1)[ch] = v
            refused(_lib.HQ_ERR_ARG, bad)
        # illegal matrices: a side that is none of 4, 8, 16; a repeated class; a class out of range
        for n in (3, 5, 32):
            bad = matrix_of(np.arange(16).reshape(4, 4))
            bad.n = n
            refused(_lib.HQ_ERR_ARG, cls=bad)
        rep = KNUTH8.copy()
        rep[0, 0] = rep[7, 7]
        refused(_lib.HQ_ERR_ARG, cls=rep)
        out = PERM4.copy()
        out[np.unravel_index(np.argmax(out), out.shape)] = 16
        refused(_lib.HQ_ERR_ARG, cls=out)
        ok = pals.copy()
        ok[:, 3::4] = np.nan  # (.w is not a channel)
        assert raw_dot(m, ok, 1.0)[0] == _lib.HQ_OK
        m.computeQuantizationErrorPopulation(pals, 2.0)
        for a, b in zip(held, state()):
            np.testing.assert_array_equal(a, b)
        # after all those refusals the evaluated state is the plain evaluation's still
        refused(_lib.HQ_ERR_ARG, s=2.0)
        refused(_lib.HQ_ERR_ARG, cls=rep)
        for a, b in zip(held, state()):
            np.testing.assert_array_equal(a, b)
        assert _sums_and_errors(m, 3, K)[:2] == (_lib.HQ_OK, _lib.HQ_OK)
        np.testing.assert_array_equal(m.computeQuantizationErrorPopulation(pals, 2.0), plain[0])
        # an image pixel outside [0, 1]: found on the device, once per image
        img = rgba.copy()
        img[w * 17 + 5, 1] = 1.5
        m.setImage(img.reshape(-1), None, w, m.illum)
        refused(_lib.HQ_ERR_UNSUPPORTED)
        refused(_lib.HQ_ERR_UNSUPPORTED)  # (the remembered answer)
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        assert raw_dot(m, pals, 1.0)[0] == _lib.HQ_OK
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 4. Profile
# ---------------------------------------------------------------------------
def test_profile_counts_under_dot_and_nothing_under_assign(gpu):
    w, h, K = 97, 53, 16
    lib = hq.load()
    m = new_ctx(gpu)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        pals = pals_of(K, 16)
        lib.hq_profile_enable(m.ctx, 1)
        lib.hq_profile_reset(m.ctx)

        def counts():
            got = {}
            for name in ("dot", "dither", "assign", "grid", "cost", "finalize"):
                ms, n = C.c_double(), C.c_int64()
                _lib.check(lib.hq_profile_get(m.ctx, name.encode(), C.byref(ms), C.byref(n)), m.ctx)
                got[name] = n.value
                assert (ms.value > 0) == (n.value > 0)
            return got

        m.computeQuantizationErrorPopulation(pals, 2.0)
        assert counts() == {"dot": 0, "dither": 0, "assign": 1, "grid": 1, "cost": 1, "finalize": 1}
        m.dotPopulation(pals, 1.0)
        m.dotPopulation(pals, 0.5, classes=PERM4)
        assert counts() == {"dot": 2, "dither": 0, "assign": 1, "grid": 1, "cost": 3, "finalize": 3}
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 5. The point of the feature, and Python
# ---------------------------------------------------------------------------
def test_ramp_costs_equal_the_restatements(gpu):
    w = h = 64
    f = o.design_filters(72, 45.0)
    rgba, pal = ramp_image(w, h), cube_corners()
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), lab.reshape(-1), w, m.illum)
        plain = m.computeQuantizationErrorPopulation(pal.reshape(1, -1), 2.0)[0]
        for s in (0.5, 1.0):
            got = m.dotPopulation(pal.reshape(1, -1), s, 2.0)[0]
            idx, used = dot(rgba, pal, w, h, s)
            np.testing.assert_array_equal(m.getIndices(0), idx.astype(np.uint8))
            err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
            want = o.average_array(err) + o.compute_penalty(used, 2.0)
            print(f"s={s}: device {got!r}, restatement {want!r}, plain {plain!r}, ratio {got / plain:.3f}")
            assert abs(got - want) <= 1e-5 * want
            assert got <= 0.6 * plain if s == 1.0 else got < plain
    finally:
        m.close()


def _find(m, rgba, w, K, **kw):
    sw = hq.SWASA(population=2, imax=100, seed=4)
    best = m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum, iterations=6, **kw)
    return np.asarray(best, np.float32), sw


def test_find_best_quantization_with_dot_and_dot_search(gpu):
    w, h, K = 96, 64, 6
    rgba = blob_image(w, h, seed=11)[0]
    m = new_ctx(gpu)
    try:
        plain, _ = _find(m, rgba, w, K)
        plain_err = m.bestError
        best, sw = _find(m, rgba, w, K, dot=1.0)
        np.testing.assert_array_equal(best.view(np.uint32), plain.view(np.uint32))
        assert m.bestError == plain_err
        assert m.bestErrorDot == m.dotPopulation(best.reshape(1, -1), 1.0, sw.delta)[0]
        found, sw = _find(m, rgba, w, K, dot=1.0, dotSearch=True, dotClasses=PERM4)
        assert m.iterations == 6
        assert m.bestError == m.bestErrorDot == m.dotPopulation(found.reshape(1, -1), 1.0, sw.delta, classes=PERM4)[0]
        # the rendering of the returned palette is quantizeDotDiffused's
        out = m.quantizeDotDiffused(found, 1.0, classes=PERM4)
        table = found.reshape(K, 4).copy()
        table[:, 3] = 0.0
        np.testing.assert_array_equal(out.view(np.uint32), table[m.getIndices(0)].reshape(-1).view(np.uint32))
        np.testing.assert_array_equal(m.getIndices(0), dot(rgba, table, w, h, 1.0, PERM4)[0].astype(np.uint8))
        np.testing.assert_array_equal(m.lastUsedColors, np.bincount(m.getIndices(0), minlength=K)[:K] > 0)
        assert m.dotError == m.dotPopulation(found.reshape(1, -1), 1.0, 0.0, classes=PERM4)[0]
        # forbidden combinations
        for kw in (dict(dotSearch=True), dict(dot=1.0, dither=1.0), dict(dot=1.0, ordered=0.2), dict(dot=1.5),
                   dict(dot=1.0, dotSearch=True, lloydEvery=2), dict(dot=1.0, dotSearch=True, repairSteps=1),
                   dict(dot=1.0, dotClasses=np.zeros((4, 5)))):
            with pytest.raises(ValueError):
                _find(m, rgba, w, K, **kw)
    finally:
        m.close()


def test_quantization_returns_the_dot_diffused_image(gpu):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    image = np.stack([rgba[:, 0], rgba[:, 1], rgba[:, 2]])
    sw = hq.SWASA(population=2, imax=100, seed=4)
    q0, best0, err0 = hq.quantization(image, w, K, sw, device=gpu, iterations=6)
    q1, best1, err1 = hq.quantization(image, w, K, sw, device=gpu, iterations=6, dot=1.0)
    np.testing.assert_array_equal(best0, best1)
    assert err0 == err1
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        want = m.quantizeDotDiffused(best1, 1.0).reshape(-1, 4)[:, :3].T
    finally:
        m.close()
    np.testing.assert_array_equal(q1, want)
    assert not np.array_equal(q0, q1)
    with pytest.raises(ValueError):
        hq.quantization(image, w, K, sw, device=gpu, iterations=6, dot=1.0, dither=0.5)

"""GPU tests of the dithered rendering (libhq's addition): hq_dither_population (the
Floyd-Steinberg instance of the error-diffusion kernel) through the C ABI and its Python surface.  The index images and used flags are checked bit for bit
against the numpy restatement (dither_ref.py), the costs against the oracle's cost of those
indices; strength 0 is the plain evaluation bit for bit.
"""

import ctypes as C

import numpy as np
import pytest

import c_oracle
import de2000_ref as d
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from dither_ref import cube_corners, dither, ramp_image
from hybridquantization_amd import _lib
from test_de2000_gpu import EXCL_DEG, _cols
from test_fast_path import LONG, caller_filters, designed_half
from test_fast_path_gpu import _ctx as filter_ctx
from test_gpu import exact_pixel_err

pytestmark = pytest.mark.gpu

DE76, DE00 = hq.deltaETypes.CIE76, hq.deltaETypes.CIEDE2000
P = 3


def new_ctx(gpu, de=DE76, **opts):
    """A context with the designed 72 dpi / 45 cm filters (half-width 10)."""
    m = pr.Context(de, device=gpu)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    for name, v in opts.items():
        m.setOption(name, v)
    return m


@pytest.fixture()
def ip(gpu):
    m = new_ctx(gpu)
    yield m
    m.close()


def noise(w, h, seed=5):
    R, G, B = o.synthetic_image(w, h, seed)
    return o.inline_rgba(R, G, B).reshape(-1, 4)


def pals_of(K, seed, n=P):
    return np.stack([o.synthetic_palette(K, seed + p).reshape(-1) for p in range(n)]).astype(np.float32)


def raw_dither(m, pals, strength, delta=2.0, Pn=None, K=None, costs_ptr=True):
    """hq_dither_population with sentinel outputs -> (status, costs, used)."""
    Pn = pals.shape[0] if Pn is None else Pn
    K = pals.shape[1] // 4 if K is None else K
    costs = np.full(max(Pn, 1), -7.0, np.float64)
    used = np.full((max(Pn, 1), max(K, 1)), -7, np.int32)
    rc = hq.load().hq_dither_population(m.ctx, _lib.fptr(pals) if pals is not None else None, Pn, K, strength, delta,
                                        _lib.dptr(costs) if costs_ptr else None, _lib.iptr(used))
    return rc, costs, used


# ---------------------------------------------------------------------------
# 1. Indices, used flags and costs against the restatement
# ---------------------------------------------------------------------------
# name: (w, h, K, filters, options).  Filters: None = the designed 72 / 45 set (half-width 10);
# an integer = the designed set of that half-width (8 x 1030 is narrower than half-width 10,
# which hq_set_image refuses: it runs at half-width 7); "caller0" = a caller-supplied set of
# half-width 0, as test_fast_path_gpu.py builds them.
CASES = {
    "97x53_k16": (97, 53, 16, None, {}),                        # odd width, one strip
    "64x64_k256": (64, 64, 256, None, {}),                      # the full LDS palette, 16-byte rows
    "70x150_k8_rows64": (70, 150, 8, None, {"dither_rows": 64}),  # three strips, the last partial
    "8x1030_k4": (8, 1030, 4, 7, {}),                           # crosses the default strip of 1024 rows
    "1x5": (1, 5, 6, "caller0", {}),                            # no left or right neighbour
    "2x3": (2, 3, 6, "caller0", {}),
    "5x1": (5, 1, 6, "caller0", {}),                            # no upper neighbour
    # strips of 64 rows: a second strip of one row and of two, and one row past two strips
    "40x65_k8_rows64": (40, 65, 8, None, {"dither_rows": 64}),
    "40x66_k8_rows64": (40, 66, 8, None, {"dither_rows": 64}),
    "40x129_k8_rows64": (40, 129, 8, None, {"dither_rows": 64}),
    # narrower than the tap window and across a strip: the carry row has no column 1, or no column 2
    "1x130_k8_rows64": (1, 130, 8, "caller0", {"dither_rows": 64}),
    "2x129_k8_rows64": (2, 129, 8, "caller0", {"dither_rows": 64}),
    "3x66_k8_rows64": (3, 66, 8, "caller0", {"dither_rows": 64}),
}
_REF = {}


def _filters(key):
    if key is None:
        return o.design_filters(72, 45.0)
    return caller_filters("asymmetric", 0) if key == "caller0" else designed_half(key)


def case_ref(name, s):
    """Image, oracle LabRef, palettes and per palette the restatement's indices, used flags
    and the oracle's cost of them; computed once per (case, strength), read-only."""
    if (name, s) not in _REF:
        w, h, K, fkey, _ = CASES[name]
        f = _filters(fkey)
        rgba = noise(w, h, seed=5 if name == "97x53_k16" else w + h)
        lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
        pals = pals_of(K, 16 if name == "97x53_k16" else 3 * K + w)
        per = []
        for p in range(P):
            pal = pals[p].reshape(K, 4)
            idx, used = dither(rgba, pal, w, h, s)
            err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
            per.append(dict(idx=idx, used=used, cost=o.average_array(err) + o.compute_penalty(used, 2.0)))
        _REF[(name, s)] = dict(f=f, rgba=rgba, lab=lab, pals=pals, per=per)
    return _REF[(name, s)]


@pytest.mark.parametrize("s", [1.0, 0.37])
@pytest.mark.parametrize("name", list(CASES))
def test_indices_used_and_costs_against_the_restatement(gpu, name, s):
    """Both image forms (the packed bytes of a k/255 image, and the planar floats: the kernel
    reads the planar floats either way, the plain argmin's values); P = 3 palettes in one
    call, each bitwise its own P = 1 call.  The cost bar is tests/test_gpu.py's 1e-5."""
    w, h, K, fkey, opts = CASES[name]
    ref = case_ref(name, s)
    for img_u8 in (1, 0):
        m = filter_ctx(gpu, ref["f"], img_u8=img_u8, **opts)
        try:
            m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
            costs, used = m.ditherPopulation(ref["pals"], s, 2.0, return_used=True)
            idx = [m.getIndices(p) for p in range(P)]
            for p in range(P):
                r = ref["per"][p]
                msg = f"{name} s={s} img_u8={img_u8} p={p}"
                np.testing.assert_array_equal(idx[p], r["idx"].astype(np.uint8), err_msg=msg)
                np.testing.assert_array_equal(used[p], r["used"], err_msg=msg)
                print(f"{msg}: cost {costs[p]!r}, oracle {r['cost']!r}")
                assert abs(costs[p] - r["cost"]) <= 1e-5 * abs(r["cost"]), msg
                c1, u1 = m.ditherPopulation(ref["pals"][p:p + 1], s, 2.0, return_used=True)
                assert c1[0] == costs[p], msg
                np.testing.assert_array_equal(u1[0], used[p], err_msg=msg)
                np.testing.assert_array_equal(m.getIndices(0), idx[p], err_msg=msg)
                np.testing.assert_array_equal(m.getIndices32(0), idx[p].astype(np.uint32), err_msg=msg)
        finally:
            m.close()


def test_a_planar_float_image(ip):
    """Pixels that are no k/255: there is no packed copy, the range check runs on the device
    (and finds nothing), and the indices are the restatement's."""
    w, h, K = 23, 17, 6
    rng = np.random.default_rng(23)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = rng.random((w * h, 3), np.float32)
    rgba[0, :3], rgba[1, :3] = 0.0, 1.0  # the ends of the range are inside it
    pals = pals_of(K, 61)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    for s in (1.0, 0.37):
        _, used = ip.ditherPopulation(pals, s, 2.0, return_used=True)
        for p in range(P):
            want_idx, want_used = dither(rgba, pals[p].reshape(K, 4), w, h, s)
            np.testing.assert_array_equal(ip.getIndices(p), want_idx.astype(np.uint8))
            np.testing.assert_array_equal(used[p], want_used)


# ---------------------------------------------------------------------------
# 2. Strength 0 is the plain evaluation
# ---------------------------------------------------------------------------
def _both(m, pals, s):
    """(plain, dithered at s): costs, used, indices and per-pixel dE of each."""
    out = []
    for call in (lambda: m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True),
                 lambda: m.ditherPopulation(pals, s, 2.0, return_used=True)):
        costs, used = call()
        n = pals.shape[0]
        out.append((costs, used, [m.getIndices(p) for p in range(n)], [m.getPixelErrors(p) for p in range(n)]))
    return out


def _assert_same(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)  # costs, bitwise (no NaN here)
    np.testing.assert_array_equal(a[1], b[1], err_msg=msg)
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        np.testing.assert_array_equal(x, y, err_msg=msg)


@pytest.mark.parametrize("cost_variant", [0, 1, 2])
@pytest.mark.parametrize("de", [DE76, DE00], ids=["de76", "de2000"])
def test_strength_zero_is_the_plain_evaluation(gpu, de, cost_variant):
    w, h, K = 97, 53, 16
    m = new_ctx(gpu, de, pixel_err=1, cost_variant=cost_variant)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        plain, dith = _both(m, pals_of(K, 16), 0.0)
        assert np.isfinite(plain[0]).all()
        _assert_same(plain, dith, f"de {de} cost_variant {cost_variant}")
    finally:
        m.close()


def test_strength_zero_with_a_long_filter(gpu):
    """halfSize 51 > 24: the generic pair, whatever cost_variant says."""
    w = h = 64
    f = designed_half(LONG[2])
    m = filter_ctx(gpu, f)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        plain, dith = _both(m, pals_of(16, 16), 0.0)
        assert np.isfinite(plain[0]).all()
        _assert_same(plain, dith)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 3. The other cost paths at strength 1
# ---------------------------------------------------------------------------
def test_fast_and_generic_costs_agree_at_strength_one(ip):
    w, h, K = 97, 53, 16
    ip.setImage(noise(w, h).reshape(-1), None, w, ip.illum)
    pals = pals_of(K, 16)
    got = {}
    for cv in (0, 1):
        ip.setOption("cost_variant", cv)
        got[cv] = (ip.ditherPopulation(pals, 1.0), [ip.getIndices(p) for p in range(P)])
    for p in range(P):
        np.testing.assert_array_equal(got[0][1][p], got[1][1][p])
    print(f"fast {got[0][0]!r} generic {got[1][0]!r}")
    np.testing.assert_allclose(got[0][0], got[1][0], rtol=1e-6)


def test_ciede2000_cost_from_the_device_indices(gpu):
    """test_de2000_gpu.py's cost check, from the device's dithered indices: the float64 mean
    of de2000_ref over the float64 candidate S-CIELAB (a pixel within 0.5 degrees of the hue
    jump at the branch the device took) + 2 per unused colour, within 1e-5."""
    w, h, K = 97, 53, 16
    f = o.design_filters(72, 45.0)
    rgba = noise(w, h)
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    pals = pals_of(K, 16)
    m = new_ctx(gpu, DE00, pixel_err=1)
    try:
        m.setImage(rgba.reshape(-1), lab.reshape(-1), w, m.illum)
        costs, used = m.ditherPopulation(pals, 1.0, 2.0, return_used=True)
        plain = m.computeQuantizationErrorPopulation(pals, 2.0)
        costs2 = m.ditherPopulation(pals, 1.0, 2.0)
        ref64 = _cols(lab[:, :3].astype(np.float64))
        for p in range(P):
            pal = pals[p].reshape(K, 4)
            idx, err = m.getIndices(p).astype(np.int32), m.getPixelErrors(p)
            np.testing.assert_array_equal(used[p], np.bincount(idx, minlength=K)[:K] > 0)
            cand64 = _cols(exact_pixel_err(idx, pal, lab, f, w, h, lab_only=True))
            ex, other = d.ciede2000(*ref64, *cand64), d.ciede2000(*ref64, *cand64, other_branch=True)
            excl = np.abs(d.hue_gap_deg(*ref64, *cand64) - 180.0) < EXCL_DEG
            near_other = excl & (np.abs(err - other) < np.abs(err - ex))
            want = float(np.where(near_other, other, ex).mean()) + 2.0 * float(np.count_nonzero(used[p] == 0))
            print(f"p={p}: dithered {costs[p]!r}, float64 {want!r}, plain {plain[p]!r}")
            assert abs(costs[p] - want) <= 1e-5 * want
            assert costs2[p] == costs[p]
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 4. The point of the feature
# ---------------------------------------------------------------------------
def test_ramp_costs_less_dithered(ip):
    w = h = 64
    ip.setImage(ramp_image(w, h).reshape(-1), None, w, ip.illum)
    pal = cube_corners().reshape(1, -1)
    plain = ip.computeQuantizationErrorPopulation(pal, 2.0)[0]
    costs = {s: ip.ditherPopulation(pal, s, 2.0)[0] for s in (0.5, 1.0)}
    print(f"plain {plain!r}, dithered {costs!r}, ratio at 1: {costs[1.0] / plain:.3f}")
    assert costs[1.0] <= 0.6 * plain


def test_noise_image_changes_a_quarter_of_its_indices(ip):
    w, h, K = 97, 53, 16
    ip.setImage(noise(w, h).reshape(-1), None, w, ip.illum)
    pal = pals_of(K, 16, 1)
    ip.computeQuantizationErrorPopulation(pal, 2.0)
    plain = ip.getIndices(0)
    ip.ditherPopulation(pal, 1.0)
    changed = float(np.mean(ip.getIndices(0) != plain))
    print(f"{changed:.3f} of the indices change")
    assert changed >= 0.25


# ---------------------------------------------------------------------------
# 5. dither_rows does not matter
# ---------------------------------------------------------------------------
def test_dither_rows_does_not_matter(ip):
    w, h, K = 70, 150, 8
    ip.setOption("pixel_err", 1)
    ip.setImage(noise(w, h, w + h).reshape(-1), None, w, ip.illum)
    pals = pals_of(K, 3 * K + w)
    got = []
    for rows in (64, 128, 1024):
        ip.setOption("dither_rows", rows)
        got.append(_both(ip, pals, 1.0)[1])
    _assert_same(got[0], got[1], "64 against 128")
    _assert_same(got[0], got[2], "64 against 1024")
    lib = hq.load()
    for bad in (0, 63, 65, 96 + 1, 1088, -64):
        assert lib.hq_set_option(ip.ctx, b"dither_rows", bad) == _lib.HQ_ERR_ARG


# ---------------------------------------------------------------------------
# 6. State
# ---------------------------------------------------------------------------
def _sums_and_errors(m, Pn, K):
    lib = hq.load()
    sums, den = np.zeros((Pn, K, 4), np.int64), C.c_int64()
    err, worst = np.zeros((Pn, K, 4), np.int64), np.zeros((Pn, K, 4), np.float32)
    return (lib.hq_cluster_sums(m.ctx, Pn, K, _lib.i64ptr(sums), C.byref(den)),
            lib.hq_cluster_errors(m.ctx, Pn, K, _lib.i64ptr(err), _lib.fptr(worst)), sums, err)


def test_state_after_a_dithered_call(ip):
    w, h, K = 97, 53, 16
    ip.setOption("pixel_err", 1)
    ip.setImage(noise(w, h).reshape(-1), None, w, ip.illum)
    pals = pals_of(K, 16)
    before = _both(ip, pals, 1.0)
    assert [rc for rc in _sums_and_errors(ip, P, K)[:2]] == [_lib.HQ_ERR_STATE, _lib.HQ_ERR_STATE]
    plain = ip.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
    s1 = _sums_and_errors(ip, P, K)
    assert s1[:2] == (_lib.HQ_OK, _lib.HQ_OK)
    again = _both(ip, pals, 1.0)
    _assert_same(before[0], again[0], "the plain evaluation, before and after dithered calls")
    _assert_same(before[1], again[1], "two identical dithered calls")
    np.testing.assert_array_equal(plain[0], before[0][0])
    ip.computeQuantizationErrorPopulation(pals, 2.0)
    s2 = _sums_and_errors(ip, P, K)
    assert s2[:2] == (_lib.HQ_OK, _lib.HQ_OK)
    np.testing.assert_array_equal(s1[2], s2[2])
    np.testing.assert_array_equal(s1[3], s2[3])


def _search16(m, K):
    sw = hq.SWASA(population=P, imax=100, seed=9, t0=0.05)
    params, h = sw.params(), C.c_void_p()
    lib = hq.load()
    _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(h)), m.ctx)
    try:
        ran = C.c_int()
        _lib.check(lib.hq_search_run(h, 16, C.byref(ran)), m.ctx)
        best, err = np.zeros(4 * K, np.float32), C.c_double()
        _lib.check(lib.hq_search_best(h, _lib.fptr(best), C.byref(err), None), m.ctx)
        return ran.value, best, err.value
    finally:
        lib.hq_search_destroy(h)


def test_a_device_search_does_not_see_an_earlier_dithered_call(gpu):
    w, h, K = 97, 53, 16
    out = []
    for dithered_first in (False, True):
        m = new_ctx(gpu)
        try:
            m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
            if dithered_first:
                m.ditherPopulation(pals_of(K, 16), 1.0)
            out.append(_search16(m, K))
        finally:
            m.close()
    assert out[0][0] == out[1][0] == 16 and out[0][2] == out[1][2]
    np.testing.assert_array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


# ---------------------------------------------------------------------------
# 7. Refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_outputs_and_state_untouched(gpu):
    w, h, K = 64, 48, 8
    rgba = noise(w, h, 2)
    pals = pals_of(K, 1)
    m = new_ctx(gpu)
    try:
        def refused(status, pl=pals, s=1.0, **kw):
            rc, costs, used = raw_dither(m, pl, s, **kw)
            assert rc == status, (rc, hq.load().hq_last_error(m.ctx))
            assert np.all(costs == -7.0) and np.all(used == -7)

        refused(_lib.HQ_ERR_STATE)  # no image set
        m.setImage(rgba.reshape(-1), None, w, m.illum, row_begin=8, row_end=40)
        refused(_lib.HQ_ERR_STATE)  # a row-block shard
        m.setOption("pixel_err", 1)
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        plain = _both(m, pals, 1.0)[0]

        def state():
            return [m.getIndices(p) for p in range(P)] + [m.getPixelErrors(p) for p in range(P)]

        m.computeQuantizationErrorPopulation(pals, 2.0)
        held = state()
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            refused(_lib.HQ_ERR_UNSUPPORTED)
            m.setOption(name, 0 if name == "palette_split" else 1)
        refused(_lib.HQ_ERR_UNSUPPORTED, pals_of(257, 1))  # K > 256
        refused(_lib.HQ_ERR_ARG, Pn=0)
        refused(_lib.HQ_ERR_ARG, K=0)
        refused(_lib.HQ_ERR_ARG, None, Pn=P, K=K)
        assert raw_dither(m, pals, 1.0, costs_ptr=False)[0] == _lib.HQ_ERR_ARG
        for s in (-0.001, 1.001, float("nan"), float("inf")):
            refused(_lib.HQ_ERR_ARG, s=s)
        for ch, v in ((0, np.nan), (5, np.inf), (2, -0.001), (4 * K * 2 + 1, 1.001)):
            bad = pals.copy()
            bad.reshape(-1)[ch] = v
            refused(_lib.HQ_ERR_ARG, bad)
        ok = pals.copy()
        ok[:, 3::4] = np.nan  # (.w is not a channel)
        assert raw_dither(m, ok, 1.0)[0] == _lib.HQ_OK
        m.computeQuantizationErrorPopulation(pals, 2.0)
        for a, b in zip(held, state()):
            np.testing.assert_array_equal(a, b)
        # after all those refusals the evaluated state is the plain evaluation's still
        refused(_lib.HQ_ERR_ARG, s=2.0)
        for a, b in zip(held, state()):
            np.testing.assert_array_equal(a, b)
        assert _sums_and_errors(m, P, K)[:2] == (_lib.HQ_OK, _lib.HQ_OK)
        np.testing.assert_array_equal(m.computeQuantizationErrorPopulation(pals, 2.0), plain[0])
        # an image pixel outside [0, 1] or not finite: found on the device, once per image
        for v in (1.5, -0.25, np.nan):
            img = rgba.copy()
            img[w * 17 + 5, 1] = v
            m.setImage(img.reshape(-1), None, w, m.illum)
            refused(_lib.HQ_ERR_UNSUPPORTED)
            refused(_lib.HQ_ERR_UNSUPPORTED)  # (the remembered answer)
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        assert raw_dither(m, pals, 1.0)[0] == _lib.HQ_OK
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 8. Profile
# ---------------------------------------------------------------------------
def test_profile_counts_dither_launches_and_no_assign(ip):
    w, h, K = 97, 53, 16
    lib = hq.load()
    ip.setImage(noise(w, h).reshape(-1), None, w, ip.illum)
    pals = pals_of(K, 16)
    lib.hq_profile_enable(ip.ctx, 1)
    lib.hq_profile_reset(ip.ctx)

    def counts():
        got = {}
        for name in ("dither", "assign", "grid", "cost", "finalize"):
            ms, n = C.c_double(), C.c_int64()
            _lib.check(lib.hq_profile_get(ip.ctx, name.encode(), C.byref(ms), C.byref(n)), ip.ctx)
            got[name] = n.value
            assert (ms.value > 0) == (n.value > 0)
        return got

    ip.computeQuantizationErrorPopulation(pals, 2.0)
    assert counts() == {"dither": 0, "assign": 1, "grid": 1, "cost": 1, "finalize": 1}
    ip.ditherPopulation(pals, 1.0)
    ip.ditherPopulation(pals, 0.5)
    assert counts() == {"dither": 2, "assign": 1, "grid": 1, "cost": 3, "finalize": 3}


# ---------------------------------------------------------------------------
# 9. Python
# ---------------------------------------------------------------------------
def test_quantize_dithered_is_the_gathered_palette(ip):
    w, h, K = 97, 53, 16
    rgba = noise(w, h)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pal = pals_of(K, 16, 1)[0]
    pal[3::4] = 0.5  # (a .w the output must not carry)
    out = ip.quantizeDithered(pal, 1.0)
    idx = ip.getIndices(0)
    table = pal.reshape(K, 4).copy()
    table[:, 3] = 0.0
    np.testing.assert_array_equal(out.view(np.uint32), table[idx].reshape(-1).view(np.uint32))
    np.testing.assert_array_equal(ip.lastUsedColors, np.bincount(idx, minlength=K)[:K] > 0)
    assert ip.ditherError == ip.ditherPopulation(pal.reshape(1, -1), 1.0, 0.0)[0]
    # at strength 0 it is quantize's image
    np.testing.assert_array_equal(ip.quantizeDithered(pal, 0.0).reshape(-1, 4)[:, :3],
                                  ip.quantize(rgba.reshape(-1), table.reshape(-1)).reshape(-1, 4)[:, :3])


def _find(m, rgba, w, K, **kw):
    sw = hq.SWASA(population=2, imax=100, seed=4)
    best = m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum, iterations=10, **kw)
    return np.asarray(best, np.float32), sw


def test_find_best_quantization_with_dither(ip):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    plain, _ = _find(ip, rgba, w, K)
    plain_err = ip.bestError
    best, sw = _find(ip, rgba, w, K, dither=1.0)
    np.testing.assert_array_equal(best.view(np.uint32), plain.view(np.uint32))
    assert ip.bestError == plain_err
    assert ip.bestErrorDithered == ip.ditherPopulation(best.reshape(1, -1), 1.0, sw.delta)[0]


def test_dither_search_reports_the_dithered_cost_of_its_palette(ip):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    best, sw = _find(ip, rgba, w, K, dither=1.0, ditherSearch=True)
    assert ip.iterations == 10
    assert ip.bestError == ip.bestErrorDithered == ip.ditherPopulation(best.reshape(1, -1), 1.0, sw.delta)[0]
    seeded, _ = _find(ip, rgba, w, K, dither=1.0, ditherSearch=True, init="mediancut")
    assert ip.bestError == ip.ditherPopulation(seeded.reshape(1, -1), 1.0, sw.delta)[0]


def test_forbidden_combinations_raise(ip):
    w, K = 32, 4
    rgba = noise(w, 32, 7)
    with pytest.raises(ValueError):
        _find(ip, rgba, w, K, ditherSearch=True)  # needs dither > 0
    for kw in (dict(lloydEvery=2), dict(repairEvery=2), dict(lloydSteps=1), dict(repairSteps=1)):
        with pytest.raises(ValueError):
            _find(ip, rgba, w, K, dither=1.0, ditherSearch=True, **kw)
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            _find(ip, rgba, w, K, dither=bad)


def test_quantization_returns_the_dithered_image(gpu):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    image = np.stack([rgba[:, 0], rgba[:, 1], rgba[:, 2]])
    sw = hq.SWASA(population=2, imax=100, seed=4)
    q0, best0, err0 = hq.quantization(image, w, K, sw, device=gpu, iterations=10)
    q1, best1, err1 = hq.quantization(image, w, K, sw, device=gpu, iterations=10, dither=1.0)
    np.testing.assert_array_equal(best0, best1)
    assert err0 == err1
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        want = m.quantizeDithered(best1, 1.0).reshape(-1, 4)[:, :3].T
    finally:
        m.close()
    np.testing.assert_array_equal(q1, want)
    assert not np.array_equal(q0, q1)

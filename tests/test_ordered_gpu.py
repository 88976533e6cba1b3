"""GPU tests of ordered dithering (libhq's addition): hq_ordered_population[_partial],
hq_set_dither_map and hq_search_set_ordered through the C ABI and their Python surface.
Index images and used flags are checked bit for bit against the numpy restatement
(ordered_ref.py), costs within 1e-6 relative of the oracle's cost of those indices;
amplitude 0 is the plain evaluation bit for bit.
"""

import ctypes as C

import numpy as np
import pytest

import c_oracle
import de2000_ref as d
import hybridquantization_amd as hq
import oracle as o
import path_ref as pr
from dither_ref import cube_corners, ramp_image
from hybridquantization_amd import _lib
from ordered_ref import amp3, bayer, ordered
from test_de2000_gpu import EXCL_DEG, _cols
from test_dither_gpu import new_ctx, noise, pals_of
from test_fast_path import LONG, caller_filters, designed_half
from test_fast_path_gpu import _ctx as filter_ctx
from test_gpu import exact_pixel_err

pytestmark = pytest.mark.gpu

DE76, DE00 = hq.deltaETypes.CIE76, hq.deltaETypes.CIEDE2000
P = 3
W, H, K16 = 97, 53, 16
AMP = (0.3, 0.0, 0.7)  # channels not interchangeable


@pytest.fixture()
def ip(gpu):
    m = new_ctx(gpu)
    yield m
    m.close()


def raw_ordered(m, pals, amp, delta=2.0, Pn=None, K=None, costs_ptr=True, amp_ptr=True):
    """hq_ordered_population with sentinel outputs -> (status, costs, used)."""
    Pn = pals.shape[0] if Pn is None else Pn
    K = pals.shape[1] // 4 if K is None else K
    costs = np.full(max(Pn, 1), -7.0, np.float64)
    used = np.full((max(Pn, 1), max(K, 1)), -7, np.int32)
    a = np.ascontiguousarray(amp, np.float32)
    rc = hq.load().hq_ordered_population(m.ctx, _lib.fptr(pals) if pals is not None else None, Pn, K,
                                         _lib.fptr(a) if amp_ptr else None, delta,
                                         _lib.dptr(costs) if costs_ptr else None, _lib.iptr(used))
    return rc, costs, used


# ---------------------------------------------------------------------------
# 1. Indices, used flags and costs against the restatement
# ---------------------------------------------------------------------------
# name: (w, h, K, amp, filters, options).  Filters: None = the designed 72 / 45 set
# (half-width 10); "caller0" = a caller-supplied set of half-width 0.
CASES = {
    "97x53_k16": (W, H, K16, AMP, None, {}),               # odd width: a thread's pixels span rows
    "64x64_k256": (64, 64, 256, 0.2, None, {}),            # the full palette table
    "5x1": (5, 1, 6, 0.5, "caller0", {}),
    "1x5": (1, 5, 6, 0.5, "caller0", {}),
    "2x3": (2, 3, 6, 0.5, "caller0", {}),
    "97x53_blocks3": (W, H, K16, AMP, None, {"assign_blocks_per_cu": 3}),  # another step count per thread
}
_REF = {}
_IMG = {}


def _filters(key):
    return o.design_filters(72, 45.0) if key is None else caller_filters("asymmetric", 0)


def image_of(w, h, fkey=None):
    """(filters, rgba, oracle LabRef) of the noise image of that shape, made once."""
    if (w, h, fkey) not in _IMG:
        f = _filters(fkey)
        rgba = noise(w, h, seed=5 if (w, h) == (W, H) else w + h)
        lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
        _IMG[(w, h, fkey)] = (f, rgba, lab)
    return _IMG[(w, h, fkey)]


def oracle_cost(idx, used, pal, lab, f, w, h):
    err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
    return o.average_array(err) + o.compute_penalty(used, 2.0)


def ref_of(w, h, K, amp, fkey=None, tmap=None, n=P, seed=None, key=None):
    """Palettes and per palette the restatement's indices, used flags and the oracle's cost of
    them; computed once per key, read-only."""
    key = key or (w, h, K, tuple(amp3(amp)), fkey, n, seed)
    if key not in _REF:
        f, rgba, lab = image_of(w, h, fkey)
        pals = pals_of(K, (16 if (w, h) == (W, H) else 3 * K + w) if seed is None else seed, n)
        per = []
        for p in range(n):
            pal = pals[p].reshape(K, 4)
            idx, used = ordered(rgba, pal, w, h, amp, tmap)
            per.append(dict(idx=idx, used=used, cost=oracle_cost(idx, used, pal, lab, f, w, h)))
        _REF[key] = dict(f=f, rgba=rgba, lab=lab, pals=pals, per=per)
    return _REF[key]


def check_against(m, ref, amp, msg, cost=True):
    n = ref["pals"].shape[0]
    costs, used = m.orderedPopulation(ref["pals"], amp, 2.0, return_used=True)
    for p in range(n):
        r = ref["per"][p]
        np.testing.assert_array_equal(m.getIndices(p), r["idx"].astype(np.uint8), err_msg=f"{msg} p={p}")
        np.testing.assert_array_equal(used[p], r["used"], err_msg=f"{msg} p={p}")
        print(f"{msg} p={p}: cost {costs[p]!r}, oracle {r['cost']!r}, rel {abs(costs[p] - r['cost']) / r['cost']:.2e}")
        if cost:
            assert abs(costs[p] - r["cost"]) <= 1e-6 * abs(r["cost"]), f"{msg} p={p}"
    return costs, used


@pytest.mark.parametrize("name", list(CASES))
def test_indices_used_and_costs_against_the_restatement(gpu, name):
    """Both image forms (the packed bytes of a k/255 image and the planar floats) give the
    restatement's indices; P = 3 palettes in one call."""
    w, h, K, amp, fkey, opts = CASES[name]
    ref = ref_of(w, h, K, amp, fkey)
    got = []
    for img_u8 in (1, 0):
        m = filter_ctx(gpu, ref["f"], img_u8=img_u8, **opts)
        try:
            m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, m.illum)
            got.append(check_against(m, ref, amp, f"{name} img_u8={img_u8}"))
            np.testing.assert_array_equal(m.getIndices32(0), ref["per"][0]["idx"].astype(np.uint32))
        finally:
            m.close()
    np.testing.assert_array_equal(got[0][0], got[1][0])  # the same costs from both forms, bitwise
    if name == "97x53_k16":  # the dither does something here
        plain = o.assign(ref["rgba"], ref["pals"][0].reshape(K, 4))[0]
        assert np.mean(ref["per"][0]["idx"] != plain) > 0.05


@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_population_sizes(ip, n):
    """Every NG instance, and a full group of 4 plus a rest group."""
    ref = ref_of(W, H, K16, AMP, n=n)
    ip.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), W, ip.illum)
    check_against(ip, ref, AMP, f"P={n}")


def _maps():
    rng = np.random.default_rng(64)
    rnd = (rng.permutation(64 * 64).astype(np.float32).reshape(64, 64) + np.float32(0.5)) / np.float32(4096) - np.float32(0.5)
    return {
        "1x1": (W, H, np.full((1, 1), 0.5, np.float32)),
        "2x2": (W, H, bayer(1)),
        "4x32": (W, H, bayer(5)[:4, :].copy()),    # 4 rows of 32 values
        "32x4": (W, H, bayer(5)[:, :4].copy()),    # 32 rows of 4: rows and columns are not swapped
        "bayer64": (W, H, bayer(6)),
        "random64_on_40x30": (40, 30, rnd),        # an image smaller than the map, distinct values
    }


@pytest.mark.parametrize("name", list(_maps()))
def test_maps(ip, name):
    w, h, tmap = _maps()[name]
    amp = 0.6
    ref = ref_of(w, h, K16, amp, tmap=tmap, key=("map", name))
    ip.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), w, ip.illum)
    ip.setDitherMap(tmap)
    check_against(ip, ref, amp, f"map {name}")
    ip.setDitherMap(None)  # the default's results are back
    check_against(ip, ref_of(w, h, K16, amp, key=("map-default", w, h)), amp, f"default after {name}")


def test_set_dither_map_argument_checks(ip):
    lib = hq.load()
    ref = ref_of(W, H, K16, AMP)
    ip.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), W, ip.illum)
    ip.setDitherMap(bayer(1))
    want = ref_of(W, H, K16, AMP, tmap=bayer(1), key=("checks", "2x2"))
    ok = np.zeros(64 * 64, np.float32)
    for mw, mh in ((0, 2), (2, 0), (3, 2), (2, 6), (128, 2), (2, 128), (-2, 2)):
        assert lib.hq_set_dither_map(ip.ctx, _lib.fptr(ok), mw, mh) == _lib.HQ_ERR_ARG, (mw, mh)
    for v in (0.5001, -0.5001, np.nan, np.inf, -np.inf):
        bad = np.zeros(4, np.float32)
        bad[3] = v
        assert lib.hq_set_dither_map(ip.ctx, _lib.fptr(bad), 2, 2) == _lib.HQ_ERR_ARG, v
    check_against(ip, want, AMP, "the old map stays", cost=False)
    # it does not end the getters' answers
    held = ip.getIndices(1)
    ip.setDitherMap(bayer(3))
    np.testing.assert_array_equal(ip.getIndices(1), held)
    for edge in (0.5, -0.5):
        assert lib.hq_set_dither_map(ip.ctx, _lib.fptr(np.full(1, edge, np.float32)), 1, 1) == _lib.HQ_OK
    assert lib.hq_set_dither_map(None, None, 0, 0) == _lib.HQ_ERR_ARG


# ---------------------------------------------------------------------------
# 2. Options and image forms
# ---------------------------------------------------------------------------
def test_grid_resolutions_give_the_same_indices(ip):
    """grid 0 is the exhaustive branch of the same kernel."""
    ref = ref_of(W, H, K16, AMP)
    ip.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), W, ip.illum)
    for grid in (0, 16, 32, 64):
        ip.setOption("grid", grid)
        check_against(ip, ref, AMP, f"grid {grid}")


def test_a_planar_float_image(ip):
    """Pixels that are no k/255: no packed copy, the range check runs on the device."""
    w, h, K = 23, 17, 6
    rng = np.random.default_rng(23)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = rng.random((w * h, 3), np.float32)
    rgba[0, :3], rgba[1, :3] = 0.0, 1.0  # the ends of the range are inside it
    pals = pals_of(K, 61)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    _, used = ip.orderedPopulation(pals, AMP, 2.0, return_used=True)
    for p in range(P):
        want_idx, want_used = ordered(rgba, pals[p].reshape(K, 4), w, h, AMP)
        np.testing.assert_array_equal(ip.getIndices(p), want_idx.astype(np.uint8))
        np.testing.assert_array_equal(used[p], want_used)


def test_generic_cost_and_a_long_filter(gpu):
    """cost_variant 1 on the designed filters, and a half-width-51 set (the generic pair)."""
    ref = ref_of(W, H, K16, AMP)
    m = filter_ctx(gpu, ref["f"], cost_variant=1)
    try:
        m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), W, m.illum)
        check_against(m, ref, AMP, "cost_variant 1")
    finally:
        m.close()
    w = h = 64
    f = designed_half(LONG[2])
    rgba = noise(w, h)
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
    pals = pals_of(16, 16, 2)
    m = filter_ctx(gpu, f)
    try:
        m.setImage(rgba.reshape(-1), lab.reshape(-1), w, m.illum)
        costs, used = m.orderedPopulation(pals, 0.4, 2.0, return_used=True)
        for p in range(2):
            pal = pals[p].reshape(16, 4)
            idx, want_used = ordered(rgba, pal, w, h, 0.4)
            np.testing.assert_array_equal(m.getIndices(p), idx.astype(np.uint8))
            np.testing.assert_array_equal(used[p], want_used)
            want = oracle_cost(idx, want_used, pal, lab, f, w, h)
            print(f"half 51 p={p}: cost {costs[p]!r}, oracle {want!r}, rel {abs(costs[p] - want) / want:.2e}")
            assert abs(costs[p] - want) <= 1e-6 * want
    finally:
        m.close()


def test_ciede2000_cost_from_the_restatements_indices(gpu):
    """test_de2000_gpu.py's cost reference: the float64 mean of de2000_ref over the float64
    candidate S-CIELAB (a pixel within 0.5 degrees of the hue jump at the branch the device
    took) + 2 per unused colour -- the oracle of that dE type -- within 1e-6."""
    ref = ref_of(W, H, K16, AMP)
    f, lab = ref["f"], ref["lab"]
    m = new_ctx(gpu, DE00, pixel_err=1)
    try:
        m.setImage(ref["rgba"].reshape(-1), lab.reshape(-1), W, m.illum)
        costs, used = m.orderedPopulation(ref["pals"], AMP, 2.0, return_used=True)
        ref64 = _cols(lab[:, :3].astype(np.float64))
        for p in range(P):
            r, pal = ref["per"][p], ref["pals"][p].reshape(K16, 4)
            np.testing.assert_array_equal(m.getIndices(p), r["idx"].astype(np.uint8))
            np.testing.assert_array_equal(used[p], r["used"])
            err = m.getPixelErrors(p)
            cand64 = _cols(exact_pixel_err(r["idx"], pal, lab, f, W, H, lab_only=True))
            ex, other = d.ciede2000(*ref64, *cand64), d.ciede2000(*ref64, *cand64, other_branch=True)
            excl = np.abs(d.hue_gap_deg(*ref64, *cand64) - 180.0) < EXCL_DEG
            near_other = excl & (np.abs(err - other) < np.abs(err - ex))
            want = float(np.where(near_other, other, ex).mean()) + 2.0 * float(np.count_nonzero(r["used"] == 0))
            print(f"de2000 p={p}: ordered {costs[p]!r}, float64 {want!r}, rel {abs(costs[p] - want) / want:.2e}")
            assert abs(costs[p] - want) <= 1e-6 * want
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 3. Row-block shards
# ---------------------------------------------------------------------------
def test_shards_equal_the_whole_images_rows_and_add_up(gpu):
    """Rows [0, 20) and [20, 53) at half-width 10: the second shard's extended rows start at
    row 10, not at its first owned row."""
    ref = ref_of(W, H, K16, AMP)
    m = new_ctx(gpu)
    try:
        m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), W, m.illum)
        whole = m.orderedPopulationPartial(ref["pals"], AMP)
        parts = []
        for r0, r1 in ((0, 20), (20, H)):
            m.setImage(ref["rgba"].reshape(-1), ref["lab"].reshape(-1), W, m.illum, row_begin=r0, row_end=r1)
            parts.append(m.orderedPopulationPartial(ref["pals"], AMP))
            for p in range(P):
                got = m.getIndices(p)[:(r1 - r0) * W]  # (the owned rows come first in the full-size buffer)
                np.testing.assert_array_equal(got, ref["per"][p]["idx"][r0 * W:r1 * W].astype(np.uint8))
            # the non-partial form needs a communicator on a shard
            assert raw_ordered(m, ref["pals"], AMP)[0] == _lib.HQ_ERR_STATE
        for p in range(P):
            np.testing.assert_array_equal(whole[p, 1:] != 0, ref["per"][p]["used"] != 0)
            np.testing.assert_array_equal((parts[0][p, 1:] != 0) | (parts[1][p, 1:] != 0), whole[p, 1:] != 0)
            s = parts[0][p, 0] + parts[1][p, 0]
            print(f"p={p}: shards {s!r}, whole {whole[p, 0]!r}")
            assert abs(s - whole[p, 0]) <= 1e-6 * whole[p, 0]
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 4. Amplitude 0, the ramp, state
# ---------------------------------------------------------------------------
def _both(m, pals, amp):
    out = []
    for call in (lambda: m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True),
                 lambda: m.orderedPopulation(pals, amp, 2.0, return_used=True)):
        costs, used = call()
        n = pals.shape[0]
        out.append((costs, used, [m.getIndices(p) for p in range(n)], [m.getPixelErrors(p) for p in range(n)]))
    return out


def _assert_same(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)  # costs, bitwise (no NaN here)
    np.testing.assert_array_equal(a[1], b[1], err_msg=msg)
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        np.testing.assert_array_equal(x, y, err_msg=msg)


@pytest.mark.parametrize("img_u8", [1, 0])
@pytest.mark.parametrize("de", [DE76, DE00], ids=["de76", "de2000"])
def test_amplitude_zero_is_the_plain_evaluation(gpu, de, img_u8):
    m = new_ctx(gpu, de, pixel_err=1, img_u8=img_u8)
    try:
        m.setImage(noise(W, H).reshape(-1), None, W, m.illum)
        plain, ordr = _both(m, pals_of(K16, 16), 0.0)
        assert np.isfinite(plain[0]).all()
        _assert_same(plain, ordr, f"de {de} img_u8 {img_u8}")
    finally:
        m.close()


def test_ramp_costs_less_ordered(ip):
    w = h = 64
    ip.setImage(ramp_image(w, h).reshape(-1), None, w, ip.illum)
    pal = cube_corners().reshape(1, -1)
    plain = ip.computeQuantizationErrorPopulation(pal, 2.0)[0]
    cost = ip.orderedPopulation(pal, 1.0, 2.0)[0]
    print(f"plain {plain!r}, ordered {cost!r}, ratio {cost / plain:.3f}")
    assert cost <= 0.6 * plain


def _sums_and_errors(m, Pn, K):
    lib = hq.load()
    sums, den = np.zeros((Pn, K, 4), np.int64), C.c_int64()
    err, worst = np.zeros((Pn, K, 4), np.int64), np.zeros((Pn, K, 4), np.float32)
    return (lib.hq_cluster_sums(m.ctx, Pn, K, _lib.i64ptr(sums), C.byref(den)),
            lib.hq_cluster_errors(m.ctx, Pn, K, _lib.i64ptr(err), _lib.fptr(worst)))


def test_state_after_an_ordered_call(gpu):
    pals = pals_of(K16, 16)
    rgba = noise(W, H)
    fresh = new_ctx(gpu, pixel_err=1)
    m = new_ctx(gpu, pixel_err=1)
    try:
        for c in (fresh, m):
            c.setImage(rgba.reshape(-1), None, W, c.illum)
        want = _both(fresh, pals, 0.0)[0]
        m.orderedPopulation(pals, AMP)
        assert _sums_and_errors(m, P, K16) == (_lib.HQ_ERR_STATE, _lib.HQ_ERR_STATE)
        got = _both(m, pals, AMP)
        _assert_same(want, got[0], "a plain evaluation after an ordered one against a fresh context's")
        assert _sums_and_errors(m, P, K16) == (_lib.HQ_ERR_STATE, _lib.HQ_ERR_STATE)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        assert _sums_and_errors(m, P, K16) == (_lib.HQ_OK, _lib.HQ_OK)
        again = _both(m, pals, AMP)
        _assert_same(got[1], again[1], "two identical ordered calls")
        assert not np.array_equal(got[1][2][0], got[0][2][0])
    finally:
        fresh.close()
        m.close()


# ---------------------------------------------------------------------------
# 5. Refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_outputs_and_state_untouched(gpu):
    w, h, K = 64, 48, 8
    rgba = noise(w, h, 2)
    pals = pals_of(K, 1)
    m = new_ctx(gpu)
    try:
        def refused(status, pl=pals, amp=AMP, **kw):
            rc, costs, used = raw_ordered(m, pl, amp, **kw)
            assert rc == status, (rc, hq.load().hq_last_error(m.ctx))
            assert np.all(costs == -7.0) and np.all(used == -7)

        refused(_lib.HQ_ERR_STATE)  # no image set
        m.setOption("pixel_err", 1)
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        m.computeQuantizationErrorPopulation(pals, 2.0)

        def state():
            return [m.getIndices(p) for p in range(P)] + [m.getPixelErrors(p) for p in range(P)]

        held = state()
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            refused(_lib.HQ_ERR_UNSUPPORTED)
            m.setOption(name, 0 if name == "palette_split" else 1)
        refused(_lib.HQ_ERR_UNSUPPORTED, pals_of(257, 1))  # K > 256
        refused(_lib.HQ_ERR_ARG, Pn=0)
        refused(_lib.HQ_ERR_ARG, K=0)
        refused(_lib.HQ_ERR_ARG, None, Pn=P, K=K)
        refused(_lib.HQ_ERR_ARG, amp_ptr=False)
        assert raw_ordered(m, pals, AMP, costs_ptr=False)[0] == _lib.HQ_ERR_ARG
        for ch in range(3):
            for v in (-0.001, 1.001, float("nan"), float("inf")):
                a = [0.5, 0.5, 0.5]
                a[ch] = v
                refused(_lib.HQ_ERR_ARG, amp=a)
        for ch, v in ((0, np.nan), (5, np.inf), (2, -0.001), (4 * K * 2 + 1, 1.001)):
            bad = pals.copy()
            bad.reshape(-1)[ch] = v
            refused(_lib.HQ_ERR_ARG, bad)
        for a, b in zip(held, state()):  # the getters still answer for the evaluation before
            np.testing.assert_array_equal(a, b)
        assert _sums_and_errors(m, P, K) == (_lib.HQ_OK, _lib.HQ_OK)
        ok = pals.copy()
        ok[:, 3::4] = np.nan  # (.w is not a channel)
        assert raw_ordered(m, ok, AMP)[0] == _lib.HQ_OK
        assert raw_ordered(m, pals, (1.0, 0.0, 1.0))[0] == _lib.HQ_OK  # the ends of the range
        # an image pixel outside [0, 1] or not finite: the range flag, once per image
        for v in (1.5, -0.25, np.nan):
            img = rgba.copy()
            img[w * 17 + 5, 1] = v
            m.setImage(img.reshape(-1), None, w, m.illum)
            refused(_lib.HQ_ERR_UNSUPPORTED)
            refused(_lib.HQ_ERR_UNSUPPORTED)  # (the remembered answer)
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        assert raw_ordered(m, pals, AMP)[0] == _lib.HQ_OK
    finally:
        m.close()


def test_profile_counts_under_grid_and_assign(ip):
    lib = hq.load()
    ip.setImage(noise(W, H).reshape(-1), None, W, ip.illum)
    pals = pals_of(K16, 16, 5)  # a full group and a rest group: one timed assign all the same
    lib.hq_profile_enable(ip.ctx, 1)
    lib.hq_profile_reset(ip.ctx)
    ip.orderedPopulation(pals, AMP)
    ip.orderedPopulation(pals, 0.5)
    got = {}
    for name in ("dither", "assign", "grid", "cost", "finalize"):
        ms, n = C.c_double(), C.c_int64()
        _lib.check(lib.hq_profile_get(ip.ctx, name.encode(), C.byref(ms), C.byref(n)), ip.ctx)
        got[name] = n.value
        assert (ms.value > 0) == (n.value > 0)
    assert got == {"dither": 0, "assign": 2, "grid": 2, "cost": 2, "finalize": 2}


# ---------------------------------------------------------------------------
# 6. The search under the ordered cost
# ---------------------------------------------------------------------------
SW, SH, SK, SAMP = 48, 40, 8, (0.5, 0.5, 0.5)


def _search(gpu, Pn, amp, runs=(30,), before=True, opts=None, probe=None):
    """A search on the 48 x 40 noise image: hq_search_set_ordered(amp) (None: not called; "null":
    a NULL pointer) before the first run, then the runs -> (best colours, best error, iteration)."""
    lib = hq.load()
    m = new_ctx(gpu, **(opts or {}))
    try:
        m.setImage(noise(SW, SH, 11).reshape(-1), None, SW, m.illum)
        sw = hq.SWASA(population=Pn, imax=100, seed=9, t0=0.05)
        params, h = sw.params(), C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), SK, sw.seed, C.byref(h)), m.ctx)
        pr.check_search(m, h, Pn, SK)  # device-resident exactly when sa_device is 1
        try:
            if amp is not None and before:
                a = None if isinstance(amp, str) else _lib.fptr(np.ascontiguousarray(amp, np.float32))
                _lib.check(lib.hq_search_set_ordered(h, a), m.ctx)
            for n in runs:
                ran = C.c_int()
                _lib.check(lib.hq_search_run(h, n, C.byref(ran)), m.ctx)
                assert ran.value == n
            pr.check_search(m, h, Pn, SK, ran=True)  # ... and captured exactly when sa_graph is 1
            best, err, it = np.zeros(4 * SK, np.float32), C.c_double(), C.c_int()
            _lib.check(lib.hq_search_best(h, _lib.fptr(best), C.byref(err), C.byref(it)), m.ctx)
            if probe:
                probe(m, h, best, err.value)
            return best, err.value, it.value
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()


def _same_search(a, b, msg):
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32), err_msg=msg)
    assert a[1] == b[1] and a[2] == b[2], (msg, a[1:], b[1:])


@pytest.mark.parametrize("Pn", [3, 5])
def test_search_forms_agree_and_runs_compose(gpu, Pn):
    def reproduces(m, h, best, err):
        cost = m.orderedPopulation(best.reshape(1, -1), SAMP, 2.0)[0]
        print(f"P={Pn}: best_error {err!r}, hq_ordered_population of the best colours {cost!r}")
        assert abs(cost - err) <= 1e-6 * err

    dev = _search(gpu, Pn, SAMP, probe=reproduces)
    assert dev[2] == 30
    _same_search(dev, _search(gpu, Pn, SAMP, opts={"sa_graph": 1}), "sa_graph 1")
    _same_search(dev, _search(gpu, Pn, SAMP, opts={"sa_device": 0}), "host-driven")
    _same_search(dev, _search(gpu, Pn, SAMP, runs=(10, 20)), "10 + 20 iterations")
    plain = _search(gpu, Pn, None)
    assert not np.array_equal(plain[0], dev[0]) and plain[1] != dev[1]  # another objective, another search
    _same_search(plain, _search(gpu, Pn, (0.0, 0.0, 0.0)), "zeros")
    _same_search(plain, _search(gpu, Pn, "null"), "NULL")
    _same_search(plain, _search(gpu, Pn, "null", opts={"sa_device": 0}), "NULL, host-driven")


@pytest.mark.parametrize("sa_device", [1, 0])
def test_search_refusals(gpu, sa_device):
    lib = hq.load()
    amp = np.asarray(SAMP, np.float32)

    def lloyd_repair_then_ordered(m, h, best, err):
        for setter in (lambda e: lib.hq_search_set_lloyd(h, e), lambda e: lib.hq_search_set_repair(h, e, -1)):
            assert setter(2) == _lib.HQ_OK
            assert lib.hq_search_set_ordered(h, _lib.fptr(amp)) == _lib.HQ_ERR_UNSUPPORTED
            assert lib.hq_search_set_ordered(h, None) == _lib.HQ_OK  # (zeros: nothing to refuse)
            assert setter(0) == _lib.HQ_OK
        assert lib.hq_search_set_ordered(h, _lib.fptr(amp)) == _lib.HQ_OK
        # the other order: once it is on, a period is refused (0 is no period)
        assert lib.hq_search_set_lloyd(h, 2) == _lib.HQ_ERR_UNSUPPORTED
        assert lib.hq_search_set_repair(h, 2, -1) == _lib.HQ_ERR_UNSUPPORTED
        assert lib.hq_search_set_lloyd(h, 0) == _lib.HQ_OK and lib.hq_search_set_repair(h, 0, -1) == _lib.HQ_OK
        for bad in ((-0.1, 0, 0), (0, 1.5, 0), (0, 0, np.nan)):
            assert lib.hq_search_set_ordered(h, _lib.fptr(np.asarray(bad, np.float32))) == _lib.HQ_ERR_ARG
        assert lib.hq_search_set_ordered(None, _lib.fptr(amp)) == _lib.HQ_ERR_ARG
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            assert lib.hq_search_set_ordered(h, _lib.fptr(np.asarray((0.25, 0.25, 0.25), np.float32))) == _lib.HQ_ERR_UNSUPPORTED
            m.setOption(name, 0 if name == "palette_split" else 1)
        ran = C.c_int()
        assert lib.hq_search_run(h, 2, C.byref(ran)) == _lib.HQ_OK and ran.value == 2

    _search(gpu, 3, None, runs=(2,), opts={"sa_device": sa_device}, probe=lloyd_repair_then_ordered)


def test_search_refuses_more_than_256_colours(gpu):
    lib = hq.load()
    m = new_ctx(gpu, sa_device=0)
    try:
        m.setImage(noise(SW, SH, 11).reshape(-1), None, SW, m.illum)
        sw = hq.SWASA(population=2, imax=100, seed=9)
        params, h = sw.params(), C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), 257, sw.seed, C.byref(h)), m.ctx)
        try:
            assert lib.hq_search_set_ordered(h, _lib.fptr(np.asarray(SAMP, np.float32))) == _lib.HQ_ERR_UNSUPPORTED
            assert lib.hq_search_set_ordered(h, None) == _lib.HQ_OK
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 7. Python
# ---------------------------------------------------------------------------
def test_quantize_ordered_is_the_gathered_palette(ip):
    rgba = noise(W, H)
    ip.setImage(rgba.reshape(-1), None, W, ip.illum)
    pal = pals_of(K16, 16, 1)[0]
    pal[3::4] = 0.5  # (a .w the output must not carry)
    out = ip.quantizeOrdered(pal, AMP)
    idx = ip.getIndices(0)
    table = pal.reshape(K16, 4).copy()
    table[:, 3] = 0.0
    np.testing.assert_array_equal(out.view(np.uint32), table[idx].reshape(-1).view(np.uint32))
    np.testing.assert_array_equal(ip.lastUsedColors, np.bincount(idx, minlength=K16)[:K16] > 0)
    assert ip.orderedError == ip.orderedPopulation(pal.reshape(1, -1), AMP, 0.0)[0]
    np.testing.assert_array_equal(ip.quantizeOrdered(pal, 0.0).reshape(-1, 4)[:, :3],
                                  ip.quantize(rgba.reshape(-1), table.reshape(-1)).reshape(-1, 4)[:, :3])


def _find(m, rgba, w, K, **kw):
    sw = hq.SWASA(population=2, imax=100, seed=4)
    best = m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum, iterations=10, **kw)
    return np.asarray(best, np.float32), sw


def test_find_best_quantization_with_ordered(ip):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    plain, _ = _find(ip, rgba, w, K)
    plain_err = ip.bestError
    best, sw = _find(ip, rgba, w, K, ordered=0.5)
    np.testing.assert_array_equal(best.view(np.uint32), plain.view(np.uint32))
    assert ip.bestError == plain_err
    assert ip.bestErrorOrdered == ip.orderedPopulation(best.reshape(1, -1), 0.5, sw.delta)[0]
    found, sw = _find(ip, rgba, w, K, ordered=(0.5, 0.4, 0.3), orderedSearch=True)
    assert ip.iterations == 10
    cost = ip.orderedPopulation(found.reshape(1, -1), (0.5, 0.4, 0.3), sw.delta)[0]
    assert ip.bestError == ip.bestErrorOrdered and abs(cost - ip.bestError) <= 1e-6 * cost
    with pytest.raises(ValueError):
        _find(ip, rgba, w, K, orderedSearch=True)
    with pytest.raises(ValueError):
        _find(ip, rgba, w, K, ordered=0.5, orderedSearch=True, lloydSteps=1)
    with pytest.raises(_lib.HQError):
        _find(ip, rgba, w, K, ordered=0.5, orderedSearch=True, lloydEvery=2)


def test_quantization_returns_the_ordered_image(gpu):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    image = np.stack([rgba[:, 0], rgba[:, 1], rgba[:, 2]])
    sw = hq.SWASA(population=2, imax=100, seed=4)
    q0, best0, err0 = hq.quantization(image, w, K, sw, device=gpu, iterations=10)
    q1, best1, err1 = hq.quantization(image, w, K, sw, device=gpu, iterations=10, ordered=0.5)
    np.testing.assert_array_equal(best0, best1)
    assert err0 == err1
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        want = m.quantizeOrdered(best1, 0.5).reshape(-1, 4)[:, :3].T
    finally:
        m.close()
    np.testing.assert_array_equal(q1, want)
    assert not np.array_equal(q0, q1)

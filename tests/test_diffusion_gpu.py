"""GPU tests of error diffusion under other kernels than Floyd-Steinberg's (libhq's addition):
hq_diffuse_population through the C ABI and its Python surface.  The index images and used flags
are checked bit for bit against the numpy restatement (diffusion_ref.py; the Floyd-Steinberg tap
set runs hq_dither_population's kernel instance and formula, so dither_ref.py restates it), the costs
against the oracle's cost of those indices at tests/test_gpu.py's 1e-5.
"""

import ctypes as C

import numpy as np
import pytest

import c_oracle
import hybridquantization_amd as hq
import oracle as o
from diffusion_ref import POSITIONS, PRESET_CLASS, PRESETS, classify, diffuse, preset, single_tap
from dither_ref import cube_corners, dither, ramp_image
from hybridquantization_amd import _lib
from mask_ref import inside, masked_sum, masks_for
from test_diffusion import TWELVE, c_taps
from test_dither_gpu import _search16, _sums_and_errors, new_ctx, noise, pals_of
from test_fast_path import caller_filters
from test_fast_path_gpu import _ctx as filter_ctx
from weights_ref import weight_maps, weight_sum, weighted_sum

pytestmark = pytest.mark.gpu

DE76, DE00 = hq.deltaETypes.CIE76, hq.deltaETypes.CIEDE2000
P = 2
STRENGTHS = (1.0, 0.37)
FS = preset("floyd_steinberg")
# one tap set per kernel instance (R, S), none of them a preset
INSTANCES = {
    (1, 2): (np.array([[0, 0, 0, 3, 1], [0, 2, 4, 1, 1], [0, 0, 0, 0, 0]]), 13),
    (1, 3): (np.array([[0, 0, 0, 3, 1], [2, 0, 4, 1, 1], [0, 0, 0, 0, 0]]), 12),
    (2, 2): (np.array([[0, 0, 0, 3, 1], [0, 2, 4, 1, 1], [1, 0, 2, 0, 1]]), 16),
    (2, 3): (np.array([[0, 0, 0, 3, 1], [1, 2, 4, 1, 1], [2, 1, 2, 0, 1]]), 20),
}


def taps_of(kernel):
    return preset(kernel) if isinstance(kernel, str) else kernel


def is_fs(kernel):
    w, div = taps_of(kernel)
    return div == FS[1] and np.array_equal(w, FS[0])


def restate(rgba, pal, w, h, s, kernel):
    """The restatement's (idx, used) of one palette under `kernel` (a preset's name or (w, div))."""
    if is_fs(kernel):
        return dither(rgba, pal, w, h, s)
    return diffuse(rgba, pal, w, h, s, *taps_of(kernel))


@pytest.fixture()
def ip(gpu):
    m = new_ctx(gpu)
    yield m
    m.close()


def raw_diffuse(m, pals, taps, strength=1.0, delta=2.0, Pn=None, K=None, costs_ptr=True):
    """hq_diffuse_population with sentinel outputs -> (status, costs, used); taps: (w, div) or None."""
    Pn = pals.shape[0] if Pn is None else Pn
    K = pals.shape[1] // 4 if K is None else K
    costs = np.full(max(Pn, 1), -7.0, np.float64)
    used = np.full((max(Pn, 1), max(K, 1)), -7, np.int32)
    t = None if taps is None else C.byref(c_taps(*taps))
    rc = hq.load().hq_diffuse_population(m.ctx, _lib.fptr(pals) if pals is not None else None, Pn, K, t, strength,
                                         delta, _lib.dptr(costs) if costs_ptr else None, _lib.iptr(used))
    return rc, costs, used


# ---------------------------------------------------------------------------
# 1. Indices, used flags and costs against the restatement
# ---------------------------------------------------------------------------
_IMG = {}


def image_of(w, h, fkey):
    """Image, filters and oracle LabRef of a shape; computed once, read-only."""
    if (w, h, fkey) not in _IMG:
        f = caller_filters("asymmetric", 0) if fkey == "caller0" else o.design_filters(72, 45.0)
        rgba = noise(w, h, w + h)
        lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)
        _IMG[(w, h, fkey)] = (f, rgba, lab)
    return _IMG[(w, h, fkey)]


def check_shape(gpu, w, h, K, kernels, fkey=None, img_u8s=(1,), strengths=STRENGTHS, **opts):
    """Every kernel of `kernels` (name -> preset name or (w, div)) at every strength on a w x h noise
    image under P palettes of K colours: indices and used flags are the restatement's bits, the
    cost the oracle's of those indices within 1e-5."""
    f, rgba, lab = image_of(w, h, fkey)
    pals = pals_of(K, 3 * K + w, P)
    want = {}
    for name, kernel in kernels.items():
        for s in strengths:
            per = []
            for p in range(P):
                pal = pals[p].reshape(K, 4)
                idx, used = restate(rgba, pal, w, h, s, kernel)
                err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
                per.append((idx.astype(np.uint8), used, o.average_array(err) + o.compute_penalty(used, 2.0)))
            want[(name, s)] = per
    for img_u8 in img_u8s:
        m = filter_ctx(gpu, f, img_u8=img_u8, **opts)
        try:
            m.setImage(rgba.reshape(-1), lab.reshape(-1), w, m.illum)
            for (name, s), per in want.items():
                costs, used = m.ditherPopulation(pals, s, 2.0, return_used=True, kernel=kernels[name])
                path = m.lastPath()
                R, S = classify(taps_of(kernels[name])[0])
                assert (path["argmin"], path["diffuse_rows"], path["diffuse_slope"]) == \
                    (("dither", 0, 0) if is_fs(kernels[name]) else ("diffuse", R, S))
                for p in range(P):
                    msg = f"{w}x{h} K={K} {name} s={s} img_u8={img_u8} p={p}"
                    np.testing.assert_array_equal(m.getIndices(p), per[p][0], err_msg=msg)
                    np.testing.assert_array_equal(used[p], per[p][1], err_msg=msg)
                    print(f"{msg}: cost {costs[p]!r}, oracle {per[p][2]!r}")
                    assert abs(costs[p] - per[p][2]) <= 1e-5 * abs(per[p][2]), msg
        finally:
            m.close()


NAMED = {n: n for n in PRESETS}


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (2, 5), (3, 4)])
def test_shapes_narrower_or_shorter_than_the_tap_window(gpu, w, h):
    check_shape(gpu, w, h, 6, NAMED, fkey="caller0")


def test_width_not_a_multiple_of_four(gpu):
    check_shape(gpu, 97, 53, 64, NAMED)


def test_vector_path(gpu):
    check_shape(gpu, 64, 48, 16, NAMED)


@pytest.mark.parametrize("K", [1, 256])
def test_palette_size_extremes(gpu, K):
    check_shape(gpu, 32, 20, K, NAMED)


def test_both_pixel_forms(gpu):
    """The packed bytes of a k/255 image or not: the kernel reads the planar floats either way."""
    check_shape(gpu, 33, 21, 16, {n: n for n in ("jarvis", "atkinson", "burkes", "sierra_lite")}, img_u8s=(1, 0))


def test_a_planar_float_image(ip):
    """Pixels that are no k/255: no packed copy, the range check runs on the device."""
    w, h, K = 23, 17, 6
    rng = np.random.default_rng(23)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = rng.random((w * h, 3), np.float32)
    rgba[0, :3], rgba[1, :3] = 0.0, 1.0
    pals = pals_of(K, 61, P)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    for name in PRESETS:
        for s in STRENGTHS:
            _, used = ip.ditherPopulation(pals, s, 2.0, return_used=True, kernel=name)
            for p in range(P):
                want_idx, want_used = restate(rgba, pals[p].reshape(K, 4), w, h, s, name)
                np.testing.assert_array_equal(ip.getIndices(p), want_idx.astype(np.uint8), err_msg=f"{name} {s}")
                np.testing.assert_array_equal(used[p], want_used)


# strips of 64 rows: three with the last partial; a second strip of one row (both of its upper rows
# from the carry); of two rows (one from the carry, one from the ring); strips of 64, 64 and 1 rows;
# and images narrower than the tap window across a strip (filters of half-width 0): the carry rows
# have no column 1, or no column 2, for the pre-load and the first steps to read
@pytest.mark.parametrize("w,h", [(70, 150), (40, 65), (40, 66), (40, 129), (1, 130), (2, 129), (3, 66)])
def test_strips(gpu, w, h):
    check_shape(gpu, w, h, 8, NAMED, fkey="caller0" if w < 4 else None, dither_rows=64)


def both(m, pals, s, kernel):
    """(costs, used, indices, per-pixel dE) of the rendering under `kernel` ("plain": the plain
    evaluation, None: hq_dither_population)."""
    if kernel == "plain":
        costs, used = m.computeQuantizationErrorPopulation(pals, 2.0, return_used=True)
    else:
        costs, used = m.ditherPopulation(pals, s, 2.0, return_used=True, kernel=kernel)
    n = pals.shape[0]
    return costs, used, [m.getIndices(p) for p in range(n)], [m.getPixelErrors(p) for p in range(n)]


def assert_same(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)  # costs, bitwise (no NaN here)
    np.testing.assert_array_equal(a[1], b[1], err_msg=msg)
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        np.testing.assert_array_equal(x, y, err_msg=msg)


def test_strip_height_does_not_change_results(ip):
    """1024 is clamped to 512 in the instances of slope 3."""
    w, h, K = 70, 150, 8
    ip.setOption("pixel_err", 1)
    ip.setImage(noise(w, h, w + h).reshape(-1), None, w, ip.illum)
    pals = pals_of(K, 3 * K + w, P)
    for name in PRESETS:
        got = []
        for rows in (64, 128, 1024):
            ip.setOption("dither_rows", rows)
            got.append(both(ip, pals, 1.0, name))
        assert_same(got[0], got[1], f"{name}: 64 against 128")
        assert_same(got[0], got[2], f"{name}: 64 against 1024")


# ---------------------------------------------------------------------------
# 2. Tap sets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,rows", [(23, 17, 1024), (40, 66, 64)])
def test_each_legal_tap_position_alone(gpu, w, h, rows):
    check_shape(gpu, w, h, 8, {f"dy{dy}dx{dx}": single_tap(dy, dx) for dy, dx in POSITIONS}, dither_rows=rows)


def test_twelve_distinct_weights(gpu):
    assert len(set(TWELVE[0][TWELVE[0] > 0])) == 12 and TWELVE[1] == int(TWELVE[0].sum()) + 3
    check_shape(gpu, 40, 66, 8, {"twelve": TWELVE}, dither_rows=64)
    check_shape(gpu, 97, 53, 64, {"twelve": TWELVE})


@pytest.mark.parametrize("RS", list(INSTANCES))
def test_each_kernel_instance(gpu, RS):
    """check_shape asserts lastPath()'s argmin, diffuse_rows and diffuse_slope for every call."""
    assert classify(INSTANCES[RS][0]) == RS
    check_shape(gpu, 40, 66, 8, {str(RS): INSTANCES[RS]}, dither_rows=64)
    m = new_ctx(gpu)
    try:
        m.setImage(noise(40, 66).reshape(-1), None, 40, m.illum)
        pals = pals_of(8, 5, P)
        m.ditherPopulation(pals, 1.0, kernel=INSTANCES[RS])
        path = m.lastPath()
        assert (path["pass"], path["argmin"], path["diffuse_rows"], path["diffuse_slope"]) == ("dither", "diffuse") + RS
        assert (path["pixels"], path["grid"], path["idx_bytes"]) == ("planar", "none", 1)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        path = m.lastPath()
        assert (path["argmin"], path["diffuse_rows"], path["diffuse_slope"], path["previous_pass"]) == \
            ("assign_pipe", 0, 0, "dither")
    finally:
        m.close()


def test_floyd_steinberg_taps_are_hq_dither_population(ip):
    w, h, K = 70, 150, 8
    ip.setOption("pixel_err", 1)
    ip.setOption("dither_rows", 64)
    ip.setImage(noise(w, h, w + h).reshape(-1), None, w, ip.illum)
    pals = pals_of(K, 3 * K + w, P)
    for s in STRENGTHS:
        a = both(ip, pals, s, None)
        assert ip.lastPath()["argmin"] == "dither"
        for kernel in ("floyd_steinberg", FS):
            b = both(ip, pals, s, kernel)
            path = ip.lastPath()
            assert (path["pass"], path["argmin"], path["diffuse_rows"], path["diffuse_slope"]) == ("dither", "dither", 0, 0)
            assert_same(a, b, f"s={s}")
    # the same weights over another div are another kernel
    ip.ditherPopulation(pals, 1.0, kernel=(FS[0], 17))
    assert ip.lastPath()["argmin"] == "diffuse"


# ---------------------------------------------------------------------------
# 3. Identities and state
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("de", [DE76, DE00], ids=["de76", "de2000"])
def test_strength_zero_is_the_plain_evaluation(gpu, de):
    w, h, K = 97, 53, 16
    m = new_ctx(gpu, de, pixel_err=1)
    try:
        m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
        pals = pals_of(K, 16, P)
        plain = both(m, pals, 0.0, "plain")
        assert np.isfinite(plain[0]).all()
        for kernel in list(PRESETS) + list(INSTANCES.values()):
            assert_same(plain, both(m, pals, 0.0, kernel), f"de {de} {kernel}")
    finally:
        m.close()


def test_cost_under_a_mask_and_under_weights(gpu):
    """The device's indices are the restatement's, mask or weights or not (they touch the cost
    alone); the cost is the oracle's per-pixel dE of those indices, averaged over the mask or by
    the weights, + 2 per unused colour, within 2e-4: a masked or weighted mean cannot be further
    from the oracle's than the worst pixel is (test_mask_gpu.py's bar)."""
    w, h, K = 97, 53, 16
    f, rgba, lab = image_of(w, h, None)
    pals = pals_of(K, 16, P)
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), lab.reshape(-1), w, m.illum)
        for name in ("stucki", "atkinson", "sierra2", "sierra_lite"):
            errs = []
            for p in range(P):
                pal = pals[p].reshape(K, 4)
                idx, used = restate(rgba, pal, w, h, 0.75, name)
                errs.append((idx, used, o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))))
            covers = [("mask", masks_for(w, h)["bernoulli"]), ("weights", weight_maps(w, h)["noise"])]
            for kind, cover in covers:
                if kind == "weights":
                    m.setWeights(cover)
                else:
                    m.setMask(cover)
                costs, used = m.ditherPopulation(pals, 0.75, 2.0, return_used=True, kernel=name)
                assert m.lastPath()["cost_instance"] == ("masked" if kind == "mask" else "weighted")
                for p in range(P):
                    idx, want_used, err = errs[p]
                    np.testing.assert_array_equal(m.getIndices(p), idx.astype(np.uint8))
                    np.testing.assert_array_equal(used[p], want_used)
                    mean = (masked_sum(err, cover) / int(inside(cover).sum()) if kind == "mask" else
                            weighted_sum(err, cover) / weight_sum(cover))
                    want = mean + 2.0 * int(np.count_nonzero(want_used == 0))
                    print(f"{name} {kind} p={p}: cost {costs[p]!r}, restated {want!r}")
                    assert abs(costs[p] - want) <= 2e-4
                m.setMask(None)
    finally:
        m.close()


def test_state_after_a_call(ip):
    w, h, K = 97, 53, 16
    ip.setOption("pixel_err", 1)
    ip.setImage(noise(w, h).reshape(-1), None, w, ip.illum)
    pals = pals_of(K, 16, P)
    first = both(ip, pals, 1.0, "jarvis")
    assert list(_sums_and_errors(ip, P, K)[:2]) == [_lib.HQ_ERR_STATE, _lib.HQ_ERR_STATE]
    plain = both(ip, pals, 0.0, "plain")
    s1 = _sums_and_errors(ip, P, K)
    assert s1[:2] == (_lib.HQ_OK, _lib.HQ_OK)
    assert_same(first, both(ip, pals, 1.0, "jarvis"), "two identical calls")
    assert not np.array_equal(first[2][0], plain[2][0])
    assert_same(plain, both(ip, pals, 0.0, "plain"), "the plain evaluation, before and after")
    s2 = _sums_and_errors(ip, P, K)
    np.testing.assert_array_equal(s1[2], s2[2])
    np.testing.assert_array_equal(s1[3], s2[3])
    # a smaller population after a larger one, and a one-row kernel after a two-row one (the carry shrinks)
    one = both(ip, pals[1:], 1.0, "burkes")
    two = both(ip, pals, 1.0, "burkes")
    np.testing.assert_array_equal(one[2][0], two[2][1])
    assert one[0][0] == two[0][1]


def test_a_device_search_does_not_see_an_earlier_call(gpu):
    w, h, K = 97, 53, 16
    out = []
    for first in (False, True):
        m = new_ctx(gpu)
        try:
            m.setImage(noise(w, h).reshape(-1), None, w, m.illum)
            if first:
                m.ditherPopulation(pals_of(K, 16), 1.0, kernel="stucki")
            out.append(_search16(m, K))
        finally:
            m.close()
    assert out[0][0] == out[1][0] == 16 and out[0][2] == out[1][2]
    np.testing.assert_array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def test_profile_counts_launches_under_dither_and_none_under_assign(ip):
    w, h, K = 97, 53, 16
    lib = hq.load()
    ip.setImage(noise(w, h).reshape(-1), None, w, ip.illum)
    pals = pals_of(K, 16, P)
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

    ip.ditherPopulation(pals, 1.0, kernel="jarvis")
    ip.ditherPopulation(pals, 0.5, kernel="sierra_lite")
    assert counts() == {"dither": 2, "assign": 0, "grid": 0, "cost": 2, "finalize": 2}
    ip.ditherPopulation(pals, 1.0)
    assert counts() == {"dither": 3, "assign": 0, "grid": 0, "cost": 3, "finalize": 3}


def test_refusals_leave_outputs_and_state_untouched(gpu):
    w, h, K, Pn = 64, 48, 8, 3
    rgba = noise(w, h, 2)
    pals = pals_of(K, 1, Pn)
    jarvis = preset("jarvis")
    m = new_ctx(gpu)
    try:
        def refused(status, pl=pals, taps=jarvis, s=1.0, **kw):
            rc, costs, used = raw_diffuse(m, pl, taps, s, **kw)
            assert rc == status, (rc, hq.load().hq_last_error(m.ctx))
            assert np.all(costs == -7.0) and np.all(used == -7)

        refused(_lib.HQ_ERR_STATE)  # no image set
        m.setImage(rgba.reshape(-1), None, w, m.illum, row_begin=8, row_end=40)
        refused(_lib.HQ_ERR_STATE)  # a row-block shard
        m.setOption("pixel_err", 1)
        m.setImage(rgba.reshape(-1), None, w, m.illum)

        def state():
            return [m.getIndices(p) for p in range(Pn)] + [m.getPixelErrors(p) for p in range(Pn)] + \
                [m.lastPath()["sequence"]]

        plain = m.computeQuantizationErrorPopulation(pals, 2.0)
        held = state()
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            refused(_lib.HQ_ERR_UNSUPPORTED)
            m.setOption(name, 0 if name == "palette_split" else 1)
        refused(_lib.HQ_ERR_UNSUPPORTED, pals_of(257, 1))  # K > 256
        refused(_lib.HQ_ERR_ARG, Pn=0)
        refused(_lib.HQ_ERR_ARG, K=0)
        refused(_lib.HQ_ERR_ARG, None, Pn=Pn, K=K)
        assert raw_diffuse(m, pals, jarvis, costs_ptr=False)[0] == _lib.HQ_ERR_ARG
        for s in (-0.001, 1.001, float("nan"), float("inf")):
            refused(_lib.HQ_ERR_ARG, s=s)
        for ch, v in ((0, np.nan), (5, np.inf), (2, -0.001), (4 * K * 2 + 1, 1.001)):
            bad = pals.copy()
            bad.reshape(-1)[ch] = v
            refused(_lib.HQ_ERR_ARG, bad)
        # a null or illegal tap set
        refused(_lib.HQ_ERR_ARG, taps=None)
        zero = np.zeros((3, 5), np.int64)
        refused(_lib.HQ_ERR_ARG, taps=(zero, 1))                # no weight
        refused(_lib.HQ_ERR_ARG, taps=(jarvis[0], 47))          # sum w > div
        refused(_lib.HQ_ERR_ARG, taps=(jarvis[0], 0))
        refused(_lib.HQ_ERR_ARG, taps=(jarvis[0], -48))
        for dy, i, v in ((0, 0, 1), (0, 1, 1), (0, 2, 1), (1, 2, -1), (2, 4, -1)):
            bad = jarvis[0].copy()
            bad[dy, i] = v
            refused(_lib.HQ_ERR_ARG, taps=(bad, 100))
        for a, b in zip(held, state()):
            np.testing.assert_array_equal(a, b)
        assert _sums_and_errors(m, Pn, K)[:2] == (_lib.HQ_OK, _lib.HQ_OK)
        np.testing.assert_array_equal(m.computeQuantizationErrorPopulation(pals, 2.0), plain)
        ok = pals.copy()
        ok[:, 3::4] = np.nan  # (.w is not a channel)
        assert raw_diffuse(m, ok, jarvis)[0] == _lib.HQ_OK
        # an image pixel outside [0, 1] or not finite: found on the device, once per image
        for v in (1.5, -0.25, np.nan):
            img = rgba.copy()
            img[w * 17 + 5, 1] = v
            m.setImage(img.reshape(-1), None, w, m.illum)
            refused(_lib.HQ_ERR_UNSUPPORTED)
            refused(_lib.HQ_ERR_UNSUPPORTED)  # (the remembered answer)
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        assert raw_diffuse(m, pals, jarvis)[0] == _lib.HQ_OK
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 4. Python
# ---------------------------------------------------------------------------
def test_kernel_on_both_calls(ip):
    w, h, K = 97, 53, 16
    rgba = noise(w, h)
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    pal = pals_of(K, 16, 1)[0]
    pal[3::4] = 0.5  # (a .w the output must not carry)
    table = pal.reshape(K, 4).copy()
    table[:, 3] = 0.0
    for kernel in ("stucki", preset("stucki"), (np.array(preset("stucki")[0], np.float64).tolist(), 42.0)):
        out = ip.quantizeDithered(pal, 1.0, kernel=kernel)
        idx = ip.getIndices(0)
        np.testing.assert_array_equal(idx, restate(rgba, table, w, h, 1.0, "stucki")[0].astype(np.uint8))
        np.testing.assert_array_equal(out.view(np.uint32), table[idx].reshape(-1).view(np.uint32))
        np.testing.assert_array_equal(ip.lastUsedColors, np.bincount(idx, minlength=K)[:K] > 0)
        assert ip.ditherError == ip.ditherPopulation(pal.reshape(1, -1), 1.0, 0.0, kernel=kernel)[0]
    # None stays hq_dither_population
    ip.quantizeDithered(pal, 1.0)
    np.testing.assert_array_equal(ip.getIndices(0), dither(rgba, table, w, h, 1.0)[0].astype(np.uint8))
    for bad in ("floyd", (np.zeros((3, 4)), 1), (np.full((3, 5), 0.5), 8), (preset("stucki")[0], 2 ** 31)):
        with pytest.raises(ValueError):
            ip.ditherPopulation(pal.reshape(1, -1), 1.0, kernel=bad)
    with pytest.raises(_lib.HQError):
        ip.ditherPopulation(pal.reshape(1, -1), 1.0, kernel=(preset("stucki")[0], 41))


def _find(m, rgba, w, K, **kw):
    sw = hq.SWASA(population=2, imax=100, seed=4)
    best = m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, m.illum, iterations=10, **kw)
    return np.asarray(best, np.float32), sw


def test_dither_kernel_in_find_best_quantization(ip):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    plain, _ = _find(ip, rgba, w, K)
    plain_err = ip.bestError
    best, sw = _find(ip, rgba, w, K, dither=1.0, ditherKernel="atkinson")
    np.testing.assert_array_equal(best.view(np.uint32), plain.view(np.uint32))
    assert ip.bestError == plain_err
    assert ip.bestErrorDithered == ip.ditherPopulation(best.reshape(1, -1), 1.0, sw.delta, kernel="atkinson")[0]
    assert ip.bestErrorDithered != ip.ditherPopulation(best.reshape(1, -1), 1.0, sw.delta)[0]
    best, sw = _find(ip, rgba, w, K, dither=1.0, ditherSearch=True, ditherKernel="atkinson")
    assert ip.lastPath()["argmin"] == "diffuse"
    assert ip.bestError == ip.bestErrorDithered == \
        ip.ditherPopulation(best.reshape(1, -1), 1.0, sw.delta, kernel="atkinson")[0]
    with pytest.raises(ValueError):
        _find(ip, rgba, w, K, dither=1.0, ditherKernel="floyd")


def test_dither_kernel_in_quantization(gpu):
    w, h, K = 32, 32, 4
    rgba = noise(w, h, 7)
    image = np.stack([rgba[:, 0], rgba[:, 1], rgba[:, 2]])
    sw = hq.SWASA(population=2, imax=100, seed=4)
    q0, best0, err0 = hq.quantization(image, w, K, sw, device=gpu, iterations=10, dither=1.0)
    q1, best1, err1 = hq.quantization(image, w, K, sw, device=gpu, iterations=10, dither=1.0, ditherKernel="jarvis")
    np.testing.assert_array_equal(best0, best1)
    assert err0 == err1
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, w, m.illum)
        want = m.quantizeDithered(best1, 1.0, kernel="jarvis").reshape(-1, 4)[:, :3].T
    finally:
        m.close()
    np.testing.assert_array_equal(q1, want)
    assert not np.array_equal(q0, q1)


# ---------------------------------------------------------------------------
# 5. The point of the feature
# ---------------------------------------------------------------------------
def test_ramp_costs_less_under_every_preset(ip):
    """The 64 x 64 ramp under the eight cube corners: every preset's cost is strictly below the
    nearest-colour cost, on the restatement first, then on the device.  No order among the kernels."""
    w = h = 64
    rgba, pal = ramp_image(w, h), cube_corners()
    f = o.design_filters(72, 45.0)
    lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), f, w)

    def cost_of(idx, used):
        err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
        return o.average_array(err) + o.compute_penalty(used, 2.0)

    ref_plain = cost_of(*o.assign(rgba, pal))
    ip.setImage(rgba.reshape(-1), None, w, ip.illum)
    plain = ip.computeQuantizationErrorPopulation(pal.reshape(1, -1), 2.0)[0]
    for name in PRESETS:
        idx, used = restate(rgba, pal, w, h, 1.0, name)
        ref = cost_of(idx, used)
        assert ref < ref_plain, name
        cost = ip.ditherPopulation(pal.reshape(1, -1), 1.0, 2.0, kernel=name)[0]
        np.testing.assert_array_equal(ip.getIndices(0), idx.astype(np.uint8), err_msg=name)
        print(f"{name} {PRESET_CLASS[name]}: restated {ref!r} / {ref_plain!r}, device {cost!r} / {plain!r}, "
              f"ratio {cost / plain:.3f}")
        assert cost < plain, name

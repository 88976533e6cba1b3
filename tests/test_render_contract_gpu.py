"""The contract of the rendered entry points, recorded once and compared ever after: for
hq_dither_population, hq_diffuse_population, hq_dot_population[_partial],
hq_ordered_population[_partial] and hq_search_set_ordered followed by hq_search_run, the status
and the exact hq_last_error text of every refusal one GPU without a communicator can give, which
refusal wins when two conditions hold at once, that a refused call touches nothing (the outputs
keep their sentinel, the path record's sequence stands, hq_get_indices answers as before), and for
one accepted call of each rendering on each shape the whole hq_last_path record and the launch
count of every profiling stage -- the dispatch and the launch sequence.

tests/golden/render_contract.json holds what the library answered at the commit DESIGN.md 27
names.  This module only compares; with HQ_RENDER_CONTRACT_RECORD=1 in the environment it writes
the file instead (off by default: a recording made by the code under test checks nothing).

Indices and costs are not looked at here: test_dither_gpu.py, test_diffusion_gpu.py,
test_dot_gpu.py, test_dot_shards_gpu.py and test_ordered_gpu.py check them bit for bit.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import hybridquantization_amd as hq
from dot_ref import KNUTH8
from hybridquantization_amd import _lib
from test_dither_gpu import new_ctx, pals_of
from test_dot_gpu import _filters, filter_ctx, matrix_of

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_contract.json")
RECORD = os.environ.get("HQ_RENDER_CONTRACT_RECORD") == "1"

P, K = 2, 5
ENTRIES = ("dither", "diffuse", "dot", "dot_partial", "ordered", "ordered_partial")
STRENGTH = ("dither", "diffuse", "dot", "dot_partial")  # the others take an amplitude per channel
STAGES = ("grid", "assign", "cost", "finalize", "sa_step", "comm", "centroid", "lloyd", "hist", "errsum", "reseed",
          "dither", "reduce", "dot")
W, H, SH = 24, 20, 40   # the whole image; the sharded one's rows
R0, R1 = 16, 24         # the shard: extended rows [6, 34), so an apron of 5 holds rows [1, 6) and [34, 39)


def planar(w, h, seed):
    """Inline RGBA of pixels that are no k/255: no packed copy, the range flag is the device's."""
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = np.random.default_rng(seed).random((w * h, 3), np.float32) * np.float32(0.999)
    return rgba


def with_pixel(rgba, pos, v=1.5):
    out = rgba.copy()
    out[pos, 1] = v
    return out


def call(m, entry, pals, param=None, Pn=None, Kn=None, pal_ptr=True, out_ptr=True, extra="default"):
    """One rendered entry point with sentinel outputs -> (status, the output arrays).  param: the
    strength, or the amplitudes (three floats; "null": a NULL pointer); extra: the diffusion taps
    (diffuse) or the class matrix (dot, dot_partial), None a NULL pointer."""
    lib = hq.load()
    Pn = pals.shape[0] if Pn is None else Pn
    Kn = pals.shape[1] // 4 if Kn is None else Kn
    costs = np.full(max(Pn, 1), -7.0, np.float64)
    used = np.full((max(Pn, 1), max(Kn, 1)), -7, np.int32)
    part = np.full((max(Pn, 1), 1 + max(Kn, 1)), -7.0, np.float64)
    pp = _lib.fptr(pals) if pal_ptr else None
    cp, dp = (_lib.dptr(costs), _lib.dptr(part)) if out_ptr else (None, None)
    if entry in STRENGTH:
        s = 0.75 if param is None else param
    else:
        a = None if param == "null" else np.asarray((0.5, 0.25, 0.75) if param is None else param, np.float32)
        ap = None if a is None else _lib.fptr(a)
    if entry == "diffuse":
        x = m._taps("jarvis") if extra == "default" else extra
    elif entry in ("dot", "dot_partial"):
        x = None if extra == "default" else extra
    xp = None if entry not in ("diffuse", "dot", "dot_partial") or x is None else C.byref(x)
    if entry == "dither":
        return lib.hq_dither_population(m.ctx, pp, Pn, Kn, s, 2.0, cp, _lib.iptr(used)), [costs, used]
    if entry == "diffuse":
        return lib.hq_diffuse_population(m.ctx, pp, Pn, Kn, xp, s, 2.0, cp, _lib.iptr(used)), [costs, used]
    if entry == "dot":
        return lib.hq_dot_population(m.ctx, pp, Pn, Kn, xp, s, 2.0, cp, _lib.iptr(used)), [costs, used]
    if entry == "dot_partial":
        return lib.hq_dot_population_partial(m.ctx, pp, Pn, Kn, xp, s, dp), [part]
    if entry == "ordered":
        return lib.hq_ordered_population(m.ctx, pp, Pn, Kn, ap, 2.0, cp, _lib.iptr(used)), [costs, used]
    return lib.hq_ordered_population_partial(m.ctx, pp, Pn, Kn, ap, dp), [part]


def state(m):
    """What a refused call must leave alone: the path record and hq_get_indices' answer."""
    idx = np.zeros(max(getattr(m, "w", 1) * getattr(m, "h", 1), 1), np.uint8)
    rc = hq.load().hq_get_indices(m.ctx, 0, idx.ctypes.data_as(_lib._u8))
    return m.lastPath(), rc, idx


def refusal(m, entry, pals, **kw):
    """-> {"status", "error"} of the call; a refused one has touched nothing."""
    before = state(m)
    rc, outs = call(m, entry, pals, **kw)
    if rc == _lib.HQ_OK:
        return {"status": rc, "error": ""}
    msg = hq.load().hq_last_error(m.ctx).decode()
    for a in outs:
        assert np.all(a == -7), (entry, kw, msg)
    after = state(m)
    assert after[0] == before[0] and after[0]["sequence"] == before[0]["sequence"], (entry, kw, msg)
    assert after[1] == before[1], (entry, kw, msg)
    np.testing.assert_array_equal(after[2], before[2], err_msg=f"{entry} {kw} {msg}")
    return {"status": rc, "error": msg}


def counts(m):
    got = {}
    for name in STAGES:
        ms, n = C.c_double(), C.c_int64()
        _lib.check(hq.load().hq_profile_get(m.ctx, name.encode(), C.byref(ms), C.byref(n)), m.ctx)
        got[name] = n.value
    return got


def path_json(m):
    return {k: sorted(v) if isinstance(v, frozenset) else v for k, v in m.lastPath().items()}


def accepted(m, entry, pals):
    """-> the status, the path record and the launch count per stage of one profiled call."""
    lib = hq.load()
    lib.hq_profile_enable(m.ctx, 1)
    lib.hq_profile_reset(m.ctx)
    rc, _ = call(m, entry, pals)
    out = {"status": rc, "error": "" if rc == _lib.HQ_OK else lib.hq_last_error(m.ctx).decode(),
           "path": path_json(m), "launches": counts(m)}
    lib.hq_profile_enable(m.ctx, 0)
    return out


def option(m, name, on):
    m.setOption(name, {"slice_ranks": 2, "palette_split": 1}[name] if on else {"slice_ranks": 1, "palette_split": 0}[name])


def set_shard(m, rgba, apron):
    m.setOption("dot_apron", apron)
    m.setImage(rgba.reshape(-1), None, W, m.illum, row_begin=R0, row_end=R1)


def eval_partial(m, pals):
    part = np.zeros((pals.shape[0], 1 + pals.shape[1] // 4), np.float64)
    _lib.check(hq.load().hq_eval_population_partial(m.ctx, _lib.fptr(pals), pals.shape[0], pals.shape[1] // 4,
                                                    _lib.dptr(part)), m.ctx)


def bad_matrix():
    rep = KNUTH8.copy()
    rep[0, 0] = rep[7, 7]
    return matrix_of(rep)


def bad_taps(m):
    t = m._taps("jarvis")
    t.div = 47  # (the weights sum to 48)
    return t


def observe_refusals(gpu, out):
    pals, img, tall = pals_of(K, 3, P), planar(W, H, 24), planar(W, SH, 40)
    over = pals.copy()
    over.reshape(-1)[5] = 1.5
    nan = pals.copy()
    nan.reshape(-1)[4 * K + 2] = np.nan
    wide, wide_over = pals_of(257, 1, P), pals_of(257, 1, P)
    wide_over.reshape(-1)[1] = 1.5
    ref, win = out["refusals"], out["winning"]
    # no image
    m = new_ctx(gpu)
    try:
        for e in ENTRIES:
            ref[e]["no_image"] = refusal(m, e, pals)
            win[e]["bad_parameter+no_image"] = refusal(m, e, pals, param=1.5 if e in STRENGTH else (0.5, 1.5, 0.5))
    finally:
        m.close()
    # the whole image, a plain evaluation on the device
    m = new_ctx(gpu)
    try:
        m.setImage(img.reshape(-1), None, W, m.illum)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        for e in ENTRIES:
            r = ref[e]
            r["null_palette"] = refusal(m, e, pals, pal_ptr=False)
            r["null_output"] = refusal(m, e, pals, out_ptr=False)
            r["P0"] = refusal(m, e, pals, Pn=0)
            for name, v in (("below", -0.5), ("above", 1.5), ("nan", float("nan"))):
                r["parameter_" + name] = refusal(m, e, pals, param=v if e in STRENGTH else (0.5, v, 0.5))
            if e not in STRENGTH:
                r["null_amp"] = refusal(m, e, pals, param="null")
            if e == "diffuse":
                r["null_taps"] = refusal(m, e, pals, extra=None)
                r["illegal_taps"] = refusal(m, e, pals, extra=bad_taps(m))
            if e in ("dot", "dot_partial"):
                r["illegal_matrix"] = refusal(m, e, pals, extra=bad_matrix())
            r["K257"] = refusal(m, e, wide)
            r["palette_1.5"] = refusal(m, e, over)
            r["palette_nan"] = refusal(m, e, nan)
            for name in ("slice_ranks", "palette_split"):
                option(m, name, True)
                r[name] = refusal(m, e, pals)
                option(m, name, False)
            win[e]["K257+palette_1.5"] = refusal(m, e, wide_over)
        m.setMask(np.arange(W * H).reshape(H, W) % 3 != 0)
        option(m, "slice_ranks", True)
        for e in ENTRIES:
            ref[e]["mask+slice_ranks"] = refusal(m, e, pals)
        option(m, "slice_ranks", False)
        # a planar image with a pixel at 1.5 (the range flag, once per image: asked twice)
        m.setImage(with_pixel(img, W * 7 + 5).reshape(-1), None, W, m.illum)
        m.computeQuantizationErrorPopulation(pals, 2.0)
        for e in ENTRIES:
            ref[e]["image_1.5"] = refusal(m, e, pals)
            ref[e]["image_1.5_again"] = refusal(m, e, pals)
    finally:
        m.close()
    # the shard, an apron of 5 and of 2
    m = new_ctx(gpu)
    try:
        set_shard(m, tall, 5)
        eval_partial(m, pals)
        for e in ENTRIES:
            ref[e]["shard"] = refusal(m, e, pals) if not e.endswith("_partial") else {"status": 0, "error": ""}
            option(m, "slice_ranks", True)
            win[e]["slice_ranks+shard"] = refusal(m, e, pals)
            option(m, "slice_ranks", False)
        set_shard(m, tall, 2)
        eval_partial(m, pals)
        ref["dot_partial"]["apron_2"] = refusal(m, "dot_partial", pals)
        set_shard(m, with_pixel(tall, W * 3 + 7), 5)  # row 3: an apron row
        eval_partial(m, pals)
        ref["dot_partial"]["apron_row_1.5"] = refusal(m, "dot_partial", pals)
    finally:
        m.close()


def observe_accepted(gpu, out):
    pals = pals_of(K, 3, P)
    acc = out["accepted"]
    m = new_ctx(gpu)
    try:
        m.setImage(planar(W, H, 24).reshape(-1), None, W, m.illum)
        acc["24x20"] = {e: accepted(m, e, pals) for e in ENTRIES}
        tall = planar(W, SH, 40)
        for apron in (5, 2):
            set_shard(m, tall, apron)
            acc[f"24x40_rows_16_24_apron_{apron}"] = {
                e: accepted(m, e, pals) for e in ("dot_partial", "ordered_partial") if apron == 5 or e != "dot_partial"}
    finally:
        m.close()
    m = filter_ctx(gpu, _filters(5, 3))  # (half-width 0: the image does not hold half-width 10)
    try:
        m.setImage(planar(5, 3, 8).reshape(-1), None, 5, m.illum)
        acc["5x3"] = {e: accepted(m, e, pals) for e in ENTRIES}
    finally:
        m.close()


def search_refusal(m, what, fn):
    before = state(m)
    rc = fn()
    msg = hq.load().hq_last_error(m.ctx).decode() if rc != _lib.HQ_OK else ""
    if rc != _lib.HQ_OK:
        after = state(m)
        assert after[0] == before[0] and after[1] == before[1], (what, msg)
        np.testing.assert_array_equal(after[2], before[2], err_msg=what)
    return {"status": rc, "error": msg}


def observe_search(gpu, out):
    lib = hq.load()
    res = out["search"]
    img = planar(W, H, 24)
    amp, ran = np.asarray((0.5, 0.5, 0.5), np.float32), C.c_int(-7)

    def search_on(m, Kn):
        sw = hq.SWASA(population=P, imax=100, seed=9, t0=0.05)
        params, h = sw.params(), C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), Kn, sw.seed, C.byref(h)), m.ctx)
        return h

    def set_ordered(h, a):
        return lambda: lib.hq_search_set_ordered(h, None if a is None else _lib.fptr(np.asarray(a, np.float32)))

    m = new_ctx(gpu)
    try:
        m.setImage(img.reshape(-1), None, W, m.illum)
        h = search_on(m, K)
        try:
            assert m.searchInfo(h)["device_resident"]
            for name, v in (("below", -0.5), ("above", 1.5), ("nan", float("nan"))):
                res["set_ordered_amp_" + name] = search_refusal(m, name, set_ordered(h, (0.5, v, 0.5)))
            _lib.check(lib.hq_search_set_lloyd(h, 2), m.ctx)
            res["set_ordered_hybrid"] = search_refusal(m, "hybrid", set_ordered(h, amp))
            res["set_ordered_amp_above+hybrid"] = search_refusal(m, "amp + hybrid", set_ordered(h, (1.5, 0.5, 0.5)))
            _lib.check(lib.hq_search_set_lloyd(h, 0), m.ctx)
            for name in ("slice_ranks", "palette_split"):
                option(m, name, True)
                res["set_ordered_" + name] = search_refusal(m, name, set_ordered(h, amp))
                option(m, name, False)
            res["set_ordered"] = search_refusal(m, "accepted", set_ordered(h, amp))
            res["set_ordered_path"] = path_json(m)
            res["set_lloyd_under_ordered"] = search_refusal(m, "lloyd", lambda: lib.hq_search_set_lloyd(h, 2))
            option(m, "slice_ranks", True)
            res["run_slice_ranks"] = search_refusal(m, "run", lambda: lib.hq_search_run(h, 3, C.byref(ran)))
            res["run_slice_ranks"]["ran"] = ran.value
            option(m, "slice_ranks", False)
            lib.hq_profile_enable(m.ctx, 1)
            lib.hq_profile_reset(m.ctx)
            rc = lib.hq_search_run(h, 3, C.byref(ran))
            res["run_3"] = {"status": rc, "ran": ran.value, "path": path_json(m), "launches": counts(m)}
            lib.hq_profile_enable(m.ctx, 0)
        finally:
            lib.hq_search_destroy(h)
        # a planar image with a pixel at 1.5
        m.setImage(with_pixel(img, W * 7 + 5).reshape(-1), None, W, m.illum)
        h = search_on(m, K)
        try:
            res["set_ordered_image_1.5"] = search_refusal(m, "image", set_ordered(h, amp))
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()
    m = new_ctx(gpu, sa_device=0)  # (K = 257: host-driven)
    try:
        m.setImage(img.reshape(-1), None, W, m.illum)
        h = search_on(m, 257)
        try:
            res["set_ordered_K257"] = search_refusal(m, "K257", set_ordered(h, amp))
        finally:
            lib.hq_search_destroy(h)
    finally:
        m.close()


@pytest.fixture(scope="module")
def observed(gpu):
    out = {"refusals": {e: {} for e in ENTRIES}, "winning": {e: {} for e in ENTRIES}, "accepted": {}, "search": {}}
    observe_refusals(gpu, out)
    observe_accepted(gpu, out)
    observe_search(gpu, out)
    out = json.loads(json.dumps(out))  # (what the file would hold: NaN-free, lists for tuples)
    if RECORD:
        with open(FIXTURE, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    return out


@pytest.fixture(scope="module")
def golden(observed):
    with open(FIXTURE) as f:
        return json.load(f)


def same(got, want, label):
    assert sorted(got) == sorted(want), f"{label}: cases {sorted(got)} against the recorded {sorted(want)}"
    for k in sorted(want):
        assert got[k] == want[k], f"{label} {k}: {got[k]!r}, recorded {want[k]!r}"


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_are_the_recorded_ones(observed, golden, entry):
    same(observed["refusals"][entry], golden["refusals"][entry], entry)
    refused = [k for k, v in golden["refusals"][entry].items() if v["status"] != 0]
    assert len(refused) >= 12, refused  # (the recording holds refusals, not a run of accepted calls)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_same_refusal_wins(observed, golden, entry):
    same(observed["winning"][entry], golden["winning"][entry], entry)
    assert all(v["status"] != 0 for v in golden["winning"][entry].values())


def test_paths_and_launch_counts_of_accepted_calls(observed, golden):
    assert sorted(observed["accepted"]) == sorted(golden["accepted"])
    for shape, per in golden["accepted"].items():
        for entry, want in per.items():
            assert want["status"] == 0, (shape, entry, want)
            same(observed["accepted"][shape][entry], want, f"{shape} {entry}")
    # hq_profile_get counts a stage once per pass that timed it, however many kernels the stage
    # launched (dot diffusion's 64 on 24 x 20 and its fewer on 5 x 3 are one count each): what the
    # recording pins is which stages a rendering runs -- dot or dither in the place of grid + assign
    for shape in ("24x20", "5x3"):
        for entry, stage in (("dot", "dot"), ("dot_partial", "dot"), ("dither", "dither"), ("diffuse", "dither")):
            n = golden["accepted"][shape][entry]["launches"]
            assert n[stage] == 1 and n["grid"] == n["assign"] == 0 and n["cost"] == n["finalize"] == 1, (shape, entry, n)
        for entry in ("ordered", "ordered_partial"):
            n = golden["accepted"][shape][entry]["launches"]
            assert n["assign"] == n["grid"] == n["cost"] == 1 and n["dot"] == n["dither"] == 0, (shape, entry, n)


def test_the_search_under_the_ordered_cost(observed, golden):
    same(observed["search"], golden["search"], "search")
    assert golden["search"]["run_3"]["status"] == 0 and golden["search"]["run_3"]["ran"] == 3
    assert golden["search"]["run_slice_ranks"]["status"] != 0 and golden["search"]["run_slice_ranks"]["ran"] == 0

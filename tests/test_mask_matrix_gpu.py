"""Every kernel instance of the masked and the weighted cost units (hq_cost_masked.hip,
hq_cost_weighted.hip: the 66 instances of DESIGN.md section 4's table, each compiled a second
and a third time) and every row of the long-filter table, under masks and weight maps cut
along the launch's own tile grid (mask_ref.tile_masks, tile_weight_maps), on grids of at least
3 x 3 tiles and P = 2 palettes, so that the live-tile list is built and decoded with more
than one tile column, a non-default tile width and more than one palette.

Per instance, against the library's own unmasked evaluation: indices, used flags and error
image bit for bit; the cost within test_mask_gpu / test_weights_gpu's check 1 of the float64
sum over that error image; equal bits with and without the tile skip; the tiles that ran
against mask_ref.live_tiles; the reported instance against tests/path_ref.py and against the
plain launch's; all ones = no mask, a 0 / 1 weight map = that mask, bit for bit.  The masks'
own conditions are tests/test_mask.py's (no GPU)."""

import itertools
import time

import numpy as np
import pytest

import path_ref as pr
from mask_ref import live_tiles, masks_for, tile_masks, tile_weight_maps
from test_dispatch_gpu import _ctx, _filters, _image, _pals
from test_fast_path import designed_half
from test_mask_gpu import filter_ctx, indices, partial_of, plain, set_image, sweep_masks, u32, u64
from test_path_ref import CHUNKS, LONG_ROWS, MATRIX, design_table_fast_instances
from test_weights_gpu import sweep_maps
from weights_ref import nonzero, weight_sum

pytestmark = pytest.mark.gpu

KINDS = ("mask", "weights")
INSTANCE = {"mask": "masked", "weights": "weighted"}
DES = {"de76": 0, "de94": 1, "de2000": 2}
NAN_CAP = 0.01  # dE94: the share of pixels without a number (README: about 3 in 10^4; test_mask.py, the oracle's)
GROUPS = list(MATRIX) + ["chunked"]
REACHED = {}  # (kind, dE) -> the (cost_instance, fast instance) pairs that test_instance_matrix saw


def _set(m, cover, kind):
    (m.setMask if kind == "mask" else m.setWeights)(cover)


def _outputs(m, pals):
    """Everything an evaluation with "pixel_err" 1 gives, as bits."""
    Pn, K = pals.shape[0], pals.shape[1] // 4
    costs, used = plain(m, pals)
    return [u64(costs), used] + [u32(m.getPixelErrors(p)) for p in range(Pn)] + [indices(m, p, K) for p in range(Pn)]


def _zero_one_is_the_mask(m, pals, covers, label):
    """Identity: under the 0 / 1 map of each cover every output's bits are the masked
    evaluation's, with the error image stored and on the skipping launch."""
    for name, (cover, _) in covers.items():
        zo = (np.asarray(cover) != 0).astype(np.uint8)
        for pixel_err in (1, 0):
            m.setOption("pixel_err", pixel_err)
            got = {}
            for kind in KINDS:
                _set(m, zo, kind)
                got[kind] = _outputs(m, pals) if pixel_err else [u64(plain(m, pals)[0])]
                assert m.lastPath()["cost_instance"] == INSTANCE[kind]
            for a, b in zip(got["mask"], got["weights"]):
                np.testing.assert_array_equal(a, b, err_msg=f"{label} {name}: 0 / 1 weights, pixel_err {pixel_err}")
        m.setOption("pixel_err", 1)
    m.setWeights(None)


def _walk(m, kind, pals, label, tile=None, de=0, pair=None, pal_fits=True, names=None):
    """One instance (tile: its tile form) or one generic pair (pair) on the context m (image
    set) under every cover of `kind`.  -> the (cost_instance, fast instance) it reported."""
    Pn, K = pals.shape[0], pals.shape[1] // 4
    w, h = m.w, m.h
    m.setOption("pixel_err", 1)
    _set(m, None, kind)
    costs0, _ = plain(m, pals)
    rec0 = pr.check(m, K, Pn, label, pal_fits=pal_fits)
    inst = pr.fast_instance(rec0)
    assert rec0["cost_instance"] == "plain" and (inst is None) == (tile is None) and pr.generic_pair(rec0) == pair, (label, rec0)
    if tile is not None:
        assert pr.fast_tiles(m.options, m.halfSize, w, h, rec0["nch"], de)[:2] == tile
        covers = (tile_masks if kind == "mask" else tile_weight_maps)(w, h, *tile)
        every = len(live_tiles(np.ones((h, w), np.uint8), w, h, *tile, de2000=de == 2))
        assert every >= 9
    elif kind == "mask":
        covers = masks_for(w, h)
    else:
        covers = tile_weight_maps(w, h, 128, 16)
    covers = {k: v for k, v in covers.items() if names is None or k in names}
    seen = set()

    def each(name, cover, skip):
        live = len(live_tiles(cover, w, h, *tile, de2000=de == 2)) if tile is not None else 0
        got = pr.check(m, K, Pn, f"{label} {name} mask_skip {skip}", mask=kind, live_tiles=live, pal_fits=pal_fits)
        assert got["cost_instance"] == INSTANCE[kind] and pr.fast_instance(got) == inst and pr.generic_pair(got) == pair, \
            (label, name, skip, got)
        if tile is None:
            assert m.maskInfo()[2:] == (0, 0), (label, name)
        else:
            assert m.maskInfo()[2:] == (got["tiles_run"], got["tiles_all"]) == (live if skip else every, every), (label, name, skip)
        seen.add((got["cost_instance"], inst))

    if kind == "mask":
        res = sweep_masks(m, pals, w, h, label, masks=covers, tile=tile, de2000=de == 2, each=each)
    else:
        res = sweep_maps(m, pals, w, h, label, maps=covers, tile=tile or (128, 16), de2000=de == 2, each=each)
    # dE94: the pixels whose dE is NaN for a palette were taken out of every cover
    dropped = int(np.count_nonzero(~res["fin"]))
    print(f"{label}: {dropped} of {w * h} pixels without a number")
    assert de == 1 or dropped == 0, label
    assert dropped < NAN_CAP * w * h and list(res["covers"]) == list(covers), (label, dropped, list(res["covers"]))
    if kind == "weights":  # (under a mask sweep_masks holds all ones to the plain bits)
        _zero_one_is_the_mask(m, pals, {k: v for k, v in res["covers"].items() if k != "ramp"}, label)
        if not dropped and "ones" in covers:
            m.setWeights(np.ones((h, w), np.uint8))
            np.testing.assert_array_equal(u64(plain(m, pals)[0]), u64(costs0), err_msg=f"{label}: weights all 1")
            m.setWeights(None)
    return seen


# ---------------------------------------------------------------------------
# 1. The instance matrix under a mask and under weights
# ---------------------------------------------------------------------------
def group_instances(group, de):
    """The rows of DESIGN's table that the options of `group` reach at the dE type `de`."""
    if group == "chunked":
        return {i for i in design_table_fast_instances() if i[2] == de and i[5] > 1}
    kernel, waves = ("cost_mfma", 4) if group.endswith("8x108") else ("cost16w", 8 if group.endswith("16x256") else 4)
    return {(kernel, int(group[1:3]), de, trim, waves, 1) for trim in (1, 0)}


def _matrix_group(gpu, kind, de, group):
    seen = set()
    if group == "chunked":  # P = 1, as test_every_fast_instance_is_reached runs it
        m = _ctx(gpu, _filters(10), (300, 45), de=de, lab=False)
        try:
            for K, trim in itertools.product(CHUNKS, (1, 0)):
                m.setOption("trim", trim)
                seen |= _walk(m, kind, _pals(K, 1).reshape(1, -1), f"{kind} de {de} K {K} trim {trim}", (128, 16), de)
        finally:
            m.close()
        return seen
    halves, fopts = MATRIX[group]
    size = (535, 45) if fopts.get("cost_tw") == 256 else (301, 93)
    tile = (108, 8) if fopts.get("cost_rows") == 8 else (fopts.get("cost_tw", 128), 16)
    for half in halves:
        m = _ctx(gpu, _filters(half), size, de=de, lab=False, **fopts)
        try:
            for trim in (1, 0):
                m.setOption("trim", trim)
                seen |= _walk(m, kind, _pals(64, 2).reshape(2, -1), f"{kind} de {de} {group} half {half} trim {trim}", tile, de)
        finally:
            m.close()
    return seen


@pytest.mark.parametrize("de", sorted(DES))
@pytest.mark.parametrize("kind", KINDS)
def test_instance_matrix(gpu, kind, de):
    """All 22 instances of one dE type with test_every_fast_instance_is_reached's options:
    every half-width of MATRIX, trim 1 and 0, every K of CHUNKS; P = 2 (P = 1 chunked)."""
    d = DES[de]
    seen = set()
    for group in GROUPS:
        t = time.perf_counter()
        got = _matrix_group(gpu, kind, d, group)
        print(f"{kind} {de} {group}: {time.perf_counter() - t:.2f} s, {sorted(got)}")
        assert got == {(INSTANCE[kind], i) for i in group_instances(group, d)}, (group, got)
        seen |= got
    want = {(INSTANCE[kind], i) for i in design_table_fast_instances() if i[2] == d}
    assert seen == want and len(seen) == 22
    REACHED[(kind, d)] = seen


def test_all_132_instances_were_reached():
    """The union of what the six matrix tests above reported, in this run: 66 masked and 66
    weighted instances, DESIGN's table twice."""
    assert sorted(REACHED) == [(k, d) for k in KINDS for d in range(3)], "run with the whole module: it sums test_instance_matrix"
    for kind in KINDS:
        got = set().union(*(REACHED[(kind, d)] for d in range(3)))
        assert got == {(INSTANCE[kind], i) for i in design_table_fast_instances()} and len(got) == 66
    print(f"fast instances reached: {sum(len(v) for v in REACHED.values())} (masked and weighted)")


# ---------------------------------------------------------------------------
# 2. The long-filter rows under a mask and under weights
# ---------------------------------------------------------------------------
# LONG_ROWS' generic rows (its first one is the fast path: section 1's), and cost_variant 1 at half-width 10
GENERIC_ROWS = [r for r in LONG_ROWS if r[4] is not None] + \
    [(10, dict(cost_variant=1), 64, True, (("gen_hmfma", 1), ("gen_vmfma", 64)))]
GENERIC_COVERS = {"mask": ("ones", "bernoulli", "edges", "values"), "weights": ("ones", "bernoulli", "edges", "ramp")}


@pytest.mark.parametrize("kind", KINDS)
def test_long_filter_rows(gpu, kind):
    """Every generic row of the long-filter table from that row's options, K and palette range,
    on test_every_long_filter_row_is_reached's image sizes: the four forms' mask and weight
    statements (hq_cost_generic.hip).  No tile is skipped there: maskInfo's tiles are (0, 0)."""
    ctxs, pairs = {}, set()
    try:
        for half, opts, K, fits, pair in GENERIC_ROWS:
            if half not in ctxs:
                ctxs[half] = _ctx(gpu, _filters(half), (max(half, 128) + 45, max(half, 64) + 22), lab=False)
            m = ctxs[half]
            assert m.halfSize == half
            for k, v in {**pr.DEFAULTS, **opts}.items():
                if k.startswith("gen_") or k == "cost_variant":
                    m.setOption(k, v)
            t = time.perf_counter()
            pals = _pals(K, 2, None if fits else 2.5).reshape(2, -1)
            _walk(m, kind, pals, f"{kind} half {half} {opts}", pair=pair, pal_fits=fits, names=GENERIC_COVERS[kind])
            print(f"{kind} half {half} {opts}: {time.perf_counter() - t:.2f} s")
            pairs.add(pair)
    finally:
        for m in ctxs.values():
            m.close()
    assert pairs == {r[4] for r in GENERIC_ROWS}
    print(f"{kind}: generic pairs reached: {sorted(pairs)}")


# ---------------------------------------------------------------------------
# 3. Shards on the non-default forms
# ---------------------------------------------------------------------------
SHARD_H = 93
UNEVEN = [0, 1, 4, 27, 28, 37, 59, 92, 93]  # test_fast_path_gpu's: single-row shards, r0 off every multiple of 8
# form -> (half-width, options, tile, image width, K)
SHARD_FORMS = {"b10-8x108": (10, dict(cost_rows=8), (108, 8), 301, 64), "b10-16x256": (10, dict(cost_tw=256), (256, 16), 535, 64),
               "b24-16x128": (24, {}, (128, 16), 301, 64), "b10-K300": (10, {}, (128, 16), 301, 300)}
# seams: every tile of every shard is live; one_tile: a sparse list (one or two tiles of a shard's own grid, most
# shards none at all), and 2048 pixels, enough for the sum's bar (a shard's dE76 differs from the whole image's
# in each pixel's last bits, test_fast_path_shards; over a few dozen pixels that does not average out to 1e-6)
SHARD_COVER = {"mask": "seams", "weights": "one_tile"}


@pytest.mark.parametrize("de", ["de76", "de2000"])
@pytest.mark.parametrize("form", sorted(SHARD_FORMS))
@pytest.mark.parametrize("kind", KINDS)
def test_shards_on_the_other_forms(gpu, kind, form, de):
    """The full image's cover on every shard of the uneven cut: each shard launches the restated
    live tiles of its own grid (from r0; dE2000: from the image's tile row, fast_grid_row0),
    divides by the full image's N or W, and the shards' sums add up to the whole image's."""
    half, fopts, tile, w, K = SHARD_FORMS[form]
    d, h, P = DES[de], SHARD_H, 2
    bounds = list(zip(UNEVEN[:-1], UNEVEN[1:]))
    assert min(r1 - r0 for r0, r1 in bounds) == 1 and all(r0 % 8 for r0, _ in bounds[1:])
    cover = (tile_masks if kind == "mask" else tile_weight_maps)(w, h, *tile)[SHARD_COVER[kind]]
    rgba, pals = _image(w, h).reshape(-1, 4), _pals(K, P).reshape(P, -1)
    n_full, w_full = nonzero(cover), weight_sum(cover)
    m = filter_ctx(gpu, designed_half(half), de=d, pixel_err=0, **fopts)
    try:
        def run(r0, r1):
            set_image(m, rgba, w, row_begin=r0, row_end=r1)
            _set(m, cover, kind)  # the FULL image's cover on every shard
            part = partial_of(m, pals)
            live = len(live_tiles(cover, w, h, *tile, r0, r1, d == 2))
            got = pr.check(m, K, P, f"{kind} {form} {de} rows [{r0},{r1})", mask=kind, live_tiles=live)
            assert m.maskInfo() == (n_full, nonzero(cover[r0:r1]), live, got["tiles_all"]), (r0, r1, m.maskInfo(), live)
            assert got["tiles_run"] == live and got["cost_instance"] == INSTANCE[kind]
            assert m.weightsInfo() == ((w_full, weight_sum(cover[r0:r1])) if kind == "weights" else m.maskInfo()[:2])
            if live:
                assert pr.fast_instance(got)[4:] == (8 if tile[0] == 256 else 4, pr.chunk_count(K)), got
            else:
                assert np.all(part[:, 0] == 0.0)
            return part[:, 0], live
        whole, live_whole = run(0, h)
        assert live_whole == len(live_tiles(np.ones((h, w)), w, h, *tile)) or kind == "weights"
        acc, lives = np.zeros(P), []
        for r0, r1 in bounds:
            s, live = run(r0, r1)
            acc += s
            lives.append(live)
        print(f"{kind} {form} {de}: live tiles per shard {lives}, shards {acc.tolist()}, whole {whole.tolist()}")
        assert (whole > 0).all() and np.isfinite(whole).all()
        np.testing.assert_allclose(acc, whole, rtol=1e-6, atol=0)
    finally:
        m.close()

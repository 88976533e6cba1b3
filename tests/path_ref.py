"""The kernel path a pass is expected to take, stated from DESIGN.md section 4's tables
("Fast-path dispatch and its tests", "Long-filter dispatch and its tests", "Chunked
palettes") and include/hq.h's option text -- not from the dispatcher.  No GPU here.

expected(...) gives the record ImageManipulation.lastPath() should return, as a dict with
the same keys and names; assert_path(got, want) compares the keys `want` holds (the
sequence counter, and the tile counts where no geometry was given, are left out).
search_device(...) says whether hq_search_create builds the device-resident search.
tests/test_path_ref.py checks the model on its own; the GPU modules hold the library to it.

gen_tile_shape 0 (by grid size) is modelled for small images only: fewer than 8 tiles per CU
on any device of 3 CUs or more, which every test image is (301 x 93 has 18 tiles) -- the
short forms.  The forced shapes 1 and 2 give the others.
"""

import types

import numpy as np

import hybridquantization_amd as hq



def bucket(half):
    """test_fast_path.bucket: the tap bucket 10 / 15 / 19 / 24 that holds `half`, 0 above 24.
    (Imported at the call: test_gpu.py, which test_fast_path imports from, imports this module.)"""
    from test_fast_path import bucket as b
    return b(half)


MAX_K8 = 256            # hq.h: K <= 256, the pruned grid argmin on 8-bit indices
MAX_K_CHUNKED = 16384   # 256 < K <= 16384: chunked palettes
MAX_NCH_FAST = 32       # the fast stencil up to K = 8192
LISTS16_NCH = (4, 32)   # option lists16 1: 4 to 32 chunks (512 < K <= 8192); 2: from 2 chunks
FAST_RANGE = (-32.0, 1.9)  # hq_eval_population: palettes outside take the exhaustive path
SA_MAX_P, SA_MAX_SUB = 64, 512  # option sa_device: population <= 64, and 512 sub-palettes
VT2_MAX_HALF = 64       # gen_vmfma / gen_vtile2: halfSize <= 64

# every option the path depends on, with hq.h's default
DEFAULTS = dict(cost_variant=0, gen_hmfma=1, gen_vmfma=1, gen_vtile2=1, gen_hrow4=1, gen_tile_shape=0,
                gen_hrow_outputs=4, cost_rows=16, cost_tw=128, trim=1, chunked=1, lists16=1, grid=32, img_u8=1,
                pixel_err=0, mask_skip=1, slice_ranks=1, slice_rank=0, sa_device=1, sa_graph=0)
DE_NAMES = {"de76": 0, "de94": 1, "de2000": 2}


def chunk_count(K):
    """Chunks of 256 colours per palette: the power of two that holds K."""
    n = 1
    while 256 * n < K:
        n <<= 1
    return n


def palette_fits(pals):
    """Every channel finite and inside FAST_RANGE (.w is not looked at)."""
    p = np.asarray(pals, np.float32).reshape(-1, 4)[:, :3]
    return bool(np.all((p >= np.float32(FAST_RANGE[0])) & (p <= np.float32(FAST_RANGE[1]))))


def chunks_of(opts, K, fits=True):
    """The chunk count of a population of K colours under `opts` (1: not chunked)."""
    o = {**DEFAULTS, **opts}
    chunked = MAX_K8 < K <= MAX_K_CHUNKED and o["chunked"] and o["grid"] > 0 and fits
    return chunk_count(K) if chunked else 1


def uses_lists16(opts, nch):
    o = {**DEFAULTS, **opts}
    lo = 2 if o["lists16"] >= 2 else LISTS16_NCH[0]
    return o["lists16"] > 0 and o["grid"] > 0 and nch > 1 and lo <= nch <= LISTS16_NCH[1]


def search_device(opts, P, K):
    """hq_search_create[_from] builds the device-resident search (its populations are clamped
    to [0, 1], so they always fit)."""
    o = {**DEFAULTS, **opts}
    nch = chunks_of(o, K)
    return bool(o["sa_device"]) and P <= SA_MAX_P and P * nch <= SA_MAX_SUB and (K <= MAX_K8 or nch > 1)


def fast_tiles(opts, half, w, own_rows, nch=1, de=0, r0=0):
    """(tile columns, tile rows, tiles per palette) of the fast cost launch."""
    o = {**DEFAULTS, **opts}
    hb = 10 if nch > 1 else bucket(half)
    rows = o["cost_rows"] if hb == 10 and nch == 1 else 16
    tw = 108 if rows == 8 else (o["cost_tw"] if hb == 10 and nch == 1 else 128)
    row0 = r0 - r0 % rows if de == 2 else r0  # CIEDE2000's shard grid starts at the image's tile row
    return tw, rows, -(-w // tw) * -(-(r0 + own_rows - row0) // rows)


def expected(opts, de, half, K, P=1, *, trim_ok=True, taps_fit=True, image_u8=True, pal_fits=True, mask=None,
             kind="full", ordered=False, w=None, h=None, rows=None, live_tiles=None):
    """The record of one pass.  opts: options that differ from DEFAULTS; de: 0 / 1 / 2 or its
    name; trim_ok, taps_fit: test_fast_path's trim_window_ok(f) and fits_split(f); image_u8:
    every channel of the image is k/255; pal_fits: palette_fits(pals); mask: None, "mask" or
    "weights"; kind: "full", "assign_only" or "dither"; w, h, rows = (r0, r1): the geometry,
    for the tile counts; live_tiles: tiles with an in-mask owned pixel (mask_ref), for
    tiles_run under a mask."""
    o = {**DEFAULTS, **opts}
    de = DE_NAMES.get(de, de)
    nch = chunks_of(o, K, pal_fits)
    wide = K > MAX_K8 and nch == 1
    dither = kind == "dither"
    assert not (wide and (dither or ordered or kind != "full")) and not (ordered and nch > 1)
    e = dict.fromkeys(("argmin_cmb", "argmin_passes", "cost_hb", "cost_de", "cost_trim", "cost_waves", "cost_nch",
                       "gen_h_outputs", "gen_h_split", "gen_h_rpt", "gen_v_rows", "tiles_run", "tiles_all"), 0)
    e.update({"pass": kind, "ordered": int(ordered), "P": P // o["slice_ranks"], "K": K, "nch": nch,
              "idx_bytes": 4 if wide else 2 if nch > 1 else 1, "cost": "none", "cost_instance": "plain",
              "gen_h": "none", "gen_v": "none", "why_not_fast": frozenset()})
    # the argmin
    e["pixels"] = "planar" if wide or dither or not (image_u8 and o["img_u8"]) else "u8"
    n16 = uses_lists16(o, nch)
    e["grid"] = "none" if wide or dither or o["grid"] == 0 else "lists16" if n16 else "build_grid"
    if wide:
        e["argmin"] = "assign_wide"
    elif dither:
        e["argmin"] = "dither"
    elif n16:
        e["argmin"] = "assign16"
    else:
        e["argmin"] = "assign_pipe_ordered" if ordered else "assign_pipe"
        e["argmin_cmb"] = min(nch, 4)
        e["argmin_passes"] = nch // 4 if nch > 4 else 1
    if kind == "assign_only":
        return e
    # the cost
    hb = bucket(half)
    why = set()
    if not hb:
        why.add("half")
    if o["cost_variant"] != 0:
        why.add("cost_variant")
    if not pal_fits:
        why.add("palette")
    if not taps_fit:
        why.add("taps")
    if nch > MAX_NCH_FAST:
        why.add("nch")
    elif nch > 1 and hb and not (hb == 10 and o["cost_rows"] == 16 and o["cost_tw"] == 128):
        why.add("chunk_form")  # the chunked kernel exists at HB = 10 on 16 x 128 tiles only
    if wide:
        why.add("wide")
    e["why_not_fast"] = frozenset(why)
    e["cost_instance"] = {None: "plain", "mask": "masked", "weights": "weighted"}[mask]
    e["cost_de"] = de
    if not why:
        if w is not None:
            r0, r1 = rows or (0, h)
            e["tiles_all"] = fast_tiles(o, half, w, r1 - r0, nch, de, r0)[2]
            skip = mask is not None and o["mask_skip"] and not o["pixel_err"]
            e["tiles_run"] = live_tiles if skip else e["tiles_all"]
        else:
            del e["tiles_run"], e["tiles_all"]
        if mask is not None and e.get("tiles_run") == 0:
            e["cost_de"] = 0
            return e  # no live tile: nothing is launched
        e["cost_trim"] = int(bool(o["trim"]) and trim_ok)
        e["cost_hb"], e["cost_waves"], e["cost_nch"], e["cost"] = hb, 4, nch, "cost16w"
        if nch == 1 and hb == 10 and o["cost_rows"] == 8:
            e["cost"] = "cost_mfma"
        elif nch == 1 and hb == 10 and o["cost_tw"] == 256:
            e["cost_waves"] = 8
        return e
    if o["cost_variant"] == 2:
        e.update(cost="pixel_generic", gen_h="gen_hpass", gen_v="gen_vpass")
        return e
    e["cost"] = "tiled_generic"
    shape = o["gen_tile_shape"]
    if o["gen_vmfma"] and pal_fits and taps_fit and half <= VT2_MAX_HALF:  # the matrix-core pair
        e.update(gen_v="gen_vmfma", gen_v_rows=128 if shape == 2 else 64)
        if o["gen_hmfma"]:
            e.update(gen_h="gen_hmfma", gen_h_rpt=4 if shape == 2 else 1)
        else:
            e.update(gen_h="gen_hrow4", gen_h_split=1, gen_h_outputs=o["gen_hrow_outputs"])
        return e
    if o["gen_hrow4"]:
        e.update(gen_h="gen_hrow4", gen_h_split=0, gen_h_outputs=o["gen_hrow_outputs"])
    else:
        e["gen_h"] = "gen_hrow"
    e["gen_v"] = "gen_vtile2" if o["gen_vtile2"] and half <= VT2_MAX_HALF else "gen_vtile"
    return e


def fast_instance(e):
    """(kernel, HB, dE, trim, waves, NCH) of a record on the fast path, else None."""
    if e["cost"] not in ("cost16w", "cost_mfma"):
        return None
    return (e["cost"], e["cost_hb"], e["cost_de"], e["cost_trim"], e["cost_waves"], e["cost_nch"])


def generic_pair(e):
    """(horizontal form and its variant, vertical form and its variant) of a record on the
    generic path, else None."""
    if e["cost"] not in ("tiled_generic", "pixel_generic"):
        return None
    hv = {"gen_hrow4": (e["gen_h_split"], e["gen_h_outputs"]), "gen_hmfma": (e["gen_h_rpt"],)}.get(e["gen_h"], ())
    vv = (e["gen_v_rows"],) if e["gen_v"] == "gen_vmfma" else ()
    return (e["gen_h"],) + hv, (e["gen_v"],) + vv


def assert_path(got, want, label=""):
    """Every key of `want` has `want`'s value in `got` (ImageManipulation.lastPath())."""
    diff = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not diff, f"{label}: path (reported, expected) differs in {diff}"


def filter_properties(m):
    """(trim_ok, taps_fit) of the filters uploaded to the ImageManipulation `m`, computed on the
    CPU from the taps it holds (test_fast_path's trim_window_ok and fits_split)."""
    from test_fast_path import fits_split, trim_window_ok
    k1, k2, k3, ak3 = m._filters
    f = types.SimpleNamespace(k1=k1, k2=k2, k3=k3, absk3=ak3, taps=k1.shape[0], half=m.halfSize)
    return trim_window_ok(f), fits_split(f)


class Context(hq.ImageManipulation):
    """An ImageManipulation that remembers, on the test side, what the test did to it: the
    options it set (name -> value), the owned rows of the image it uploaded and, per row of
    that image, whether every channel is k/255 in fp32.  The GPU modules create their
    contexts through it so that check() and check_search() need no second account."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.options, self.rows, self.row_lattice = {}, None, None

    def setOption(self, name, value):
        super().setOption(name, value)
        self.options[name] = int(value)

    def setImage(self, rgbInline, labInline, w, illuminant, row_begin=0, row_end=None):
        super().setImage(rgbInline, labInline, w, illuminant, row_begin, row_end)
        rgb = np.asarray(rgbInline, np.float32).reshape(-1, int(w), 4)[:, :, :3]
        k = np.rint(rgb.astype(np.float64) * 255).astype(np.float32)
        self.row_lattice = np.all(k / np.float32(255) == rgb, axis=(1, 2))
        self.rows = (int(row_begin), self.h if row_end is None else int(row_end))


def on_lattice(m):
    """Every channel of the rows the context holds (owned and halo) is k/255 in fp32, the
    condition under which the library keeps a packed 8-bit copy of the image."""
    (r0, r1), half = m.rows, m.halfSize
    return bool(m.row_lattice[max(0, r0 - half):min(m.h, r1 + half)].all())


def check(m, K, P=1, label="", opts=None, **kw):
    """The record of `m`'s last pass against expected() for the options set on it (those the
    test set through m.setOption, or `opts`), its dE type, its filters and the image geometry;
    kw: expected()'s other arguments.  -> the record."""
    trim_ok, taps_fit = filter_properties(m)
    o = dict(m.options if opts is None else opts)
    o = {k: v for k, v in o.items() if k in DEFAULTS}
    kw.setdefault("w", getattr(m, "w", None))
    kw.setdefault("h", getattr(m, "h", None))
    if "image_u8" not in kw:
        kw["image_u8"] = on_lattice(m)
    if "rows" not in kw and getattr(m, "rows", None) not in (None, (0, kw["h"])):
        kw["rows"] = m.rows
    want = expected(o, m.deltaEType, m.halfSize, K, P, trim_ok=trim_ok, taps_fit=taps_fit, **kw)
    got = m.lastPath()
    assert_path(got, want, label)
    return got


def check_search(m, handle, P, K, ran=False, label="", host_ok=False):
    """hq_search_info of a live search on `m` against search_device() for the options set on
    `m`: device-resident exactly when option sa_device is 1 (host_ok: a case that is meant to
    exceed the device-resident limits), its chunk count, and -- ran: after a run, with
    profiling off -- that the run was captured exactly when sa_graph is 1.  -> the info."""
    info = m.searchInfo(handle)
    want = search_device(m.options, P, K)
    asked = bool(m.options.get("sa_device", DEFAULTS["sa_device"]))
    assert info["device_resident"] == want, f"{label}: {info}, the model says device-resident {want}"
    assert host_ok or want == asked, f"{label}: P={P}, K={K} is host-driven under sa_device 1: it compares the host driver with itself"
    assert info["nch"] == (chunks_of(m.options, K) if want else 1), (label, info)
    if ran:
        assert info["graph"] == (want and bool(m.options.get("sa_graph", DEFAULTS["sa_graph"]))), (label, info)
    return info

"""State classes of a long-lived context and a walk over every transition between them.

No GPU here: the table of classes ("Context reuse and its tests"), their
images, palettes and filters, the oracle's results for each class, and euler_walk.
tests/test_reuse_walk.py checks the table and the walk on the CPU;
tests/test_context_reuse_gpu.py drives contexts through them.
"""

import os

import numpy as np

import c_oracle
import oracle as o
from dither_ref import dither
from mask_ref import masked_cost, rectangle
from ordered_ref import ordered

# Every option of hq_set_option that an evaluation reads, with its default.  The first two
# lines are test_long_filters_gpu.GEN_DEFAULTS and what test_fast_path_gpu.DEFAULTS adds
# (test_context_reuse_gpu.py asserts that they still agree).
OPTION_DEFAULTS = dict(
    cost_variant=0, gen_hmfma=1, gen_vmfma=1, gen_vtile2=1, gen_hrow4=1, gen_tile_shape=0, gen_hrow_outputs=4,
    cost_rows=16, cost_tw=128, trim=1, chunked=1, lists16=1,
    grid=32, img_u8=1, pixel_err=0, assign_blocks_per_cu=0, dither_rows=1024, palette_split=0,
    slice_ranks=1, slice_rank=0, mask_skip=1)

# (dpi, viewing distance in cm, half-width)
HALF10, HALF19, HALF51 = (72, 45.0, 10), (96, 60.0, 19), (300, 50.0, 51)

# image: (kind, w, h, seed, rows); rows None = the whole image, else the owned rows [r0, r1)
IMG_U8FAST = ("lattice", 97, 53, 3, None)
IMG_64 = ("lattice", 64, 48, 7, None)
# mask: (x0, x1, y0, y1), the rectangle of columns [x0, x1) and rows [y0, y1) that counts.  On
# IMG_U8FAST's 53 rows (four 16-row tiles, seven 8-row tiles, one tile column either way) rows
# [5, 20) leave whole tiles dead and, with columns [10, 60), every live tile partly live.
RECT = (10, 60, 5, 20)
ORDERED_AMP = (0.06, 0.03, 0.0)


def custom_map():
    """An 8 x 4 threshold map (4 rows of 8) that is not a Bayer map: the 32 ranks shuffled,
    (rank + 0.5) / 32 - 0.5, so every value lies inside [-0.5, 0.5]."""
    def make():
        ranks = np.random.default_rng(58).permutation(32).astype(np.float32).reshape(4, 8)
        m = (ranks + np.float32(0.5)) / np.float32(32) - np.float32(0.5)
        m.setflags(write=False)
        return m
    return _once(("map",), make)


def _cls(name, filters, image, P, K, op="eval", lab="oracle", out_of_range=False, mask=None, map=None, **opts):
    """mask: None or a rectangle (RECT's form); map: None for the default Bayer map, or "custom"
    (custom_map).  enter() sets or clears both at every step."""
    unknown = set(opts) - set(OPTION_DEFAULTS)
    assert not unknown, unknown
    return dict(name=name, filters=filters, image=image, P=P, K=K, op=op, lab=lab, out_of_range=out_of_range,
                opts={**OPTION_DEFAULTS, **opts}, strength=1.0 if op == "dither" else None, mask=mask, map=map,
                amp=ORDERED_AMP if op == "ordered" else None)


# lab: "device" = hq_set_image with lab4 NULL (the S-CIELAB of the image computed on the
# device), "oracle" = the oracle's LabRef uploaded.  The classes that share an image share its
# LabRef too, so a step between them sets no image.
CLASSES = [
    _cls("u8-fast", HALF10, IMG_U8FAST, 5, 16, lab="device", pixel_err=1),
    _cls("planar-generic", HALF10, ("float", 64, 48, 11, None), 1, 64, lab="device", cost_variant=1),
    _cls("bucket-19", HALF19, IMG_64, 6, 7, pixel_err=1, cost_tw=128),
    _cls("long-filter", HALF51, ("lattice", 129, 67, 5, None), 3, 16, lab="device"),
    _cls("chunk-grids", HALF10, IMG_U8FAST, 2, 300, lab="device", lists16=0),
    _cls("lists16", HALF10, IMG_U8FAST, 3, 600, lab="device", pixel_err=1),
    _cls("wide-u32", HALF10, IMG_64, 2, 20000),
    _cls("grid-0", HALF10, IMG_U8FAST, 4, 255, lab="device", grid=0),
    _cls("shard", HALF10, ("lattice", 193, 131, 9, (40, 90)), 4, 64, op="partial", lab="device", pixel_err=1),
    _cls("dither", HALF10, IMG_U8FAST, 2, 16, op="dither", lab="device", dither_rows=64),
    _cls("out-of-range", HALF10, IMG_U8FAST, 2, 16, lab="device", out_of_range=True),
    _cls("slice", HALF10, IMG_64, 4, 64, op="partial", slice_ranks=2, slice_rank=1),
    # the three below share u8-fast's image, filters and LabRef: a step between them and u8-fast,
    # grid-0 or dither changes the mask and the map only
    _cls("ordered", HALF10, IMG_U8FAST, 3, 16, op="ordered", lab="device", map="custom"),
    _cls("masked", HALF10, IMG_U8FAST, 4, 16, lab="device", mask=RECT, pixel_err=0),
    _cls("masked-8row", HALF10, IMG_U8FAST, 4, 16, lab="device", mask=RECT, cost_rows=8),
]
NAMES = [c["name"] for c in CLASSES]
FAST_RANGE = (-32.0, 1.9)  # hq_eval.hip, palette_fits_fast


def by_name(name):
    return CLASSES[NAMES.index(name)]


def euler_walk(n):
    """A closed walk over the complete directed graph on n vertices that uses every ordered
    pair (i, j), i != j, exactly once: n (n - 1) + 1 vertices, the first and last 0.
    Hierholzer's algorithm, the lowest unused successor first: deterministic."""
    if n < 2:
        return [0]
    nxt = [[j for j in range(n - 1, -1, -1) if j != i] for i in range(n)]  # popped from the end
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


# ---------------------------------------------------------------------------
# Inputs (computed once, read-only)
# ---------------------------------------------------------------------------
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def filters(cls):
    dpi, vd, half = cls["filters"]

    def make():
        f = o.design_filters(dpi, vd)
        assert f.half == half, (dpi, vd, f.half)
        return f
    return _once(("f", dpi, vd), make)


def image(cls):
    """The FULL image as inline RGBA float32 (n, 4), .w = 0."""
    kind, w, h, seed, _ = cls["image"]

    def make():
        R, G, B = o.synthetic_image(w, h, seed=seed)
        rgba = o.inline_rgba(R, G, B).reshape(-1, 4).copy()
        if kind == "float":  # off the k/255 lattice, inside [0, 1]
            rng = np.random.default_rng(seed)
            v = rgba[:, :3] * np.float32(0.75) + rng.random((w * h, 3), np.float32) * np.float32(0.25)
            rgba[:, :3] = np.clip(v, 0.0, 1.0)
        rgba.setflags(write=False)
        return rgba
    return _once(("img", kind, w, h, seed), make)


def rows(cls):
    _, w, h, _, r = cls["image"]
    return (0, h) if r is None else r


def palettes(cls):
    """(P, 4 K) float32."""
    def make():
        P, K = cls["P"], cls["K"]
        pals = np.stack([o.synthetic_palette(K, 40 + 7 * K + p).reshape(-1) for p in range(P)]).astype(np.float32)
        if cls["out_of_range"]:
            pals[1, 4 * 5 + 1] = 2.5
        pals.setflags(write=False)
        return pals
    return _once(("pal", cls["name"]), make)


def mask_of(cls):
    """The class's mask as uint8 (h, w), or None."""
    if cls["mask"] is None:
        return None
    _, w, h, _, _ = cls["image"]
    return rectangle(w, h, *cls["mask"])


def map_of(cls):
    return custom_map() if cls["map"] == "custom" else None


def oracle_lab(cls):
    """The oracle's S-CIELAB of the full image, (n, 4)."""
    kind, w, h, seed, _ = cls["image"]

    def make():
        rgba = image(cls)
        lab = c_oracle.srgb_to_scielab(rgba[:, 0].copy(), rgba[:, 1].copy(), rgba[:, 2].copy(), filters(cls), w,
                                       nthreads=_threads())
        lab.setflags(write=False)
        return lab
    return _once(("lab", cls["filters"], kind, w, h, seed), make)


def local_palettes(cls):
    """The palettes whose index images the context holds: hq_eval.hip's palette_slice."""
    R, r, P = cls["opts"]["slice_ranks"], cls["opts"]["slice_rank"], cls["P"]
    return range(P) if R == 1 else range(r * (P // R), (r + 1) * (P // R))


def oracle_outputs(cls, lab=None):
    """What the oracle gives for the class with LabRef `lab` ((n, 4) of the full image; rows
    outside the owned ones are not read; None: the oracle's own).  Per palette p:
    idx[p] (int32, the owned rows), used[p] (K flags: the owned and halo rows' for a shard),
    sum[p] (fp64 sum of the fp32 dE over the owned rows) and cost[p] = mean dE + 2 per
    unused colour for a whole image.  A palette outside the slice: None, zeros, 0.
    The dither class: dither_ref's indices, the oracle's dE of that rendering; the ordered
    class: ordered_ref's indices, the same way.  A masked class: mask_ref's masked mean."""
    _, w, h, _, _ = cls["image"]
    f, rgba, pals, K = filters(cls), image(cls), palettes(cls), cls["K"]
    lab = oracle_lab(cls) if lab is None else np.ascontiguousarray(lab, np.float32).reshape(-1, 4)
    r0, r1 = rows(cls)
    own = slice(r0 * w, r1 * w)
    e0, e1 = max(0, r0 - f.half), min(h, r1 + f.half)
    out = dict(idx=[], used=[], sum=[], cost=[])
    for p in range(cls["P"]):
        pal = pals[p].reshape(K, 4)
        if p not in local_palettes(cls):
            out["idx"].append(None)
            out["used"].append(np.zeros(K, np.int32))
            out["sum"].append(0.0)
            out["cost"].append(None)
            continue
        if cls["op"] in ("dither", "ordered"):
            if cls["op"] == "dither":
                idx, used = dither(rgba, pal, w, h, cls["strength"])
            else:
                idx, used = ordered(rgba[:, :3], pal, w, h, cls["amp"], map_of(cls))
            err = o.ciede76(lab, o.candidate_scielab(idx, pal, f, w, h))
            cost = o.average_array(err) + o.compute_penalty(used, 2.0)
        else:
            cost, parts = c_oracle.eval_palette(rgba, lab, pal, f, w, nthreads=_threads(), return_parts=True)
            idx, used, err = parts["idx"], parts["used"], parts["err"]
            if (r0, r1) != (0, h):  # a colour is used when an owned or halo pixel takes it
                _, used = c_oracle.assign(rgba[e0 * w:e1 * w], pal, nthreads=_threads())
                cost = None
            if cls["mask"] is not None:
                mask = mask_of(cls)
                cost = masked_cost(err, mask, int(np.count_nonzero(mask)), np.count_nonzero(np.asarray(used) == 0), 2.0)
        out["idx"].append(np.asarray(idx, np.int32)[own])
        out["used"].append((np.asarray(used) > 0).astype(np.int32))
        out["sum"].append(float(np.sum(np.asarray(err, np.float32)[own].astype(np.float64))))
        out["cost"].append(cost)
    return out

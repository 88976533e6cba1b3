"""The walk and the class table of tests/reuse_walk.py, on the CPU: the walk uses every
ordered pair of classes once, and each class meets the precondition of the path it is
named after, from the table and the oracle alone."""

import numpy as np
import pytest

import path_ref as pr
import reuse_walk as rw
from mask_ref import live_tiles_brute
from ordered_ref import bayer
from test_fast_path import bucket

ASSIGN_CHUNK = 256 * 6  # hq_eval.hip, assign_blocks: pixels per assign workgroup (HQ_ASSIGN_MINPX 6)
FAST_TILE = {16: (128, 16), 8: (108, 8)}  # option cost_rows -> the fast cost launch's tile (columns, rows)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 12, 13, 15])
def test_walk_uses_every_ordered_pair_once(n):
    walk = rw.euler_walk(n)
    assert len(walk) == n * (n - 1) + 1
    assert walk[0] == walk[-1] == 0
    pairs = list(zip(walk[:-1], walk[1:]))
    assert all(i != j for i, j in pairs)
    assert sorted(pairs) == [(i, j) for i in range(n) for j in range(n) if i != j]
    assert walk == rw.euler_walk(n)  # deterministic


def test_fifteen_classes_make_211_steps():
    assert len(rw.CLASSES) == 15 and len(set(rw.NAMES)) == 15
    assert len(rw.euler_walk(len(rw.CLASSES))) == 15 * 14 + 1 == 211


def tile_states(c):
    """(dead, partly live) tile counts of the class's fast cost launch under its mask, pixel by
    pixel (mask_ref's brute force)."""
    _, w, h, _, _ = c["image"]
    tw, th = FAST_TILE[c["opts"]["cost_rows"]]
    mask = rw.mask_of(c)
    live = live_tiles_brute(mask, w, h, tw, th)
    tx, ty = -(-w // tw), -(-h // th)
    partly = [t for t in live if not mask[t // tx * th:(t // tx + 1) * th, t % tx * tw:(t % tx + 1) * tw].all()]
    return tx * ty - len(live), len(partly)


@pytest.mark.parametrize("name", rw.NAMES)
def test_class_meets_its_path(name):
    c = rw.by_name(name)
    f, (kind, w, h, _, _), (r0, r1) = rw.filters(c), c["image"], rw.rows(c)
    half, P, K, opts = f.half, c["P"], c["K"], c["opts"]
    assert set(opts) == set(rw.OPTION_DEFAULTS)  # every option has an explicit value
    assert half == c["filters"][2] and w >= half and h >= half
    rgb = rw.image(c)[:, :3]
    k = np.rint(rgb.astype(np.float64) * 255).astype(np.float32)
    on_lattice = bool(np.all(k / np.float32(255) == rgb))  # fp32 k/255, as the device packs it
    assert on_lattice == (kind == "lattice")
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0
    pals = rw.palettes(c).reshape(P, K, 4)
    fits = bool(np.all((pals[..., :3] >= rw.FAST_RANGE[0]) & (pals[..., :3] <= rw.FAST_RANGE[1])))
    assert fits == (not c["out_of_range"]) and np.all(pals[..., 3] == 0)
    # several assign workgroups, more than one cost tile (16 x 128), a halo where there is a shard
    e0, e1 = max(0, r0 - half), min(h, r1 + half)
    assert w * (e1 - e0) > ASSIGN_CHUNK and (r1 - r0 > 16 or w > 128)
    assert fits == pr.palette_fits(pals) and rw.FAST_RANGE == pr.FAST_RANGE
    nch = pr.chunks_of(opts, K, fits)  # (the predicates below: tests/path_ref.py)
    path = pr.expected(opts, 0, half, K, P, pal_fits=fits, image_u8=on_lattice,
                       kind="dither" if c["op"] == "dither" else "full", ordered=c["op"] == "ordered")
    want = {
        "u8-fast": bucket(half) == 10 and nch == 1 and opts["cost_variant"] == 0 and opts["pixel_err"] == 1,
        "planar-generic": opts["cost_variant"] == 1 and K <= 256,
        "bucket-19": bucket(half) == 19 and half == 19 and K < 8,
        "long-filter": bucket(half) == 0 and 24 < half <= 64,
        "chunk-grids": nch == 2 and opts["lists16"] == 0 and not pr.uses_lists16(opts, nch)
        and (path["grid"], path["argmin"], path["argmin_cmb"]) == ("build_grid", "assign_pipe", 2),
        "lists16": 4 <= nch <= 32 and opts["lists16"] == 1 and opts["grid"] > 0 and pr.uses_lists16(opts, nch)
        and (path["grid"], path["argmin"]) == ("lists16", "assign16"),
        "wide-u32": K > 16384 and nch == 1 and path["argmin"] == "assign_wide" and path["idx_bytes"] == 4,
        "grid-0": opts["grid"] == 0 and K <= 256,
        "shard": c["op"] == "partial" and r0 - half > 0 and r1 + half < h and r0 % 16 != 0,
        "dither": c["op"] == "dither" and K <= 256 and opts["dither_rows"] == 64 and c["strength"] == 1.0,
        "out-of-range": not fits and K <= 256,
        "slice": c["op"] == "partial" and opts["slice_ranks"] == 2 and P % 2 == 0 and opts["slice_rank"] == 1,
        "ordered": c["op"] == "ordered" and K <= 256 and c["map"] == "custom" and c["amp"] == (0.06, 0.03, 0.0),
        "masked": c["mask"] == (10, 60, 5, 20) and opts["cost_rows"] == 16 and opts["pixel_err"] == 0,
        "masked-8row": c["mask"] == (10, 60, 5, 20) and opts["cost_rows"] == 8,
    }[name]
    assert want, name
    assert (c["map"] is not None) == (name == "ordered") and (c["mask"] is not None) == name.startswith("masked")
    if name == "ordered":
        tmap = rw.map_of(c)
        assert tmap.shape == (4, 8) and tmap.dtype == np.float32 and np.all((tmap >= -0.5) & (tmap <= 0.5))
        assert sorted(np.unique(tmap)) == sorted(tmap.reshape(-1)) and not np.array_equal(tmap, bayer(4)[:4, :8])
    if c["mask"] is not None:
        # the fast path of the 21-tap bucket, where both tile shapes exist; in either shape a tile
        # that is skipped and one that runs with pixels outside the mask
        assert bucket(half) == 10 and nch == 1 and opts["cost_variant"] == 0 and opts["mask_skip"] == 1
        dead, partly = tile_states(c)
        assert dead >= 1 and partly >= 1, (name, dead, partly)
        other = rw.by_name("masked-8row" if name == "masked" else "masked")
        # the step between the two masked classes changes the tile shape and nothing else
        assert {k for k in opts if opts[k] != other["opts"][k]} == {"cost_rows"}
        assert (c["image"], c["filters"], c["lab"], c["mask"]) == tuple(other[k] for k in ("image", "filters", "lab", "mask"))
    if name != "slice":
        assert opts["slice_ranks"] == 1 and list(rw.local_palettes(c)) == list(range(P))
    else:
        assert list(rw.local_palettes(c)) == [2, 3]
    ref = rw.oracle_outputs(c)
    for p in rw.local_palettes(c):
        assert np.isfinite(ref["sum"][p]) and ref["sum"][p] > 0
        assert ref["idx"][p].shape == (w * (r1 - r0),) and ref["idx"][p].max() < K
        if c["op"] != "partial":
            assert np.isfinite(ref["cost"][p])

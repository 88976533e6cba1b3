"""tests/path_ref.py on its own (no GPU): the model of the expected kernel path produces
exactly the instances of DESIGN.md section 4's tables over the option matrices of the GPU
tests that claim to reach them, and every row of the long-filter table from that row's
options."""

import itertools

import pytest

import path_ref as pr
from test_fast_path import BUCKETS, bucket

# test_fast_path_gpu.MATRIX and CHUNKS, restated (importing that module needs the built library)
MATRIX = {"b10-16x128": ((10, 7), {}), "b15-16x128": ((15, 12), {}), "b19-16x128": ((19, 17), {}),
          "b24-16x128": ((24, 21), {}), "b10-16x256": ((10, 7), dict(cost_tw=256)),
          "b10-8x108": ((10, 7), dict(cost_rows=8))}
CHUNKS = {300: 2, 512: 2, 513: 4, 1100: 8, 2100: 16, 4200: 32, 8192: 32}


def design_table_fast_instances():
    """The 66 instances of "Fast-path dispatch and its tests", row by row."""
    rows = [("cost16w", hb, de, trim, 4, 1) for hb in BUCKETS for de in range(3) for trim in (0, 1)]  # 24
    rows += [("cost16w", 10, de, trim, 8, 1) for de in range(3) for trim in (0, 1)]                   # 6
    rows += [("cost_mfma", 10, de, trim, 4, 1) for de in range(3) for trim in (0, 1)]                 # 6
    rows += [("cost16w", 10, de, trim, 4, nch) for nch in (2, 4, 8, 16, 32) for de in range(3) for trim in (0, 1)]
    return rows


def fast_matrix():
    """(options, dE, half, K) of every evaluation of test_instance_matrix and
    test_chunked_cost_matrix that is meant to run a fast kernel."""
    for (halves, fopts), de, trim in itertools.product(MATRIX.values(), range(3), (1, 0)):
        for half, K in itertools.product(halves, (64, 256)):
            yield dict(fopts, trim=trim), de, half, K
    for K, de, trim in itertools.product(CHUNKS, range(3), (1, 0)):
        for lists16 in (0, 1 if CHUNKS[K] >= 4 else 2):
            yield dict(trim=trim, lists16=lists16), de, 10, K


def test_fast_matrix_gives_exactly_the_66_instances():
    table = design_table_fast_instances()
    assert len(table) == len(set(table)) == 66
    got = set()
    for opts, de, half, K in fast_matrix():
        e = pr.expected(opts, de, half, K)
        assert e["why_not_fast"] == frozenset() and pr.fast_instance(e) is not None, (opts, de, half, K)
        assert e["nch"] == CHUNKS.get(K, 1)
        got.add(pr.fast_instance(e))
    assert got == set(table)


def test_chunked_matrix_argmin_forms():
    """test_chunked_cost_matrix runs both argmin forms at every chunk count: the per-chunk grids
    with CMB = 2 / 4 and nch / 4 passes, and the 16-bit lists."""
    for K, nch in CHUNKS.items():
        a = pr.expected(dict(lists16=0), 0, 10, K)
        assert (a["grid"], a["argmin"], a["argmin_cmb"], a["argmin_passes"], a["idx_bytes"]) == \
            ("build_grid", "assign_pipe", min(nch, 4), max(nch // 4, 1), 2)
        b = pr.expected(dict(lists16=1 if nch >= 4 else 2), 0, 10, K)
        assert (b["grid"], b["argmin"], b["idx_bytes"]) == ("lists16", "assign16", 2)
    # the default keeps 2 chunks on the per-chunk grids
    assert pr.expected({}, 0, 10, 300)["argmin"] == "assign_pipe"


# "Long-filter dispatch and its tests", row by row: (half, options, K, palette fits) -> the pair
LONG_ROWS = [
    (24, {}, 64, True, None),  # the fast path
    (24, dict(cost_variant=1), 64, True, (("gen_hmfma", 1), ("gen_vmfma", 64))),
    (25, {}, 64, True, (("gen_hmfma", 1), ("gen_vmfma", 64))),
    (64, dict(gen_tile_shape=1), 64, True, (("gen_hmfma", 1), ("gen_vmfma", 64))),
    (64, dict(gen_tile_shape=2), 64, True, (("gen_hmfma", 4), ("gen_vmfma", 128))),
    (51, dict(gen_hmfma=0), 64, True, (("gen_hrow4", 1, 4), ("gen_vmfma", 64))),
    (51, dict(gen_hmfma=0, gen_hrow_outputs=8), 64, True, (("gen_hrow4", 1, 8), ("gen_vmfma", 64))),
    (51, dict(gen_hmfma=0, gen_tile_shape=2), 64, True, (("gen_hrow4", 1, 4), ("gen_vmfma", 128))),
    (51, dict(gen_vmfma=0), 64, True, (("gen_hrow4", 0, 4), ("gen_vtile2",))),
    (51, dict(gen_vmfma=0, gen_hrow_outputs=8), 64, True, (("gen_hrow4", 0, 8), ("gen_vtile2",))),
    (51, {}, 64, False, (("gen_hrow4", 0, 4), ("gen_vtile2",))),  # a palette outside the fast range
    (51, dict(gen_vmfma=0, gen_hrow4=0), 64, True, (("gen_hrow",), ("gen_vtile2",))),
    (51, dict(gen_vmfma=0, gen_vtile2=0), 64, True, (("gen_hrow4", 0, 4), ("gen_vtile",))),
    (51, dict(gen_vmfma=0, gen_vtile2=0, gen_hrow4=0), 64, True, (("gen_hrow",), ("gen_vtile",))),
    (65, {}, 64, True, (("gen_hrow4", 0, 4), ("gen_vtile",))),
    (96, dict(gen_hrow_outputs=8), 64, True, (("gen_hrow4", 0, 8), ("gen_vtile",))),
    (127, dict(gen_hrow4=0), 64, True, (("gen_hrow",), ("gen_vtile",))),
    (127, dict(cost_variant=2), 64, True, (("gen_hpass",), ("gen_vpass",))),
    (10, dict(cost_variant=2), 64, True, (("gen_hpass",), ("gen_vpass",))),
]


@pytest.mark.parametrize("row", range(len(LONG_ROWS)))
def test_long_filter_table_rows(row):
    half, opts, K, fits, pair = LONG_ROWS[row]
    e = pr.expected(opts, 0, half, K, pal_fits=fits)
    assert pr.generic_pair(e) == pair
    if pair is None:
        assert pr.fast_instance(e) == ("cost16w", 24, 0, 1, 4, 1)
    else:
        want = {"half"} if half > 24 else set()
        want |= {"cost_variant"} if opts.get("cost_variant") else set()
        want |= set() if fits else {"palette"}
        assert e["why_not_fast"] == frozenset(want)
        assert e["cost"] == ("pixel_generic" if opts.get("cost_variant") == 2 else "tiled_generic")
    assert e["idx_bytes"] == 1


def test_long_filter_index_widths():
    """The table's H = 51 row: u16 for chunked palettes (per-chunk grids at K = 300, lists16 at
    600), u32 for chunked 0 and K = 16500."""
    for opts, K, width, argmin in (({}, 300, 2, "assign_pipe"), ({}, 600, 2, "assign16"),
                                   (dict(chunked=0), 300, 4, "assign_wide"), ({}, 16500, 4, "assign_wide")):
        e = pr.expected(opts, 0, 51, K, 2)
        assert (e["idx_bytes"], e["argmin"], e["P"]) == (width, argmin, 2)
        assert pr.generic_pair(e) == (("gen_hmfma", 1), ("gen_vmfma", 64))
        assert ("wide" in e["why_not_fast"]) == (width == 4) and "half" in e["why_not_fast"]


def test_boundaries_of_the_model():
    ex = pr.expected
    assert [pr.chunks_of({}, K) for K in (256, 257, 512, 513, 8192, 8193, 16384, 16385)] == [1, 2, 2, 4, 32, 64, 64, 1]
    assert ex({}, 0, 10, 8193)["why_not_fast"] == {"nch"} and ex({}, 0, 10, 8193)["argmin_passes"] == 16
    assert ex({}, 0, 10, 16385)["why_not_fast"] == {"wide"}
    assert ex(dict(grid=0), 0, 10, 600)["argmin"] == "assign_wide" and ex(dict(grid=0), 0, 10, 16)["grid"] == "none"
    for o in (dict(cost_rows=8), dict(cost_tw=256)):
        assert ex(o, 0, 10, 300)["why_not_fast"] == {"chunk_form"}
    assert ex({}, 0, 15, 300)["why_not_fast"] == {"chunk_form"} and ex({}, 0, 25, 300)["why_not_fast"] == {"half"}
    assert ex({}, 0, 10, 16, taps_fit=False)["why_not_fast"] == {"taps"}
    assert pr.generic_pair(ex({}, 0, 10, 16, taps_fit=False)) == (("gen_hrow4", 0, 4), ("gen_vtile2",))
    assert ex({}, 0, 10, 16, trim_ok=False)["cost_trim"] == 0
    assert ex({}, 0, 10, 16, image_u8=False)["pixels"] == "planar" and ex(dict(img_u8=0), 0, 10, 16)["pixels"] == "planar"
    assert [bucket(h) for h in (10, 11, 24, 25)] == [10, 15, 24, 0]
    # the search
    sd = pr.search_device
    assert sd({}, 64, 16) and not sd({}, 65, 16) and sd({}, 8, 16384) and not sd({}, 9, 16384)
    assert sd({}, 2, 16384) and not sd({}, 2, 16385) and not sd(dict(grid=0), 2, 600) and sd(dict(grid=0), 2, 16)
    assert not sd(dict(sa_device=0), 2, 16) and not sd(dict(chunked=0), 2, 600)

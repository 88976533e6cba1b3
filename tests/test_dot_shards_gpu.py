"""GPU tests of dot diffusion on row-block shards (hq_dot_population_partial, option "dot_apron",
hq_dot_apron): a shard that holds the class matrix's reach in rows around its extended rows
renders the whole image's indices for its rows bit for bit, with no exchange; the shards'
partials add up to the whole image's at test_ordered_gpu.py's bar for the same identity (1e-6)
and their used flags OR to it.  The image is 53 x 61 at half-width 10, so the shard boundaries
below are no multiples of any matrix side and the extended rows reach well past the owned ones.
"""

import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import hybridquantization_amd as hq
import oracle as o
from dot_ref import KNUTH8, dot, random_classes
from hybridquantization_amd import _lib
from test_dither_gpu import _sums_and_errors, new_ctx, noise, pals_of

pytestmark = pytest.mark.gpu

W, H, K, P, HALF = 53, 61, 16, 3, 10
PERM4 = random_classes(4, 44)  # reaches (7, 5): further than its side
ROWMAJOR16 = np.arange(256, dtype=np.int32).reshape(16, 16)  # reaches (15, 1)
# name -> (matrix, reach, the shards' owned rows).  Knuth's: a middle shard whose extended rows
# start at row 3, so the apron above is clipped to 3 rows, and first and last shards clipped to
# none; the 4 x 4 one: a middle shard of 6 rows, shorter than reach + half; the 16 x 16 one: two
# shards, the second needing 15 rows above and none below.
CASES = {"knuth8": (None, (5, 5), ((0, 13), (13, 30), (30, H))),
         "perm4": (PERM4, (7, 5), ((0, 21), (21, 27), (27, H))),
         "rowmajor16": (ROWMAJOR16, (15, 1), ((0, 27), (27, H)))}
_REF = {}


def image():
    if "rgba" not in _REF:
        _REF["rgba"], _REF["pals"] = noise(W, H, 61), pals_of(K, 16)
    return _REF["rgba"], _REF["pals"]


def ref_of(name, s):
    """The restatement's indices and used flags of the whole image, per palette; read-only."""
    if (name, s) not in _REF:
        rgba, pals = image()
        _REF[name, s] = [dot(rgba, pals[p].reshape(K, 4), W, H, s, CASES[name][0]) for p in range(P)]
    return _REF[name, s]


def extended(r0, r1):
    return max(0, r0 - HALF), min(H, r1 + HALF)


def held(r0, r1, apron):
    e0, e1 = extended(r0, r1)
    return min(apron, e0), min(apron, H - e1)


def set_shard(m, rgba, r0, r1):
    m.setImage(rgba.reshape(-1), None, W, m.illum, row_begin=r0, row_end=r1)


def owned(m, p, r0, r1):
    return m.getIndices(p)[:(r1 - r0) * W]  # (the owned rows come first in the full-size buffer)


def raw_partial(m, pals, s, cls=None, Pn=None, Kn=None):
    """hq_dot_population_partial with sentinel outputs -> (status, partial)."""
    Pn = pals.shape[0] if Pn is None else Pn
    Kn = pals.shape[1] // 4 if Kn is None else Kn
    part = np.full((max(Pn, 1), 1 + max(Kn, 1)), -7.0, np.float64)
    mat = None if cls is None else m._classes(cls)
    rc = hq.load().hq_dot_population_partial(m.ctx, _lib.fptr(pals), Pn, Kn, None if mat is None else C.byref(mat),
                                             s, _lib.dptr(part))
    return rc, part


def eval_partial(m, pals):
    part = np.zeros((pals.shape[0], 1 + pals.shape[1] // 4), np.float64)
    _lib.check(hq.load().hq_eval_population_partial(m.ctx, _lib.fptr(pals), pals.shape[0], pals.shape[1] // 4,
                                                    _lib.dptr(part)), m.ctx)
    return part


def assert_adds_up(parts, whole, msg):
    for p in range(whole.shape[0]):
        s = sum(part[p, 0] for part in parts)
        print(f"{msg} p={p}: shards {s!r}, whole {whole[p, 0]!r}")
        assert abs(s - whole[p, 0]) <= 1e-6 * whole[p, 0], f"{msg} p={p}"
        flags = np.zeros(whole.shape[1] - 1, bool)
        for part in parts:
            flags |= part[p, 1:] != 0
        np.testing.assert_array_equal(flags, whole[p, 1:] != 0, err_msg=f"{msg} p={p}")


# ---------------------------------------------------------------------------
# 1. Shards against the whole image
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_shards_render_the_whole_images_rows_and_add_up(gpu, name):
    cls, reach, shards = CASES[name]
    rgba, pals = image()
    assert hq.ImageManipulation.dotReach(cls) == reach
    m = new_ctx(gpu, dot_apron=max(reach))
    try:
        for s in (1.0, 0.5):
            ref = ref_of(name, s)
            m.setImage(rgba.reshape(-1), None, W, m.illum)
            assert m.dotApron() == (0, 0)
            whole = m.dotPopulationPartial(pals, s, classes=cls)
            for p in range(P):
                np.testing.assert_array_equal(m.getIndices(p), ref[p][0].astype(np.uint8), err_msg=f"whole p={p}")
                np.testing.assert_array_equal(whole[p, 1:] != 0, ref[p][1] != 0)
            parts = []
            for r0, r1 in shards:
                set_shard(m, rgba, r0, r1)
                assert m.dotApron() == held(r0, r1, max(reach))
                parts.append(m.dotPopulationPartial(pals, s, classes=cls))
                assert m.lastPath()["argmin"] == "dot"
                for p in range(P):
                    np.testing.assert_array_equal(owned(m, p, r0, r1), ref[p][0][r0 * W:r1 * W].astype(np.uint8),
                                                  err_msg=f"{name} s={s} rows [{r0}, {r1}) p={p}")
            assert_adds_up(parts, whole, f"{name} s={s}")
    finally:
        m.close()


def test_the_used_flags_are_those_of_the_extended_rows(gpu):
    """... as hq_eval_population_partial's are: the colours of the whole image's indices on
    [e0, e1), and none that only an apron row takes."""
    rgba, pals = image()
    ref = ref_of("knuth8", 1.0)
    m = new_ctx(gpu, dot_apron=5)
    try:
        r0, r1 = 24, 36
        e0, e1 = extended(r0, r1)
        set_shard(m, rgba, r0, r1)
        part = m.dotPopulationPartial(pals, 1.0)
        for p in range(P):
            want = np.bincount(ref[p][0][e0 * W:e1 * W], minlength=K) > 0
            np.testing.assert_array_equal(part[p, 1:] != 0, want)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 2. The whole image, strength 0, the state afterwards
# ---------------------------------------------------------------------------
def test_on_a_whole_image_it_is_hq_dot_population(gpu):
    rgba, pals = image()
    m = new_ctx(gpu, pixel_err=1, dot_apron=200)  # (a whole image ignores the option)
    try:
        m.setImage(rgba.reshape(-1), None, W, m.illum)
        assert m.dotApron() == (0, 0)
        for cls in (None, PERM4):
            costs, used = m.dotPopulation(pals, 0.75, 2.0, classes=cls, return_used=True)
            idx = [m.getIndices(p) for p in range(P)]
            err = [m.getPixelErrors(p) for p in range(P)]
            part = m.dotPopulationPartial(pals, 0.75, classes=cls)
            for p in range(P):
                np.testing.assert_array_equal(m.getIndices(p), idx[p])
                np.testing.assert_array_equal(m.getPixelErrors(p).view(np.uint32), err[p].view(np.uint32))
                np.testing.assert_array_equal(part[p, 1:] != 0, used[p] != 0)
                # hq_eval_population's last step on the partial: bit for bit
                cost = part[p, 0] / float(W * H) + 2.0 * np.count_nonzero(part[p, 1:] == 0)
                assert cost == costs[p], (cost, costs[p])
    finally:
        m.close()


def test_strength_zero_on_a_shard_is_the_plain_partial(gpu):
    rgba, pals = image()
    m = new_ctx(gpu, pixel_err=1, dot_apron=7)
    try:
        for r0, r1 in ((0, 21), (21, 27), (27, H)):
            set_shard(m, rgba, r0, r1)
            plain = eval_partial(m, pals)
            idx = [m.getIndices(p) for p in range(P)]
            err = [m.getPixelErrors(p) for p in range(P)]
            for cls in (None, PERM4):
                part = m.dotPopulationPartial(pals, 0.0, classes=cls)
                np.testing.assert_array_equal(part.view(np.uint64), plain.view(np.uint64))
                for p in range(P):
                    np.testing.assert_array_equal(m.getIndices(p), idx[p])
                    np.testing.assert_array_equal(m.getPixelErrors(p).view(np.uint32), err[p].view(np.uint32))
    finally:
        m.close()


def test_state_after_a_call_on_a_shard(gpu):
    """The getters answer for the dot-diffused owned rows: the stored errors sum to the partial;
    clusterSums and clusterErrors give HQ_ERR_STATE until the next plain evaluation."""
    rgba, pals = image()
    m = new_ctx(gpu, pixel_err=1, dot_apron=5)
    try:
        r0, r1 = 13, 30
        set_shard(m, rgba, r0, r1)
        part = m.dotPopulationPartial(pals, 1.0)
        for p in range(P):
            e = m.getPixelErrors(p)[:(r1 - r0) * W].astype(np.float64)
            assert np.isfinite(e).all() and abs(e.sum() - part[p, 0]) <= 1e-5 * part[p, 0]
            np.testing.assert_array_equal(m.getIndices32(p)[:(r1 - r0) * W], owned(m, p, r0, r1).astype(np.uint32))
        assert list(_sums_and_errors(m, P, K)[:2]) == [_lib.HQ_ERR_STATE, _lib.HQ_ERR_STATE]
        eval_partial(m, pals)
        assert _sums_and_errors(m, P, K)[0] == _lib.HQ_OK
        again = m.dotPopulationPartial(pals, 1.0)
        np.testing.assert_array_equal(again.view(np.uint64), part.view(np.uint64))
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 3. The option, the getter, the refusals
# ---------------------------------------------------------------------------
def test_the_apron_held_decides(gpu):
    rgba, pals = image()
    lib = hq.load()
    m = new_ctx(gpu)
    try:
        def refused(status, cls=None, pl=pals, s=1.0, **kw):
            path = m.lastPath()
            idx = [m.getIndices(p) for p in range(P)]
            rc, part = raw_partial(m, pl, s, cls, **kw)
            msg = lib.hq_last_error(m.ctx).decode()
            assert rc == status, (rc, msg)
            assert np.all(part == -7.0)
            assert m.lastPath() == path
            for p in range(P):
                np.testing.assert_array_equal(m.getIndices(p), idx[p])
            return msg

        # an interior shard: 16 rows of the image on each side of its extended rows [16, 45)
        r0, r1 = 26, 35
        for apron, cls, ok in ((0, None, False), (4, None, False), (5, None, True), (14, ROWMAJOR16, False),
                               (14, ROWMAJOR16[::-1], False), (15, ROWMAJOR16, True), (15, ROWMAJOR16[::-1], True),
                               (1, ROWMAJOR16, False), (255, PERM4, True)):
            m.setOption("dot_apron", apron)
            set_shard(m, rgba, r0, r1)
            assert m.dotApron() == held(r0, r1, apron) == (min(apron, 16), min(apron, 16))
            eval_partial(m, pals)
            if ok:
                rc, part = raw_partial(m, pals, 1.0, cls)
                assert rc == _lib.HQ_OK and np.all(part[:, 0] > 0)
            else:
                msg = refused(_lib.HQ_ERR_STATE, cls)
                assert "needed" in msg and "held" in msg and f"{apron} and {apron}" in msg, msg
        # 14 rows held: enough above for the flipped matrix (1, 15) only on that side, and the reverse
        m.setOption("dot_apron", 14)
        set_shard(m, rgba, r0, r1)
        eval_partial(m, pals)
        assert "15 and 1 rows are needed" in refused(_lib.HQ_ERR_STATE, ROWMAJOR16)
        assert "1 and 15 rows are needed" in refused(_lib.HQ_ERR_STATE, ROWMAJOR16[::-1])
        # the option is read when the shard is set: changing it later changes nothing held
        m.setOption("dot_apron", 5)
        set_shard(m, rgba, 13, 30)
        assert m.dotApron() == (3, 5)
        m.setOption("dot_apron", 0)
        assert m.dotApron() == (3, 5)
        assert raw_partial(m, pals, 1.0)[0] == _lib.HQ_OK
        set_shard(m, rgba, 13, 30)  # ... and the next image has the apron of the option then in force
        assert m.dotApron() == (0, 0)
        eval_partial(m, pals)
        refused(_lib.HQ_ERR_STATE)
        for bad in (-1, 256):
            with pytest.raises(Exception):
                m.setOption("dot_apron", bad)
        a, b = C.c_int(-7), C.c_int(-7)
        assert lib.hq_dot_apron(m.ctx, None, C.byref(b)) == _lib.HQ_ERR_ARG
        assert lib.hq_dot_apron(None, C.byref(a), C.byref(b)) == _lib.HQ_ERR_ARG

        # hq_dot_population's other refusals, on a shard that holds enough
        m.setOption("dot_apron", 7)
        set_shard(m, rgba, 13, 30)
        eval_partial(m, pals)
        for name in ("palette_split", "slice_ranks"):
            m.setOption(name, 1 if name == "palette_split" else 2)
            refused(_lib.HQ_ERR_UNSUPPORTED)
            m.setOption(name, 0 if name == "palette_split" else 1)
        refused(_lib.HQ_ERR_UNSUPPORTED, pl=pals_of(257, 1))  # K > 256
        refused(_lib.HQ_ERR_ARG, Pn=0)
        refused(_lib.HQ_ERR_ARG, Kn=0)
        for s in (-0.001, 1.001, float("nan")):
            refused(_lib.HQ_ERR_ARG, s=s)
        bad = pals.copy()
        bad.reshape(-1)[5] = 1.001
        refused(_lib.HQ_ERR_ARG, pl=bad)
        rep = KNUTH8.copy()
        rep[0, 0] = rep[7, 7]
        refused(_lib.HQ_ERR_ARG, rep)
        assert lib.hq_dot_population_partial(m.ctx, _lib.fptr(pals), P, K, None, 1.0, None) == _lib.HQ_ERR_ARG
        # hq_dot_population itself still refuses the shard
        costs, used = np.full(P, -7.0), np.full((P, K), -7, np.int32)
        assert lib.hq_dot_population(m.ctx, _lib.fptr(pals), P, K, None, 1.0, 2.0, _lib.dptr(costs),
                                     _lib.iptr(used)) == _lib.HQ_ERR_STATE
        assert np.all(costs == -7.0) and np.all(used == -7)
        assert raw_partial(m, pals, 1.0)[0] == _lib.HQ_OK
    finally:
        m.close()


@pytest.mark.parametrize("planar", [False, True])
def test_an_out_of_range_pixel_in_a_held_row_is_refused(gpu, planar):
    """Rows [24, 36): extended rows [14, 46), apron rows [9, 14) and [46, 51).  1.5 in an apron row
    only, or in an extended row outside the owned ones, is refused as the whole image refuses
    it; in a row the shard does not hold it is not the shard's to see."""
    rgba, pals = image()
    if planar:
        rgba = rgba * np.float32(0.999)  # (no k/255 image: the range flag is found on the device)
    m = new_ctx(gpu, dot_apron=5)
    try:
        r0, r1 = 24, 36
        for row, shard_ok in ((10, False), (48, False), (16, False), (40, False), (3, True), (55, True)):
            img = rgba.copy()
            img[row * W + 7, 1] = 1.5
            m.setImage(img.reshape(-1), None, W, m.illum)
            rc, part = raw_partial(m, pals, 1.0)
            assert rc == _lib.HQ_ERR_UNSUPPORTED and np.all(part == -7.0), row
            set_shard(m, img, r0, r1)
            assert m.dotApron() == (5, 5)
            rc, part = raw_partial(m, pals, 1.0)
            assert rc == (_lib.HQ_OK if shard_ok else _lib.HQ_ERR_UNSUPPORTED), (row, rc)
            assert shard_ok or np.all(part == -7.0)
            rc, part = raw_partial(m, pals, 1.0)  # (the remembered answer)
            assert rc == (_lib.HQ_OK if shard_ok else _lib.HQ_ERR_UNSUPPORTED), (row, rc)
        set_shard(m, rgba, r0, r1)
        assert raw_partial(m, pals, 1.0)[0] == _lib.HQ_OK
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 4. Mask and weights
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mask", "weights"])
def test_masked_and_weighted_partials_add_up(gpu, kind):
    rgba, pals = image()
    rng = np.random.default_rng(5)
    if kind == "mask":
        field = (rng.random((H, W)) < 0.4).astype(np.uint8)
        field[20:28] = 0  # (whole rows out, a shard boundary among them)
    else:
        field = rng.integers(0, 256, (H, W)).astype(np.uint8)
        field[:, 10:20] = 0

    def put(m):
        (m.setMask if kind == "mask" else m.setWeights)(field)

    ref = ref_of("knuth8", 1.0)
    m = new_ctx(gpu, dot_apron=5)
    try:
        m.setImage(rgba.reshape(-1), None, W, m.illum)
        plain = m.dotPopulationPartial(pals, 1.0)
        put(m)
        whole = m.dotPopulationPartial(pals, 1.0)
        assert np.all(whole[:, 0] > 0) and np.all(whole[:, 0] != plain[:, 0])
        np.testing.assert_array_equal(whole[:, 1:], plain[:, 1:])
        parts = []
        for r0, r1 in CASES["knuth8"][2]:
            set_shard(m, rgba, r0, r1)
            put(m)
            parts.append(m.dotPopulationPartial(pals, 1.0))
            for p in range(P):
                np.testing.assert_array_equal(owned(m, p, r0, r1), ref[p][0][r0 * W:r1 * W].astype(np.uint8))
        assert_adds_up(parts, whole, kind)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 5. Two processes, the partials all-reduced over gloo
# ---------------------------------------------------------------------------
def _worker(rank, world, port, out):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle"), os.path.join(root, "tests")]
    import torch.distributed as dist

    import hybridquantization_amd as hqm
    from hybridquantization_amd import dist as hqd

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    R, G, B = o.synthetic_image(W, H, 61)
    pals = pals_of(K, 16)
    r0, r1 = hqd.shard_rows(H, world, rank)
    m = hqm.ImageManipulation(device=0)
    sp = hqm.ScielabProcessor(72, 45.0, hqm.Whitepoint.D65, None, m)
    m.setOption("dot_apron", 5)
    lib = hqm.load()
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), W, H,
                                             _lib.fptr(sp.illuminant), r0, r1), m.ctx)
    part = np.zeros(P * (1 + K))
    _lib.check(lib.hq_dot_population_partial(m.ctx, _lib.fptr(pals), P, K, None, 1.0, _lib.dptr(part)), m.ctx)
    idx = np.zeros((P, (r1 - r0) * W), np.uint8)
    for p in range(P):
        _lib.check(lib.hq_get_indices(m.ctx, p, idx[p].ctypes.data_as(_lib._u8)), m.ctx)
    total = hqd.allreduce_partials(dist, part)
    m.close()
    out.put((rank, total, (r0, r1), idx))
    dist.barrier()
    dist.destroy_process_group()


def test_two_process_shards_allreduce_to_the_whole(gpu):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=100) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[2] for r in res] == [(0, H // 2), (H // 2, H)]
    np.testing.assert_array_equal(res[0][1], res[1][1])
    total = res[0][1].reshape(P, 1 + K)
    rgba, pals = image()
    m = new_ctx(gpu)
    try:
        m.setImage(rgba.reshape(-1), None, W, m.illum)
        whole = m.dotPopulationPartial(pals, 1.0)
        assert_adds_up([total], whole, "two processes")
        for p in range(P):
            both = np.concatenate([res[0][3][p], res[1][3][p]])
            np.testing.assert_array_equal(both, m.getIndices(p))
    finally:
        m.close()

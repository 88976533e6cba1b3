"""GPU tests of hq_set_image_reduced and hq_get_image (libhq's addition: the image pyramid of
the coarse-to-fine search).  The reduced image is read back and compared bit for bit with
tests/reduce_ref.py's numpy restatement of the two arithmetic forms; the context that received
it is held, bit for bit, to a fresh context given the restated image through hq_set_image.
Caller-supplied 3-tap filters (halfSize 1) make the tiny images legal.  Nothing asserts a time.
"""

import numpy as np
import pytest

import hybridquantization_amd as hq
import path_ref as pr
import reduce_ref as rr
from hybridquantization_amd import _lib

pytestmark = pytest.mark.gpu

ILLUM = np.array([0.95047, 1.0, 1.0883], np.float32)
# (w, h, f): odd sizes; rows that do not start 16-byte aligned with a partial last block
# (130 x 9); a single output column (5 x 9 at 16); f = 1
SHAPES = [(13, 7, 2), (10, 11, 3), (16, 16, 4), (130, 9, 2), (130, 9, 4), (5, 9, 16), (11, 6, 1)]
# the block sizes n whose sums must land exactly on a half in the byte image
TIES = {(13, 7, 2): {4, 2}, (10, 11, 3): {6, 2}, (16, 16, 4): {16}, (130, 9, 2): {4, 2}, (130, 9, 4): {16, 8, 4, 2},
        (5, 9, 16): set(), (11, 6, 1): set()}
P, K, DELTA = 3, 8, 2.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def short_filters():
    """3 taps per filter (halfSize 1), positive and negative, nothing designed."""
    k1 = [np.array(t, np.float32) for t in ([0.2, 0.6, 0.2], [0.25, 0.5, 0.25], [0.1, 0.8, 0.1])]
    k2 = [np.array(t, np.float32) for t in ([0.3, 0.4, 0.3], [0.33, 0.34, 0.33], [0.2, 0.6, 0.2])]
    k3 = np.array([-0.05, 0.1, -0.05], np.float32)
    return [[k1[0], k2[0], k3], [k1[1], k2[1]], [k1[2], k2[2]]], np.abs(k3)


def new_ctx(gpu):
    m = pr.Context(hq.deltaETypes.CIE76, device=gpu)
    m.updateOpenCLFilters(*short_filters())
    assert m.halfSize == 1
    return m


@pytest.fixture()
def ctxs(gpu):
    made = []

    def make():
        made.append(new_ctx(gpu))
        return made[-1]

    yield make
    for m in made:
        m.close()


def byte_image(w, h, f, seed):
    """Random bytes (h w, 3); in the red channel every second block is rewritten so that its
    sum lands exactly on a half (n even: n / 2 pixels of k + 1, the rest k) or as near to one
    as an odd n allows (sums n k + (n - 1) / 2 and n k + (n + 1) / 2 by turns)."""
    rng = np.random.default_rng(seed)
    by = rng.integers(0, 256, (h, w, 3))
    for i, (X, Y, x0, x1, y0, y1) in enumerate(rr.blocks(w, h, f)):
        if (X + Y) % 2:
            continue
        n = (x1 - x0) * (y1 - y0)
        k = int(rng.integers(0, 255))
        ones = n // 2 if n % 2 == 0 else (n - 1) // 2 + i % 2
        blk = np.full(n, k)
        blk[rng.permutation(n)[:ones]] += 1
        by[y0:y1, x0:x1, 0] = blk.reshape(y1 - y0, x1 - x0)
    return by.reshape(-1, 3)


def tie_sizes(by, w, h, f):
    """The block sizes n for which some block's red sum s has 2 s = n (mod 2 n): mean k + 0.5."""
    m = np.asarray(by).reshape(h, w, 3)
    out = set()
    for _, _, x0, x1, y0, y1 in rr.blocks(w, h, f):
        n, s = (x1 - x0) * (y1 - y0), int(m[y0:y1, x0:x1, 0].sum())
        if (2 * s) % (2 * n) == n:
            out.add(n)
    return out


def source_image(form, w, h, f):
    rgba = np.zeros((w * h, 4), np.float32)
    if form == "u8":
        by = byte_image(w, h, f, seed=w * 100 + f)
        assert TIES[(w, h, f)] <= tie_sizes(by, w, h, f)
        rgba[:, :3] = rr.unit(by)
        return rgba, rr.reduce_u8(rgba, w, h, f)
    rng = np.random.default_rng(w * 100 + f + 1)
    rgba[:, :3] = rng.random((w * h, 3), dtype=np.float32)
    rgba[0, 0], rgba[1, 1] = 0.0, 1.0
    return rgba, rr.reduce_planar(rgba, w, h, f)


def palettes(seed=5):
    rng = np.random.default_rng(seed)
    pal = np.zeros((P, K, 4), np.float32)
    pal[:, :, :3] = rng.random((P, K, 3), dtype=np.float32)
    return pal.reshape(P, 4 * K)


def snapshot(m, with_sums=True):
    """Everything an evaluation of the small population leaves readable on `m`, as bits."""
    m.setOption("pixel_err", 1)
    costs, used = m.computeQuantizationErrorPopulation(palettes(), DELTA, return_used=True)
    out = {"costs": costs.view(np.uint64).copy(), "used": used.copy(), "path": m.lastPath()["pixels"]}
    out.update(readback(m))
    if with_sums:
        sums, den = m.clusterSums(P, K)
        out["sums"], out["den"] = sums, den
    return out


def readback(m):
    return {"idx": np.stack([m.getIndices(p) for p in range(P)]),
            "err": np.stack([bits(m.getPixelErrors(p)) for p in range(P)])}


def assert_same(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label}: {k}")
        else:
            assert a[k] == b[k], (label, k, a[k], b[k])


@pytest.mark.parametrize("form", ["u8", "planar"])
@pytest.mark.parametrize("w,h,f", SHAPES)
def test_reduced_image_and_the_context_that_holds_it(ctxs, form, w, h, f):
    rgba, want = source_image(form, w, h, f)
    rw, rh = rr.reduced_size(w, h, f)
    src, dst, fresh = ctxs(), ctxs(), ctxs()
    src.setImage(rgba.reshape(-1), None, w, ILLUM)
    before = snapshot(src, with_sums=False)
    assert before["path"] == form

    dst.setImageReduced(src, f)
    assert (dst.w, dst.h) == (rw, rh)
    # 1. the image, bit for bit the restatement (f = 1: the source itself)
    got = dst.getImage().reshape(-1, 4)
    np.testing.assert_array_equal(bits(got), bits(want))
    if f == 1:
        np.testing.assert_array_equal(bits(got), bits(rgba))
    # 2. src: what its getters still read, and a new evaluation, are the same bits
    assert_same(readback(src), {k: before[k] for k in ("idx", "err")}, "src's getters after the call")
    assert_same(snapshot(src, with_sums=False), before, "src evaluated again")
    np.testing.assert_array_equal(bits(src.getImage()), bits(rgba.reshape(-1)))
    # 3. dst against a fresh context given the restated image through hq_set_image
    fresh.setImage(want.reshape(-1), None, rw, ILLUM)
    np.testing.assert_array_equal(bits(dst.getLabRef()), bits(fresh.getLabRef()))
    got_eval, want_eval = snapshot(dst), snapshot(fresh)
    assert got_eval["path"] == form  # the packed source gives a packed image, the planar one a planar image
    assert_same(got_eval, want_eval, "dst against a fresh context")
    assert got_eval["den"] == (255 if form == "u8" else 1 << 32)


def test_illuminant_is_the_sources_unless_given(ctxs):
    rgba, want = source_image("u8", 13, 7, 2)
    other = np.array([0.966797, 1.0, 0.825188], np.float32)
    src, dst, fresh = ctxs(), ctxs(), ctxs()
    src.setImage(rgba.reshape(-1), None, 13, other)
    dst.setImageReduced(src, 2)  # src's D50, not dst's default
    fresh.setImage(want.reshape(-1), None, 7, other)
    np.testing.assert_array_equal(bits(dst.getLabRef()), bits(fresh.getLabRef()))
    dst.setImageReduced(src, 2, ILLUM)
    fresh.setImage(want.reshape(-1), None, 7, ILLUM)
    np.testing.assert_array_equal(bits(dst.getLabRef()), bits(fresh.getLabRef()))


def test_mask_and_weights_are_dropped_and_dst_is_reusable(ctxs):
    """dst held a larger image under weights; the reduction drops them, and afterwards dst takes
    a plain hq_set_image and equals a fresh context."""
    rgba, want = source_image("u8", 130, 9, 4)
    big, _ = source_image("planar", 16, 16, 4)
    src, dst, fresh = ctxs(), ctxs(), ctxs()
    src.setImage(rgba.reshape(-1), None, 130, ILLUM)
    dst.setImage(big.reshape(-1), None, 16, ILLUM)
    dst.setWeights(np.arange(256, dtype=np.uint8).reshape(16, 16))
    snapshot(dst)
    dst.setImageReduced(src, 4)
    with pytest.raises(hq.HQError):  # the record of the last evaluation went with the old image
        dst.getIndices(0)
    assert dst.weightsInfo() == (33 * 3, 33 * 3) and dst.maskInfo()[:2] == (33 * 3, 33 * 3)
    fresh.setImage(want.reshape(-1), None, 33, ILLUM)
    assert_same(snapshot(dst), snapshot(fresh), "after the reduction")
    # reuse: a plain image again, of the other form and another size
    dst.setImage(big.reshape(-1), None, 16, ILLUM)
    fresh.setImage(big.reshape(-1), None, 16, ILLUM)
    np.testing.assert_array_equal(bits(dst.getImage()), bits(big.reshape(-1)))
    np.testing.assert_array_equal(bits(dst.getLabRef()), bits(fresh.getLabRef()))
    assert_same(snapshot(dst), snapshot(fresh), "dst reused")


def test_img_u8_option_of_the_source_does_not_choose_the_form(ctxs):
    """The form follows what src holds (the packed copy), not src's option "img_u8"."""
    rgba, want = source_image("u8", 10, 11, 3)
    src, dst = ctxs(), ctxs()
    src.setOption("img_u8", 0)
    src.setImage(rgba.reshape(-1), None, 10, ILLUM)
    dst.setImageReduced(src, 3)
    np.testing.assert_array_equal(bits(dst.getImage().reshape(-1, 4)), bits(want))
    assert snapshot(dst)["path"] == "u8"


def test_refusals_leave_dst_as_it_was(ctxs, gpu):
    lib = hq.load()
    rgba, _ = source_image("u8", 13, 7, 2)
    held, _ = source_image("planar", 10, 11, 3)
    src, dst, empty, shard, bare = ctxs(), ctxs(), ctxs(), ctxs(), pr.Context(hq.deltaETypes.CIE76, device=gpu)
    try:
        src.setImage(rgba.reshape(-1), None, 13, ILLUM)
        shard.setImage(rgba.reshape(-1), None, 13, ILLUM, 2, 5)
        dst.setImage(held.reshape(-1), None, 10, ILLUM)
        dst.setMask(np.arange(110) % 3)
        before = snapshot(dst)
        wide = ctxs()  # halfSize 5: a 7 x 4 reduction is too small for it
        k = np.full(11, 1 / 11, np.float32)
        wide.updateOpenCLFilters([[k, k, k], [k, k], [k, k]], k)
        assert wide.halfSize == 5
        wide.setImage(held.reshape(-1), None, 10, ILLUM)
        wide_before = snapshot(wide)

        def refused(d, s, f, status):
            rc = lib.hq_set_image_reduced(d.ctx if d is not None else None, s.ctx if s is not None else None, f, None)
            assert rc == status, (rc, status)

        refused(None, src, 2, _lib.HQ_ERR_ARG)
        refused(dst, None, 2, _lib.HQ_ERR_ARG)
        refused(dst, dst, 2, _lib.HQ_ERR_ARG)
        refused(dst, empty, 2, _lib.HQ_ERR_STATE)      # src without an image
        refused(dst, shard, 2, _lib.HQ_ERR_STATE)      # src a row-block shard
        refused(bare, src, 2, _lib.HQ_ERR_STATE)       # dst without filters
        for f in (0, -1, 17):
            refused(dst, src, f, _lib.HQ_ERR_ARG)
        refused(wide, src, 2, _lib.HQ_ERR_ARG)         # 7 x 4 below halfSize 5
        assert "smaller than the stencil" in lib.hq_last_error(wide.ctx).decode()
        with pytest.raises(hq.HQError):
            dst.setImageReduced(src, 17)
        # dst after every refusal: the getters still answer, the mask still counts, the bits stay
        assert (dst.w, dst.h) == (10, 11)
        assert_same(readback(dst), {k: before[k] for k in ("idx", "err")}, "dst's getters after the refusals")
        assert dst.maskInfo()[0] == int(np.count_nonzero(np.arange(110) % 3))
        assert_same(snapshot(dst), before, "dst evaluated again")
        np.testing.assert_array_equal(bits(dst.getImage()), bits(held.reshape(-1)))
        assert_same(snapshot(wide), wide_before, "the context with long filters")
    finally:
        bare.close()


def test_get_image_of_a_shard_and_without_an_image(ctxs):
    rgba, _ = source_image("u8", 13, 7, 2)
    m = ctxs()
    out = np.zeros(4, np.float32)
    assert hq.load().hq_get_image(m.ctx, _lib.fptr(out)) == _lib.HQ_ERR_STATE
    assert hq.load().hq_get_image(m.ctx, None) == _lib.HQ_ERR_ARG
    m.setImage(rgba.reshape(-1), None, 13, ILLUM, 2, 5)  # the owned rows only
    got = np.zeros(4 * 13 * 3, np.float32)
    _lib.check(hq.load().hq_get_image(m.ctx, _lib.fptr(got)), m.ctx)
    np.testing.assert_array_equal(bits(got), bits(rgba.reshape(7, 13, 4)[2:5].reshape(-1)))

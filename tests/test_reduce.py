"""CPU tests of the image pyramid's host-only calls, hq_reduced_size and hq_reduce_weights,
against tests/reduce_ref.py's restatement, bit for bit.  No GPU."""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import reduce_ref as rr
from hybridquantization_amd import _lib

IM = hq.ImageManipulation


def lib_size(w, h, f):
    rw, rh = C.c_int(-7), C.c_int(-7)
    rc = hq.load().hq_reduced_size(w, h, f, C.byref(rw), C.byref(rh))
    return rc, rw.value, rh.value


@pytest.mark.parametrize("f", range(0, 18))
def test_reduced_size_against_the_formula(f):
    for w, h in ((13, 7), (16, 16), (5, 9), (1, 1), (4096, 4096), (130, 9)):
        rc, rw, rh = lib_size(w, h, f)
        if 1 <= f <= 16:
            assert (rc, rw, rh) == (_lib.HQ_OK, -(-w // f), -(-h // f))
            assert IM.reducedSize(w, h, f) == rr.reduced_size(w, h, f)
        else:
            assert (rc, rw, rh) == (_lib.HQ_ERR_ARG, -7, -7)  # (a refusal writes nothing)
            with pytest.raises(hq.HQError):
                IM.reducedSize(w, h, f)


def check_map(src, w, h, f):
    for is_mask in (False, True):
        got = IM.reduceWeights(src, w, f, is_mask)
        want = rr.reduce_weights(src, w, h, f, is_mask)
        assert got.dtype == np.uint8 and got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=f"{w}x{h} f={f} mask={is_mask}")
    return IM.reduceWeights(src, w, f, False)


@pytest.mark.parametrize("w,h,f", [(13, 7, 2), (10, 11, 3), (16, 16, 4), (5, 9, 16)])
def test_random_maps(w, h, f):
    rng = np.random.default_rng(100 * w + f)
    src = rng.integers(0, 256, (h, w)).astype(np.uint8)
    src[rng.random((h, w)) < 0.3] = 0
    check_map(src, w, h, f)
    check_map(src.reshape(-1), w, h, f)  # flat


def test_ties_round_up():
    # 3 x 3 at f = 2: blocks of n = 4, 2, 2 and 1 whose means end in .5
    src = np.array([[1, 1, 1], [0, 0, 0], [2, 1, 7]], np.uint8)
    got = check_map(src, 3, 3, 2)
    np.testing.assert_array_equal(got, [[1, 1], [2, 7]])
    # n = 4 with sums 2, 6, 10 (0.5, 1.5, 2.5), n = 3 and n = 6 (3 x 2 at f = 3 and 5 x 3 edges)
    quad = np.array([[1, 1, 3, 3, 5, 5], [0, 0, 0, 0, 0, 0]], np.uint8)
    np.testing.assert_array_equal(check_map(quad, 6, 2, 2), [[1, 2, 3]])
    six = np.array([[1, 1, 1, 0, 0], [0, 0, 0, 9, 0], [5, 5, 5, 9, 9]], np.uint8)
    got = check_map(six, 5, 3, 3)  # blocks: 9 pixels sum 18 -> 2; 6 pixels sum 27 -> 4.5 -> 5
    np.testing.assert_array_equal(got, [[2, 5]])


def test_raise_to_one_and_the_all_zero_block():
    src = np.zeros((4, 8), np.uint8)
    src[0, 0] = 1          # 1 / 4 rounds to 0: raised to 1
    src[2, 7] = 1          # 1 / 16 of the f = 4 block
    got = check_map(src, 8, 4, 2)
    np.testing.assert_array_equal(got, [[1, 0, 0, 0], [0, 0, 0, 1]])
    np.testing.assert_array_equal(check_map(src, 8, 4, 4), [[1, 1]])
    np.testing.assert_array_equal(check_map(np.zeros((4, 8), np.uint8), 8, 4, 4), [[0, 0]])
    one_in_256 = np.zeros((16, 16), np.uint8)
    one_in_256[15, 15] = 1
    assert IM.reduceWeights(one_in_256, 16, 16, False)[0, 0] == 1
    assert IM.reduceWeights(one_in_256, 16, 16, True)[0, 0] == 1  # (510 + 256) // 512


def test_factor_one_is_the_identity():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (7, 13)).astype(np.uint8)
    src[2] = 0
    np.testing.assert_array_equal(IM.reduceWeights(src, 13, 1, False), src)
    np.testing.assert_array_equal(IM.reduceWeights(src, 13, 1, True), np.where(src != 0, 255, 0))


def test_mask_against_weights():
    src = np.array([[1, 0], [0, 0]], np.uint8)
    assert IM.reduceWeights(src, 2, 2, True)[0, 0] == 64    # 255 / 4 = 63.75
    assert IM.reduceWeights(src, 2, 2, False)[0, 0] == 1    # 0.25, raised
    sevens = np.full((2, 2), 7, np.uint8)
    assert IM.reduceWeights(sevens, 2, 2, True)[0, 0] == 255
    assert IM.reduceWeights(sevens, 2, 2, False)[0, 0] == 7
    # a bool mask is a mask of ones
    np.testing.assert_array_equal(IM.reduceWeights(src.astype(bool), 2, 2, True), [[64]])
    assert IM.reduceWeights(np.full((16, 16), 255, np.uint8), 16, 16, False)[0, 0] == 255


def test_bad_arguments():
    lib = hq.load()
    src, out = np.full(4, 9, np.uint8), np.full(4, 0xAB, np.uint8)
    for args in ((None, 2, 2, 1, 0, _lib.u8ptr(out)), (_lib.u8ptr(src), 2, 2, 1, 0, None),
                 (_lib.u8ptr(src), 2, 2, 0, 0, _lib.u8ptr(out)), (_lib.u8ptr(src), 2, 2, 17, 0, _lib.u8ptr(out)),
                 (_lib.u8ptr(src), 0, 2, 1, 0, _lib.u8ptr(out))):
        assert lib.hq_reduce_weights(*args) == _lib.HQ_ERR_ARG
    assert np.all(out == 0xAB)
    with pytest.raises(ValueError):
        IM.reduceWeights(np.zeros((2, 3), np.float32), 3, 1)
    with pytest.raises(ValueError):
        IM.reduceWeights(np.zeros((2, 3), np.uint8), 4, 1)
    with pytest.raises(ValueError):
        IM.reduceWeights(np.full((2, 3), 300, np.int32), 3, 1)


def test_restated_image_forms_agree_on_the_lattice():
    """The two restated forms are different arithmetic; on a constant k/255 image both must
    return the image's own value (a check of reduce_ref itself)."""
    rgba = np.zeros((6 * 5, 4), np.float32)
    rgba[:, :3] = np.float32(51) / np.float32(255)
    u8 = rr.reduce_u8(rgba, 6, 5, 4)
    assert u8.shape == (2 * 2, 4) and np.all(u8[:, :3] == rgba[0, 0]) and np.all(u8[:, 3] == 0)

"""The CPU statement of CIEDE2000 (tests/de2000_ref.py) against the published
test data of Sharma, Wu & Dalal (2005), tests/golden/ciede2000_sharma.json.
This pins the checker that tests/test_de2000_gpu.py measures libhq with."""

import numpy as np

import de2000_ref as d

TABLE_ATOL = 5e-5  # half a unit of the table's last digit


def _cols(t):
    return [t[:, i] for i in range(6)]


def test_float64_reproduces_sharma_table():
    t = d.sharma_table()
    assert t.shape == (34, 7)
    e = d.ciede2000(*_cols(t))
    assert e.dtype == np.float64
    worst = float(np.abs(e - t[:, 6]).max())
    print(f"float64 against the table: worst {worst:.3g}")
    assert worst <= TABLE_ATOL


def test_symmetric_under_swap():
    t = d.sharma_table()
    e = d.ciede2000(*_cols(t))
    s = d.ciede2000(t[:, 3], t[:, 4], t[:, 5], t[:, 0], t[:, 1], t[:, 2])
    np.testing.assert_allclose(s, e, rtol=0, atol=1e-12)


def test_float32_form_is_float32_and_close():
    t = d.sharma_table()
    e32 = d.ciede2000(*_cols(t), dtype=np.float32)
    assert e32.dtype == np.float32
    np.testing.assert_allclose(e32, d.ciede2000(*_cols(t)), rtol=0, atol=1e-5)


def test_other_branch_flag_gives_the_neighbouring_values():
    """Pairs 10 and 14 sit exactly on |h'1 - h'2| = 180 degrees: the flag moves
    them to the values of pairs 11 and 15.  A pair without a hue difference
    (C'1 C'2 = 0) has no branch to flip."""
    t = d.sharma_table()
    gap = d.hue_gap_deg(*_cols(t))
    assert abs(gap[9] - 180.0) < 1e-9 and abs(gap[13] - 180.0) < 1e-9
    other = d.ciede2000(*_cols(t), other_branch=True)
    assert abs(other[9] - 7.2195) <= TABLE_ATOL and abs(other[13] - 4.7461) <= TABLE_ATOL
    # identical, grey/grey and grey/chromatic pairs have no hue difference: no branch to flip
    z = np.zeros(3)
    L1, L2 = np.array([50.0, 40.0, 30.0]), np.array([50.0, 70.0, 35.0])
    a2, b2 = np.array([0.0, 0.0, 12.0]), np.array([0.0, 0.0, -7.0])
    e = d.ciede2000(L1, z, z, L2, a2, b2)
    np.testing.assert_array_equal(e, d.ciede2000(L1, z, z, L2, a2, b2, other_branch=True))
    assert e[0] == 0.0 and np.isnan(d.hue_gap_deg(L1, z, z, L2, a2, b2)).all()
    sl = 1 + 0.015 * (55.0 - 50.0) ** 2 / np.sqrt(20 + (55.0 - 50.0) ** 2)
    assert abs(e[1] - 30.0 / sl) < 1e-12  # two greys: |dL| / S_L

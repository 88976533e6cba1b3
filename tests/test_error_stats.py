"""errorQuantile (the host helper beside errorStats) on hand-written histogram rows.  No GPU needed."""
import pytest

from hybridquantization_amd import ImageManipulation

# (row, top, q, the upper edge of the first bin where the cumulative count reaches q of the total)
ROWS = [([0, 0, 9, 0], 8.0, 0.5, 6.0),          # all the mass in one bin
        ([1, 3, 4, 2], 8.0, 0.4, 4.0),          # an exact cumulative hit: 1 + 3 = 0.4 x 10
        ([5, 0, 0, 1], 8.0, 1.0, 8.0)]          # q = 1 lands in the overflow bin: top, a lower bound


@pytest.mark.parametrize("row,top,q,want", ROWS)
def test_error_quantile(row, top, q, want):
    assert ImageManipulation.errorQuantile(row, top, q) == want


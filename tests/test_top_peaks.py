"""CPU (-m "not gpu"): ``peak_search.top_rows``, the host definition of the device's top-L selection
(``ops.peak_top``, csrc/estimate.hip).  Expected values are the reference callers' own two lines
(main_for_net.py:119,126 / test/test_model_peaksearch.py:88,91) evaluated here by Python itself:
``sorted(list(rows), key=lambda x: x[2], reverse=True)[:L]``."""
import numpy as np
import pytest

from admm_net_amd import peak_search


def _callers_lines(rows, L):
    res = sorted(list(rows), key=lambda x: x[2], reverse=True)
    return np.asarray(res[:L], dtype=np.float64).reshape(-1, 3)


def _rows(heights):
    """A peak list whose (x, y) name the list position, so that the order of equal heights is visible."""
    h = np.asarray(heights, dtype=np.float64)
    k = np.arange(len(h), dtype=np.float64)
    return np.stack([k, -k, h], axis=1).reshape(-1, 3)


CASES = {
    "distinct": [0.3, 2.5, 0.1, 9.0, 4.0, 1.5, 7.25],
    "tie_blocks": [1.0, 5.0, 5.0, 0.5, 1.0, 5.0, 0.5, 0.5, 9.0, 1.0, 9.0],   # equal heights at head, middle and tail
    "all_zero": [0.0] * 9,
    "one_row": [3.0],
    "empty": [],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_top_rows_is_the_callers_sort_and_cut(name):
    rows = _rows(CASES[name])
    n = rows.shape[0]
    for L in sorted({0, 1, 2, 3, max(n - 1, 0), n, n + 1, n + 5, 64}):
        got = peak_search.top_rows(rows, L)
        want = _callers_lines(rows, L)
        assert got.shape == (min(n, L), 3) and got.dtype == np.float64
        assert np.array_equal(got, want), (name, L)


def test_top_rows_keeps_list_order_among_equal_heights():
    rows = _rows(CASES["tie_blocks"])
    got = peak_search.top_rows(rows, 6)
    assert got[:, 0].tolist() == [8.0, 10.0, 1.0, 2.0, 5.0, 0.0]      # 9, 9, 5, 5, 5, then the first of the 1.0 rows
    assert np.array_equal(peak_search.top_rows(_rows(CASES["all_zero"]), 4), _rows(CASES["all_zero"])[:4])
    # the rank definition of include/admmnet.h: rank(k) = #{j : h_j > h_k} + #{j < k : h_j == h_k}
    h = rows[:, 2]
    rank = [int((h > h[k]).sum() + (h[:k] == h[k]).sum()) for k in range(len(h))]
    full = peak_search.top_rows(rows, len(h))
    assert [int(r[0]) for r in full] == [rank.index(r) for r in range(len(h))]


def test_zero_rounds_leave_zero_heights_so_the_cut_is_the_head_of_the_list():
    """alt_peak_search with iter = 0 never writes a height (peakSearchUtils.py:136-171 is skipped): every maximum ties
    at 0.0 and the stable sort leaves np.where order -- the tie rule on a real input."""
    rng = np.random.default_rng(7)
    phi = (rng.standard_normal(100) + 1j * rng.standard_normal(100)).astype(np.complex64)
    res = peak_search.alt_peak_search({"phi": phi, "xbase": 10, "ybase": 10}, {"xstep": 1 / 40, "ystep": 1 / 40, "iter": 0})
    assert res.shape[0] > 8 and not res[:, 2].any()
    for L in (1, 3, 8, res.shape[0], res.shape[0] + 3):
        got = peak_search.top_rows(res, L)
        assert np.array_equal(got, res[:L]) and np.array_equal(got, _callers_lines(res, L))

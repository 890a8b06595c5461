"""The numpy restatement of the pairwise-distance kernels (tests/pdist_reference.py) against the live reference's
recorded results (tests/golden/stats_pdist.npz), bit for bit, and against the reference's statements pair by pair over
the boundaries of numpy's summation order.  No GPU."""
import numpy as np
import pytest

import pdist_cases as pc
import pdist_reference as ref


@pytest.mark.parametrize('name,slide_span', pc.WINDOW_CASES)
def test_window_dists_equal_the_reference(name, slide_span):
    g = pc.gold()
    ref.same_bits(ref.window_dists(g['%s_rows' % name], slide_span), g['%s_dists_s%d' % (name, slide_span)])


def test_fixture_holds_the_hard_cases():
    g = pc.gold()
    d0, d3 = g['w27_dists_s0'], g['w27_dists_s3']
    assert d0[1, 0] == 0.0 and np.all(d0[np.triu_indices(35, 1)] == 0.0)
    assert np.isnan(d0[34, :]).all() and np.isnan(d0[33, :34]).all()
    # the NaN of row 34 sits in its first window only, that of row 33 in its last windows only: min() keeps the first
    assert np.isnan(d3[34, :]).all() and not np.isnan(d3[33, :33]).any()
    assert np.any((d3 < d0) & (d3 > 0)) and np.count_nonzero(d3[np.tril_indices(35)] == 0.0) > np.count_nonzero(
        d0[np.tril_indices(35)] == 0.0)     # shifted copies meet in some window
    big = g['wbig_dists_s0']
    assert np.isinf(big[1, 0]) and big[3, 3] == 0.0 and big[3, 2] > 0.0


@pytest.mark.parametrize('name', ['pvals', 'llrs'])
def test_nanmean_dists_equal_the_reference(name):
    g = pc.gold()
    raw = g['%s_raw_dists' % name]
    ref.same_bits(ref.nanmean_dists(g['%s_trimmed' % name]), raw)
    assert np.isnan(raw).any()
    filled = raw.copy()
    filled[np.isnan(filled)] = np.nanmax(filled) + 1
    ref.same_bits(filled, g['%s_dists' % name])


@pytest.mark.parametrize('nb', [1, 7, 8, 9, 127, 128, 129, 130, 257])
@pytest.mark.parametrize('slide_span', [0, 1, 3])
def test_window_dists_equal_the_loops(nb, slide_span):
    rng = np.random.default_rng(nb * 10 + slide_span)
    rows = ref.full_mantissa(rng, (5, nb + 2 * slide_span))
    rows[3] = rows[1]
    ref.same_bits(ref.window_dists(rows, slide_span), ref.window_dists_loops(rows, slide_span))


@pytest.mark.parametrize('row_len', [1, 7, 8, 9, 127, 128, 129, 130, 257])
def test_nanmean_dists_equal_the_loops(row_len):
    rng = np.random.default_rng(row_len)
    rows = ref.full_mantissa(rng, (6, row_len))
    ref.same_bits(ref.nanmean_dists(rows), ref.nanmean_dists_loops(rows))
    rows[rng.random(rows.shape) < 0.3] = np.nan
    rows[4] = np.nan
    rows[0, 0], rows[1, 0] = 1e160, -1e160
    ref.same_bits(ref.nanmean_dists(rows), ref.nanmean_dists_loops(rows))


def test_sqrt_of_the_square_is_not_fabs():
    """order_reads' metric squares first: a difference of 2e160 gives inf, one of 1e-170 gives 0"""
    rows = np.array([[1e160, 1e-170, 1.0], [-1e160, 0.0, 3.0]])
    d = ref.nanmean_dists(rows)
    assert np.isinf(d[0])
    assert ref.nanmean_dists(rows[:, 1:])[0] == 1.0      # (0 + 2) / 2, not (1e-170 + 2) / 2

"""TEST INFRASTRUCTURE: the two pairwise-distance modes of csrc/k_pdist.h restated in numpy, pinned bit for bit to
the live reference's recorded results (tests/golden/stats_pdist.npz) by tests/test_pdist_reference.py and, over the
boundaries of numpy's summation order, to the literal loops of the reference below.

  window_dists    get_pairwise_dists / sliding_window_dist / euclidian_dist (tombo/tombo_stats.py:158-196)
  nanmean_dists   pdist(reg_stats, lambda u, v: np.nanmean(np.sqrt((u - v)**2))) (order_reads, :142-156)

Both work on all pairs at once: `x.sum(-1)` of a C-contiguous array adds every row in the order np.sum adds a
vector (pairwise from eight values on), so the bits are those of the per-pair calls."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stats_pdist.npz')


def load():
    return np.load(GOLDEN)


def window_dists(rows, slide_span=0):
    """float64[R, R]: [i, j], j <= i, the sqrt of Python's min() over the window starts (i1 outer, i2 inner) of the
    summed squared differences; 0 for j > i"""
    rows = np.asarray(rows, dtype=np.float64)
    n, nb = rows.shape[0], rows.shape[1] - 2 * slide_span
    assert nb >= 1
    best = None
    with np.errstate(all='ignore'):
        for i1 in range(2 * slide_span + 1):
            for i2 in range(2 * slide_span + 1):
                s = np.square(rows[:, None, i1:i1 + nb] - rows[None, :, i2:i2 + nb]).sum(-1)
                best = s if best is None else np.where(s < best, s, best)   # (min() keeps the first unless a later is smaller)
        out = np.sqrt(best)
    out[np.triu_indices(n, 1)] = 0.0
    return out


def nanmean_dists(rows):
    """float64[R (R - 1) / 2] in scipy's condensed order: the sum of the |differences| that are numbers over their
    count; NaN without one"""
    rows = np.asarray(rows, dtype=np.float64)
    i, j = np.triu_indices(rows.shape[0], 1)
    with np.errstate(all='ignore'):
        d = np.sqrt((rows[i] - rows[j]) ** 2)
        nan = np.isnan(d)
        return np.where(nan, 0.0, d).sum(-1) / (~nan).sum(-1)


def window_dists_loops(rows, slide_span=0):
    """the reference's statements, pair by pair"""
    rows = np.asarray(rows, dtype=np.float64)
    n, nb = rows.shape[0], rows.shape[1] - 2 * slide_span
    out = np.zeros((n, n))
    with np.errstate(all='ignore'):
        for i in range(n):
            for j in range(i + 1):
                if slide_span > 0:
                    out[i, j] = np.sqrt(min(np.sum(np.square(rows[i][i1:i1 + nb] - rows[j][i2:i2 + nb]))
                                            for i1 in range((slide_span * 2) + 1) for i2 in range((slide_span * 2) + 1)))
                else:
                    out[i, j] = np.sqrt(np.sum(np.square(rows[i] - rows[j])))
    return out


def nanmean_dists_loops(rows):
    import warnings
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[0]
    out = []
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', category=RuntimeWarning)
        for i in range(n - 1):
            for j in range(i + 1, n):
                out.append(np.nanmean(np.sqrt(((rows[i] - rows[j]) ** 2))))
    return np.array(out, dtype=np.float64)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok])
    assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))


def full_mantissa(rng, shape, scale=1.0):
    """random doubles whose low bits are set: a changed summation order shows in the last bit"""
    return rng.standard_normal(shape) * scale + rng.random(shape) * 1e-3

"""The pairwise-distance kernels of csrc/k_pdist.h (Engine.pairwise_window_dists, pairwise_nanmean_dists) against
the live reference's recorded results (tests/golden/stats_pdist.npz) and, beyond the fixture, against the numpy
restatement that tests/test_pdist_reference.py pins to the same fixture.  Bits are compared, without tolerance.

Shapes: row counts 1, 2, 3 and around the tile of pairs (T - 1, T, T + 1, 2 T + 1: diagonal tiles, a partial last
tile, tiles above the diagonal that no workgroup computes yet hold zeros); window lengths at the boundaries of numpy's
summation order (sequential below 8, eight accumulators to 128, halves beyond); slide spans 0, 1, 3; one row length
past the LDS tile (the global-memory path)."""
import ctypes as C

import numpy as np
import pytest

import pdist_cases as pc
import pdist_reference as ref
from tombo_amd import tombo_stats as ts, resquiggle as rq, _native

pytestmark = pytest.mark.gpu

T = _native.PDIST_TILE
LDS_MAX = _native.PDIST_LDS_ROW_MAX
N_ROWS = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1]
WINDOWS = [1, 7, 8, 9, 127, 128, 129, 130]
SPANS = [0, 1, 3]
TBA_E_ARG = -1


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


def test_tile_constants_of_the_library(eng):
    assert eng._L.tba_pdist_tile() == T and eng._L.tba_pdist_lds_row_max() == LDS_MAX


# ---- the fixture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,slide_span', pc.WINDOW_CASES)
def test_get_pairwise_dists_equal_the_reference(eng, name, slide_span):
    pc.check_window_case(eng, name, slide_span)
    assert eng.last_pdist_kernel_ms > 0.0


@pytest.mark.parametrize('name', ['pvals', 'llrs'])
def test_order_reads_distances_equal_the_reference(eng, name):
    g = pc.gold()
    ref.same_bits(eng.pairwise_nanmean_dists(np.ascontiguousarray(g['%s_trimmed' % name])), g['%s_raw_dists' % name])
    assert eng.last_pdist_kernel_ms > 0.0


@pytest.mark.parametrize('name', ['pvals', 'llrs'])
def test_order_reads_leaves_equal_the_reference(eng, name):
    pytest.importorskip('scipy')
    pc.check_order_reads(eng, name)


# ---- beyond the fixture: sizes ----------------------------------------------------------------------------
def special_rows(rng, n, row_len):
    """full-mantissa rows with, where there is room: two identical rows, an all-zero row, a zero stretch, multiples of
    1/64 that repeat with a shift (ties for the minimum)"""
    rows = ref.full_mantissa(rng, (n, row_len))
    if n >= 2:
        rows[1] = rows[0]
    if n >= 3:
        rows[2, row_len // 3:] = 0.0
    if n >= 6:
        base = rng.integers(-96, 97, row_len + 4) / 64.0
        rows[3], rows[4], rows[5] = base[:row_len], base[2:row_len + 2], 0.0
    return rows


@pytest.mark.parametrize('nb', WINDOWS)
def test_window_dists_sizes(eng, nb):
    for n in N_ROWS:
        for s in SPANS:
            rows = special_rows(np.random.default_rng(1000 * nb + 10 * n + s), n, nb + 2 * s)
            got = eng.pairwise_window_dists(rows, s)
            ref.same_bits(got, ref.window_dists(rows, s))
            assert got.shape == (n, n) and np.all(got[np.triu_indices(n, 1)] == 0.0)
            if n >= 2:
                assert got[1, 0] == 0.0


def test_window_dists_one_row(eng):
    assert eng.pairwise_window_dists(np.array([[1.5, -2.0, 0.25]]), 1).tolist() == [[0.0]]
    assert eng.pairwise_nanmean_dists(np.array([[1.5, -2.0, 0.25]])).shape == (0,)


@pytest.mark.parametrize('row_len,s', [(LDS_MAX, 3), (LDS_MAX + 1, 0), (LDS_MAX + 1, 3), (LDS_MAX + 46, 1)])
def test_rows_at_and_past_the_lds_tile(eng, row_len, s):
    rows = special_rows(np.random.default_rng(row_len + s), T + 2, row_len)
    ref.same_bits(eng.pairwise_window_dists(rows, s), ref.window_dists(rows, s))
    rows[np.random.default_rng(s).random(rows.shape) < 0.1] = np.nan
    ref.same_bits(eng.pairwise_nanmean_dists(rows), ref.nanmean_dists(rows))


def test_window_dists_overflow_underflow_and_nan(eng):
    rng = np.random.default_rng(9)
    rows = ref.full_mantissa(rng, (T + 3, 15))
    rows[0, :4], rows[1, :4] = 1e160, -1e160          # squares overflow: inf, as in numpy
    rows[2], rows[3, 5] = 1e-170, 1e-170              # squares underflow
    rows[4, 0] = np.nan                               # in the first window only
    rows[5, 14] = np.nan                              # in the last windows only
    rows[6, 7] = np.nan                               # in every window
    for s in (0, 1, 3):
        got = eng.pairwise_window_dists(rows, s)
        ref.same_bits(got, ref.window_dists(rows, s))
        ref.same_bits(got, ref.window_dists_loops(rows, s))
    assert np.isinf(eng.pairwise_window_dists(rows, 0)[1, 0])
    got = eng.pairwise_window_dists(rows, 3)
    assert np.isnan(got[4, :5]).all() and not np.isnan(got[5, :4]).any() and np.isnan(got[6, :7]).all()
    assert eng.pairwise_window_dists(rows[2:4], 0)[1, 0] > 0.0 and eng.pairwise_window_dists(rows[2:3], 0)[0, 0] == 0.0


@pytest.mark.parametrize('row_len', WINDOWS)
def test_nanmean_dists_sizes(eng, row_len):
    for n in N_ROWS:
        rng = np.random.default_rng(100 * row_len + n)
        rows = special_rows(rng, n, row_len)
        ref.same_bits(eng.pairwise_nanmean_dists(rows), ref.nanmean_dists(rows))
        rows[rng.random(rows.shape) < 0.25] = np.nan
        got = eng.pairwise_nanmean_dists(rows)
        ref.same_bits(got, ref.nanmean_dists(rows))
        assert got.shape == (n * (n - 1) // 2,)


def test_nanmean_dists_nan_patterns_and_trim_values(eng):
    trim = 10.0
    rng = np.random.default_rng(21)
    rows = np.clip(rng.standard_normal((T + 2, 20)) * 8, -trim, trim)
    rows[0] = np.nan                                        # an all-NaN row: NaN against every row
    rows[1, :10], rows[2, 10:] = np.nan, np.nan             # disjoint patterns: NaN
    rows[3], rows[4] = trim, -trim                          # values at +-trim
    rows[5, :3], rows[6, :3] = 1e160, -1e160                # sqrt(d * d) is inf where fabs(d) is 2e160
    rows[7, 3], rows[8, 3] = 1e-170, 0.0                    # ... and 0 where fabs(d) is 1e-170
    got = eng.pairwise_nanmean_dists(rows)
    ref.same_bits(got, ref.nanmean_dists(rows))
    ref.same_bits(got, ref.nanmean_dists_loops(rows))
    n = rows.shape[0]
    k = lambda i, j: n * i - i * (i + 1) // 2 + j - i - 1
    assert np.isnan(got[:n - 1]).all() and np.isnan(got[k(1, 2)]) and got[k(3, 4)] == 2 * trim and np.isinf(got[k(5, 6)])
    again = eng.pairwise_nanmean_dists(rows)
    ref.same_bits(again, got)


def test_host_functions_on_the_device(eng):
    """get_pairwise_dists from a list of profiles, slide_span None; order_reads of one read launches nothing"""
    rows = pc.gold()['w27_rows']
    with np.errstate(all='ignore'):
        ref.same_bits(ts.get_pairwise_dists(list(rows), None, engine=eng), pc.gold()['w27_dists_s0'])
    assert ts.order_reads(rows[:1], engine=eng) == [0]


# ---- argument errors: TBA_E_ARG, nothing launched ---------------------------------------------------------------
def _c_window(eng, n_rows, row_len, slide_span, rows, out, e=True):
    ms = _native.f64(-1.0)
    rc = eng._L.tba_pairwise_window_dists(eng._h if e else None, _native.i64(n_rows), _native.i64(row_len),
                                          _native.i64(slide_span), rows, out, C.byref(ms))
    return rc, ms.value


def _c_nanmean(eng, n_rows, row_len, rows, out, e=True):
    ms = _native.f64(-1.0)
    rc = eng._L.tba_pairwise_nanmean_dists(eng._h if e else None, _native.i64(n_rows), _native.i64(row_len),
                                           rows, out, C.byref(ms))
    return rc, ms.value


def test_bad_arguments_launch_nothing(eng):
    rows = np.arange(12, dtype=np.float64).reshape(3, 4)
    out = np.full((3, 3), 7.0)
    cond = np.full(3, 7.0)
    big = np.zeros((_native.PDIST_MAX_ROWS + 1, 1))
    eng.pairwise_window_dists(rows, 1)
    before = eng.last_pdist_kernel_ms
    bad_window = [(3, 4, 0, None, out, True), (3, 4, 0, rows, None, True), (3, 4, 0, rows, out, False),
                  (0, 4, 0, rows, out, True), (-1, 4, 0, rows, out, True), (3, 0, 0, rows, out, True),
                  (3, 4, -1, rows, out, True), (3, 4, 2, rows, out, True), (3, 4, 3, rows, out, True),
                  (3, 4, 2 ** 62, rows, out, True), (_native.PDIST_MAX_ROWS + 1, 1, 0, big, out, True),
                  (2, _native.PDIST_MAX_ELEMS // 2 + 1, 0, rows, out, True)]
    for args in bad_window:
        rc, ms = _c_window(eng, *args)
        assert rc == TBA_E_ARG and ms == -1.0, args[:3]         # (the timer's output is not touched either)
    bad_nanmean = [(3, 4, None, cond, True), (3, 4, rows, None, True), (3, 4, rows, cond, False), (0, 4, rows, cond, True),
                   (3, 0, rows, cond, True), (3, -5, rows, cond, True), (_native.PDIST_MAX_ROWS + 1, 1, big, cond, True),
                   (2, _native.PDIST_MAX_ELEMS // 2 + 1, rows, cond, True)]
    for args in bad_nanmean:
        rc, ms = _c_nanmean(eng, *args)
        assert rc == TBA_E_ARG and ms == -1.0, args[:2]
    assert np.all(out == 7.0) and np.all(cond == 7.0)
    assert eng.last_pdist_kernel_ms == before
    # one row: valid in both modes; mode N writes nothing and needs no output
    rc, ms = _c_nanmean(eng, 1, 4, rows, None)
    assert rc == 0 and ms == 0.0
    rc, ms = _c_window(eng, 1, 4, 1, rows, out)
    assert rc == 0 and ms > 0.0 and out[0, 0] == 0.0
    # the binding checks before it calls
    for bad in (lambda: eng.pairwise_window_dists(rows, 2), lambda: eng.pairwise_window_dists(rows.astype(np.float32)),
                lambda: eng.pairwise_nanmean_dists(rows.T), lambda: eng.pairwise_nanmean_dists(rows[:0])):
        with pytest.raises(ValueError):
            bad()

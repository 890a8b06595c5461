"""The arg-max of a forward-pass row (csrc/k_dp.h: the lane's maximum as a pairwise tree, the first maximal cell of
the winning lane by a descent of one compare per level in the 8-cell class, the linear search in the others) through
k_dp<CPL, true> on z matrices made for it, against the oracle's forward pass over the same matrix (dp_zmat_case.py).
Every comparison is exact: forward rows bit for bit, moves, band starts, top_pos.

Classes 4, 5, 8 and 12 cells per lane at W = 64 CPL - 3 (the last lane with cells holds CPL - 3), 70 rows, 20 of them
static.  What the rows are made for:
  (a) one maximum at every in-lane position of lane 0, of a middle lane and of the last lane with cells;
  (b) two equal maxima in one lane, every pair of positions: the first wins;
  (c) equal maxima in two lanes: the lower lane wins, whatever the positions inside the lanes;
  (d) a plateau (every z 0, both penalties 0): cell 0;
  (e) +0.0 and -0.0 as the two maxima of one lane, in both orders, every pair of positions: they compare equal, the
      first wins.  A forward row that starts from zeros cannot hold -0.0 (x + y is -0.0 only for two -0.0), so these
      rows continue a GIVEN forward row, through tba_c_adaptive_banded_forward_pass against the oracle's function of
      that name;
  (f) a row whose cells are all -inf but one (skip_pen = +inf, so that no move reaches a cell whose z is -inf).

One move is left out of the comparison: band cell 0's where that cell is -inf, which happens under skip_pen = +inf
only.  The oracle writes that cell's move without comparing anything, the kernel -- this one and the one before it --
derives it like every cell's and gets "stay" for -inf; no traceback reads a move of a -inf cell
(dp_zmat_case.assert_same)."""
import numpy as np
import pytest

import dp_zmat_case as zc

pytestmark = pytest.mark.gpu


def _cells(cpl, lane):
    W = zc.band(cpl)
    return [b for b in range(lane * cpl, (lane + 1) * cpl) if b < W]


def _peak_case(cpl, cells, offset):
    z, static, ref = zc.tail_case(cpl, offset, lambda prev, off: zc.peaks_row(prev, off, cells))
    assert ref[3] == min(cells)                     # the case is what it says: the first of the maxima, by the oracle
    last = ref[0][zc.N_ROWS]
    assert np.flatnonzero(last == last.max()).tolist() == sorted(cells)
    zc.assert_same(zc.run_gpu(z, static), ref, (cpl, cells, offset))


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_base_matrix(cpl):
    """the shared rows on their own: random multiples of 1/8 (ties in every row), static rows with offsets 0 .. 3,
    50 adaptive rows whose starts follow the arg-max"""
    z, static, _ = zc.base(cpl)
    ref = zc.reference(z, static)
    assert len(set(np.diff(ref[2][zc.N_STATIC:]).tolist())) > 1     # the adaptive band moves, and not always alike
    zc.assert_same(zc.run_gpu(z, static), ref, cpl)


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_single_maximum_at_every_position(cpl):
    """(a); the last row's band 1, 2 or 3 cells past the row before (cell 0 of the band has a z of its own only then)"""
    n = 0
    for lane in (0, 31, 63):
        cells = _cells(cpl, lane)
        assert len(cells) == (cpl if lane < 63 else cpl - 3)
        for j, b in enumerate(cells):
            _peak_case(cpl, [b], 1 + j % 3)
            n += 1
    assert n == 3 * cpl - 3


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_two_equal_maxima_in_one_lane(cpl):
    """(b): every pair of positions a < b of a middle lane (band offsets 0 .. 3) and of lane 0"""
    for lane in (20, 0):
        cells = _cells(cpl, lane)
        for a in range(cpl):
            for b in range(a + 1, cpl):
                _peak_case(cpl, [cells[a], cells[b]], (a + b) % 4 if lane else 1 + (a + b) % 3)


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_equal_maxima_in_two_lanes(cpl):
    """(c): the lower lane wins with its maximum in its last cell and the higher lane's in its first, and the other
    way round; three lanes; neighbouring lanes; the partial last lane"""
    lo, hi, last = _cells(cpl, 9), _cells(cpl, 41), _cells(cpl, 63)
    for k, cells in enumerate(([lo[-1], hi[0]], [lo[0], hi[-1]], [lo[1], hi[1], last[0]], [lo[-1], lo[-1] + 1],
                               [hi[2], last[-1]], [lo[-2], lo[-1], hi[0], hi[1]])):
        _peak_case(cpl, cells, k % 4)


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_plateau(cpl):
    """(d): z = 0 everywhere, no penalties: every cell of every row is 0, every move a tie, every arg-max cell 0"""
    W = zc.band(cpl)
    z = np.zeros((zc.N_ROWS, W))
    static = np.cumsum(np.arange(zc.N_STATIC) % 3).astype(np.int64)
    ref = zc.reference(z, static, 0.0, 0.0)
    assert ref[3] == 0 and not ref[0].any() and np.all(ref[2][zc.N_STATIC:] == ref[2][zc.N_STATIC - 1])
    zc.assert_same(zc.run_gpu(z, static, 0.0, 0.0), ref, cpl)
    z[1::2] = -1.0                      # ... and with every other row below it: the skip move carries the plateau on,
    ref = zc.reference(z, static, 0.0, 0.0)     # behind a first cell that has no skip move where the band has moved
    assert np.all(ref[0][zc.N_ROWS][1:] == 0.0)
    zc.assert_same(zc.run_gpu(z, static, 0.0, 0.0), ref, cpl)


def _signed_zero_case(cpl, lane, a, b, first_negative):
    """three bases, the forward row after the first one given: -50 everywhere but a peak of 100 (it places the next
    band `diff` cells on) and the two zeros; the second base's events equal its level exactly under the two cells the
    zeros feed by their diagonal move (z = z_shift - 0 = -0.0 with z_shift = -0.0: the cells are -0.0 + -0.0 = -0.0
    and +0.0 + -0.0 = +0.0) and lie 500 sd away everywhere else; penalties of 1000 keep every other move far below.
    The third base's band start shows which cell won."""
    import oracle
    from tombo_amd.resquiggle import get_engine
    W = zc.band(cpl)
    half, diff = W // 2, 3
    ta, tb = lane * cpl + a, lane * cpl + b
    assert half <= ta < tb < W
    row = np.full(W, -50.0)
    row[half - 1 + diff] = 100.0                                    # arg-max of the given row: the band moves by diff
    row[ta + diff - 1], row[tb + diff - 1] = (-0.0, 0.0) if first_negative else (0.0, -0.0)
    n_bases, start0 = 3, 5
    n_events = start0 + 4 * W
    mu, sd = np.array([0.0, 0.25, -0.5]), np.array([1.0, 0.5, 2.0])
    ev = np.full(n_events, mu[1] + 500 * sd[1])
    ev[start0 + diff + ta] = ev[start0 + diff + tb] = mu[1]

    def fresh():
        fwd = np.zeros((n_bases + 1, W))
        fwd[1] = row
        starts = np.zeros(n_bases, np.int64)
        starts[0] = start0
        return fwd, starts
    fwd_o, starts_o = fresh()
    tb_o = np.zeros((n_bases + 1, W), np.int8)
    assert oracle.adaptive_banded_forward_pass(fwd_o, tb_o, starts_o, ev, mu, sd, -0.0, 1000.0, 1000.0, 1, -15.0,
                                               False, 5.0) == 0
    # the case is what it says: the two zeros of either sign are the row's maxima, the first one places the next band
    assert starts_o[1] == start0 + diff and starts_o[2] == starts_o[1] + ta - half + 1
    assert np.flatnonzero(fwd_o[2] == 0.0).tolist() == [ta, tb] and fwd_o[2].max() == 0.0
    assert np.signbit(fwd_o[2][[ta, tb]]).tolist() == [first_negative, not first_negative]
    eng = get_engine(0)
    fwd_g, starts_g = fresh()
    tb_g = np.zeros((n_bases + 1, W), np.int64)
    rc = eng._L.tba_c_adaptive_banded_forward_pass(eng._h, fwd_g, tb_g, n_bases, W, starts_g, ev, n_events, mu, sd,
                                                   -0.0, 1000.0, 1000.0, 1, -15.0, 0, 5.0)
    what = (cpl, lane, a, b, first_negative)
    assert rc == 0, what
    assert np.array_equal(starts_g, starts_o), (what, starts_g, starts_o)
    assert np.array_equal(zc.bits(fwd_g[2:]), zc.bits(fwd_o[2:])), what
    assert np.array_equal(tb_g[2:], tb_o[2:].astype(np.int64)), what


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_positive_and_negative_zero_share_a_lane(cpl):
    """(e): every pair of positions of a lane of the band's right half, the negative zero first and second"""
    for a in range(cpl):
        for b in range(a + 1, cpl):
            for first_negative in (True, False):
                _signed_zero_case(cpl, 45, a, b, first_negative)


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_rows_of_minus_infinity_but_one_cell(cpl):
    """(f): with skip_pen = +inf a cell whose z is -inf is -inf.  Rows 9 (static), 31, 52 and the last one have a
    single finite z, under a cell of the band's right half whose diagonal source is finite: one live cell, every
    lane's maximum but one is -inf, and the row behind it grows back from that cell by stay moves alone"""
    W = zc.band(cpl)
    rng = np.random.default_rng(77 + cpl)
    z = rng.integers(-48, 33, (zc.N_ROWS, W)) / 8.0
    static = np.cumsum(rng.integers(0, 3, zc.N_STATIC)).astype(np.int64)
    inf = float('inf')
    for r in (9, 31, 52, zc.N_ROWS - 1):
        fwd, _, starts, _ = zc.reference(z[:r + 1], static[:r + 1], inf, zc.STAY_PEN)   # (row r's start: not from its z)
        diff = int(starts[r] - starts[r - 1])
        ok = [b for b in range(W // 2 + 3, W) if b + diff - 1 < W and np.isfinite(fwd[r][b + diff - 1])]
        assert ok, (cpl, r)
        b = ok[(r * 7) % len(ok)]
        z[r] = -inf
        z[r, b] = 1.25
    ref = zc.reference(z, static, inf, zc.STAY_PEN)
    for r in (9, 31, 52, zc.N_ROWS - 1):
        assert np.isfinite(ref[0][r + 1]).sum() == 1
    assert np.isfinite(ref[0][zc.N_ROWS][ref[3]])
    zc.assert_same(zc.run_gpu(z, static, inf, zc.STAY_PEN), ref, cpl)

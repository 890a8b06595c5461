"""The stay chain of a forward-pass row (csrc/k_dp.h: sweep 1 starts from its first candidate, the first carry sweep
runs without a convergence test in front of it) through k_dp<CPL, true> on z matrices made for it, against the
oracle's forward pass over the same matrix (dp_zmat_case.py: classes 4, 5, 8, 12 at W = 64 CPL - 3, 70 rows, 20 of
them static).  Every comparison is exact: forward rows bit for bit, moves, band starts, top_pos.

  - stay runs over 30 and more cells (three lanes and more; starting on a lane's first cell, inside a lane, on band
    cell 1; ending at the band's end): as many carry sweeps as lanes crossed;
  - a run that dies in cell 0 of the lane it enters (z = -inf there), and one that dies in that lane's second cell;
  - a run's value in cell 0 of a lane equal to that cell's skip candidate, bit for bit: the oracle's strict `>` keeps
    the stay, so must the kernel (and the same tie in a lane's last cell);
  - rows in which no lane hands anything on (the last cell of every lane is -inf under skip_pen = +inf: the row the
    kernel's dropped first test was for) between rows that do; such a row is not dead -- its other cells live, and
    the rows behind it go on from them.  A row whose cells are ALL -inf can only be followed by rows like it (-inf is
    all a move can take from it): the matrix ends in three of them;
  - a NaN in one z entry (the z-matrix entry) and in one event (tba_c_adaptive_banded_forward_pass): the status is the
    oracle's -- its forward pass goes on and reports nothing -- and every row before the NaN's equals the oracle's.
    The rows from there on are not compared: the oracle's comparisons carry a NaN on as a stay move's value and ignore
    it as a candidate, v_max_f64 ignores it in both.

The moves of band cell 0 are compared except where that cell is -inf (dp_zmat_case.assert_same says why)."""
import numpy as np
import pytest

import dp_zmat_case as zc

pytestmark = pytest.mark.gpu

RUN_Z = 50.0     # above stay_pen: every stay move of a run gains


def _runs_matrix(cpl):
    """the class's base rows with stay runs laid over rows 5 .. 65, static and adaptive"""
    z, static, _ = zc.base(cpl, seed=1)
    z = z.copy()
    W = z.shape[1]
    L = lambda lane, j=0: lane * cpl + j
    runs = [(5, L(3), 34), (12, L(10, cpl // 2), 40), (23, 1, 45), (30, L(40), 3 * cpl + 1), (37, W - 35, 35),
            (44, L(20, cpl - 1), 31), (51, L(2), W - L(2)), (58, L(50, 1), 64), (65, L(7), 30)]
    for r, b0, n in runs:
        n = min(n, W - b0)
        z[r, b0:b0 + n] = RUN_Z
        z[r, b0 + n:] = np.minimum(z[r, b0 + n:], -1.0)
    # a run that dies on the first cell of the lane it enters, and one that dies on that lane's second cell
    z[16, L(30, 1):L(33)] = RUN_Z
    z[16, L(33)] = -np.inf
    z[47, L(30, 1):L(33, 1)] = RUN_Z
    z[47, L(33, 1)] = -np.inf
    return z, static, runs


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_stay_runs_across_lanes(cpl):
    z, static, runs = _runs_matrix(cpl)
    ref = zc.reference(z, static)
    fwd, tb = ref[0], ref[1]
    for r, b0, n in runs:       # the cases are what they say: an unbroken stretch of stay moves over three lanes and more
        n = min(n, z.shape[1] - b0)
        stays = ''.join('s' if m == 0 else '.' for m in tb[r + 1, b0 + 1:b0 + n])
        assert n < 30 or max(len(x) for x in stays.split('.')) >= 2 * cpl + 2, (r, b0, n, stays)     # (cells in three lanes at least)
    b = 33 * cpl
    assert tb[17, b] != 0 and tb[17, b - 1] == 0 and np.isfinite(fwd[17, b])       # died in cell 0: another move's cell
    assert tb[48, b] == 0 and tb[48, b + 1] != 0
    zc.assert_same(zc.run_gpu(z, static), ref, cpl)


def _tie_row(prev, offset, cell, cpl):
    """a z row with a stay run over the two lanes before `cell` whose value IN `cell` equals the cell's skip candidate
    exactly: z[cell] = (skip - run value before it) + stay_pen, every term a multiple of 1/8"""
    W = prev.shape[0]
    z = np.full(W, zc.LOW)
    b0 = cell - 2 * cpl
    z[b0:cell] = RUN_Z
    cur = prev[b0 + offset - 1] + z[b0]                 # the run starts by a diagonal move from a finite cell ...
    assert np.isfinite(cur)
    for b in range(b0 + 1, cell):
        stay = (cur - zc.STAY_PEN) + z[b]
        assert stay > prev[b + offset - 1] + z[b] and stay > prev[b + offset] - zc.SKIP_PEN     # ... and stays
        cur = stay
    skip = prev[cell + offset] - zc.SKIP_PEN
    z[cell] = (skip - cur) + zc.STAY_PEN
    assert (cur - zc.STAY_PEN) + z[cell] == skip and prev[cell + offset - 1] + z[cell] < skip
    return z


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_stay_ties_the_candidate_exactly(cpl):
    """in cell 0 of a lane (the incoming value against the lane's first candidate) and in a lane's last cell, at band
    offsets 0 .. 3: the move is the stay, the value the common one"""
    for k, cell in enumerate((17 * cpl, 40 * cpl, 25 * cpl + cpl - 1, 61 * cpl)):
        z, static, ref = zc.tail_case(cpl, k % 4, lambda prev, off: _tie_row(prev, off, cell, cpl))
        assert ref[1][zc.N_ROWS, cell] == 0 and ref[1][zc.N_ROWS, cell + 1] != 0
        zc.assert_same(zc.run_gpu(z, static), ref, (cpl, cell))


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_rows_no_lane_hands_on_and_dead_rows(cpl):
    W = zc.band(cpl)
    rng = np.random.default_rng(300 + cpl)
    z = rng.integers(-48, 33, (zc.N_ROWS, W)) / 8.0
    static = np.cumsum(rng.integers(0, 3, zc.N_STATIC)).astype(np.int64)
    inf = float('inf')
    quiet = (7, 8, 26, 40, 41, 60)
    for r in quiet:
        z[r, cpl - 1::cpl] = -inf           # the last cell of every lane
    z[33, 0::cpl] = -inf                    # (the first cell of every lane: every chain dies on entry, none is quiet)
    z[zc.N_ROWS - 3:] = -inf                # dead to the end
    ref = zc.reference(z, static, inf, zc.STAY_PEN)
    fwd = ref[0]
    for r in quiet:
        assert np.all(np.isneginf(fwd[r + 1, cpl - 1::cpl])) and np.isfinite(fwd[r + 1]).sum() >= W // 4
        assert np.isfinite(fwd[r + 2]).sum() >= W // 4
    assert np.all(np.isneginf(fwd[zc.N_ROWS - 2:])) and np.isfinite(fwd[zc.N_ROWS - 3]).any() and ref[3] == 0
    zc.assert_same(zc.run_gpu(z, static, inf, zc.STAY_PEN), ref, cpl)


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_nan_in_one_z_entry(cpl):
    """in a lane's first cell, in its last, and in band cell 1, of an adaptive row"""
    z0, static, _ = zc.base(cpl)
    ref0 = zc.reference(z0, static)
    r = 40
    for b in (22 * cpl, 22 * cpl + cpl - 1, 1):
        z = z0.copy()
        z[r, b] = np.nan
        rc, fwd, tb, starts, top = zc.run_gpu(z, static)
        assert rc == 0, (cpl, b, rc)                       # the oracle's forward pass has no failure for it either
        assert np.array_equal(starts[:r + 1], ref0[2][:r + 1]), (cpl, b)
        assert np.array_equal(zc.bits(fwd[:r + 1]), zc.bits(ref0[0][:r + 1])), (cpl, b)
        assert np.array_equal(tb[1:r + 1], ref0[1][1:r + 1]), (cpl, b)


@pytest.mark.parametrize('cpl', zc.CLASSES)
def test_nan_in_one_event(cpl):
    """the adaptive entry from a given row of zeros: the status is the oracle's (0), the rows whose band ends before
    the NaN event equal the oracle's"""
    import oracle
    from tombo_amd.resquiggle import get_engine
    W = zc.band(cpl)
    n_bases = 12
    rng = np.random.default_rng(900 + cpl)
    n_events = 3 * W
    ev = rng.integers(-16, 17, n_events) / 8.0
    nan_at = W + 3                 # behind the first rows' bands (they start at event 0), inside the later ones'
    ev[nan_at] = np.nan
    mu, sd = rng.integers(-8, 9, n_bases) / 8.0, np.full(n_bases, 0.5)

    def fresh():
        return np.zeros((n_bases + 1, W)), np.zeros(n_bases, np.int64)
    fwd_o, starts_o = fresh()
    tb_o = np.zeros((n_bases + 1, W), np.int8)
    st_o = oracle.adaptive_banded_forward_pass(fwd_o, tb_o, starts_o, ev, mu, sd, 4.0, zc.SKIP_PEN, zc.STAY_PEN, 1,
                                               -15.0, False, 5.0)
    clean = [r for r in range(1, n_bases) if starts_o[r] + W <= nan_at]       # rows whose band lies before the NaN
    assert st_o == 0 and 1 <= len(clean) < n_bases - 1 and clean == list(range(1, len(clean) + 1))
    eng = get_engine(0)
    fwd_g, starts_g = fresh()
    tb_g = np.zeros((n_bases + 1, W), np.int64)
    rc = eng._L.tba_c_adaptive_banded_forward_pass(eng._h, fwd_g, tb_g, n_bases, W, starts_g, ev, n_events, mu, sd,
                                                   4.0, zc.SKIP_PEN, zc.STAY_PEN, 1, -15.0, 0, 5.0)
    assert rc == st_o, (cpl, rc)
    k = clean[-1]
    assert np.array_equal(starts_g[:k + 1], starts_o[:k + 1]), cpl
    assert np.array_equal(zc.bits(fwd_g[2:k + 2]), zc.bits(fwd_o[2:k + 2])), cpl
    assert np.array_equal(tb_g[2:k + 2], tb_o[2:k + 2].astype(np.int64)), cpl

"""The ROC kernels of csrc/k_roc.h (Engine.roc_motif_labels, roc_loc_labels, roc_rank_counts) against the live
reference's recorded results (tests/golden/stats_roc.npz) and, beyond the fixture, against the numpy restatement that
tests/test_roc_reference.py pins to the same fixture.  No tolerance: integer counts and single divisions."""
import numpy as np
import pytest

import roc_cases as rc
import roc_reference as ref
from roc_stub_engine import NumpyRocEngine
from launch_caps import GRID_PASS   # threads of one launch (grid_for in csrc/tba_engine.hip)
from tombo_amd import tombo_stats as ts, resquiggle as rq, _native

pytestmark = pytest.mark.gpu

T = _native.ROC_SORT_TILE
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
CASES = sorted(rc.meta()['cases'])


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


# ---- roc_rank_counts ------------------------------------------------------------------------------------
def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def _labels(rng, n):
    return rng.integers(0, 2, n).astype(bool)


PATTERNS = {
    'all_equal': lambda rng, n: (np.full(n, 1.25), _labels(rng, n)),
    'two_keys': lambda rng, n: (rng.choice([0.5, -3.0], n), _labels(rng, n)),
    'sorted': lambda rng, n: (np.arange(n) / 64.0 - 7, _labels(rng, n)),
    'reversed': lambda rng, n: (np.arange(n)[::-1] / 64.0 - 7, _labels(rng, n)),
    'low_byte': lambda rng, n: (_from_bits(np.float64(1.0).view(np.uint64) + rng.integers(0, 256, n).astype(np.uint64)),
                                _labels(rng, n)),
    # the eight highest bits vary, the four exponent bits below them are 0: never inf or NaN
    'high_byte': lambda rng, n: (_from_bits((rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56)) |
                                            np.uint64(0x0001234567890ABC)), _labels(rng, n)),
    'neg_zero': lambda rng, n: (lambda z: (np.where(z, -0.0, 0.0), z))(_labels(rng, n)),   # -0.0 True, 0.0 False
    'inf': lambda rng, n: (rng.choice([-np.inf, np.inf, 0.0, 1e308, -1e308], n), _labels(rng, n)),
    'denormal': lambda rng, n: (rng.choice([5e-324, -5e-324, 1e-310, 0.0, -1e-310, 2.2250738585072014e-308], n),
                                _labels(rng, n)),
    'all_true': lambda rng, n: (rng.integers(-300, 300, n) / 64.0, np.ones(n, dtype=bool)),
    'all_false': lambda rng, n: (rng.integers(-300, 300, n) / 64.0, np.zeros(n, dtype=bool)),
    'ties': lambda rng, n: (rng.integers(-20, 20, n) / 64.0 * rng.choice([1, 1024], n), _labels(rng, n)),
}


def plot_ranks(n):
    """the index sets of compute_accuracy_rates (1000 and 1001 points), merged"""
    return np.union1d(np.linspace(0, n - 1, 1000).astype(np.int64), np.linspace(0, n - 1, 1001).astype(np.int64))


def check_rank_counts(eng, stats, has_mod, ranks):
    got = eng.roc_rank_counts(stats, has_mod, ranks)
    want = ref.rank_counts(stats, has_mod, ranks)
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0])
    assert got[1:] == want[1:]
    return got


def test_sort_tile_of_the_library(eng):
    assert eng._L.tba_roc_sort_tile() == T


@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_rank_counts_sizes(eng, pattern):
    for n in SIZES:
        rng = np.random.default_rng(n)
        stats, has_mod = PATTERNS[pattern](rng, n)
        check_rank_counts(eng, stats, has_mod, np.arange(n, dtype=np.int64))
        check_rank_counts(eng, stats, has_mod, plot_ranks(n))


def test_neg_zero_orders_by_label(eng):
    """bitwise -0.0 sorts below 0.0; as floats they tie and False comes first"""
    stats, has_mod = np.array([-0.0, 0.0, -0.0, 0.0]), np.array([True, False, True, False])
    tp_at, total, n_nan = eng.roc_rank_counts(stats, has_mod, np.arange(4, dtype=np.int64))
    assert tp_at.tolist() == [0, 0, 1, 2] and total == 2 and n_nan == 0


@pytest.mark.parametrize('pattern', ['ties', 'low_byte'])
def test_rank_counts_beyond_one_grid_pass(eng, pattern):
    n = GRID_PASS + 1
    stats, has_mod = PATTERNS[pattern](np.random.default_rng(5), n)
    ranks = plot_ranks(n)
    got = check_rank_counts(eng, stats, has_mod, ranks)
    again = eng.roc_rank_counts(stats, has_mod, ranks)
    assert np.array_equal(got[0], again[0]) and got[1:] == again[1:]


def test_rank_counts_random_doubles(eng):
    """all eight passes: keys that differ in every byte"""
    n = 3 * T + 17
    rng = np.random.default_rng(11)
    stats = rng.standard_normal(n) * np.exp(rng.uniform(-300, 300, n))
    has_mod = _labels(rng, n)
    got = check_rank_counts(eng, stats, has_mod, np.arange(n, dtype=np.int64))
    again = eng.roc_rank_counts(stats, has_mod, np.arange(n, dtype=np.int64))
    assert np.array_equal(got[0], again[0]) and got[1:] == again[1:]


def test_rank_counts_reports_nan(eng):
    stats = np.array([0.5, np.nan, 1.0, -np.nan, 0.25])
    tp_at, total, n_nan = eng.roc_rank_counts(stats, np.array([True, False, True, True, False]), np.array([4], dtype=np.int64))
    assert n_nan == 2 and total == 3
    with pytest.raises(ValueError, match='^NaN statistic$'):
        ts.prep_accuracy_rates({'x': ts.MotifStats(stats, [True, False, True, True, False])}, engine=eng)


def test_rank_counts_empty_and_bad_ranks(eng):
    tp_at, total, n_nan = eng.roc_rank_counts(np.zeros(0), np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64))
    assert tp_at.shape == (0,) and total == 0 and n_nan == 0
    with pytest.raises(ValueError):
        eng.roc_rank_counts(np.zeros(3), np.zeros(3, dtype=bool), np.array([3], dtype=np.int64))
    # the C entry refuses what the binding would have refused
    st, hm, rk = np.zeros(3), np.zeros(3, dtype=np.uint8), np.array([2, 1], dtype=np.int64)
    out, tot, nn = np.zeros(2, dtype=np.int64), _native.i64(0), _native.i64(0)
    import ctypes as C
    rc_ = eng._L.tba_roc_rank_counts(eng._h, _native.i64(3), st, hm, _native.i64(2), rk, out, C.byref(tot), C.byref(nn), None)
    assert rc_ == -1 and b'ranks' in eng._L.tba_last_error()


# ---- label kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_fixture_labels(eng, case):
    rc.check_case(case, rc.run_case(case, eng))


def test_edge_rule(eng, tmp_path):
    rc.check_edge_rule(eng, tmp_path)


def _codes(seq):
    return ts._SEQ_CODE[np.frombuffer(seq.encode(), dtype=np.uint8)]


def both_motif(eng, *args, **kw):
    got = eng.roc_motif_labels(*args, return_index=True, **kw)
    want = NumpyRocEngine().roc_motif_labels(*args, return_index=True, **kw)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert rc.same_signed(g[0], w[0]) and rc.same(g[1], w[1]) and rc.same(g[2], w[2])
    return got


def motif(text, mod_pos):
    return ts.motif_base_sets(ts.th.TomboMotif(text, mod_pos))


def test_motif_as_long_as_the_window(eng):
    seq = 'CCAGG'
    args = (np.array([0, 1], dtype=np.uint8), np.array([100, 100], dtype=np.int64), np.array([0, 5, 10], dtype=np.int64),
            np.concatenate([_codes(seq), _codes('CCTGG')]), np.array([0, 5, 10], dtype=np.int64),
            np.tile(np.arange(100, 105), 2).astype(np.int64), np.arange(10) / 8.0, [motif('CCWGG', 2), motif('CCWGG', 4)])
    got = both_motif(eng, *args)
    assert got[0][2].tolist() == [0, 1, 8, 9] and got[0][1].tolist() == [False, True, True, False]
    got = both_motif(eng, *args, ctrl_label=False)
    assert got[0][2].tolist() == [1, 8] and not got[0][1].any()
    assert both_motif(eng, *args, ctrl_label=True)[1][1].all()


def test_blocks_without_records_and_absent_mod_base(eng):
    seq = 'ACCAGGACGA' * 3          # no T
    args = (np.array([0, 1, 0], dtype=np.uint8), np.array([0, 50, 7], dtype=np.int64), np.array([0, 30, 30, 60], dtype=np.int64),
            np.concatenate([_codes(seq), _codes(seq)]), np.array([0, 0, 0, 4], dtype=np.int64),
            np.array([7, 8, 36, 30], dtype=np.int64), np.array([1.0, -0.0, 0.0, 2.0]),
            [motif('TG', 1), motif('CG', 1), motif('NCG', 2)])
    got = both_motif(eng, *args)
    assert got[0][0].shape == (0,) and got[1][0].shape[0] > 0
    # no record at all: nothing is launched
    empty = args[:4] + (np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)) + args[7:]
    assert all(r[0].shape == (0,) for r in eng.roc_motif_labels(*empty))


def test_many_blocks_and_chunks(eng):
    """300 blocks of one record, then blocks of many: more than one chunk per motif, three motifs"""
    rng = np.random.default_rng(8)
    per = np.concatenate([np.ones(300, dtype=np.int64), [0, 1500, 0, 0, 2049, 7]])
    n_blk = per.shape[0]
    lens = rng.integers(20, 60, n_blk)
    seq = rng.choice(np.array([0, 1, 2, 3, 4], dtype=np.uint8), int(lens.sum()), p=[.24, .24, .24, .24, .04])
    s_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ss = rng.integers(0, 1000, n_blk).astype(np.int64)
    blk = np.repeat(np.arange(n_blk), per)
    pos = ss[blk] + rng.integers(-2, 62, blk.shape[0])             # some outside their block's sequence
    args = (rng.integers(0, 2, n_blk).astype(np.uint8), ss, s_off, seq, np.concatenate([[0], np.cumsum(per)]).astype(np.int64),
            pos.astype(np.int64), rng.integers(-64, 64, blk.shape[0]) / 64.0,
            [motif('CG', 1), motif('NNANN', 3), motif('GATC', 2)])
    both_motif(eng, *args)
    both_motif(eng, *args, ctrl_label=True)


def test_location_in_both_lists(eng):
    mod, unmod = np.array([5, 9, 40, 7], dtype=np.int64), np.array([9, 11, 3, 7, 8], dtype=np.int64)
    blk_loc = np.array([[0, 3, 0, 2], [0, 0, 0, 0], [3, 4, 2, 5]], dtype=np.int64)
    off = np.array([0, 6, 6, 10], dtype=np.int64)
    pos = np.array([9, 5, 11, 12, 9, 40, 7, 3, 5, 8], dtype=np.int64)
    stat = np.arange(10) / 4.0
    got = eng.roc_loc_labels(blk_loc, mod, unmod, off, pos, stat, return_index=True)
    want = ref.loc_labels(blk_loc, mod, unmod, off, pos, stat)
    assert all(rc.same(g, w) for g, w in zip(got, want))
    assert got[2].tolist() == [0, 1, 2, 4, 5, 6, 7, 9] and got[1].tolist() == [True, True, False, True, True, True, False, False]
    with pytest.raises(ValueError):
        eng.roc_loc_labels(np.array([[0, 5, 0, 0]], dtype=np.int64), mod, unmod, off[[0, 3]], pos, stat)


def test_c_entries_validate_before_the_empty_return(eng):
    """no record: nothing is launched, but a bad motif, bad sequence offsets or a bad location slice are still refused"""
    import ctypes as C
    i64, f64, p = _native.i64, _native.f64, lambda a, t: a.ctypes.data_as(C.POINTER(t))
    minus, ss, rec_off = np.zeros(1, np.uint8), np.zeros(1, np.int64), np.zeros(2, np.int64)
    seq, sets = np.zeros(4, np.uint8), np.array([2, 4], dtype=np.uint8)
    out_s, out_l, counts = np.zeros(1), np.zeros(1, np.uint8), np.zeros(1, np.int64)

    def motif_call(seq_off, table):
        seq_off, table = np.array(seq_off, dtype=np.int64), np.array(table, dtype=np.int32)
        return eng._L.tba_roc_motif_labels(
            eng._h, i64(1), p(minus, C.c_uint8), p(ss, i64), p(seq_off, i64), p(seq, C.c_uint8), p(rec_off, i64),
            p(ss, i64), p(out_s, f64), i64(1), p(table, _native.i32), p(sets, C.c_uint8), C.c_int(0), C.c_int(0),
            p(out_s, f64), p(out_l, C.c_uint8), None, p(counts, i64), None)

    assert motif_call([0, 4], [2, 1, 1]) == 0
    assert motif_call([0, 4], [2, 3, 1]) == -1 and b'motif' in eng._L.tba_last_error()
    assert motif_call([0, 4], [0, 1, 1]) == -1
    assert motif_call([1, 4], [2, 1, 1]) == -1 and b'offset' in eng._L.tba_last_error()
    assert motif_call([4, 0], [2, 1, 1]) == -1
    locs = np.array([5, 9], dtype=np.int64)

    def loc_call(blk_loc):
        blk_loc = np.array(blk_loc, dtype=np.int64)
        return eng._L.tba_roc_loc_labels(
            eng._h, i64(1), p(blk_loc, i64), p(locs, i64), i64(2), p(locs, i64), i64(2), p(rec_off, i64), p(ss, i64),
            p(out_s, f64), p(out_s, f64), p(out_l, C.c_uint8), None, p(counts, i64), None)

    assert loc_call([0, 2, 0, 2]) == 0
    assert loc_call([0, 3, 0, 2]) == -1 and b'slice' in eng._L.tba_last_error()
    assert loc_call([0, 2, 2, 1]) == -1


# ---- end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['motif_pr_cg_plain', 'motif_pr_two_plain', 'ctrl_pr_self_plain', 'truth_ms'])
def test_stats_to_plot_numbers(eng, case):
    g, res = rc.gold(), rc.run_case(case, eng)
    rc.check_case(case, res)
    summary = {}
    tp, fp, prec, names = ts.prep_accuracy_rates(dict((k, v) for k, v in res.items() if len(v)), engine=eng,
                                                 summary=summary)
    assert rc.same(np.array(tp, dtype=np.float64), g['rates|%s|tp' % case])
    assert rc.same(np.array(fp, dtype=np.float64), g['rates|%s|fp' % case])
    assert rc.same(np.array(prec, dtype=np.float64), g['rates|%s|precision' % case])
    rc.check_rates(case, eng)

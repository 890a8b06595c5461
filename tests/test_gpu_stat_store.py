"""Stored per-read statistics aggregated on the device (Engine.site_aggregate, kernel k_site_rec of csrc/k_site.h)
against the live reference's _agg_stats_worker (tests/golden/stats_store.npz) and, at the size edges, against the
numpy restatement that tests/test_stat_store_reference.py pins to the same fixture.  No tolerance: integer counts
and single divisions."""
import numpy as np
import pytest

import stat_store_cases as sc
from stat_store_stub_engine import NumpyStatStoreEngine
from launch_caps import GRID_PASS   # threads of one launch (grid_for in csrc/tba_engine.hip)
from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq, _native

pytestmark = pytest.mark.gpu

AGGS = ('lower', 'abs', 'all', 'lower_damp')


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


def records(pos, stat):
    rec = np.zeros(len(pos), dtype=_native.PER_READ_DTYPE)
    rec['pos'], rec['stat'], rec['read_id'] = pos, stat, np.arange(len(pos)) % 7
    return rec


def both(eng, args, single, lower=None, abs_rule=False, damp=None):
    got = eng.site_aggregate(*args, single, lower, abs_rule, damp)
    sc.check_equal_results(got, NumpyStatStoreEngine().site_aggregate(*args, single, lower, abs_rule, damp))
    return got


@pytest.mark.parametrize('name', AGGS)
@pytest.mark.parametrize('with_damp', [True, False])
def test_fixture_parity(eng, name, with_damp):
    stat_type, single, lower, damp, _ = sc.agg_case(name)
    args = sc.agg_inputs(name) + (single, lower, stat_type == 'model_compare', damp if with_damp else None)
    res = eng.site_aggregate(*args)
    sc.check_site_fractions(name, res, with_damp)
    empty = np.flatnonzero(np.diff(args[2]) == 0)                             # (the block without records)
    assert res.per_read is None and empty.shape[0] == 1 and res.counts[empty[0]] == 0 == res.n_stats[empty[0]]
    sc.check_equal_results(res, eng.site_aggregate(*args))


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 257, GRID_PASS + 1])
def test_record_counts(eng, n):
    rng = np.random.default_rng(n)
    starts = np.array([5000, 100, 70000, 0, 4000000000, 9, 300], dtype=np.int64)
    ends = starts + np.array([1000, 37, 1, 64, 290, 1000, 129])
    per = rng.multinomial(n, [0.3, 0.1, 0.0, 0.1, 0.2, 0.2, 0.1])
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    blk = np.repeat(np.arange(7), per)
    pos = starts[blk] + rng.integers(0, 1 << 30, n) % (ends - starts)[blk]
    stat = rng.integers(0, 65, n) / 64.0
    res = both(eng, (starts, ends, off, records(pos, stat)), 0.5, 0.25, False, (2, 1))
    assert res.n_stats.sum() == n


def test_one_block_of_one_position(eng):
    rec = records([77] * 5, [0.1, 0.9, 0.5, 0.3, 0.7])
    res = both(eng, ([77], [78], [0, 5], rec), 0.5, None, False, (0, 0))
    assert (res.counts[0], res.poss[0], res.cov[0], res.valid[0], res.frac[0]) == (1, 77, 5, 5, 0.6)


def test_300_blocks_of_one_record(eng):
    starts = np.arange(300, dtype=np.int64) * 13
    rng = np.random.default_rng(3)
    pos = starts + rng.integers(0, 13, 300)
    res = both(eng, (starts, starts + 13, np.arange(301), records(pos, rng.integers(0, 3, 300) / 2.0)), 0.5)
    assert np.all(res.counts == 1) and np.array_equal(res.poss[res.pos_off[:-1]], pos)


def test_all_records_at_the_last_position(eng):
    res = both(eng, ([10, 500], [110, 600], [0, 0, 40], records([599] * 40, np.arange(40) / 40.0)), 0.5, 0.25)
    assert res.counts.tolist() == [0, 1] and res.poss[100] == 599 and res.cov[100] == 40


def test_nan_statistics_are_dropped(eng):
    stat = np.array([0.9, np.nan, 0.1, np.nan, np.nan, 0.6])
    res = both(eng, ([0], [10], [0, 6], records([3, 3, 3, 4, 4, 9], stat)), 0.5, None, False, (2, 0))
    assert res.counts[0] == 2 and res.poss[:2].tolist() == [3, 9] and res.cov[:2].tolist() == [2, 1] and res.n_stats[0] == 3


@pytest.mark.parametrize('single, lower, abs_rule', [(0.5, 0.25, False), (2.0, None, True), (0.5, None, False),
                                                     (2.5, -1.5, True)])
def test_statistics_equal_to_a_threshold(eng, single, lower, abs_rule):
    vals = [single, np.nextafter(single, -np.inf), np.nextafter(single, np.inf), -single, np.nextafter(-single, 0)]
    if lower is not None:
        vals += [lower, np.nextafter(lower, -np.inf), np.nextafter(lower, np.inf)]
    pos = np.arange(len(vals)).repeat(3)
    res = both(eng, ([0], [len(vals)], [0, pos.shape[0]], records(pos, np.repeat(vals, 3))), single, lower, abs_rule)
    assert res.valid[0] == 3 and res.frac[0] == 1.0      # a statistic equal to single_read_thresh is valid and counted


def test_record_outside_its_block_fails_the_call(eng):
    starts, ends, off = [100, 300, 500], [200, 400, 600], [0, 3, 6, 9]
    good = records([100, 199, 150, 300, 399, 301, 500, 599, 501], np.arange(9) / 8.0)
    for where, pos in ((4, 400), (4, 299), (0, 99), (8, 600), (3, 0), (5, 4294967295)):
        bad = good.copy()
        bad['pos'][where] = pos
        with pytest.raises(_native.EngineError, match=r'tba_site_aggregate failed \(-1\): record position outside'):
            eng.site_aggregate(starts, ends, off, bad, 0.5)
        both(eng, (starts, ends, off, good), 0.5, None, False, (2, 0))    # the next, valid call is not disturbed


def test_host_argument_errors_launch_nothing(eng):
    """straight at the C entry (the binding's own checks would stop these first): TBA_E_ARG and untouched outputs"""
    import ctypes as C
    i64, f64 = C.c_int64, C.c_double
    rec = records([1, 2], [0.5, 0.5])

    def call(starts, ends, off, recs=rec, frac_out=True):
        bs, be, o = (np.array(v, dtype=np.int64) for v in (starts, ends, off))
        frac = np.full(64, -3.0)
        ints = [np.full(64, -3, dtype=np.int64) for _ in range(5)]
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
        rc = eng._L.tba_site_aggregate(
            eng._h, i64(bs.shape[0]), p(bs, i64), p(be, i64), p(o, i64), None if recs is None else C.c_void_p(recs.ctypes.data),
            f64(0.5), None, C.c_int(0), None, p(frac, f64) if frac_out else None, p(ints[0], i64), p(ints[1], i64),
            p(ints[2], i64), None, p(ints[3], i64), p(ints[4], i64), None)
        assert np.all(frac == -3.0) and all(np.all(x == -3) for x in ints)
        return rc
    assert call([0], [10], [1, 2]) == -1                                   # offsets do not start at 0
    assert call([0, 10], [10, 20], [0, 2, 1]) == -1                        # ... decrease
    assert call([0], [0], [0, 2]) == -1 and call([5], [3], [0, 2]) == -1   # end <= start
    assert call([0, 0], [2 ** 30, 2 ** 30], [0, 1, 2]) == -1               # 2^31 positions
    assert call([0], [10], [0, 2], recs=None) == -1                        # NULL records
    assert call([0], [10], [0, 2], frac_out=False) == -1                   # NULL output
    assert b'2^31' in eng._L.tba_last_error() or b'bad arguments' in eng._L.tba_last_error()


def test_detect_store_reaggregate(eng):
    assert sc.check_detect_store_reaggregate(ts, th) >= 15

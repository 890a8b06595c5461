"""The documented per-read functions of tombo_stats on the device (csrc/k_norm_api.h) against what the reference
returned (tests/golden/stats_norm_api.npz, cases in tests/norm_api_cases.py): every comparison is by bytes."""
import json

import numpy as np
import pytest

import norm_api_cases as nc
from test_norm_api_reference import check_norm_record, pa_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    g = np.load(nc.GOLDEN)
    return dict((k, g[k]) for k in g.files), json.loads(str(g['meta']))


@pytest.fixture(scope='module')
def cases():
    return nc.norm_cases()


@pytest.fixture(scope='module')
def signal_of():
    cache = {}

    def get(c):
        key = (c.kind, c.dtype, c.n_sig, c.seed)
        if key not in cache:
            cache[key] = nc.case_signal(c)
        return cache[key]
    return get


def _channel():
    from tombo_amd import tombo_helper as th
    return th.channelInfo(nc.CHANNEL[0], nc.CHANNEL[1], nc.CHANNEL[2], 7, 4000.0)


def _scale_values(c):
    from tombo_amd import tombo_helper as th
    return None if c.sv is None else th.scaleValues(c.sv[0], c.sv[1], c.sv[2], c.sv[3], None)


def _single(c, sig):
    """normalize_raw_signal of a case -> (norm, shift, scale, lower, upper) or 'zero_scale'"""
    from tombo_amd import tombo_stats as ts
    try:
        norm, sv = ts.normalize_raw_signal(sig, c.start, c.n, c.norm_type, c.thresh, _channel(), _scale_values(c),
                                           const_scale=c.const_scale)
    except FloatingPointError:
        return 'zero_scale'
    assert sv.outlier_thresh == c.thresh
    return norm, sv.shift, sv.scale, sv.lower_lim, sv.upper_lim


@pytest.fixture(scope='module')
def single_results(cases, signal_of):
    return [_single(c, signal_of(c)) for c in cases]


def test_every_recorded_case_through_the_single_read_function(golden, cases, single_results):
    g, n_checked = golden[0], [0]
    for i, res in enumerate(single_results):
        check_norm_record(g, 'norm', i, res, n_checked)
    n_ok = int((g['norm/failed'] == 0).sum())
    n_full = sum(1 for c, f in zip(cases, g['norm/failed']) if not f and c.n <= nc.MAX_FULL)
    assert n_checked[0] == 3 * n_ok + n_full + (len(cases) - n_ok)


def _same(a, b):
    """two results of _single / entries of the batch form"""
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str)
    return a[0].tobytes() == b[0].tobytes() and all(
        (x is None and y is None) or (x is not None and y is not None and type(x) is type(y)
                                      and np.float64(x).tobytes() == np.float64(y).tobytes())
        for x, y in zip(a[1:], b[1:]))


def test_the_grid_as_one_batch_per_norm_type(cases, signal_of, single_results):
    """all cases that share the call's parameters in one normalize_raw_signal_batch call, reads of all lengths mixed
    and a read with a given scale of 0 in the middle: the results of the single calls, None for that read and for
    the reads whose single call raised"""
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c.dtype, c.norm_type, c.thresh, c.const_scale), []).append(i)
    assert set(k[1] for k in groups) >= set(nc.NORM_TYPES)
    n_none_only_inserted = 0
    for (dtype, norm_type, thresh, const_scale), idx in sorted(groups.items(), key=repr):
        mid = len(idx) // 2
        raws = [signal_of(cases[i]) for i in idx]
        starts, lens = [cases[i].start for i in idx], [cases[i].n for i in idx]
        svs = [_scale_values(cases[i]) for i in idx]
        raws.insert(mid, nc.make_signal('noise', dtype, 777, 9))
        starts.insert(mid, 5)
        lens.insert(mid, 700)
        svs.insert(mid, th.scaleValues(1.0, 0.0, None, None, None))
        out = ts.normalize_raw_signal_batch(raws, starts, lens, norm_type, thresh, [_channel()] * len(raws), svs, const_scale)
        assert len(out) == len(idx) + 1 and out[mid] is None
        del out[mid]
        for i, o in zip(idx, out):
            got = 'zero_scale' if o is None else (o[0],) + tuple(o[1])[:4]
            assert _same(got, single_results[i]), cases[i].name
        n_none_only_inserted += all(o is not None for o in out)
    assert n_none_only_inserted >= 2 * 3 * 3    # 'none', 'pA_raw', 'median_const_scale' under every threshold


def test_int16_equals_the_same_values_as_float64(cases, signal_of, single_results, golden):
    g = golden[0]
    n = 0
    for i, c in enumerate(cases):
        if c.dtype != 'int16' or c.n > 16385:
            continue
        res = _single(c, signal_of(c).astype(np.float64))
        assert _same(res, single_results[i]), c.name     # (also for 'none': shift and scale are the ints 0 and 1)
        if c.norm_type == 'none' and c.sv is None:
            assert g['norm/is_int'][i] and type(res[1]) is int and type(res[2]) is int
        n += 1
    assert n > 250


def test_mom_sums_fit_and_pA(golden):
    from tombo_amd import tombo_stats as ts, resquiggle as rq
    g = golden[0]
    eng = rq.get_engine()
    prev_shift, prev_scale = -1 * nc.CHANNEL[0], nc.CHANNEL[2] / nc.CHANNEL[1]
    pts = [nc.points(n, 100 + n)[:3] for n in nc.POINT_SIZES]
    n_checked, lapack_is_the_recorders, recorded_ok = 0, True, True
    # all reads in one call, and each alone
    off = np.concatenate([[0], np.cumsum(nc.POINT_SIZES)]).astype(np.int64)
    sums = eng.mom_sums(*(np.concatenate([p[j] for p in pts]) for j in range(3)), off)
    for k, (e, m, iv) in enumerate(pts):
        want = nc.mom_sums(e, m, iv)                    # numpy's .sum()
        assert sums[k].tobytes() == want.tobytes(), k
        assert eng.mom_sums(e, m, iv, np.array([0, e.shape[0]], dtype=np.int64))[0].tobytes() == want.tobytes()
        fit = ts.calc_kmer_fitted_shift_scale(prev_shift, prev_scale, e, m, iv, method='mom')
        assert np.array(fit).tobytes() == np.array(nc.mom_fit(prev_shift, prev_scale, want)).tobytes()
        n_checked += 3
        solved = np.array(nc.mom_fit(prev_shift, prev_scale, g['mom/sums'][k]))
        lapack_is_the_recorders = lapack_is_the_recorders and solved.tobytes() == g['mom/fit'][k].tobytes()
        recorded_ok = recorded_ok and np.array(fit).tobytes() == g['mom/fit'][k].tobytes()
    # 'pA': the fit inside normalize_raw_signal
    pa_checked = [0]
    for i, (dtype, sig, start, n, thresh, (e, m, iv)) in enumerate(pa_cases()):
        norm, sv = ts.normalize_raw_signal(sig, start, n, 'pA', thresh, _channel(), None, e, m, iv)
        shift, scale, _, _ = nc.mom_fit(prev_shift, prev_scale, nc.mom_sums(e, m, iv))
        want = nc.normalize(sig, start, n, 'median', thresh, (shift, scale, None, None), None)
        assert _same((norm, sv.shift, sv.scale, sv.lower_lim, sv.upper_lim), want)
        n_checked += 1
        if lapack_is_the_recorders:
            check_norm_record(g, 'pA', i, (norm, sv.shift, sv.scale, sv.lower_lim, sv.upper_lim), pa_checked)
    assert n_checked == 3 * len(nc.POINT_SIZES) + 8
    if not lapack_is_the_recorders:
        pytest.skip("np.linalg.solve of the recorded coefficient matrices does not reproduce the recorded solutions: "
                    "this machine's LAPACK is not the recorder's, the comparison with the recorded 'mom' values is left out")
    assert recorded_ok and pa_checked[0] >= 8 * 3


def test_theil_sen_and_seg_scores(golden):
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    g, meta = golden
    for k, n in enumerate(nc.THEIL_SIZES):
        e, m, _, _ = nc.points(n, 200 + n)
        np.random.seed(300 + n)
        fit = ts.calc_kmer_fitted_shift_scale(0.25, 1.5, e, m, method='theil_sen')
        assert np.array(fit).tobytes() == g['theil_sen/fit'][k].tobytes(), n
    e, _, _, _ = nc.points(50, 250)
    with pytest.raises(th.TomboError) as err:
        ts.calc_kmer_fitted_shift_scale(0.25, 1.5, e, np.full(50, 0.75), method='theil_sen')
    assert str(err.value) == meta['zero_slope_msg']
    triples = []
    for k, n in enumerate(nc.POINT_SIZES):
        e, m, _, sds = nc.points(n, 100 + n)
        triples.append((e, m, sds))
        assert np.float64(ts.get_read_seg_score(e, m, sds)).tobytes() == g['seg_score'][k].tobytes(), n
    batch = ts.get_read_seg_scores_batch(triples)
    assert np.array(batch).tobytes() == g['seg_score'].tobytes()


def test_compute_base_means():
    from tombo_amd import tombo_stats as ts
    sig = nc.make_signal('noise', 'int16', 5000, 77)
    starts = np.concatenate([[0], np.cumsum(np.random.default_rng(3).integers(1, 40, 200))]).astype(np.int64)
    got = ts.compute_base_means(sig, starts)
    x = sig.astype(np.float64)
    want = np.array([np.cumsum(x[a:b])[-1] / (b - a) for a, b in zip(starts[:-1], starts[1:])])     # c_new_means
    assert got.tobytes() == want.tobytes()

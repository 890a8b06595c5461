"""The documented per-read functions of tombo_stats without a GPU: the fixture recorded from the reference
(tests/golden/stats_norm_api.npz) is reproduced bit for bit by the numpy restatement of tests/norm_api_cases.py, the
public functions have the reference's signatures, and their host logic (argument checks, error messages, what becomes
of a failed read, the returned scaleValues) runs against a stub engine that answers with the restatement."""
import inspect
import json

import numpy as np
import pytest

import norm_api_cases as nc


@pytest.fixture(scope='module')
def golden():
    g = np.load(nc.GOLDEN)
    return dict((k, g[k]) for k in g.files), json.loads(str(g['meta']))


@pytest.fixture(scope='module')
def cases(golden):
    cs = nc.norm_cases()
    meta = golden[1]
    assert len(cs) == meta['n_norm_cases'] and nc.sha(np.array('\n'.join(c.name for c in cs))) == meta['case_names_sha']
    return cs


def _signals():
    cache = {}

    def get(c):
        key = (c.kind, c.dtype, c.n_sig, c.seed)
        if key not in cache:
            cache[key] = nc.case_signal(c)
        return '/'.join(map(str, key)), cache[key]
    return get


def check_norm_record(g, prefix, i, res, n_checked):
    """one normalisation result (norm, shift, scale, lower, upper) or 'zero_scale' against record i; counts the
    comparisons into n_checked"""
    if g[prefix + '/failed'][i]:
        assert isinstance(res, str) and res == 'zero_scale'
        n_checked[0] += 1
        return
    norm, shift, scale, lower, upper = res
    want = g[prefix + '/sv'][i]
    none = bool(g[prefix + '/lims_none'][i])
    assert (lower is None) == none and (upper is None) == none
    got = np.array([shift, scale, np.nan if none else lower, np.nan if none else upper], dtype=np.float64)
    assert got.tobytes() == want.tobytes(), (i, got, want)
    assert (isinstance(shift, int) and isinstance(scale, int)) == bool(g[prefix + '/is_int'][i])
    assert norm.dtype == np.float64
    assert bytes.fromhex(nc.sha(norm)) == g[prefix + '/sha'][i].tobytes(), i
    n_checked[0] += 3
    a, b = g[prefix + '/full_off'][i:i + 2]
    if norm.shape[0] <= nc.MAX_FULL:
        assert norm.tobytes() == g[prefix + '/full'][a:b].tobytes(), i
        n_checked[0] += 1
    else:
        assert a == b


def test_fixture_is_small_and_complete(golden, cases):
    import os
    g, meta = golden
    assert os.path.getsize(nc.GOLDEN) < 200 * 1024
    n = len(cases)
    assert g['norm/sv'].shape == (n, 4) and g['norm/sha'].shape == (n, 32) and g['norm/full_off'].shape == (n + 1,)
    failed = [c.name for c, f in zip(cases, g['norm/failed']) if f]
    assert all(any(t in name for t in ('flat/', '/1/', '/2/', '/3/')) for name in failed), failed
    assert sum('flat/' in name for name in failed) == 16
    # both dtypes, every norm type, every threshold, every length as the whole signal and as a window inside one
    seen = set((c.dtype, c.norm_type, c.thresh, c.n, c.start > 0) for c in cases)
    for dtype in ('int16', 'float64'):
        for n_ in nc.LENGTHS:
            for t in nc.NORM_TYPES:
                assert all((dtype, t, th_, n_, False) in seen for th_ in nc.THRESHES)
                assert any((dtype, t, th_, n_, True) in seen for th_ in nc.THRESHES)
    assert g['norm/is_int'].sum() == sum(c.norm_type == 'none' and c.sv is None for c in cases)
    assert 200 * (46.5 / 100.0) == 93.0       # length 201: a whole virtual index


def test_restatement_reproduces_every_recorded_normalisation(golden, cases):
    g, meta = golden
    get, n_checked = _signals(), [0]
    for i, c in enumerate(cases):
        key, sig = get(c)
        assert meta['inputs'][key] == nc.sha(sig), key
        check_norm_record(g, 'norm', i, nc.normalize(sig, c.start, c.n, c.norm_type, c.thresh, c.sv, c.const_scale), n_checked)
    n_ok = int((g['norm/failed'] == 0).sum())
    n_full = sum(1 for c, f in zip(cases, g['norm/failed']) if not f and c.n <= nc.MAX_FULL)
    assert n_checked[0] == 3 * n_ok + n_full + (len(cases) - n_ok)


def test_restatement_reproduces_the_fits_and_scores(golden):
    g, meta = golden
    prev_shift, prev_scale = -1 * nc.CHANNEL[0], nc.CHANNEL[2] / nc.CHANNEL[1]
    for k, n in enumerate(nc.POINT_SIZES):
        e, m, iv, sds = nc.points(n, 100 + n)
        assert meta['inputs']['points/%d' % n] == nc.sha(np.concatenate([e, m, iv, sds]))
        sums = nc.mom_sums(e, m, iv)
        assert sums.tobytes() == g['mom/sums'][k].tobytes()
        fit = np.array(nc.mom_fit(prev_shift, prev_scale, sums))
        if fit[2:].tobytes() == np.array(nc.mom_fit(prev_shift, prev_scale, g['mom/sums'][k]))[2:].tobytes() == g['mom/fit'][k, 2:].tobytes():
            assert fit.tobytes() == g['mom/fit'][k].tobytes()
        else:       # another LAPACK than the recorder's: its solve is not this project's arithmetic
            np.testing.assert_allclose(fit, g['mom/fit'][k], rtol=1e-12)
        assert np.float64(nc.seg_score(e, m, sds)).tobytes() == g['seg_score'][k].tobytes()
    for k, n in enumerate(nc.THEIL_SIZES):
        e, m, _, _ = nc.points(n, 200 + n)
        np.random.seed(300 + n)
        assert np.array(nc.theil_sen_fit(0.25, 1.5, e, m)).tobytes() == g['theil_sen/fit'][k].tobytes(), n
    e, _, _, _ = nc.points(50, 250)
    assert nc.theil_sen_fit(0.25, 1.5, e, np.full(50, 0.75)) == 'zero_slope'


def pa_cases():
    """[(dtype, signal, start, n, thresh, points)] in the fixture's order"""
    out = []
    for dtype in ('int16', 'float64'):
        for n_sig, n_pts in ((65, 129), (4096, 8193)):
            sig = nc.make_signal('noise', dtype, n_sig, 6000 + n_sig)
            for thresh in (None, 5.0):
                out.append((dtype, sig, 3, n_sig - 7, thresh, nc.points(n_pts, 100 + n_pts)[:3]))
    return out


def test_restatement_reproduces_pA(golden):
    g, meta = golden
    prev_shift, prev_scale = -1 * nc.CHANNEL[0], nc.CHANNEL[2] / nc.CHANNEL[1]
    n_checked = [0]
    for i, (dtype, sig, start, n, thresh, (e, m, iv)) in enumerate(pa_cases()):
        assert meta['inputs']['pA/%s/%d' % (dtype, sig.shape[0])] == nc.sha(sig)
        shift, scale, _, _ = nc.mom_fit(prev_shift, prev_scale, nc.mom_sums(e, m, iv))
        if np.array([shift, scale]).tobytes() != g['pA/sv'][i, :2].tobytes():
            continue    # another LAPACK than the recorder's
        res = nc.normalize(sig, start, n, 'median', thresh, (shift, scale, None, None), None)
        check_norm_record(g, 'pA', i, res, n_checked)
    assert g['pA/failed'].sum() == 0


# ---- the public functions ------------------------------------------------------------------------------------
SIGNATURES = {
    'normalize_raw_signal': [('all_raw_signal', None), ('read_start_rel_to_raw', 0), ('read_obs_len', None),
                             ('norm_type', 'median'), ('outlier_thresh', None), ('channel_info', None),
                             ('scale_values', None), ('event_means', None), ('model_means', None),
                             ('model_inv_vars', None), ('const_scale', None)],
    'compute_base_means': [('all_raw_signal', None), ('base_starts', None)],
    'get_read_seg_score': [('r_means', None), ('r_ref_means', None), ('r_ref_sds', None)],
    'calc_kmer_fitted_shift_scale': [('prev_shift', None), ('prev_scale', None), ('r_event_means', None),
                                     ('r_model_means', None), ('r_model_inv_vars', None), ('method', 'theil_sen')],
    'normalize_raw_signal_batch': [('raws', None), ('read_starts', None), ('read_obs_lens', None), ('norm_type', 'median'),
                                   ('outlier_thresh', None), ('channel_infos', None), ('scale_values', None),
                                   ('const_scale', None), ('event_means', None), ('model_means', None),
                                   ('model_inv_vars', None), ('engine', None)],
}
REQUIRED = {'normalize_raw_signal': 1, 'compute_base_means': 2, 'get_read_seg_score': 3, 'calc_kmer_fitted_shift_scale': 4,
            'normalize_raw_signal_batch': 1}


def test_public_names_have_the_reference_signatures():
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    for name, want in SIGNATURES.items():
        params = list(inspect.signature(getattr(ts, name)).parameters.values())
        assert [p.name for p in params] == [w[0] for w in want], name
        for k, (p, w) in enumerate(zip(params, want)):
            if k < REQUIRED[name]:
                assert p.default is inspect.Parameter.empty, (name, p.name)
            else:
                assert p.default == w[1] and type(p.default) is type(w[1]), (name, p.name)
    assert callable(ts.get_read_seg_scores_batch)
    assert th.channelInfo._fields == ('offset', 'range', 'digitisation', 'number', 'sampling_rate')
    assert th.scaleValues._fields == ('shift', 'scale', 'lower_lim', 'upper_lim', 'outlier_thresh')
    assert ts.NORM_TYPES == ('none', 'pA', 'pA_raw', 'median', 'robust_median', 'median_const_scale')


class StubEngine(object):
    """the three engine entries answered by the restatement; records its calls"""

    def __init__(self):
        self.calls = []

    def normalize_raw_batch(self, raws, starts, lens, norm_type, sv_in=None, sv_flags=None, channel=None,
                            outlier_thresh=None, const_scale=None):
        from tombo_amd import _native
        self.calls.append(('normalize_raw_batch', len(raws), raws[0].dtype, norm_type))
        assert len(set(r.dtype for r in raws)) == 1 and raws[0].dtype in (np.int16, np.float64)
        names = {_native.NORMTYPE_NONE: 'none', _native.NORMTYPE_PA_RAW: 'pA_raw', _native.NORMTYPE_MEDIAN: 'median',
                 _native.NORMTYPE_MEDIAN_CONST_SCALE: 'median_const_scale', _native.NORMTYPE_ROBUST_MEDIAN: 'robust_median'}
        n = len(raws)
        sv, has_lims, status, norms = np.zeros((n, 4)), np.zeros(n, np.int32), np.zeros(n, np.int32), []
        for i in range(n):
            given = None
            if sv_flags is not None and sv_flags[i] & 1:
                given = (sv_in[i, 0], sv_in[i, 1]) + ((sv_in[i, 2], sv_in[i, 3]) if sv_flags[i] & 2 else (None, None))
            if names[norm_type] == 'pA_raw' and given is None:
                assert tuple(channel[i]) == nc.CHANNEL
            res = nc.normalize(raws[i], starts[i], lens[i], names[norm_type], outlier_thresh, given, const_scale)
            if isinstance(res, str):
                status[i] = 1
                norms.append(np.zeros(lens[i]))
                continue
            norms.append(res[0])
            has_lims[i] = res[3] is not None
            sv[i] = res[1], res[2], 0.0 if res[3] is None else res[3], 0.0 if res[4] is None else res[4]
        return sv, has_lims, norms, status

    def mom_sums(self, e, m, iv, off):
        self.calls.append(('mom_sums', off.shape[0] - 1))
        return np.array([nc.mom_sums(e[a:b], m[a:b], iv[a:b]) for a, b in zip(off[:-1], off[1:])])

    def seg_scores(self, means, ref_means, ref_sds, off):
        self.calls.append(('seg_scores', off.shape[0] - 1))
        return np.array([nc.seg_score(means[a:b], ref_means[a:b], ref_sds[a:b]) for a, b in zip(off[:-1], off[1:])])


@pytest.fixture
def stub(monkeypatch):
    from tombo_amd import tombo_stats as ts
    eng = StubEngine()
    monkeypatch.setattr(ts, '_engine', lambda engine=None: eng if engine is None else engine)
    return eng


def test_normalize_raw_signal_host_logic(stub, golden):
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    meta = golden[1]
    sig = nc.make_signal('noise', 'int16', 300, 1)
    with pytest.raises(th.TomboError) as err:
        ts.normalize_raw_signal(sig, norm_type='no_such_type')
    assert str(err.value) == meta['invalid_type_msg']
    assert stub.calls == []
    # scale values make any type name acceptable; the given objects come back as they are
    given = th.scaleValues(497.5, 81.25, None, None, None)
    norm, sv = ts.normalize_raw_signal(sig, 5, 100, 'no_such_type', scale_values=given)
    assert sv == given and sv.shift is given.shift and norm.shape == (100,)
    norm, sv = ts.normalize_raw_signal(sig, norm_type='none')
    assert (sv.shift, sv.scale) == (0, 1) and type(sv.shift) is int and type(sv.scale) is int and sv.lower_lim is None
    assert norm.tobytes() == sig.astype(np.float64).tobytes()
    norm, sv = ts.normalize_raw_signal(sig, outlier_thresh=5.0)
    assert sv.outlier_thresh == 5.0 and isinstance(sv.lower_lim, np.float64) and isinstance(sv.shift, np.float64)
    with pytest.raises(AssertionError):
        ts.normalize_raw_signal(sig, norm_type='median_const_scale')
    norm, sv = ts.normalize_raw_signal(sig, norm_type='median_const_scale', const_scale=-12.5)
    assert sv.scale == -12.5
    # a window that runs past the end is cut there, as the reference's slice is
    assert ts.normalize_raw_signal(sig, 290, 100)[0].shape == (10,)
    with pytest.raises(FloatingPointError):
        ts.normalize_raw_signal(np.full(50, 7, np.int16))
    with pytest.raises(AttributeError):
        ts.normalize_raw_signal(sig, norm_type='pA_raw')
    # any other dtype is computed in float64
    for other in (np.float32, np.int32, np.uint16):
        del stub.calls[:]
        norm, sv = ts.normalize_raw_signal(np.abs(sig).astype(other), outlier_thresh=5.0)
        assert stub.calls[0][2] == np.float64
        want = nc.normalize(np.abs(sig).astype(np.float64), 0, 300, 'median', 5.0, None, None)
        assert norm.tobytes() == want[0].tobytes()


def test_batch_returns_none_for_the_failed_read_only(stub):
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    raws = [nc.make_signal('noise', 'int16', n, n) for n in (50, 700)]
    raws.insert(1, np.full(80, 7, np.int16))
    out = ts.normalize_raw_signal_batch(raws, outlier_thresh=5.0)
    assert [o is None for o in out] == [False, True, False] and len(stub.calls) == 1
    for raw, o in zip(raws, out):
        if o is not None:
            want = nc.normalize(raw, 0, raw.shape[0], 'median', 5.0, None, None)
            assert o[0].tobytes() == want[0].tobytes() and tuple(o[1])[:4] == want[1:]
    # a batch that mixes int16 and float64 is computed in float64
    del stub.calls[:]
    ts.normalize_raw_signal_batch([raws[0], raws[2].astype(np.float64)])
    assert stub.calls == [('normalize_raw_batch', 2, np.float64, 2)]
    with pytest.raises(ValueError):
        ts.normalize_raw_signal_batch(raws, read_starts=[0, 0])
    with pytest.raises(ValueError):
        ts.normalize_raw_signal_batch(raws, read_starts=[0, 80, 0])
    assert ts.normalize_raw_signal_batch([]) == []
    # per-read scale values beside reads without any
    given = th.scaleValues(497.5, 81.25, -2.0, 2.0, None)
    out = ts.normalize_raw_signal_batch(raws, scale_values=[None, given, None])
    assert out[1][1] == given and out[0][1].lower_lim is None and np.abs(out[1][0]).max() <= 2.0


def test_fits_and_scores_host_logic(stub, golden):
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    g, meta = golden
    e, m, iv, sds = nc.points(129, 229)
    with pytest.raises(NotImplementedError, match='robust'):
        ts.calc_kmer_fitted_shift_scale(0.0, 1.0, e, m, method='robust')
    with pytest.raises(th.TomboError) as err:
        ts.calc_kmer_fitted_shift_scale(0.0, 1.0, e, m, method='nope')
    assert str(err.value) == ('Invalid k-mer fitted normalization parameter method: nope\n\t\tValid methods are '
                              '"robust" and "mom".')
    got = ts.calc_kmer_fitted_shift_scale(0.25, 1.5, e, m, iv, method='mom')
    assert np.array(got).tobytes() == np.array(nc.mom_fit(0.25, 1.5, nc.mom_sums(e, m, iv))).tobytes()
    assert stub.calls == [('mom_sums', 1)]
    assert ts.get_read_seg_score(e, m, sds) == nc.seg_score(e, m, sds)
    scores = ts.get_read_seg_scores_batch([(e, m, sds), (e[:5], m[:5], sds[:5])])
    assert scores == [nc.seg_score(e, m, sds), nc.seg_score(e[:5], m[:5], sds[:5])] and stub.calls[-1] == ('seg_scores', 2)
    assert ts.get_read_seg_scores_batch([]) == []
    with pytest.raises(ValueError):
        ts.get_read_seg_scores_batch([(e, m, sds[:-1])])
    assert meta['zero_slope_msg'] == ts._SLOPE_ZERO_MSG


def test_pA_through_the_stub(stub, golden):
    """'pA': one mom_sums call for the reads without scale values, then one normalisation call with the fitted values"""
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    g, meta = golden
    channel = th.channelInfo(nc.CHANNEL[0], nc.CHANNEL[1], nc.CHANNEL[2], 7, 4000.0)
    pa = pa_cases()
    n_checked = [0]
    for i, (dtype, sig, start, n, thresh, (e, m, iv)) in enumerate(pa):
        del stub.calls[:]
        norm, sv = ts.normalize_raw_signal(sig, start, n, 'pA', thresh, channel, None, e, m, iv)
        assert [c[0] for c in stub.calls] == ['mom_sums', 'normalize_raw_batch']
        if np.array([sv.shift, sv.scale]).tobytes() == g['pA/sv'][i, :2].tobytes():        # (the recorder's LAPACK)
            check_norm_record(g, 'pA', i, (norm, sv.shift, sv.scale, sv.lower_lim, sv.upper_lim), n_checked)
        else:
            np.testing.assert_allclose([sv.shift, sv.scale], g['pA/sv'][i, :2], rtol=1e-12)

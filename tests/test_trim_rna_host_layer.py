"""The host layers of RNA adapter trimming and estimate_global_scale without a GPU: a numpy stand-in engine (the
restatement of tests/trim_rna_reference.py over the CPU oracle, np.median) under ts.trim_rna / ts.trim_rna_batch /
ts.estimate_global_scale, the worker's order and slicing, the error mapping, the argument checks and the header."""
import os
import re
import warnings

import numpy as np
import pytest

from tombo_amd import _native, mapping, resquiggle as rq, tombo_helper as th, tombo_stats as ts
import trim_rna_cases as tc
import trim_rna_reference as tr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
RNA = th.seqSampleType('RNA', True)
DNA = th.seqSampleType('DNA', False)


class NumpyTrimEngine(object):
    """Engine.trim_rna / Engine.raw_med_mad on the CPU, behind the argument checks of the real binding"""

    def __init__(self):
        self.calls = []

    def trim_rna(self, raws, seg_params, trim_params):
        import oracle
        dt, pre, seg, trim = _native._check_trim_rna_args(raws, seg_params, trim_params)
        self.calls.append(('trim_rna', len(pre), dt, max([p.shape[0] for p in pre] or [0])))
        ends, status = np.zeros(len(pre), np.int64), np.zeros(len(pre), np.int32)
        for i, x in enumerate(pre):
            try:
                ends[i] = tr.trim_rna(x, seg, trim, oracle.valid_cpts, oracle.new_mean_stds)
            except tr.TomboErrorLike:
                status[i] = 2
            except ValueError:
                status[i] = _native.TRIM_TOO_FEW_EVENTS
        return ends, status

    def raw_med_mad(self, raws):
        dt, raws = _native._check_raw_reads(raws, 1)
        self.calls.append(('raw_med_mad', len(raws), dt))
        med = np.array([np.median(r) for r in raws], dtype=np.float64)
        return med, np.array([np.median(np.abs(r - m)) for r, m in zip(raws, med)], dtype=np.float64)


def rna_params():
    return ts.load_resquiggle_parameters(RNA)


def test_defaults_are_the_references():
    from tombo_amd import _default_parameters as dp
    assert dp.TRIM_RNA_ADAPTER is False and dp.NUM_READS_FOR_SCALE == 1000
    assert th.trimRnaParams._fields == ('moving_window_size', 'min_running_values', 'thresh_scale', 'max_raw_obs')
    assert tuple(ts.DEFAULT_TRIM_RNA_PARAMS) == (50, 100, 0.7, 40000) == tc.DEFAULT_TRIM
    p = rna_params()
    assert (p.running_stat_width, p.min_obs_per_base, p.mean_obs_per_event) == tc.RNA_SEG


def test_trim_rna_and_its_errors_on_the_stand_in():
    eng = NumpyTrimEngine()
    by = tc.BY_NAME
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'stats_trim_rna.npz'))
    raw = tc.signal(by['n2250'])
    end = ts.trim_rna(raw, rna_params(), engine=eng)
    assert type(end) is int and end == int(g['f64_n2250']) > 0
    assert ts.trim_rna(tc.signal(by['n2235']), rna_params(), engine=eng) == 0
    with pytest.raises(ValueError) as exc:
        ts.trim_rna(tc.signal(by['n2234']), rna_params(), engine=eng)
    assert 'ValueError: %s' % exc.value == str(g['err_n2234'])
    with pytest.raises(th.TomboError) as exc:
        ts.trim_rna(tc.signal(by['fewer_cpts']), rna_params(), engine=eng)
    assert 'TomboError: %s' % exc.value == str(g['err_fewer_cpts'])
    # the batch form: one engine call, failures beside answers; only the prefix is handed over; dtypes
    names = ('n2250', 'n2234', 'first_window', 'fewer_cpts', 'n2235')
    eng.calls = []
    ends, errs = ts.trim_rna_batch([tc.dac(tc.signal(by[k])) for k in names], rna_params(),
                                   th.trimRnaParams(50, 100, 0.7, 5000), engine=eng)
    assert eng.calls == [('trim_rna', 5, np.dtype(np.int16), 5000)]
    assert ends.dtype == np.int64 and ends.shape == (5,) and ends[1] == ends[3] == 0
    assert [type(e) for e in errs] == [type(None), ValueError, type(None), th.TomboError, type(None)]
    ends32, _ = ts.trim_rna_batch([tc.dac(tc.signal(by['n2250'])).astype(np.int32), raw], rna_params(), engine=eng)
    assert eng.calls[-1][2] == np.dtype(np.float64) and ends32[1] == end
    assert ts.trim_rna_batch([], rna_params(), engine=eng)[1] == []
    assert isinstance(ts._trim_error(100), RuntimeError) and ts._trim_error(0) is None


def test_argument_checks():
    x = np.zeros(3000)
    ok = _native._check_trim_rna_args([x, x[:100]], tc.RNA_SEG, (50, 100, 0.7, 1000))
    assert ok[0] == np.dtype(np.float64) and [p.shape[0] for p in ok[1]] == [1000, 100]
    assert np.shares_memory(ok[1][0], x) and ok[2] == tc.RNA_SEG and ok[3] == (50, 100, 0.7, 1000)
    for raws, seg, trim in (([x], (12, 6), tc.DEFAULT_TRIM), ([x], (12, 0, 15), tc.DEFAULT_TRIM),
                            ([x], (12.5, 6, 15), tc.DEFAULT_TRIM), ([x], tc.RNA_SEG, (50, 100, 0.7)),
                            ([x], tc.RNA_SEG, (0, 100, 0.7, 40000)), ([x], tc.RNA_SEG, (50, 0, 0.7, 40000)),
                            ([x], tc.RNA_SEG, (50, 100, 0.7, 0)), ([x], tc.RNA_SEG, (50, 100, float('nan'), 40000)),
                            ([x], tc.RNA_SEG, (_native.TRIM_MAX_WINDOW + 1, 100, 0.7, 40000)),
                            ([x.astype(np.float32)], tc.RNA_SEG, tc.DEFAULT_TRIM),
                            ([x, x.astype(np.int16)], tc.RNA_SEG, tc.DEFAULT_TRIM),
                            ([x.reshape(2, -1)], tc.RNA_SEG, tc.DEFAULT_TRIM)):
        with pytest.raises(ValueError):
            _native._check_trim_rna_args(raws, seg, trim)
    with pytest.raises(ValueError):
        _native._check_raw_reads([x[:0]], 1)
    with pytest.raises(ValueError):
        _native._check_raw_reads([x.astype(np.int32)], 1)


def _map_res(raw):
    return th.resquiggleResults(align_info='r', genome_loc=None, genome_seq='ACGT', mean_q_score=1.0, raw_signal=raw)


def test_adjust_map_res_trims_then_flips_then_finds_stalls(monkeypatch):
    raw = np.arange(100, dtype=np.int16)
    seen = []

    def fake_trim(sig, params):
        seen.append(('trim', sig.copy(), params))
        return 30

    def fake_stalls(sig):
        seen.append(('stalls', sig.copy()))
        return [(1, 2)]
    monkeypatch.setattr(ts, 'trim_rna', fake_trim)
    monkeypatch.setattr(ts, 'identify_stalls', fake_stalls)
    out = rq.adjust_map_res(_map_res(raw), RNA, True, 'params')
    assert [s[0] for s in seen] == ['trim', 'stalls'] and seen[0][2] == 'params'
    assert np.array_equal(seen[0][1], raw)                       # trimming sees the signal in acquisition order
    assert np.array_equal(seen[1][1], raw[30:][::-1])            # ... the stall detector what is left, flipped
    assert np.array_equal(out.raw_signal, raw[30:][::-1]) and np.shares_memory(out.raw_signal, raw)
    assert out.stall_ints == [(1, 2)]
    # None is the module constant (off), DNA is never trimmed, trimming needs the parameters
    seen[:] = []
    assert np.array_equal(rq.adjust_map_res(_map_res(raw), RNA).raw_signal, raw[::-1])
    assert np.array_equal(rq.adjust_map_res(_map_res(raw), DNA, True, 'params').raw_signal, raw)
    assert [s[0] for s in seen] == ['stalls']
    monkeypatch.setattr('tombo_amd._default_parameters.TRIM_RNA_ADAPTER', True)
    assert np.array_equal(rq.adjust_map_res(_map_res(raw), RNA, None, 'params').raw_signal, raw[30:][::-1])
    with pytest.raises(ValueError):
        rq.adjust_map_res(_map_res(raw), RNA, True)


def test_worker_slices_views_and_fails_a_read_once(monkeypatch):
    raws = [np.arange(50, dtype=np.int16) + 100 * i for i in range(4)]
    calls = []

    def fake_trim_batch(sigs, params, trim_rna_params=None, engine=None):
        calls.append(('trim', [s is r for s, r in zip(sigs, raws)], params))
        return (np.array([7, 0, 0, 11], dtype=np.int64),
                [None, ValueError(tr.TOO_FEW_EVENTS_MSG), None, None])

    def fake_batch(map_results, std_ref, params, outlier_thresh=None, all_raw_signals=None, **kw):
        calls.append((params, [m.align_info for m in map_results], [m.raw_signal for m in map_results], kw))
        return [th.TomboError('boom') if m.align_info == 3 else m._replace(segs=[0, 1], norm_params_changed=False)
                for m in map_results]
    monkeypatch.setattr(ts, 'trim_rna_batch', fake_trim_batch)
    monkeypatch.setattr(rq, 'resquiggle_batch', fake_batch)
    mrs = [_map_res(r)._replace(align_info=i) for i, r in enumerate(raws)]
    res, passes = rq.resquiggle_batch_iters(mrs, None, 'main', 'save', seq_samp_type=RNA, device_prep=True,
                                            trim_rna_adapter=True, return_passes=True)
    assert calls[0] == ('trim', [True] * 4, 'main')
    assert calls[1][:2] == ('main', [0, 2, 3]) and calls[2][:2] == ('save', [3]) and len(calls) == 3
    for sig, i, end in zip(calls[1][2], (0, 2, 3), (7, 0, 11)):
        assert np.array_equal(sig, raws[i][end:]) and np.shares_memory(sig, raws[i])     # a view, no copy
    assert calls[1][3]['reverse_raw'] is True and calls[1][3]['stall_params'] is not None
    assert isinstance(res[1], ValueError) and str(res[1]) == tr.TOO_FEW_EVENTS_MSG and passes == [1, 0, 1, 2]
    assert isinstance(res[3], th.TomboError) and not isinstance(res[0], Exception)
    assert all(m.raw_signal is r for m, r in zip(mrs, raws))                            # the input is left alone
    # off: no trimming call; DNA: none either; host-side preparation cannot be trimmed afterwards
    calls[:] = []
    rq.resquiggle_batch_iters(mrs, None, 'main', seq_samp_type=RNA, device_prep=True)
    rq.resquiggle_batch_iters(mrs, None, 'main', seq_samp_type=DNA, device_prep=True, trim_rna_adapter=True)
    assert [c[0] for c in calls] == ['main', 'main'] and all(s is r for s, r in zip(calls[0][2], raws))
    with pytest.raises(ValueError):
        rq.resquiggle_batch_iters(mrs, None, 'main', seq_samp_type=RNA, trim_rna_adapter=True)


def test_process_fast5_batch_reports_trimming_failures(monkeypatch):
    seen = {}

    def fake_read(f5, *a, **k):
        return _map_res(np.zeros(10, np.int16))._replace(align_info=f5)

    def fake_iters(mapped, std_ref, params, **kw):
        seen.update(kw)
        return [ValueError(tr.TOO_FEW_EVENTS_MSG), th.TomboError(tr.FEWER_CPTS_MSG)]
    monkeypatch.setattr(mapping, 'read_fast5_for_mapping', fake_read)
    monkeypatch.setattr(rq, 'resquiggle_batch_iters', fake_iters)
    recs, failures = mapping.process_fast5_batch([('a', 'a.fast5'), ('b', 'b.fast5')], None, None, 'main', RNA,
                                                 write=False, trim_rna_adapter=True)
    assert seen['trim_rna_adapter'] is True and seen['device_prep'] is True and recs == []
    assert failures == [(tr.TOO_FEW_EVENTS_MSG, 'BaseCalled_template:::a.fast5', False),
                        (tr.FEWER_CPTS_MSG, 'BaseCalled_template:::b.fast5', True)]
    mapping.process_fast5_batch([('a', 'a.fast5'), ('b', 'b.fast5')], None, None, 'main', RNA, write=False)
    assert seen['trim_rna_adapter'] is False


class _Fast5(object):
    def __init__(self, sig):
        self.sig = sig

    def __getitem__(self, key):
        if key != '/Raw/Reads' or self.sig is None:
            raise KeyError(key)
        return {'Read_1': {'Signal': self.sig}}


def test_estimate_global_scale_host_layer():
    rng = np.random.default_rng(3)
    sigs = [np.round(rng.normal(500, 20 + i, size=400 + i)).astype(np.int16) for i in range(10)]
    items = [_Fast5(s) for s in sigs]
    items[2], items[7] = _Fast5(None), _Fast5(sigs[7][:0])          # no raw slot; no sample
    order = list(range(10))
    np.random.seed(4)
    np.random.shuffle(order)
    taken = [i for i in order if i not in (2, 7)][:5]
    want = np.mean([np.median(np.abs(sigs[i] - np.median(sigs[i]))) for i in taken])
    eng = NumpyTrimEngine()
    np.random.seed(4)
    shuffled = list(items)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = ts.estimate_global_scale(shuffled, 5, engine=eng)
    assert got == want and eng.calls == [('raw_med_mad', 5, np.dtype(np.int16))]
    assert [items.index(x) for x in shuffled] == order               # shuffled in place, numpy's global RNG
    # raw arrays, fewer reads than asked for: the reference's warning; none at all: its error
    with pytest.warns(UserWarning) as rec:
        few = ts.estimate_global_scale([sigs[0].astype(np.float64), _Fast5(None), sigs[1].astype(np.float64)], 3,
                                       engine=eng)
    assert str(rec[0].message) == ('Few reads contain raw signal for global scale parameter estimation. Results may '
                                   'not be optimal.')
    assert few == np.mean([np.median(np.abs(s - np.median(s))) for s in (sigs[0], sigs[1])])
    with pytest.raises(th.TomboError) as exc:
        ts.estimate_global_scale([_Fast5(None)], 3, engine=eng)
    assert str(exc.value) == 'No reads contain raw signal for global scale parameter estimation.'
    import inspect
    assert inspect.signature(ts.estimate_global_scale).parameters['num_reads'].default == 1000


def test_header_names_the_entries():
    hdr = open(os.path.join(ROOT, 'include', 'tombo_amd.h')).read()
    assert re.search(r'#define TBA_ABI_VERSION 13\b', hdr) and _native.ABI_VERSION == 13
    assert int(re.search(r'#define\s+TBA_ABI_MINOR\s+(\d+)', hdr).group(1)) >= 4
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('tba_trim_rna_batch', 'tba_raw_med_mad', 'tba_engine_set_trim_budget'):
        assert re.search(r'\bint\s+%s\s*\(' % name, code) and name in _native.PROTOTYPES
    assert re.search(r'TBA_TRIM_TOO_FEW_EVENTS = %d,' % _native.TRIM_TOO_FEW_EVENTS, hdr)
    for name in ('trim_rna', 'raw_med_mad', 'set_trim_budget'):
        assert callable(getattr(_native.Engine, name))
    src = open(os.path.join(_native.CSRC, 'k_trim_rna.h')).read()
    for k in ('k_trim_seg_sds', 'k_trim_pick', 'k_raw_med_mad'):
        assert k in src
    assert 'atomic' not in src.replace('No atomics', '')

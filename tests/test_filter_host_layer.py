"""The host layer of the read filters (tombo_amd.filter_reads, th.parse_obs_filter / parse_genome_regions,
mapping.filter_and_index_records_batch) on the numpy stand-in engine of tests/filter_stub_engine.py: every case of
tests/golden/stats_filters.npz through the reference-signature wrappers and the index forms -- index tuples in
order, counts, messages, the seeded draw, both error cases -- without a GPU.  The same cases run on the device in
test_gpu_filters.py."""
import os
import re

import numpy as np
import pytest

from tombo_amd import _native, filter_reads as flt, mapping, tombo_helper as th
import filter_cases as fc
import filter_reference as fref
from filter_stub_engine import NumpyFilterEngine

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
DOC = fc.DOC


@pytest.fixture()
def eng():
    return NumpyFilterEngine()


@pytest.mark.parametrize('name', sorted(fc.CASES))
def test_wrapper_equals_the_reference(name, eng, tmp_path):
    fc.check_case(name, eng, tmp_path)


@pytest.mark.parametrize('name', [n for n in sorted(fc.CASES) if fc.CASES[n]['error'] is None])
def test_index_form_equals_the_reference(name, eng):
    case = fc.CASES[name]
    index, (f, a) = fc.reads_index(case), (case['func'], case['args'])
    if f == 'clear_filters':
        new, counts = flt.clear_filters_index(index)
    elif f == 'filter_reads_for_stuck':
        new, counts = flt.filter_reads_for_stuck_index(index, a[1], fc.base_lens, eng)
    elif f == 'filter_reads_for_coverage':
        seen = []
        np.random.seed(case['seed'])
        new, counts = flt.filter_reads_for_coverage_index(index, a[1], eng, before_draw=seen.append)
        assert seen == [counts]
    elif f == 'filter_reads_for_qscore':
        new, counts = flt.filter_reads_for_qscore_index(index, a[2], flt.fastq_q_score_accessor(a[0], fc.open_fast5))
    elif f == 'filter_reads_for_signal_matching':
        new, counts = flt.filter_reads_for_signal_matching_index(index, a[1], flt.sig_match_score_accessor(fc.open_fast5))
    else:
        new, counts = flt.filter_reads_for_genome_pos_index(index, fc.regs_arg(a[1]), a[2])
    assert fc.as_lists(new) == case['out']
    assert fc.as_lists(index) == fref.case_index(DOC, case)     # the input is left alone
    want = fref.run_case(case, DOC, fc.LENS)[1]
    if want is not None:
        assert counts == want


def test_empty_index_and_no_unfiltered_reads():
    with pytest.raises(th.TomboError) as exc:
        flt.replace_index('/nowhere/reads', DOC['corr_grp'], {('chr1', '+'): []})
    assert str(exc.value) == DOC['empty_index_error']
    with pytest.raises(th.TomboError) as exc:
        flt.filter_message(0, 0, 5, 'd', 'q-score')
    assert str(exc.value) == 'No unfiltered reads present in current Tombo index.'
    with pytest.raises(th.TomboError):
        flt.filter_reads_for_coverage_index(fc.reads_index(all_filtered=True), 0.25, NumpyFilterEngine())


def test_index_file_name():
    assert flt.get_index_fn('a/b/reads/', 'G') == flt.get_index_fn('a/b/reads', 'G') == os.path.join('a/b', '.reads.G.tombo.index')
    assert flt.get_index_fn('reads', 'G') == '.reads.G.tombo.index'


def test_stuck_reads_go_to_the_engine_in_bounded_calls(eng):
    index = fc.reads_index()
    todo = [rd for rds in index.values() for rd in rds if not rd.filtered and fc.base_lens(rd) is not None]
    one, _ = flt.filter_reads_for_stuck_index(index, [(99, 200)], fc.base_lens, eng)
    assert eng.calls == [(len(todo), sum(len(fc.base_lens(rd)) + 1 for rd in todo))]     # one call, not one per read
    eng.calls = []
    small, _ = flt.filter_reads_for_stuck_index(index, [(99, 200)], fc.base_lens, eng, call_bytes=8 * 400)
    assert small == one and len(eng.calls) > 3 and sum(c[0] for c in eng.calls) == len(todo)
    assert all(c[1] * 8 <= 8 * 400 or c[0] == 1 for c in eng.calls)
    lens = [np.array([3, 4, 5]), np.zeros(0, dtype=np.uint32), np.array([900])]
    assert flt.stuck_flags(lens, [(100, 5)], eng).tolist() == [False, True, True]


def test_parsers():
    for text, parsed in zip(DOC['obs_texts'], DOC['obs_parsed']):
        assert th.parse_obs_filter(text) == parsed
    assert th.parse_obs_filter([]) is None
    for bad, msg in ((['99-200'], 'Invalid format for observation filter'), (['a:5'], 'Invalid format for observation filter'),
                     (['101:5'], 'Invalid percentile value.'), (['-1:5'], 'Invalid percentile value.')):
        with pytest.raises(th.TomboError) as exc:
            th.parse_obs_filter(bad)
        assert str(exc.value) == msg
    for text, parsed in zip(DOC['reg_texts'], DOC['reg_parsed']):
        assert th.parse_genome_regions(text) == parsed
    for bad in (['chr1:1:2'], ['chr1:a-b']):
        with pytest.raises(th.TomboError) as exc:
            th.parse_genome_regions(bad)
        assert str(exc.value) == 'Invalid [--include-region] format.'


def _results(rng, n):
    res = []
    for i in range(n):
        nb = int(rng.integers(1, 120))
        lens = rng.geometric(0.1, nb) + 1
        if i % 5 == 0:
            lens[rng.integers(0, nb)] = 6000
        segs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        res.append(th.resquiggleResults(
            align_info=th.alignInfo('id%d' % i, 'BaseCalled_template', 0, 0, 0, 0, nb, 0),
            genome_loc=th.genomeLocation(100 + i, '+-'[i % 2], 'chr%d' % (i % 3)), genome_seq='A' * nb,
            mean_q_score=9.0 + i, read_start_rel_to_raw=7 * i, segs=segs,
            sig_match_score=float(rng.choice([0.8, 1.0, 1.3]))))
    return res


@pytest.mark.parametrize('obs_filter', [None, [(99, 200)], [(50, 8), (100, 5000)]])
def test_batch_form_equals_the_per_read_rule(eng, obs_filter):
    rng = np.random.default_rng(3)
    res = _results(rng, 40)
    fns = ['f%d.fast5' % i for i in range(len(res))]
    samp = th.seqSampleType('DNA', False)
    want = [mapping.filter_and_index_record(r, fn, 'Grp', 'BaseCalled_template', samp, 1.1, obs_filter)
            for r, fn in zip(res, fns)]
    got = mapping.filter_and_index_records_batch(res, fns, 'Grp', 'BaseCalled_template', samp, 1.1, obs_filter, engine=eng)
    assert got == want
    assert len(eng.calls) == (0 if obs_filter is None else 1)
    assert obs_filter is None or len(set(w[2].filtered for w in want)) == 2
    # the resident form: the engine holds the same boundaries, two reads have failed
    failed = [4, 17]
    status = np.zeros(len(res), dtype=np.int32)
    status[failed] = 3
    off = np.concatenate([[0], np.cumsum([r.segs.shape[0] for r in res])]).astype(np.int64)
    eng.resident = (np.concatenate([r.segs for r in res]), off, status)
    res_f = [RuntimeError('failed') if i in failed else r for i, r in enumerate(res)]
    got = mapping.filter_and_index_records_batch(res_f, fns, 'Grp', 'BaseCalled_template', samp, 1.1, obs_filter,
                                                 engine=eng, resident=True)
    assert got == [None if i in failed else w for i, w in enumerate(want)]


def test_bindings_and_abi_entries():
    hdr = open(os.path.join(ROOT, 'include', 'tombo_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('tba_dwell_pctl_flags', 'tba_batch_dwell_pctl_flags'):
        assert re.search(r'\bint\s+%s\s*\(' % name, code) and name in _native.PROTOTYPES
    for name in ('dwell_pctl_flags', 'batch_dwell_pctl_flags'):
        assert callable(getattr(_native.Engine, name)) and callable(getattr(NumpyFilterEngine, name))
    src = open(os.path.join(_native.CSRC, 'k_filter.h')).read()
    assert 'np_pctl_lerp' in src and 'np_pctl_lerp' in open(os.path.join(_native.CSRC, 'k_plot.h')).read()
    ok = (np.array([0, 3, 5, 0, 2], dtype=np.int64), np.array([0, 3, 3, 5], dtype=np.int64), [(50, 3)])
    _native._check_dwell_pctl_args(*ok)
    for segs, off, pairs in ((ok[0].astype(np.int32), ok[1], ok[2]), (ok[0], ok[1][1:], ok[2]), (ok[0], ok[1], []),
                             (ok[0], ok[1], [(101, 3)]), (ok[0], ok[1], [(50, np.nan)]),
                             (np.array([0, 3, 2, 0, 2], dtype=np.int64), ok[1], ok[2]),
                             (np.array([0, 3, 5, 0, 2 ** 31], dtype=np.int64), ok[1], ok[2]), (ok[0][:4], ok[1], ok[2])):
        with pytest.raises(ValueError):
            _native._check_dwell_pctl_args(segs, off, pairs)

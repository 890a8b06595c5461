"""The host layer of the statistics files on a numpy engine (tests/stat_store_stub_engine.py):
aggregate_per_read_stats (grouping into engine calls, layout, writing), write_stats_from_regions, the statistics
types of write_all_browser_files, argument checks and the C header."""
import os
import re

import numpy as np
import pytest

import stat_store_cases as sc
from stat_store_stub_engine import NumpyStatStoreEngine, aggregate_block
from store_memh5 import StoreGroup, flat_tree, same_array
from tombo_amd import tombo_stats as ts, tombo_helper as th, text_output, _native

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
AGGS = ('lower', 'abs', 'all', 'lower_damp')


def aggregate(name, max_records=None, eng=None):
    stat_type, single, lower, damp, n_signif = sc.agg_case(name)
    out = StoreGroup()
    eng = eng or NumpyStatStoreEngine()
    ts.aggregate_per_read_stats(sc.per_read_store(ts, stat_type), single, lower, out, damp, sc.meta()['min_test_reads'],
                                n_signif, engine=eng, max_records=max_records)
    return out, eng


@pytest.mark.parametrize('name', AGGS)
def test_aggregated_file_equals_the_reference(name):
    out, _ = aggregate(name)
    assert out.closed
    sc.check_tree('agg_' + name, out)


@pytest.mark.parametrize('name', ['lower', 'abs'])
def test_chunking_does_not_change_the_file(name):
    one, eng_one = aggregate(name, max_records=1)
    every, eng_all = aggregate(name, max_records=10 ** 9)
    assert [c[0] for c in eng_one.calls] == [1] * 8 and len(eng_all.calls) == 1 and eng_all.calls[0][0] == 8
    some, eng_some = aggregate(name, max_records=1000)
    assert 1 < len(eng_some.calls) < 8 and sum(c[0] for c in eng_some.calls) == 8
    a, b, c = flat_tree(one), flat_tree(every), flat_tree(some)
    assert list(a) == list(b) == list(c)
    assert all(same_array(a[k], b[k]) and same_array(a[k], c[k]) for k in a)
    sc.check_tree('agg_' + name, one)


def test_default_chunk_comes_from_the_engines_free_memory():
    class Eng(NumpyStatStoreEngine):
        def device_mem(self):
            return 2 * 76 * 250, 1 << 30     # room for 250 records and their positions in half of it
    _, eng = aggregate('all', eng=Eng())
    assert ts._default_max_records(Eng()) == 250
    assert len(eng.calls) > 1 and sum(c[0] for c in eng.calls) == 8


def test_cov_damp_counts_as_the_reference_dict():
    stat_type, single, lower, damp, n_signif = sc.agg_case('abs')
    out = StoreGroup()
    ts.aggregate_per_read_stats(sc.per_read_store(ts, stat_type), single, lower, out, dict(unmod=damp[0], mod=damp[1]),
                                1, n_signif, engine=NumpyStatStoreEngine())
    sc.check_tree('agg_abs', out)


def test_nothing_to_aggregate_raises_the_reference_message():
    grp = StoreGroup()
    ts.PerReadStats(grp, 'de_novo', 100).close()
    with pytest.raises(th.TomboError, match='No genomic positions contain --minimum-test-reads.'):
        ts.aggregate_per_read_stats(grp, 0.5, None, StoreGroup(), (2, 0), 1, 10, engine=NumpyStatStoreEngine())


def test_a_file_name_needs_h5py(tmp_path):
    try:
        import h5py  # noqa: F401
        have = True
    except ImportError:
        have = False
    for make in (lambda: ts.PerReadStats(str(tmp_path / 'x.tombo.per_read_stats'), 'de_novo', 100),
                 lambda: ts.ModelStats(str(tmp_path / 'x.tombo.stats'), 'de_novo', 100, (2, 0), 1, 10)):
        if have:
            make().close()
        else:
            with pytest.raises(ImportError):
                make()
    with pytest.raises(th.TomboError, match='does not exist'):
        ts.ModelStats(str(tmp_path / 'missing.tombo.stats'))


def test_write_stats_from_regions_and_back():
    """detect -> store -> re-aggregate on the numpy engine: the re-aggregated blocks equal the stored ones"""
    region, damp = 100, (2, 0)
    rng = np.random.default_rng(5)
    results, per_read = [], []
    for r, (chrm, strand, start) in enumerate([('c', '+', 200), ('c', '+', 0), ('c', '-', 100)]):
        block = np.empty(300, dtype=_native.PER_READ_DTYPE)
        block['pos'], block['stat'] = rng.integers(start, start + region, 300), rng.integers(0, 65, 300) / 64.0
        block['read_id'] = rng.integers(0, 7, 300)
        lookup = dict(('read%d_%d' % (r, i), i) for i in range(7))
        f, p, c, v = aggregate_block(block, 0.5, 0.25, False)
        results.append([('de_novo', th.regionStats(f, p, chrm, strand, start, c, [0] * 300, v))])
        per_read.append([('de_novo', (block, lookup, chrm, strand, start))])
    results.append(th.TomboError('No valid positions in this region.'))
    per_read.append([])
    direct, pr_grp, again = StoreGroup(), StoreGroup(), StoreGroup()
    stats, pr = ts.ModelStats(direct, 'de_novo', region, damp, 1, 50), ts.PerReadStats(pr_grp, 'de_novo', region)
    ts.write_stats_from_regions(results, per_read, stats, pr)
    stats.close()
    pr.close()
    ts.aggregate_per_read_stats(pr_grp, 0.5, 0.25, again, damp, 1, 50, engine=NumpyStatStoreEngine())
    a, b = ts.ModelStats(direct), ts.ModelStats(again)
    assert a.num_blocks == b.num_blocks == 3
    want = dict(((c, s, st), blk) for c, s, st, _, blk in a)
    for c, s, st, _, blk in b:
        assert same_array(blk, want[(c, s, st)])
    assert same_array(a.most_signif_stats, b.most_signif_stats)


def test_detect_store_reaggregate_on_the_numpy_engines():
    from stats_stub_engine import NumpyStatsEngine

    class Both(NumpyStatsEngine, NumpyStatStoreEngine):
        def __init__(self):
            NumpyStatsEngine.__init__(self)
            NumpyStatStoreEngine.__init__(self)
    assert sc.check_detect_store_reaggregate(ts, th, engine=Both()) >= 15


# ---- text_output
def test_statistics_types_still_refused_without_a_container():
    for t in text_output.STATS_WIG_TYPES:
        with pytest.raises(NotImplementedError, match=t):
            text_output.write_all_browser_files({}, None, 'x', [t])


def test_all_browser_files_from_a_container(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out, _ = aggregate('lower_damp')
    text_output.write_all_browser_files(None, None, 'st', ['fraction', 'dampened_fraction', 'valid_coverage'],
                                        all_stats=ts.TomboStats(out))
    want = sc.js('agg_lower_damp_wigs')
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(want)
    for fn, text in want.items():
        assert (tmp_path / fn).read_bytes() == text.encode()
    with pytest.raises(th.TomboError, match='Cannot output `--file-type statistics` for aggregated per-read'):
        text_output.write_all_browser_files(None, None, 'st', ['statistic'], all_stats=ts.TomboStats(out))
    with pytest.raises(ValueError, match='need reads'):
        text_output.write_all_browser_files(None, None, 'st', ['coverage', 'fraction'], all_stats=ts.TomboStats(out))
    with pytest.raises(NotImplementedError, match='motif'):
        text_output.write_frac_wigs(ts.TomboStats(out), 'st', True, False, False, False, 'genome.fa', ['CCWGG:2:5mC'])


def test_level_container_writes_the_statistic_type_only(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    grp = StoreGroup()
    ls = ts.LevelStats(grp, 'ks_stat_test', 100, 2, 10)
    ls._write_stat_block(th.groupStats(np.array([0.25, np.nan, 0.5]), np.array([3, 4, 9]), 'c', '-', 0,
                                       np.array([5, 5, 6]), np.array([7, 7, 8])))
    ls.close()
    text_output.write_all_browser_files(None, None, 'st', ['statistic'], all_stats=ts.TomboStats(grp))
    assert (tmp_path / 'st.statistic.minus.wig').read_text().splitlines()[1:] == [
        'variableStep chrom=c span=1', '4 0.7500', '10 0.5000']
    with pytest.raises(th.TomboError, match='for level sample compare statistics'):
        text_output.write_all_browser_files(None, None, 'st', ['fraction'], all_stats=ts.TomboStats(grp))


# ---- argument checks of the binding (shared with the numpy engine)
def test_site_aggregate_argument_checks():
    rec = np.zeros(4, dtype=_native.PER_READ_DTYPE)
    rec['pos'] = [0, 1, 10, 11]
    ok = ([0, 10], [10, 20], [0, 2, 4], rec)
    _native._check_site_aggregate_args(*ok)
    bad = [([0, 10], [10, 20], [1, 2, 4], rec), ([0, 10], [10, 20], [0, 3, 2], rec), ([0, 10], [10, 20], [0, 2, 3], rec),
           ([0, 10], [10, 10], [0, 2, 4], rec), ([0, 10], [10, 5], [0, 2, 4], rec), ([0, 10], [10, 20], [0, 4], rec),
           ([0, 10], [10], [0, 2, 4], rec), ([0, 0], [2 ** 30, 2 ** 30], [0, 2, 4], rec),
           ([0, 10], [10, 20], [0, 2, 4], rec.astype([('pos', 'u4'), ('stat', 'f8'), ('read_id', 'u4')], copy=True).view(np.uint8)),
           ([0, 10], [10, 20], [0, 2, 4], np.zeros(4, dtype=np.dtype(_native.PER_READ_DTYPE.descr, align=True)))]
    for args in bad:
        with pytest.raises(ValueError):
            _native._check_site_aggregate_args(*args)
    with pytest.raises(_native.EngineError, match='outside its block'):
        NumpyStatStoreEngine().site_aggregate([0, 10], [10, 20], [0, 3, 4], rec, 0.5)
    assert _native.PER_READ_DTYPE.itemsize == 16 and _native.PER_READ_DTYPE.fields['stat'][1] == 4


def test_header_declares_the_entry_and_keeps_the_abi():
    text = open(os.path.join(ROOT, 'include', 'tombo_amd.h')).read()
    assert re.search(r'\bint tba_site_aggregate\(tba_engine \*e,', text)
    assert re.search(r'#define TBA_ABI_VERSION 13\b', text)

"""TEST INFRASTRUCTURE: the recorded statistics files of tests/golden/stats_store.npz (written by
tests/golden/gen_golden_stat_store.py from the live reference) and the comparisons the CPU and GPU tests share."""
import os
import json

import numpy as np

from store_memh5 import StoreGroup, flat_tree, same_array
from tombo_amd import _native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stats_store.npz')
_CACHE = {}


def gold():
    if 'g' not in _CACHE:
        with np.load(GOLDEN) as z:
            _CACHE['g'] = dict((k, z[k]) for k in z.files)
        _CACHE['meta'] = json.loads(str(_CACHE['g']['meta']))
    return _CACHE['g']


def meta():
    gold()
    return _CACHE['meta']


def js(key):
    return json.loads(str(gold()[key]))


def check_tree(name, group):
    """the flattened tree of `group` against the recorded one: same paths in the same order, same dtypes, same
    values, no tolerance"""
    g, mine = gold(), flat_tree(group)
    assert list(mine) == js(name + '_keys')
    for k, v in mine.items():
        assert same_array(v, g['%s|%s' % (name, k)]), (name, k, v, g['%s|%s' % (name, k)])


def per_read_blocks(stat_type):
    """[(chrm, strand, start, block, {read id: number})] in stored order"""
    g, fn = gold(), 'pr_' + stat_type
    return [(c, s, start, g['%s_block|%d' % (fn, i)],
             dict(zip(g['%s_ids|%d' % (fn, i)].tolist(), g['%s_id_vals|%d' % (fn, i)].tolist())))
            for i, (c, s, start, _) in enumerate(meta()['blocks'])]


def per_read_store(ts, stat_type):
    """a per-read file of this project's PerReadStats holding the recorded blocks -> the group"""
    grp = StoreGroup()
    pr = ts.PerReadStats(grp, stat_type, meta()['region_size'])
    for c, s, start, block, lookup in per_read_blocks(stat_type):
        pr._write_per_read_block(block, lookup, c, s, start)
    pr.close()
    return grp


def agg_case(name):
    """-> (stat type, single_read_thresh, lower_thresh, cov_damp_counts, num_most_signif)"""
    t, single, lower, damp, n = meta()['aggs'][name]
    return t, single, lower, tuple(damp), n


def agg_inputs(name):
    """the blocks of aggregation `name` in the order the reference aggregated them (PerReadStats' own) as the
    arguments of site_aggregate -> (blk_start, blk_end, rec_off, records)"""
    g, fn = gold(), 'pr_' + agg_case(name)[0]
    order = js(fn + '_iter')
    blocks = [g['%s_iter|%d' % (fn, i)] for i in range(len(order))]
    return (np.array([o[2] for o in order], dtype=np.int64), np.array([o[3] for o in order], dtype=np.int64),
            np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.int64),
            np.concatenate(blocks).astype(_native.PER_READ_DTYPE))


def check_site_fractions(name, res, with_damp):
    """a SiteFractions against the recorded outputs of the reference's _agg_stats_worker for every block"""
    g = gold()
    for t in range(res.counts.shape[0]):
        a = int(res.pos_off[t])
        b = a + int(res.counts[t])
        want = dict((k, g['agg_%s_%s|%d' % (name, k, t)]) for k in ('frac', 'poss', 'cov', 'valid', 'damp'))
        # (for a block without records the reference's np.split gives one empty piece: a NaN fraction without a
        # position; the written block is empty either way)
        n = want['poss'].shape[0]
        assert b - a == n, (name, t)
        assert np.array_equal(res.frac[a:b], want['frac'][:n], equal_nan=True)
        assert np.array_equal(res.poss[a:b], want['poss'])
        assert np.array_equal(res.cov[a:b], want['cov'][:n]) and np.array_equal(res.valid[a:b], want['valid'][:n])
        assert res.n_stats[t] == want['cov'][:n].sum()
        if with_damp:
            assert np.array_equal(res.damp[a:b], want['damp'][:n], equal_nan=True)
        else:
            assert res.damp is None


def check_equal_results(a, b):
    """two SiteFractions: the same bytes in every kept entry"""
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.n_stats, b.n_stats)
    for t in range(a.counts.shape[0]):
        lo = int(a.pos_off[t])
        hi = lo + int(a.counts[t])
        for x, y in ((a.frac, b.frac), (a.poss, b.poss), (a.cov, b.cov), (a.valid, b.valid), (a.damp, b.damp)):
            assert (x is None) == (y is None)
            if x is not None:
                assert x[lo:hi].tobytes() == y[lo:hi].tobytes()


def check_detect_store_reaggregate(ts, th, engine=None):
    """detect -> store -> re-aggregate on the reads of tests/golden/stats_site.npz (regions of 20 to 100 positions,
    blocks of 100): compute_reg_stats_batch(..., return_per_read=True), write_stats_from_regions, then
    aggregate_per_read_stats under the same thresholds.  Every re-aggregated block equals the directly written
    one in frac, cov, valid_cov and damp_frac (the control coverage is not stored per read).  -> blocks compared"""
    import site_stats_reference as ssr
    g = np.load(os.path.join(os.path.dirname(GOLDEN), 'stats_site.npz'))
    m = json.loads(str(g['meta']))
    model = ts.TomboModel(seq_samp_type=th.seqSampleType('DNA', False))
    gr = np.load(os.path.join(os.path.dirname(GOLDEN), 'stats_reads.npz'))   # (the alternate-model tables)
    alt_refs = [(am['name'], ts.AltModel(
        [(r['kmer'].decode(), int(r['pos']), float(r['mean']), float(r['sd'])) for r in gr[am['key']]],
        model.central_pos, am['alt_base'], name=am['name'], motif=th.TomboMotif(am['motif'], am['mod_pos'])))
        for am in json.loads(str(gr['meta']))['alt_models']]
    damp, n = (m['cov_damp_counts']['unmod'], m['cov_damp_counts']['mod']), 0
    for c in m['cases']:
        if c['stat_type'] == 'sample_compare' or c['fm'] > 1:
            continue
        refs = alt_refs[:1] if c['stat_type'] == 'model_compare' else alt_refs   # one statistic name per file
        samp, _ = ssr.golden_regions(g, th, c['fm'], model.kmer_width)
        results, per_read = ts.compute_reg_stats_batch(
            samp, c['fm'], m['min_test_reads'], c['single'], c['lower'], None, model, refs, False, c['stat_type'],
            None, return_per_read=True, engine=engine)
        direct, pr_grp, again = StoreGroup(), StoreGroup(), StoreGroup()
        stats, pr = ts.ModelStats(direct, c['stat_type'], 100, damp, m['min_test_reads'], 100), \
            ts.PerReadStats(pr_grp, c['stat_type'], 100)
        ts.write_stats_from_regions(results, per_read, stats, pr)
        stats.close()
        pr.close()
        ts.aggregate_per_read_stats(pr_grp, c['single'], c['lower'], again, damp, m['min_test_reads'], 100,
                                    engine=engine)
        a, b = ts.ModelStats(direct), ts.ModelStats(again)
        want = dict(((chrm, s, st), blk) for chrm, s, st, _, blk in a)
        got = dict(((chrm, s, st), blk) for chrm, s, st, _, blk in b)
        assert len(want) == a.num_blocks and sorted(want) == sorted(got) and len(want) >= 3, c
        for key, blk in want.items():
            assert blk.shape[0] > 0
            for f in ('pos', 'frac', 'cov', 'valid_cov', 'damp_frac'):
                assert same_array(got[key][f], blk[f]), (c, key, f)
            n += 1
    return n

"""The numpy restatement of the reference's per-site collation (tests/site_stats_reference.py) against
the live reference (tests/golden/stats_site.npz, written by gen_golden_site_stats.py): from the
recorded per-read statistics to the recorded per-site records, every value exact."""
import os
import json
import numpy as np
import pytest

import site_stats_reference as ssr


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(os.path.dirname(__file__), 'golden', 'stats_site.npz'))


def _cases(g):
    return json.loads(str(g['meta']))['cases']


def test_collation_matches_reference(gold):
    meta = json.loads(str(gold['meta']))
    n_tracks = 0
    for c in meta['cases']:
        st, fm = c['stat_type'], c['fm']
        for ri in range(gold['reg_start'].shape[0]):
            key = '%s_fm%d_l%d_s%d_r%d' % (st, fm, c['li'], c['use_ref'], ri)
            pr_key = '%s_fm%d_l0_s1_r%d' % (st, fm, ri)   # per-read blocks do not depend on thresholds
            if fm >= 3 or c['use_ref'] != 1 or str(gold[key + '_err']):
                continue
            names = gold[key + '_names'].tolist()
            cc = ssr.ctrl_cov_dict(gold, ri, fm, meta['min_test_reads']) if st == 'sample_compare' else None
            for k, name in enumerate(names):
                assert str(gold['%s_pr%d_name' % (pr_key, k)]) == name
                res = ssr.collate(gold['%s_pr%d_stat' % (pr_key, k)], gold['%s_pr%d_pos' % (pr_key, k)].astype(np.int64),
                                  c['single'], c['lower'], st == 'model_compare', cc, st == 'sample_compare')
                frac, poss, cov, ccl, valid = res
                p = '%s_n%d_' % (key, k)
                assert np.array_equal(frac, gold[p + 'frac'], equal_nan=True), key
                assert np.array_equal(poss, gold[p + 'poss']) and np.array_equal(cov, gold[p + 'cov']), key
                assert np.array_equal(valid, gold[p + 'valid_cov']) and ccl == gold[p + 'ctrl_cov'].tolist(), key
                damp = ssr.damp_fraction(meta['cov_damp_counts'], frac, valid)
                assert np.array_equal(damp, gold[p + 'damp'], equal_nan=True), key
                blk = ssr.stat_block(frac, poss, cov, ccl, valid, meta['cov_damp_counts'])
                assert blk.dtype == gold[p + 'block'].dtype and np.array_equal(blk, gold[p + 'block']), key
                n_tracks += 1
    assert n_tracks > 30


def test_no_statistic_left():
    assert ssr.collate([np.nan, np.nan], [3, 4], 0.5, None, False) is None


def test_golden_covers_the_issue_cases(gold):
    cases = _cases(gold)
    assert {c['stat_type'] for c in cases} == {'de_novo', 'sample_compare', 'model_compare'}
    assert {c['fm'] for c in cases if c['stat_type'] != 'model_compare'} == {0, 1, 3}
    assert {c['lower'] is None for c in cases} == {True, False}
    assert {c['use_ref'] for c in cases if c['stat_type'] == 'sample_compare'} == {0, 1}
    errs = {str(gold[k]) for k in gold.files if k.endswith('_err')}
    assert errs == {'', 'No valid positions in this region.', 'Reads contains no statistics in this region.'}
    assert max(int(gold[k].max()) for k in gold.files if k.endswith('_cov') and gold[k].size) > 64
    assert gold['reg_minus'].any() and not gold['reg_minus'].all()

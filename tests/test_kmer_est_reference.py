"""The numpy restatement of the k-mer level extraction (tests/kmer_est_reference.py) pinned to the live
reference (tests/golden/stats_kmer_est.npz) under the parity rule of kmer_est_cases: its lists are bit-equal to
the reference run with a stable sort in get_reads_events and within four times the recorded spread of the run as
the reference is (medians and counts: bit-equal to both).  CPU only."""
import numpy as np
import pytest

from tombo_amd import tombo_helper as th
import kmer_est_cases as kc
import kmer_est_reference as kr
from tracks_stub_engine import NumpyTracksEngine


def restated(name):
    c = kc.CASES[name]
    idx = kc.reads_index(c['reads'])
    regs = list(th.iter_cov_regs(idx, c['cov_thresh'], kc.REGION_SIZE, engine=NumpyTracksEngine()))
    if c.get('seed') is not None:
        np.random.seed(c['seed'])
    all_regs = kr.extract(idx, regs, kc.REGION_SIZE, c['cov_thresh'], c['upstrm'], c['dnstrm'], c.get('cs_cov_thresh'),
                          c['est_mean'], kc.motif_of(c), kc.valid_poss_of(c))
    K = c['upstrm'] + c['dnstrm'] + 1
    return all_regs, (kr.all_kmers(K) if not c.get('motif') else kr.motif_keys(K, kc.motif_of(c)))


@pytest.mark.parametrize('name', sorted(kc.CASES))
def test_restatement_gives_the_reference_lists(name):
    c = kc.CASES[name]
    all_regs, keys = restated(name)
    counts, lv, sd = kr.flatten(all_regs, keys)
    assert len(all_regs) == c['n_regions'] and np.array_equal(counts, kc.GOLD[name + '_reg_counts'])
    kc.assert_under_rule(lv, kc.GOLD[name + '_levels'], kc.GOLD[name + '_asis_levels'], c['spread'][0],
                         not c['est_mean'], name + ' levels')
    kc.assert_under_rule(sd, kc.GOLD[name + '_sds'], kc.GOLD[name + '_asis_sds'], c['spread'][1], False, name + ' sds')


@pytest.mark.parametrize('name', ['canon_med', 'canon_mean', 'canon_cs', 'canon_clean', 'motif_cg'])
def test_restated_medians_give_the_reference_table(name):
    all_regs, keys = restated(name)
    off, lv, sd = kr.table(*kr.flatten(all_regs, keys))
    rows = [(k if isinstance(k, tuple) else (k,)) + (m, s) for k, m, s in zip(keys, kr.medians(lv, off), kr.medians(sd, off))]
    kc.assert_tabulated(rows, name)


def test_the_golden_file_holds_the_cases_it_is_meant_to():
    """the shapes of the issue are in the recorded reads: reads with an N, a NaN level, fewer levels than bases, no
    levels at all; a region without an interval; '-' windows; the pile sizes on both sides of the sorter classes"""
    main = [rd for rds in kc.reads_index('main').values() for rd in rds]
    assert any(rd.seq is not None and 'N' in rd.seq for rd in main)
    assert any(rd.means is not None and np.isnan(rd.means).any() for rd in main)
    assert any(rd.means is not None and len(rd.means) != rd.end - rd.start for rd in main)
    assert any(rd.means is None for rd in main)
    assert all(20 <= rd.end - rd.start <= 120 for rd in main)
    regs = list(th.iter_cov_regs(kc.reads_index('main'), 3, kc.REGION_SIZE, engine=NumpyTracksEngine()))
    assert ('chr1', '+', 400) in [(c, s, int(p)) for c, s, p in regs] and kc.CASES['canon_med']['n_regions'] == len(regs) - 2
    deep = kc.reads_index('deep')
    cov = dict((s, np.bincount(np.concatenate([np.arange(rd.start, rd.end) for rd in deep[('chr1', s)]]))) for s in '+-')
    assert set([4095, 4096, 4097, 4100]) <= set(cov['+'].tolist()) and set([63, 64, 65]) <= set(cov['-'].tolist())
    assert kc.CASES['deep_mean']['spread'][1] > 0      # the deep pile tells the two sort orders apart
    assert np.isnan(kc.GOLD['canon_med_levels']).any()  # a NaN level makes its position's pair NaN
    # no read of the region reaches past 400: the flank of an interval that ends with its region reads '-'
    assert th.get_region_seq(kr.region_reads(kc.reads_index('main'), 'chr1', '+', 300, 100), 299, 401).endswith('-')

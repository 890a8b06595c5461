"""The host layer of the k-mer model estimation (tombo_stats.extract_kmer_levels ... estimate_motif_alt_model,
tombo_helper.get_region_seq, TomboMotif) on the numpy stand-in engine of tests/kmer_est_stub_engine.py, against
the live reference's recorded runs (tests/golden/stats_kmer_est.npz) under the parity rule of kmer_est_cases.
CPU only: what the device computes is checked in test_gpu_kmer_est.py."""
import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th, _native
import kmer_est_cases as kc
import kmer_est_reference as kr
from kmer_est_stub_engine import KmerEstStubEngine

TABULATED = ['canon_med', 'canon_mean', 'canon_cs', 'canon_clean', 'motif_cg']


@pytest.fixture(scope='module')
def tables():
    return dict((name, kc.extract(name, KmerEstStubEngine())) for name in kc.CASES)


@pytest.mark.parametrize('name', sorted(kc.CASES))
def test_extract_gives_the_reference_lists(tables, name):
    kc.assert_table(tables[name], name)


@pytest.mark.parametrize('name', TABULATED)
def test_tabulate_gives_the_reference_table(tables, name):
    eng = KmerEstStubEngine()
    kc.assert_tabulated(kc.tabulate(tables[name], name, eng), name)
    assert [c[0] for c in eng.calls] == ['segment_medians', 'segment_medians']   # one call per column


@pytest.mark.parametrize('name', sorted(set(kc.CASES) - set(TABULATED)))
def test_tabulate_raises_the_reference_text(tables, name):
    c = kc.CASES[name]
    with pytest.raises(th.TomboError) as err:
        kc.tabulate(tables[name], name, KmerEstStubEngine())
    if c['error'] == 'NameError':
        # the reference names an undefined `motif` here and dies; the message it meant, with the least count
        least = int(np.diff(tables[name].off).min())
        assert 0 < least < c['min_kmer_obs']
        assert str(err.value) == ('K-mers represeneted in fewer observations than requested in the provided reads. '
                                  'Consider a shorter k-mer or providing more reads.\n\t%d observations found in least '
                                  'common kmer.' % least)
    else:
        assert str(err.value) == c['error']


def test_no_region_raises_the_reference_text():
    with pytest.raises(th.TomboError) as err:
        ts.extract_kmer_levels(kc.reads_index('main'), kc.REGION_SIZE, 1000, 1, 1, None, engine=KmerEstStubEngine())
    assert str(err.value) == ('No genomic positions contain --minimum-test-reads. Consider setting this option to a '
                              'lower value.')


def test_regions_are_cut_into_calls_by_the_level_budget(tables):
    one, many = KmerEstStubEngine(), KmerEstStubEngine()
    together = kc.extract('motif_cg', one)
    apart = kc.extract('motif_cg', many, max_levels=1)
    n_calls = lambda e: sum(c[0] == 'region_key_levels' for c in e.calls)
    assert n_calls(one) == 1 and n_calls(many) == kc.CASES['motif_cg']['n_regions']
    for a, b in ((together, apart), (together, tables['motif_cg'])):
        assert np.array_equal(a.off, b.off) and np.array_equal(kc.bits(a.levels), kc.bits(b.levels)) and \
            np.array_equal(kc.bits(a.sds), kc.bits(b.sds))


def test_subsampling_that_leaves_no_read_contributes_nothing(monkeypatch):
    """the reference fails on len(None) where the cut leaves no read; here that region alone drops out: with the
    cut of ONE region forced to nothing the table is the recorded one minus that region's lists"""
    target = ('chr1', '+', 100)
    real = ts._subsample_region_reads

    def cut(reads, reg_start, reg_end, region_size, cs_cov_thresh):
        kept = real(reads, reg_start, reg_end, region_size, cs_cov_thresh)     # (the shuffle is drawn all the same)
        return [] if (reads[0].strand, reg_start) == target[1:] else kept
    monkeypatch.setattr(ts, '_subsample_region_reads', cut)
    c = kc.CASES['canon_cs']
    regs = [r for r in th.iter_cov_regs(kc.reads_index('main'), c['cov_thresh'], kc.REGION_SIZE, engine=KmerEstStubEngine())
            if kr.region_reads(kc.reads_index('main'), r[0], r[1], int(r[2]), kc.REGION_SIZE)]
    drop = [(ch, st, int(p)) for ch, st, p in regs].index(target)
    counts = kc.GOLD['canon_cs_reg_counts'].astype(np.int64)
    assert counts.shape[0] == len(regs) - 2 and counts[drop].sum() > 0     # (two regions have no interval: [400, 500))
    at = np.concatenate([[0], np.cumsum(counts.sum(axis=1))])
    keep = np.r_[0:at[drop], at[drop + 1]:at[-1]]
    off, lv, sd = kr.table(np.delete(counts, drop, axis=0), kc.GOLD['canon_cs_levels'][keep], kc.GOLD['canon_cs_sds'][keep])
    got = kc.extract('canon_cs', KmerEstStubEngine())
    assert got.n_regions == c['n_regions'] - 1 and np.array_equal(got.off, off)
    assert np.array_equal(kc.bits(got.levels), kc.bits(lv)) and np.array_equal(kc.bits(got.sds), kc.bits(sd))


def test_extract_checks_its_arguments():
    idx, eng = kc.reads_index('main'), KmerEstStubEngine()
    for bad in (dict(region_size=0), dict(upstrm_bases=-1), dict(max_levels=0),
                dict(valid_poss={('chr1', '+'): np.array([5])})):
        kw = dict(region_size=100, cov_thresh=3, upstrm_bases=1, dnstrm_bases=1, cs_cov_thresh=None, engine=eng)
        kw.update(bad)
        with pytest.raises(ValueError):
            ts.extract_kmer_levels(idx, **kw)
    with pytest.raises(ValueError):
        ts.tabulate_mod_kmer_levels(kc.extract('motif_cg', eng), 1, th.TomboMotif('CCWGG', 2), engine=eng)
    with pytest.raises(th.TomboError) as err:
        ts.estimate_motif_alt_model(idx, 'CG', 1, 1, None, 1, 3, None, 100, engine=eng)
    assert str(err.value) == 'Invalid motif decription format.'


def test_estimators_end_to_end():
    kc.assert_models(kc.end_to_end_models(KmerEstStubEngine()))


@pytest.mark.parametrize('name', sorted(kc.CENTER_RUNS))
def test_centring_gives_the_reference_factors(name):
    """max_reads below, at and above the number of successes; the read whose slope is 0 is skipped; the 1200-base
    read is drawn with np.random.choice in read order; without a success the reference's message"""
    kc.assert_centring(name, KmerEstStubEngine())


def test_centring_skips_failed_reads_and_refuses_rna():
    good = kc.center_reads([0])[0]
    bad = [good._replace(seq=good.seq[:5] + 'N' + good.seq[6:]), good._replace(event_starts=good.event_starts[:-1]),
           good._replace(read_start_rel_to_raw=10 ** 6), good._replace(raw_signal=good.raw_signal[:300])]
    for rd in bad:
        with pytest.raises(th.TomboError, match='No reads succcessfully processed'):
            ts.center_model_to_median_norm([rd], kc.center_init(), engine=KmerEstStubEngine())
    np.random.seed(1)
    with pytest.warns(UserWarning, match='Fewer reads succcessfully processed'):
        one = ts.center_model_to_median_norm([good], kc.center_init(), engine=KmerEstStubEngine())
    np.random.seed(1)
    with pytest.warns(UserWarning):
        among = ts.center_model_to_median_norm(bad + [good], kc.center_init(), engine=KmerEstStubEngine())
    assert np.array_equal(one.level_means, among.level_means)
    with pytest.raises(NotImplementedError, match='RNA'):
        ts.center_model_to_median_norm([good._replace(rna=True)], kc.center_init(), engine=KmerEstStubEngine())


def test_an_uncentred_model_comes_with_a_warning():
    c = kc.CASES['canon_clean']
    with pytest.warns(UserWarning, match='not centred'):
        model = ts.estimate_kmer_model(kc.reads_index('clean'), c['cov_thresh'], 1, 1, 1, True, None, False, kc.REGION_SIZE,
                                       engine=KmerEstStubEngine())
    assert np.array_equal(kc.bits(model.level_means), kc.bits(kc.GOLD['canon_clean_tab'][:, 0]))


def test_model_centring_and_constant_sd():
    kmers = kr.all_kmers(2)
    m = ts.TomboModel(kmer_ref=[(k, 0.1 * i, 0.2 + 0.01 * i) for i, k in enumerate(kmers)], central_pos=0)
    want = dict((k, (0.1 * i * 1.25) + -0.3) for i, k in enumerate(kmers))
    m._center_model(-0.3, 1.25)
    assert m.means == want and m.sds['AC'] == 0.2 + 0.01
    m._make_constant_sd()
    assert set(m.sds.values()) == {float(np.median([0.2 + 0.01 * i for i in range(16)]))}
    alt = ts.AltModel([('ACG', 1, 0.5, 0.1), ('CGA', 0, 0.7, 0.3), ('TCG', 1, 0.2, 0.2)], 1, 'C')
    alt._make_constant_sd()
    assert alt.sds == {('ACG', 1): 0.2, ('CGA', 0): 0.2, ('TCG', 1): 0.2} and alt.means[('CGA', 0)] == 0.7


def test_motif_partial_matches():
    """find_mod_poss / matches_seq count partial matches at both ends that hold the modified position"""
    cg = th.TomboMotif('CG', 1)
    assert cg.find_mod_poss('ACG') == [2] and cg.find_mod_poss('AAC') == [3] and cg.find_mod_poss('GAA') == []
    assert cg.find_mod_poss('CGC') == [1, 3] and cg.matches_seq('TTC') and not cg.matches_seq('GTT')
    m = th.TomboMotif('CCWGG', 2)
    assert m.rev_comp_pat.pattern == 'CC[AT]GG' and m.is_palindrome
    assert m.find_mod_poss('CCAGG') == [2] and m.find_mod_poss('CAG') == [1] and m.find_mod_poss('ACC') == [3]
    assert m.find_mod_poss('CTG') == [1] and m.find_mod_poss('GCC') == [3] and not m.matches_seq('AGG')
    assert th.TomboMotif('GATC', 2).rev_comp_pat.pattern == 'GATC' and th.TomboMotif('ACH').rev_comp_pat.pattern == '[AGT]GT'


def test_region_seq_greedy_cover_and_dashes():
    R = lambda s, e, strand, seq: th.resquiggledRead(s, e, False, 0, strand, None, None, False, means=None, seq=seq)
    assert th.get_region_seq([], 5, 9) == '----' and th.get_region_seq(None, 5, 9) == '----'
    assert th.get_region_seq([R(0, 12, '+', 'ACGTACGTACGT')], 2, 6) == 'GTAC'           # one read covers it
    assert th.get_region_seq([R(0, 12, '-', 'ACGTACGTACGT')], 2, 6) == 'GTAC'           # ... its reverse complement
    assert th.get_region_seq([R(4, 8, '+', 'TTTT')], 2, 10) == '--TTTT--'                # uncovered flanks
    assert th.get_region_seq([R(0, 5, '+', 'AAAAA'), R(3, 9, '+', 'CCCCCC')], 2, 12) == 'ACCCCCC---'   # (the later read writes over the overlap)
    assert th.get_region_seq([R(4, 8, '+', None)], 2, 10) == '--------'                  # a read without bases


def test_engine_argument_checks():
    good = [np.zeros(2, np.int64), np.zeros(2, np.uint8), np.array([0, 3, 5]), np.zeros(5), np.array([0, 2]),
            np.array([0, 1]), np.zeros(4, np.int64), np.arange(4), np.array([0, 3, 3]), np.array([1, 0, 6]), 7]
    _native._check_region_key_levels_args(*good)
    for i, bad in ((0, np.zeros(2, np.int32)), (1, np.zeros(2, np.int8)), (3, np.zeros(5, np.float32)), (3, np.zeros(4)),
                   (2, np.array([0, 3, 2])), (4, np.array([1, 2])), (5, np.array([0, 2])), (5, np.array([0, -1])),
                   (6, np.ones(4, np.int64)), (6, np.zeros(3, np.int64)), (8, np.array([0, 3, 4])),
                   (8, np.array([0, 3])), (9, np.array([1, 0, 7])), (9, np.array([1, 0, -1])), (10, 0), (10, 2 ** 24 + 1),
                   (10, 6.5)):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            _native._check_region_key_levels_args(*args)
    _native._check_segment_medians_args(np.zeros(3), np.array([0, 1, 3]))
    for v, off in ((np.zeros(3, np.float32), np.array([0, 3])), (np.zeros(3), np.array([0, 2])),
                   (np.zeros(3), np.array([1, 3])), (np.zeros((3, 1)), np.array([0, 3])), (np.zeros(3), np.array([0, 3.0]))):
        with pytest.raises(ValueError):
            _native._check_segment_medians_args(v, off)

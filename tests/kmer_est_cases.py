"""TEST INFRASTRUCTURE: the recorded cases of tests/golden/stats_kmer_est.npz (written by
tests/golden/gen_golden_kmer_est.py from the live reference) as the objects the k-mer model estimation takes,
and the comparisons the CPU and GPU tests share.

Parity rule (the golden file holds two runs of the reference, see its generator): against the run with a stable
sort in get_reads_events everything is compared bit for bit; against the run as the reference is, counts and the
est_mean=False levels bit for bit and the order-dependent columns within four times the recorded spread of that
column (exact where the spread is zero)."""
import os
import json

import numpy as np

from tombo_amd import tombo_stats as ts, tombo_helper as th
import kmer_est_reference as kr

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stats_kmer_est.npz'))
META = json.loads(str(GOLD['meta']))
CASES = dict((c['name'], c) for c in META['cases'])
REGION_SIZE, CHRM = META['region_size'], META['chrm']
_INDEX = {}


def reads_index(name):
    """{(chrm, strand): [th.resquiggledRead]} of the recorded read set, in the recorded order"""
    if name == 'clean':     # the reads of 'main' without those that hold a NaN level
        return dict((cs, [rd for rd in rds if rd.means is None or not np.isnan(rd.means).any()])
                    for cs, rds in reads_index('main').items())
    if name not in _INDEX:
        g = lambda k: GOLD[name + '_' + k]
        seq, off = g('seq').tobytes().decode(), g('off')
        means = GOLD['deep_means_q256'] / 256.0 if name == 'deep' else g('means')
        idx = {}
        for i, (minus, s, e, has) in enumerate(zip(g('minus').tolist(), g('start').tolist(), g('end').tolist(),
                                                   g('has').tolist())):
            strand = '-' if minus else '+'
            idx.setdefault((CHRM, strand), []).append(th.resquiggledRead(
                s, e, False, 0, strand, None, None, False, read_id='%s%d' % (name, i),
                means=means[off[i]:off[i + 1]].copy() if has else None, seq=seq[off[i]:off[i + 1]] if has else None))
        _INDEX[name] = idx
    return _INDEX[name]


def center_reads(which=None):
    """the recorded centring reads as ts.CenterRead (which: indices; default all ten)"""
    roff, off, seq = GOLD['center_raw_off'], GOLD['center_off'], GOLD['center_seq'].tobytes().decode()
    reads = [ts.CenterRead(GOLD['center_raw'][roff[i]:roff[i + 1]], GOLD['center_start'][off[i]:off[i + 1]],
                           seq[off[i]:off[i + 1]], int(GOLD['center_rsr'][i])) for i in range(off.shape[0] - 1)]
    return reads if which is None else [reads[i] for i in which]


CENTER_RUNS = dict((r['name'], r) for r in META['center_runs'])


def center_init():
    init = GOLD['center_init']
    return ts.TomboModel(kmer_ref=list(zip(kr.all_kmers(3), init[:, 0].tolist(), init[:, 1].tolist())), central_pos=1)


def run_centring(name, engine):
    """ts.center_model_to_median_norm as the generator ran the reference's -> (model, [(shift, scale)])"""
    run = CENTER_RUNS[name]
    model, factors = center_init(), []
    real = model._center_model
    model._center_model = lambda shift, scale: (factors.append((float(shift), float(scale))), real(shift, scale))[1]
    np.random.seed(run['seed'])
    ts.center_model_to_median_norm(center_reads(run['reads']), model, run['max_reads'], engine=engine)
    return model, factors


def assert_centring(name, engine):
    """factors and centred model of a recorded run, bit for bit; its warning or error text"""
    import warnings
    import pytest
    run = CENTER_RUNS[name]
    if run['error']:
        with pytest.raises(th.TomboError) as err:
            run_centring(name, engine)
        assert str(err.value) == run['error']
        return
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        model, factors = run_centring(name, engine)
    assert [str(w.message) for w in caught if 'succcessfully' in str(w.message)] == ([run['warning']] if run['warning'] else [])
    print('%s: factors %r, recorded %r' % (name, factors, run['factors']))
    assert np.array_equal(bits(factors[0]), bits(run['factors']))
    assert np.array_equal(bits(model.level_means), bits(GOLD['center_' + name + '_means']))


def motif_of(case):
    if not case.get('motif'):
        return None
    raw, pos = case['motif'].split(':')
    return th.TomboMotif(raw, int(pos))


def valid_poss_of(case):
    return None if case.get('valid_poss') is None else {(CHRM, '+'): np.array(case['valid_poss'], dtype=np.int64)}


def extract(name, engine, **kw):
    """ts.extract_kmer_levels as the generator ran the reference's"""
    c = CASES[name]
    if c.get('seed') is not None:
        np.random.seed(c['seed'])
    return ts.extract_kmer_levels(reads_index(c['reads']), REGION_SIZE, c['cov_thresh'], c['upstrm'], c['dnstrm'],
                                  c.get('cs_cov_thresh'), c['est_mean'], motif_of(c), valid_poss_of(c), engine=engine,
                                  **kw)


def bits(a):
    """the bit patterns of float64 values; every NaN as one pattern (a NaN's sign and payload are not compared)"""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.int64)


def recorded_table(name, run=''):
    """(off, levels, sds) per key of a recorded run ('' the stable one, 'asis_' the reference as it is)"""
    return kr.table(GOLD[name + '_reg_counts'].astype(np.int64), GOLD[name + '_' + run + 'levels'],
                    GOLD[name + '_' + run + 'sds'])


def assert_under_rule(got, stable, asis, spread, order_free, what):
    """the parity rule for one column: bit-equal to the stable-sort run; to the as-is run bit-equal where the
    column does not depend on the order (or the recorded spread is zero), else within four times the spread"""
    got = np.asarray(got, dtype=np.float64)
    assert np.array_equal(bits(got), bits(stable)), what + ': differs from the stable-sort run'
    if order_free or spread == 0:
        assert np.array_equal(bits(got), bits(asis)), what + ': differs from the as-is run'
        return
    assert np.array_equal(np.isnan(got), np.isnan(asis))
    ok = ~np.isnan(asis)
    diff = float(np.max(np.abs(got[ok] - asis[ok]))) if ok.any() else 0.0
    print('%s: max |difference| to the as-is run %.3g, recorded spread %.3g' % (what, diff, spread))
    assert diff <= 4 * spread


def assert_table(table, name):
    """a ts.KmerLevelTable against the recorded per-region lists"""
    c = CASES[name]
    off, _, _ = recorded_table(name)
    K = c['upstrm'] + c['dnstrm'] + 1
    assert list(table.keys) == (kr.all_kmers(K) if not c.get('motif') else kr.motif_keys(K, motif_of(c)))
    assert table.off.dtype == np.int64 and np.array_equal(table.off, off)
    assert table.n_regions == c['n_regions']
    _, lv, sd = recorded_table(name)
    _, lv2, sd2 = recorded_table(name, 'asis_')
    assert_under_rule(table.levels, lv, lv2, c['spread'][0], not c['est_mean'], name + ' levels')
    assert_under_rule(table.sds, sd, sd2, c['spread'][1], False, name + ' sds')


def tabulate(table, name, engine):
    c = CASES[name]
    if c.get('motif'):
        return ts.tabulate_mod_kmer_levels(table, c['min_kmer_obs'], motif_of(c), engine=engine)
    return ts.tabulate_kmer_levels(table, c['min_kmer_obs'], engine=engine)


def assert_tabulated(rows, name):
    c = CASES[name]
    assert [r[:-2] for r in rows] == [((k,) if not c.get('motif') else k) for k in
                                      (kr.all_kmers(3) if not c.get('motif') else kr.motif_keys(3, motif_of(c)))]
    got = np.array([r[-2:] for r in rows], dtype=np.float64)
    for j in (0, 1):
        assert_under_rule(got[:, j], GOLD[name + '_tab'][:, j], GOLD[name + '_asis_tab'][:, j], c['tab_spread'][j],
                          j == 0 and not c['est_mean'], name + ' tabulated column %d' % j)


def end_to_end_models(engine):
    """(kmer-specific-sd model, constant-sd model, motif model) as the generator ran the reference's lines"""
    import warnings
    c, m = CASES['canon_clean'], CASES['motif_cg']
    args = (reads_index('clean'), c['cov_thresh'], c['upstrm'], c['dnstrm'], c['min_kmer_obs'])
    models = []
    for kmer_specific_sd in (True, False):
        np.random.seed(META['model_center_seed'])
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')    # (fewer centring reads than NUM_READS_TO_ADJUST_MODEL)
            models.append(ts.estimate_kmer_model(*args, kmer_specific_sd, None, False, REGION_SIZE,
                                                 center_reads=center_reads(), engine=engine))
    return models + [ts.estimate_motif_alt_model(reads_index('main'), m['motif'], m['upstrm'], m['dnstrm'], None,
                                                 m['min_kmer_obs'], m['cov_thresh'], None, REGION_SIZE, engine=engine)]


def assert_models(models):
    import memh5
    full, const, alt = models
    for model, rec in ((full, GOLD['model_kmer_sd']), (const, GOLD['model_const_sd'])):
        assert model.kmer_width == 3 and model.central_pos == 1
        assert np.array_equal(bits(model.level_means), bits(rec[:, 0]))
        assert np.array_equal(bits(model.level_sds), bits(rec[:, 1]))
    rec = GOLD['alt_model']
    assert [(k, p) for k, p in alt.means] == [(r['kmer'].decode(), int(r['pos'])) for r in rec]
    assert np.array_equal(bits([alt.means[kp] for kp in alt.means]), bits(rec['mean']))
    assert np.array_equal(bits([alt.sds[kp] for kp in alt.sds]), bits(rec['sd']))
    for model, name in ((const, 'model_const_sd'), (alt, 'alt_model')):
        grp = memh5.MemGroup()
        model.write_model(grp)
        tree = memh5.tree(grp)
        tab = tree.pop('/model')
        want = GOLD[name + '_written_model']
        assert tab.dtype == want.dtype and tab.tobytes() == want.tobytes()
        assert dict((k, v if isinstance(v, (int, str)) or v is None else int(v)) for k, v in tree.items()) == \
            META[name + '_written_attrs']
        assert grp.items['model'].kw == META[name + '_written_dataset_kw']

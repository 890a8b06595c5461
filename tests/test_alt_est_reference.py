"""The host layer of the alternate-model estimation against the live reference's recorded output
(tests/golden/stats_alt_est.npz), on the numpy stand-in engine: no GPU."""
import hashlib
import warnings

import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th
import alt_est_cases as ac
import memh5
from alt_est_stub_engine import AltEstStubEngine


@pytest.mark.parametrize('name', ['a_overshoot', 'a2_batch_of_7'])
def test_parse_base_levels_batches_and_completion(name):
    """k-mers complete after a batch, keep that batch's levels (so they pass the cap) and are skipped afterwards"""
    eng = AltEstStubEngine()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = ac.parse_case(name, eng)
    ac.assert_levels_bit_equal(got, name)
    c = ac.PARSE_CASES[name]
    n = np.diff(got[1])
    assert n.max() > c['max_kmer_obs']
    assert len(eng.calls) >= 2 and all(k == 'kmer_levels' and r <= c['batch'] for k, r in eng.calls)


def test_parse_base_levels_warns_when_the_reads_run_out():
    """(b), with the reads of (d): shorter than K, exactly K, with Ns, a NaN level"""
    with pytest.warns(UserWarning) as rec:
        got = ac.parse_case('b_reads_run_out', AltEstStubEngine())
    assert [str(w.message) for w in rec] == [ac.PARSE_CASES['b_reads_run_out']['warning']]
    ac.assert_levels_bit_equal(got, 'b_reads_run_out')
    assert np.isnan(got[0]).sum() == 1   # the NaN level is kept


def test_parse_base_levels_raises_where_the_reference_exits():
    with pytest.raises(th.TomboError) as e:
        ac.parse_case('c_too_few', AltEstStubEngine())
    assert str(e.value) == ac.PARSE_CASES['c_too_few']['error']


def test_isolate_alt_density_without_an_engine():
    alt = dict(zip(ac.KMERS, ac.GOLD['g_alt_dens']))
    std = dict(zip(ac.KMERS, ac.GOLD['g_std_dens']))
    before = ac.GOLD['g_alt_dens'].copy()
    model = ts.isolate_alt_density(alt, std, ac.META['alt_base'], ac.META['alt_frac_pctl'], ac.std_ref(), ac.SAVE_G)
    ac.assert_model_close(model, ac.GOLD['g_model'])
    assert np.array_equal(before, np.array(list(alt.values())))
    assert sorted(set(k.count('A') for k, _ in model.means)) == [1, 2, 3]
    assert model.central_pos == ac.CP and model.alt_base == 'A' and model.kmer_width == ac.K


def test_estimate_alt_model_from_reads_and_from_density_files(tmp_path):
    eng = AltEstStubEngine()
    base = str(tmp_path / 'dens')
    model = ac.estimate(eng, density_basename=base)
    ac.assert_model_close(model, ac.GOLD['g_model'])
    assert [k for k, _ in eng.calls].count('kde_eval') == 2   # one call per sample for all k-mers
    # the files this run wrote: the reference's format (same header, same line count; the text itself
    # differs from the reference's only where a density differs in its last digits)
    for nm in ('alternate', 'control'):
        text = open('%s.%s_density.txt' % (base, nm)).read()
        rec = ac.META['density_files'][nm]
        assert text.split('\n')[0] == rec['head'][0] and text.count('\n') == rec['n_lines']
        assert [ln.split('\t')[:2] for ln in text.split('\n')[1:3]] == [ln.split('\t')[:2] for ln in rec['head'][1:3]]
    from_files = ac.estimate(None, alt_dens_fn=base + '.alternate_density.txt',
                             std_dens_fn=base + '.control_density.txt')
    ac.assert_model_close(from_files, ac.GOLD['g_model_from_files'])


def test_density_file_round_trip(tmp_path):
    """the recorded densities written in the reference's text format hash to what the reference wrote, and
    parse back to the same values"""
    for nm, key in (('alternate', 'g_alt_dens'), ('control', 'g_std_dens')):
        fn = str(tmp_path / (nm + '.txt'))
        dens = dict(zip(ac.KMERS, ac.GOLD[key]))
        ts.write_kmer_densities_file(fn, dens, ac.SAVE_G)
        assert hashlib.sha256(open(fn).read().encode()).hexdigest() == ac.META['density_files'][nm]['sha256']
        back = ts.parse_kmer_densities_file(fn)
        assert list(back) == ac.KMERS
        assert np.array_equal(np.array(list(back.values())), ac.GOLD[key])
    bad = str(tmp_path / 'bad.txt')
    open(bad, 'w').write('Kmer\tSignal\tDensity\nAAA\t0.0\t1.0\nAAA\t0.1\t1.0\nAAC\t0.0\t1.0\n')
    with pytest.raises(th.TomboError, match='Density file is valid.'):
        ts.parse_kmer_densities_file(bad)
    short = str(tmp_path / 'short.txt')
    ts.write_kmer_densities_file(short, dict((k, v[:10]) for k, v in dens.items()), ac.SAVE_G[:10])
    with pytest.raises(th.TomboError, match='do not correspond'):
        ts.load_kmer_densities(fn, short, ac.std_ref())


def test_write_model_tree():
    tab = ac.GOLD['g_model']
    model = ts.AltModel([(r['kmer'].decode(), int(r['pos']), float(r['mean']), float(r['sd'])) for r in tab],
                        ac.CP, 'A')
    grp = memh5.MemGroup()
    model.write_model(grp)
    tree = memh5.tree(grp)
    written = tree.pop('/model')
    assert written.dtype == ac.GOLD['g_written_model'].dtype
    assert np.array_equal(written, ac.GOLD['g_written_model'])
    assert dict((k, v) for k, v in tree.items()) == ac.META['written_attrs']
    assert grp.items['model'].kw == ac.META['written_dataset_kw']


def test_stub_densities_meet_the_recorded_scipy_densities():
    """the stand-in's density formula is the one the device implements: it has to meet the tolerance of
    the GPU test on the same segments"""
    got = AltEstStubEngine().kde_eval(ac.GOLD['dens_levels'], ac.GOLD['dens_lv_off'], ac.SAVE_X, ac.META['bw'])
    ac.assert_density_close(got, ac.GOLD['dens_scipy'])
    assert ac.META['dens_direct_spread'] < 1e-13

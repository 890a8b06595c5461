"""The host layer of batch centring (tombo_stats.center_model_to_median_norm_batch, estimate_kmer_model's
center_batch) on the numpy stand-in engine of tests/center_stub_engine.py, against the live reference's recorded
runs: DNA from tests/golden/stats_kmer_est.npz, RNA from tests/golden/stats_center_rna.npz.  Equality of bits everywhere.
CPU only: what the device computes is checked in test_gpu_center_batch.py."""
import warnings

import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th, _native
import kmer_est_cases as kc
import center_batch_cases as cc
from center_stub_engine import CenterStubEngine


@pytest.mark.parametrize('name', sorted(kc.CENTER_RUNS))
def test_dna_runs_give_the_reference_factors(name):
    """max_reads below, at and above the successes (the stop, the warning), no success at all (the error)"""
    cc.assert_dna_run(name, CenterStubEngine())


@pytest.mark.parametrize('name', sorted(cc.RNA_RUNS))
def test_rna_runs_give_the_reference_factors(name):
    """... and the reads the reference skipped are the reads that fail, each of the others has its recorded factors:
    the long read without change points takes no draw from the read drawn after it"""
    spy = cc.assert_rna_run(name, CenterStubEngine())
    if spy is not None:
        assert spy.calls[0][2] == np.int16


def test_rna_float64_input_gives_the_same_bits():
    cc.assert_rna_run('all_reads', CenterStubEngine(), np.float64)


@pytest.mark.parametrize('kind', ['dna', 'rna'])
def test_chunks_of_one_three_and_all_give_the_same_bits(kind):
    """max_reads (3) is reached inside a chunk of three and the work stops with that chunk"""
    name = 'first_three'
    run_of = cc.assert_dna_run if kind == 'dna' else cc.assert_rna_run
    n_reads = len((kc.CENTER_RUNS if kind == 'dna' else cc.RNA_RUNS)[name]['reads'])
    seen = {}
    for chunk in (1, 3, n_reads):
        spy = run_of(name, CenterStubEngine(), chunk_reads=chunk)
        seen[chunk] = sum(c[1] for c in spy.calls if c[0] == 'center_prepare')
        assert all(c[1] <= chunk for c in spy.calls if c[0] == 'center_prepare')
    assert seen[n_reads] == n_reads and seen[1] <= seen[3] < n_reads and seen[3] % 3 == 0
    run_of('all_reads', CenterStubEngine(), chunk_reads=1)
    run_of('all_reads', CenterStubEngine(), chunk_reads=3)


def test_the_default_chunk_is_no_larger_than_the_successes_wanted(monkeypatch):
    monkeypatch.setattr(ts, '_default_center_chunk', lambda *a: 4)
    spy = cc.assert_dna_run('all_reads', CenterStubEngine())
    assert [c[1] for c in spy.calls if c[0] == 'center_prepare'] == [4, 4, 2]


def test_messages_and_the_mixed_list():
    good = kc.center_reads([0])[0]
    with pytest.raises(th.TomboError) as err:
        ts.center_model_to_median_norm_batch([], kc.center_init(), engine=CenterStubEngine())
    assert str(err.value) == 'No reads succcessfully processed for sequence-based normalization parameter re-fitting.'
    with pytest.warns(UserWarning) as caught:
        ts.center_model_to_median_norm_batch([good], kc.center_init(), engine=CenterStubEngine())
    assert [str(w.message) for w in caught] == ['Fewer reads succcessfully processed for sequence-based normalization '
                                                'parameter re-fitting than requested.']
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ts.center_model_to_median_norm_batch([good], kc.center_init(), 1, engine=CenterStubEngine())
    with pytest.raises(ValueError, match='RNA and DNA'):
        ts.center_model_to_median_norm_batch([good, cc.rna_reads([0])[0]], kc.center_init(), engine=CenterStubEngine())
    for kw in (dict(max_reads=0), dict(chunk_reads=0)):
        with pytest.raises(ValueError):
            ts.center_model_to_median_norm_batch([good], kc.center_init(), engine=CenterStubEngine(), **kw)
    # a model without a downstream base: every read fails, as in the per-read form
    flat = ts.TomboModel(kmer_ref=[(k, 0.1 * i, 0.2) for i, k in enumerate('ACGT')], central_pos=0)
    with pytest.raises(th.TomboError, match='No reads succcessfully processed'):
        ts.center_model_to_median_norm_batch([good], flat, engine=CenterStubEngine())


def test_center_read_fields():
    rd = ts.CenterRead('raw', 'starts', 'seq', 7)
    assert rd.rna is False and rd.map_len is None and rd._fields[-1] == 'map_len'
    assert ts.CenterRead('raw', 'starts', 'seq', 7, True).map_len is None
    assert rd._replace(rna=True, map_len=12)[-2:] == (True, 12)


def test_map_len_defaults_to_the_number_of_bases():
    """read 8 of the fixture: 10-14 samples a base, so compute_num_events takes int(map_len * 1.1); its recorded
    map_len is 5 above its bases.  None counts the bases, which asks for five change points less"""
    rd = cc.rna_reads([8])[0]
    seen = []

    class Eng(CenterStubEngine):
        def center_prepare(self, params, opts, raws, codes, starts, rsr, num_events=None):
            seen.append(list(num_events))
            return CenterStubEngine.center_prepare(self, params, opts, raws, codes, starts, rsr, num_events)
    for r in (rd, rd._replace(map_len=None), rd._replace(map_len=len(rd.seq))):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ts.center_model_to_median_norm_batch([r], cc.rna_init(), engine=Eng())
    assert seen == [[int(305 * 1.1)], [int(300 * 1.1)], [int(300 * 1.1)]] and len(rd.seq) == 300


@pytest.mark.parametrize('kind', ['dna', 'rna'])
def test_bad_reads_among_good_ones_change_nothing(kind):
    """the bad reads of test_kmer_est_host_layer (an N in the sequence, one row short, events past the signal, raw too
    short) between good reads: each fails alone; for DNA the per-read form agrees"""
    reads, init = (kc.center_reads([0, 1, 2]), kc.center_init) if kind == 'dna' else (cc.rna_reads([0, 1, 2]), cc.rna_init)
    good = reads[0]
    bad = [good._replace(seq=good.seq[:5] + 'N' + good.seq[6:]), good._replace(event_starts=good.event_starts[:-1]),
           good._replace(read_start_rel_to_raw=10 ** 6), good._replace(raw_signal=good.raw_signal[:300])]
    mixed = [reads[0], bad[0], bad[1], reads[1], bad[2], bad[3], reads[2]]
    for rd in bad:
        with pytest.raises(th.TomboError, match='No reads succcessfully processed'):
            ts.center_model_to_median_norm_batch([rd], init(), engine=CenterStubEngine())
    alone = cc.run_batch(list(reads), init(), 3, 50, CenterStubEngine())
    among = cc.run_batch(list(mixed), init(), 3, 50, CenterStubEngine())
    assert np.array_equal(cc.bits(alone[1]), cc.bits(among[1]))
    order = cc.shuffled(len(mixed), 3)
    failed = among[3].statuses()[1] != 0
    assert [any(mixed[i] is b for b in bad) for i in order] == failed.tolist()
    if kind == 'dna':
        np.random.seed(3)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            per_read = ts.center_model_to_median_norm(list(mixed), init(), 50, engine=CenterStubEngine())
        assert np.array_equal(cc.bits(per_read.level_means), cc.bits(among[0].level_means))


def test_estimate_kmer_model_center_batch_equals_the_per_read_path():
    c = kc.CASES['canon_clean']
    args = (kc.reads_index('clean'), c['cov_thresh'], c['upstrm'], c['dnstrm'], c['min_kmer_obs'], True, None, False,
            kc.REGION_SIZE)
    models = []
    for center_batch in (False, True):
        eng = CenterStubEngine()
        np.random.seed(kc.META['model_center_seed'])
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            models.append(ts.estimate_kmer_model(*args, center_reads=kc.center_reads(), engine=eng,
                                                 center_batch=center_batch))
        assert any(call[0] == 'center_prepare' for call in eng.calls) == center_batch
    assert np.array_equal(cc.bits(models[0].level_means), cc.bits(models[1].level_means))
    assert np.array_equal(cc.bits(models[1].level_means), cc.bits(kc.GOLD['model_kmer_sd'][:, 0]))
    # RNA reads take the batch form by themselves (the per-read form refuses them)
    eng = CenterStubEngine()
    np.random.seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ts.estimate_kmer_model(*args, center_reads=cc.rna_reads([0, 1]), engine=eng)
    assert any(call[0] == 'center_prepare' for call in eng.calls)


def test_engine_argument_checks():
    raw, codes, starts = [np.zeros(50, np.int16), np.zeros(40, np.int16)], [np.zeros(5, np.uint8)] * 2, [np.arange(5)] * 2
    out = _native._check_center_prepare_args(raw, codes, starts, [3, 4], None, False)
    assert out[0].dtype == np.int16 and out[1].tolist() == [0, 50, 90] and out[5].tolist() == [0, 5, 10] and out[7] is None
    mixed = _native._check_center_prepare_args([raw[0], raw[1].astype(np.float64)], codes, starts, [3, 4], [2, 2], True)
    assert mixed[0].dtype == np.float64 and mixed[7].tolist() == [2, 2]
    for bad in (dict(raws=[]), dict(codes=codes[:1]), dict(event_starts=starts[:1]), dict(rsr=[3]),
                dict(raws=[raw[0], np.zeros((2, 2))]), dict(codes=[codes[0], np.zeros(5, np.int8)]),
                dict(event_starts=[starts[0], np.zeros(5)]), dict(num_events=[2]), dict(num_events=[2, 0]), dict(rna=True)):
        kw = dict(raws=raw, codes=codes, event_starts=starts, rsr=[3, 4], num_events=None, rna=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            _native._check_center_prepare_args(kw['raws'], kw['codes'], kw['event_starts'], kw['rsr'], kw['num_events'], kw['rna'])
    samp = np.zeros((2, _native.MAX_POINTS_FOR_THEIL_SEN), np.int64)
    s, p = _native._check_center_fit_args(2, [3, 1200], samp, None, 5)
    assert s is samp and p.shape == (0, 2)
    for args in ((None, None, None, None, 5), (2, [3, 3], None, None, 0), (2, [3, 3], samp[:1], None, 5),
                 (2, [3, 1200], None, None, 5), (2, [3, 3], None, np.zeros(3), 5)):
        with pytest.raises(ValueError):
            _native._check_center_fit_args(*args)
    with pytest.raises(ValueError, match='center_prepare has not been called'):
        CenterStubEngine().center_fit()

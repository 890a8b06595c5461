"""Batch centring on the device (tba_center_prepare / tba_center_fit: k_center_place, k_center_pick and the centring
step list of the engine; tombo_stats.center_model_to_median_norm_batch on top) against the live reference's recorded
runs -- DNA from tests/golden/stats_kmer_est.npz, RNA from tests/golden/stats_center_rna.npz -- and against the per-read
form on the same engine.  Equality of bits everywhere."""
import warnings

import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq, _native
import kmer_est_cases as kc
import center_batch_cases as cc

pytestmark = pytest.mark.gpu
FEWER_CPTS, ZERO_LEN, NEG_START, PAST_END, RESCALE_FAIL, SEQ_SEG_MISMATCH, INVALID_SEQ = 2, 16, 17, 18, 19, 20, 22


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


@pytest.mark.parametrize('name', sorted(kc.CENTER_RUNS))
def test_dna_runs_match_the_reference_and_the_per_read_form(eng, name):
    run = kc.CENTER_RUNS[name]
    cc.assert_dna_run(name, eng)
    if run['error']:
        with pytest.raises(th.TomboError):
            kc.run_centring(name, eng)
        return
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model, factors = kc.run_centring(name, eng)     # the per-read form, same engine, same seed
    batch = cc.run_batch(kc.center_reads(run['reads']), kc.center_init(), run['seed'], run['max_reads'], eng)
    assert np.array_equal(cc.bits(factors[0]), cc.bits(batch[1]))
    assert np.array_equal(cc.bits(model.level_means), cc.bits(batch[0].level_means))


@pytest.mark.parametrize('dtype', [np.int16, np.float64])
@pytest.mark.parametrize('name', sorted(cc.RNA_RUNS))
def test_rna_runs_match_the_reference(eng, name, dtype):
    """factors, centred levels and every fitted read's own factors; the statuses name the reads the reference
    skipped: the long read without change points after the first call, the homopolymer after the second"""
    spy = cc.assert_rna_run(name, eng, dtype)
    run = cc.RNA_RUNS[name]
    if spy is None:
        spy = cc.Spy(eng)
        np.random.seed(run['seed'])
        with pytest.raises(th.TomboError):
            ts.center_model_to_median_norm_batch(cc.rna_reads(run['reads'], dtype), cc.rna_init(), run['max_reads'], engine=spy)
    order = [run['reads'][i] for i in cc.shuffled(len(run['reads']), run['seed'])]
    prepared, fitted = spy.statuses()
    for pos, rd in enumerate(order[:fitted.shape[0]]):
        want = (FEWER_CPTS, FEWER_CPTS) if rd == 6 else (0, RESCALE_FAIL) if rd == 7 else (0, 0)
        assert (int(prepared[pos]), int(fitted[pos])) == want, rd


def test_a_read_that_fails_before_the_fit_takes_no_draw(eng):
    """the run whose shuffle puts the 1200-base read without change points in front of the drawn 1100-base read: the
    recorded factors of the drawn read, which another draw changes (the same reads under another seed)"""
    a, b = cc.RNA_RUNS['all_reads'], cc.RNA_RUNS['max_equals_successes']
    assert a['processed'].index(6) < a['processed'].index(5) and a['drew'] == [5]
    drawn = [r['read_factors'][r['succeeded'].index(5)] for r in (a, b)]
    assert drawn[0] != drawn[1]
    for run in (a, b):
        spy = cc.assert_rna_run(run['name'], eng)
        order = [run['reads'][i] for i in cc.shuffled(len(run['reads']), run['seed'])]
        got = spy.factors()[order.index(5)]
        assert np.array_equal(cc.bits(got), cc.bits(run['read_factors'][run['succeeded'].index(5)]))


@pytest.mark.parametrize('kind', ['dna', 'rna'])
@pytest.mark.parametrize('chunk', [1, 3])
def test_chunks_give_the_bits_of_one_call(eng, kind, chunk):
    """max_reads = 3 is reached inside a chunk; all reads in chunks"""
    run_of = cc.assert_dna_run if kind == 'dna' else cc.assert_rna_run
    for name in ('first_three', 'all_reads'):
        spy = run_of(name, eng, chunk_reads=chunk)
        assert all(st.shape[0] <= chunk for st in spy.prepared)
        if name == 'first_three':
            n = len((kc.CENTER_RUNS if kind == 'dna' else cc.RNA_RUNS)[name]['reads'])
            assert sum(st.shape[0] for st in spy.prepared) < n


def dna_setup(eng):
    rp = ts.load_resquiggle_parameters(th.seqSampleType(ts.DNA_SAMP_TYPE, False))
    eng.ensure_model(kc.center_init())
    return _native.make_params(rp), _native.make_opts()


def prepare(eng, reads):
    params, opts = dna_setup(eng)
    return eng.center_prepare(params, opts, [rd.raw_signal for rd in reads], [ts.encode_seq(rd.seq) for rd in reads],
                              [rd.event_starts for rd in reads], [rd.read_start_rel_to_raw for rd in reads])


def test_center_place_statuses_and_untouched_neighbours(eng):
    """every case between good reads: the status is the read's own, the neighbours' boundaries and factors are those
    of a call without the bad reads"""
    good = kc.center_reads([0, 1, 2, 3])
    g = good[0]
    st = np.asarray(g.event_starts).astype(np.int64)
    K, up = 3, 1
    end = int(g.read_start_rel_to_raw) + int(st[len(st) - 1])      # read_start + norm_len (dn = 1: the last row ends it)
    swap, rep, huge = st.copy(), st.copy(), st.copy()
    swap[[40, 41]] = swap[[41, 40]]
    rep[60] = rep[59]
    huge[70] = 2 ** 62
    cases = [
        (g._replace(event_starts=swap), ZERO_LEN),                                      # boundaries that decrease
        (g._replace(event_starts=rep), ZERO_LEN),                                       # ... that repeat
        (g._replace(raw_signal=g.raw_signal[:end - 1]), PAST_END),                      # ... that end one past the signal
        (g._replace(raw_signal=g.raw_signal[:end]), 0),                                 # (and exactly at its end)
        (g._replace(read_start_rel_to_raw=-int(st[up]) - 1), NEG_START),                # read_start -1
        (g._replace(read_start_rel_to_raw=-int(st[up])), 0),                            # (and 0)
        (g._replace(event_starts=st[:-1]), SEQ_SEG_MISMATCH),                           # one row short
        (g._replace(event_starts=st[:K], seq=g.seq[:K]), SEQ_SEG_MISMATCH),             # fewer than K + 1 bases
        (g._replace(event_starts=huge), ZERO_LEN),                                      # a value no sum may take
        (g._replace(read_start_rel_to_raw=2 ** 62), ZERO_LEN),
        (g._replace(seq=g.seq[:9] + 'N' + g.seq[10:]), INVALID_SEQ),
    ]
    reads, want = [], []
    for i, (rd, code) in enumerate(cases):
        reads += [good[i % 4], rd]
        want += [0, code]
    reads.append(good[1])
    want.append(0)
    status = prepare(eng, reads)
    print('statuses', status.tolist())
    assert status.tolist() == want
    segs, seg_off = eng.get(_native.GET_SEGS), eng.seg_off
    read_start = eng.get(_native.GET_DP_READ_START)
    for i, rd in enumerate(reads):
        if want[i] == 0:
            s = np.asarray(rd.event_starts).astype(np.int64)[up:]
            assert np.array_equal(segs[seg_off[i]:seg_off[i + 1]], s - s[0])
            assert read_start[i] == int(rd.read_start_rel_to_raw) + int(s[0])
    fit_status, factors, medians, n_used = eng.center_fit()
    assert fit_status.tolist() == want and n_used == want.count(0)
    assert np.isnan(factors[np.array(want) != 0]).all()
    clean = [rd for rd, code in zip(reads, want) if code == 0 and any(rd is x for x in good)]
    assert prepare(eng, clean).tolist() == [0] * len(clean)
    _, clean_factors, _, _ = eng.center_fit()
    at = [i for i, rd in enumerate(reads) if any(rd is x for x in good)]
    assert np.array_equal(cc.bits(factors[at]), cc.bits(clean_factors))


@pytest.mark.parametrize('n_good,max_reads,n_prior', [(1, 50, 0), (4, 50, 0), (5, 50, 0), (5, 2, 0), (5, 3, 0), (4, 6, 3),
                                                      (3, 4, 3), (0, 5, 2), (600, 10 ** 6, 0), (601, 555, 0)])
def test_center_pick_against_np_median(eng, n_good, max_reads, n_prior):
    """one success, an even and an odd number, max_reads below them, successes of earlier calls in front, more
    reads than the workgroup has threads: the medians are np.median of the counted factors"""
    good = kc.center_reads([0, 1, 2, 3, 4, 5, 6, 7])
    bad = good[0]._replace(read_start_rel_to_raw=-10 ** 6)
    reads = []
    for i in range(n_good):
        reads += [good[i % 8], bad] if i % 3 == 0 else [good[i % 8]]
    reads = reads or [bad]
    prior = np.array([[0.01 * i - 0.02, 1.0 + 0.03 * i] for i in range(n_prior)]).reshape(-1, 2)
    status = prepare(eng, reads)
    assert (status == 0).sum() == n_good
    fit_status, factors, medians, n_used = eng.center_fit(None, prior, max_reads)
    assert np.array_equal(fit_status, status)
    counted = np.concatenate([prior, factors[fit_status == 0]])[:max_reads]
    assert n_used == counted.shape[0] == min(n_good + n_prior, max_reads)
    print('counted %d, medians %r' % (n_used, medians))
    assert np.array_equal(cc.bits(medians), cc.bits([np.median(counted[:, 0]), np.median(counted[:, 1])]))


def test_center_pick_without_a_success_and_the_call_order(eng):
    bad = kc.center_reads([0])[0]._replace(read_start_rel_to_raw=-10 ** 6)
    assert prepare(eng, [bad, bad]).tolist() == [NEG_START, NEG_START]
    status, factors, medians, n_used = eng.center_fit()
    assert status.tolist() == [NEG_START, NEG_START] and medians is None and n_used == 0 and np.isnan(factors).all()
    with pytest.raises(ValueError, match='center_prepare has not been called'):
        eng.center_fit()                                   # one fit per prepared batch


def test_estimate_kmer_model_centres_on_rna_reads(eng, monkeypatch):
    """estimate_kmer_model's centring step on the recorded RNA reads gives the reference's centred levels"""
    run = cc.RNA_RUNS['all_reads']
    model = cc.rna_init()
    monkeypatch.setattr(ts, 'TomboModel', lambda **kw: model)     # (for the tabulated model: the recorded initial one)
    c = kc.CASES['canon_clean']
    np.random.seed(run['seed'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = ts.estimate_kmer_model(kc.reads_index('clean'), c['cov_thresh'], c['upstrm'], c['dnstrm'], c['min_kmer_obs'],
                                     True, None, False, kc.REGION_SIZE, center_reads=cc.rna_reads(run['reads']), engine=eng)
    assert got is model and np.array_equal(cc.bits(got.level_means), cc.bits(cc.GOLD['run_all_reads_means']))

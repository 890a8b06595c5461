"""Row N4 on the GPU: the per-read statistics driver (tombo_amd.tombo_stats.compute_*_read_stats)
against vectors recorded from the live reference (tests/golden/gen_golden_stats.py), and the
resident-batch de novo statistic against the array form.

Tolerance: the p-values go through erfc / log / exp / lgamma of the device library against
scipy's (cephes) norm.cdf / chi2.sf -- 1e-12 relative (observed ~1e-15; window log sums in
numpy's order; wide windows and saturated p-values: test_gpu_stats_edges.py); log-likelihood
ratios: the constant-variance form is bit-equal, the scaled form (exp, pow) 1e-12.  Positions are
integers: exact.  Error messages are the reference's strings."""
import numpy as np
import pytest

from stats_cases import load_read_cases as _load, check_z_read_cases, check_alt_read_cases

pytestmark = pytest.mark.gpu


def test_de_novo_and_sample_compare_match_the_reference():
    from tombo_amd import tombo_stats as ts
    assert check_z_read_cases(ts.compute_de_novo_read_stats, ts.compute_sample_compare_read_stats) >= 60


def test_alt_model_llhrs_match_the_reference():
    from tombo_amd import tombo_stats as ts
    assert check_alt_read_cases(ts.compute_alt_model_read_stats) > 50


def test_batch_forms_equal_single_read_calls():
    from tombo_amd import tombo_stats as ts
    g, meta, model, alts, reads = _load()
    one = [ts.compute_de_novo_read_stats_batch([rd], model, 1)[0] for rd in reads]
    many = ts.compute_de_novo_read_stats_batch(reads, model, 1)
    for a, b in zip(one, many):
        assert isinstance(a, Exception) == isinstance(b, Exception)
        if not isinstance(a, Exception):
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
    am1 = [ts.compute_alt_model_read_stats_batch([rd], model, alts)[0] for rd in reads]
    amn = ts.compute_alt_model_read_stats_batch(reads, model, alts)
    for a, b in zip(am1, amn):
        assert isinstance(a, Exception) == isinstance(b, Exception)
        if not isinstance(a, Exception):
            for name, _ in alts:
                np.testing.assert_array_equal(a[0][name], b[0][name])


def test_resident_batch_de_novo_equals_the_array_form():
    """tba_batch_de_novo_stats on the finished resident batch (nothing uploaded) == the array form
    fed with the Events table of the same reads"""
    from tombo_amd import resquiggle as rq, synth, tombo_stats as ts, tombo_helper as th
    samp = th.seqSampleType('DNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)
    mrs = [synth.synth_map_res(model, nb, 4000 + nb, **synth.DNA_SYNTH) for nb in (400, 650, 20, 900)]
    res, tabs = rq.resquiggle_batch_events(mrs, model, params, outlier_thresh=5.0, seq_samp_type=samp)
    for fm in (0, 1, 3):
        got = rq.batch_de_novo_stats(fm_offset=fm)
        for i, r in enumerate(res):
            if isinstance(r, Exception):
                assert got[i] is None
                continue
            rd = th.read_from_results(r, tabs[i]['norm_mean'])
            try:
                want = ts.compute_de_novo_read_stats_batch([rd], model, fm)[0]
            except th.TomboError:
                want = None
            if isinstance(want, Exception) or want is None:
                assert got[i] is None or np.all(np.isnan(got[i][0]))
                continue
            np.testing.assert_array_equal(got[i][0], want[0])
            np.testing.assert_array_equal(got[i][1], want[1])

"""The batch forms of the forward pass (csrc/k_dp.h: k_dp_c1, k_dp_cdiv, k_dp<CPL>) after the row's no-op arithmetic
left it, on small batches against the oracle, read by read and stage by stage (test_gpu_parity.compare_batch): 300-base
reads (the static whole-read path) and two longer ones (start discovery and adaptive rows) at W = 500 (8 cells per lane)
and W = 300 (5), at W = 500 also a read of CONSTANT signal (its status is the oracle's).  Each batch runs on each of the
three forms, forced the way test_gpu_dp_one_sd.py forces them, and the engine's report says which one ran.  Every
comparison is exact; the traceback verifier's failure count (TBA_GET_TB_VERIFY_FAIL) is zero.

No read here has a NaN sample.  A batch with one does not reach the forward pass the way the oracle's does -- the
medians of the engine's normalisation leave a NaN out where numpy's make the whole signal NaN, so the read differs from
its oracle from the first stage on -- and the stages behind event detection have never been held to anything with a
NaN in the signal.  That is work on those stages, not on the row arithmetic tested here."""
import copy

import numpy as np
import pytest

from test_div_const_proof import DNA_SD, RNA_SD
from test_gpu_parity import run_batch, compare_batch, _engine
from test_gpu_dp_forms import _model

pytestmark = pytest.mark.gpu

BANDS = {'dna_w500': 500, 'dna_w300': 300}
FORMS = ('one_sd', 'cdiv', 'general')
CONST_READ = 4
_cache = {}


def batch(name):
    """(model, params, reads) of a batch; made once.  reads: (raw, seq, None, None)"""
    if name not in _cache:
        from tombo_amd import synth, tombo_stats as ts
        samp, mdl = _model('DNA')
        params = ts.load_resquiggle_parameters(samp)._replace(bandwidth=BANDS[name])
        reads = []
        for nb, seed in ((300, 501), (300, 502), (300, 503), (650, 504), (300, 505), (300, 506), (700, 507)):
            seq, raw, _ = synth.synth_read(mdl, nb, seed + BANDS[name], **synth.DNA_SYNTH)
            reads.append([np.asarray(raw, np.float64).copy(), seq, None, None])
        if name == 'dna_w500':
            reads[CONST_READ][0][:] = reads[CONST_READ][0][0]
        _cache[name] = (mdl, params, [tuple(r) for r in reads])
    return _cache[name]


def _two_sd_model(mdl, reads):
    """the model with the sd of one k-mer no read contains replaced by a second proven divisor (test_gpu_dp_one_sd.py)"""
    from tombo_amd import tombo_stats as ts
    K = mdl.kmer_width
    seen = set()
    for r in reads:
        codes = ts.encode_seq(r[1])
        for p in range(len(codes) - K + 1):
            seen.add(int(sum(int(c) << (2 * (K - 1 - j)) for j, c in enumerate(codes[p:p + K]))))
    kmer = next(k for k in range(4 ** K) if k not in seen)
    m2 = copy.copy(mdl)
    m2.level_sds = np.array(mdl.level_sds, dtype=np.float64, copy=True)
    assert m2.level_sds[kmer] == DNA_SD
    m2.level_sds[kmer] = RNA_SD
    return m2


def run_form(name, form):
    from tombo_amd import _native as N
    mdl, params, reads = batch(name)
    eng = _engine()
    try:
        if form == 'general':
            eng.set_dp_const_division(False)
        eng_, out, oracles = run_batch(_two_sd_model(mdl, reads) if form == 'cdiv' else mdl, params, 'DNA', reads)
        ran = eng.last_dp_const_division()
        one = eng.get(N.GET_DP_ONE_SD)
        k_dp = eng.get(N.GET_DP_FORM)[:, 0] == N.DP_FORM_K_DP
        verify_fail = eng.get(N.GET_TB_VERIFY_FAIL)
    finally:
        eng.set_dp_const_division(True)
    assert eng_ is eng
    bad = compare_batch(eng, oracles, out, '%s/%s' % (name, form))
    assert not bad, '\n'.join(bad[:40])
    status = [o['status'] for o in oracles]
    assert status == [int(s) for s in out['status']]
    assert all(s == 0 for i, s in enumerate(status) if i != CONST_READ or name != 'dna_w500'), status
    assert not verify_fail.any(), verify_fail.tolist()
    assert ran == ((False, False) if form == 'general' else (True, True))
    if form == 'one_sd':
        assert np.array_equal(one[:, 0] == 1, k_dp) and k_dp.sum() >= 5, (one.tolist(), k_dp.tolist())
    else:
        assert not one.any()
    return status


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', sorted(BANDS))
def test_small_batches_on_every_form(name, form):
    run_form(name, form)

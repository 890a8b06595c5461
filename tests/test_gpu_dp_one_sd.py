"""k_dp_c1, the forward pass of a level model with ONE proven sd (csrc/k_dp.h: the reciprocal pair comes from
the host as two kernel arguments, a row reads its level mean alone, a static row leaves the arg-max nobody reads alone): against the
oracle, against the other three forms of the same pass bit for bit, and with the engine's report of which form ran
(TBA_GET_DP_ONE_SD beside tba_engine_last_dp_const_division).  Every comparison is exact.

The reads come from the generators of the existing parity tests (synth.synth_read under test_gpu_parity._si, leaders
as test_gpu_dp_forms.retry_reads makes them), the batches run on the default engine as theirs do.

A batch read's static rows are its masked start: mask_seq_len = max(MASK_BASES, ..) >= 50 rows (k_prep, k_dp.h), or
the whole read on the static path.  The static / adaptive boundary of a read that k_dp_c1 takes therefore never
falls on row 0 -- only the per-kernel C entries can place it there, and those run k_dp<CPL, true>, not this kernel.
The boundaries tested are the smallest one (row 50) and the two level-block boundaries (rows 64 and 128)."""
import copy

import numpy as np
import pytest

import div_const_model as model_math
from test_div_const_proof import DNA_SD, RNA_SD
from test_gpu_parity import run_batch, compare_batch, _engine, _si
from test_gpu_dp_forms import check_dp_forms, cpl_class, _model
from test_zz_gpu_dp_const_division import _forward_products, _bits

pytestmark = pytest.mark.gpu

DNA_START = (750, 2500, 250)        # start_bw, start_save_bw, start_n_bases of the DNA defaults
EDGE_START = (200, 600, 100)        # ... of the row-count edge reads: short reads that still go through start discovery

# name -> (sample type, bandwidth, start parameters or None for the defaults, [(bases, seed, synth arguments)])
# A leader is `lead` samples of noise (DNA) in front of the read: 11 250 samples = 2 250 events put the sequence start
# past the first start band (750 events) and inside the save band (2 500): the first try fails, the retry finds it.
# 300 bases without a leader are fewer events than start discovery needs: the static whole-read path.
BATCHES = {
    'dna_w500': ('DNA', 500, None, [(700, 101, {}), (300, 102, {}), (650, 103, dict(lead=11250)), (600, 104, {}),
                                    (700, 105, dict(lead=1500)), (620, 106, {})]),
    'dna_w300': ('DNA', 300, None, [(700, 111, {}), (300, 112, {}), (650, 113, dict(lead=11250)), (600, 114, {}),
                                    (700, 115, dict(lead=1500)), (620, 116, {})]),
    'dna_w100': ('DNA', 100, None, [(700, 121, {}), (300, 122, {}), (650, 140, dict(lead=11250)), (600, 124, {}),
                                    (700, 125, dict(lead=1500)), (620, 126, {})]),
    # (RNA leaders: a fraction of the save band in events, test_gpu_dp_forms.retry_reads.  400 RNA bases alone are about
    # as many events as start discovery needs, so two reads get a short leader; half a save band fails the first try
    # and leaves too few events for the retry: a static band of 2 489 cells, the 48-cell class)
    'rna_b400': ('RNA', 500, None, [(400, 131, dict(up=0.1)), (400, 132, {}), (400, 133, dict(up=0.9)),
                                    (400, 134, dict(up=0.15)), (200, 135, {}), (400, 136, dict(up=0.5))]),
    # rows past the static rows: 63, 64, 65, 129 (mask_seq_len 50 at bandwidth 150; found with the oracle)
    'edges': ('DNA', 150, EDGE_START, [(113, 8300, dict(lead=450)), (114, 8301, dict(lead=450)),
                                       (115, 8300, dict(lead=450)), (179, 8279, dict(lead=600))]),
    # the static / adaptive boundary on rows 50, 64 and 128 (found with the oracle)
    'bound50': ('DNA', 140, None, [(650, 9401, {})]),
    'bound64': ('DNA', 230, None, [(650, 9403, {})]),
    'bound128': ('DNA', 470, None, [(650, 9403, {})]),
}
ROWS_PAST_STATIC = (63, 64, 65, 129)
BOUNDARY = {'bound50': 50, 'bound64': 64, 'bound128': 128}

_cache = {}


def batch(name):
    """(sample name, model, params, reads) of a batch; made once.  reads: (raw, seq, stall_ints, samp_ind)"""
    if name not in _cache:
        import oracle
        from tombo_amd import synth, tombo_stats as ts
        samp_name, bw, start, specs = BATCHES[name]
        samp, mdl = _model(samp_name)
        params = ts.load_resquiggle_parameters(samp)
        if start is not None:
            params = ts.load_resquiggle_parameters(samp, (4.2, 4.2, bw, 1500, 20.0, 40) + start)
        params = params._replace(bandwidth=bw)
        if bw == 100:   # (test_gpu_parity.test_many_seeds_w100_on_gpu: the band-boundary check scaled with the band)
            params = params._replace(band_bound_thresh=10)
        reads = []
        for nb, seed, kw in specs:
            if samp_name == 'RNA':
                # (test_gpu_dp_forms.retry_reads: an RNA leader is the signal of an unrelated sequence upstream)
                kw = dict(kw)
                up = kw.pop('up', None)
                seq, raw, _ = synth.synth_read(mdl, nb, seed, **dict(synth.RNA_SYNTH, **kw))
                if up is not None:
                    lead = int(up * params.start_save_bw * params.mean_obs_per_event)
                    _, sig, _ = synth.synth_read(mdl, lead // 40 + 50, seed + 7, **dict(synth.RNA_SYNTH, lead=0, n_trail=0))
                    assert sig.shape[0] >= lead
                    seq, raw, _ = synth.synth_read(mdl, nb, seed, **dict(synth.RNA_SYNTH, lead=0))
                    raw = np.concatenate([sig[:lead], raw])
                reads.append((raw, seq, oracle.identify_stalls(raw), _si(nb, seed % 7)))
            else:
                seq, raw, _ = synth.synth_read(mdl, nb, seed, **dict(synth.DNA_SYNTH, **kw))
                reads.append((raw, seq, None, _si(nb, seed % 7)))
        _cache[name] = (samp_name, mdl, params, reads)
    return _cache[name]


def check_one_sd_report(eng, want_main, want_start):
    """TBA_GET_DP_ONE_SD of the last run, read by read, against TBA_GET_DP_FORM: k_dp_c1 took the main pass of
    exactly the reads k_dp<CPL> is reported for (never k_dp_multi's, k_dp_wide's), the first try of every read that
    had one, and no retry that went to k_dp_wg"""
    from tombo_amd import _native as N
    one, form = eng.get(N.GET_DP_ONE_SD), eng.get(N.GET_DP_FORM)
    assert one.shape == (eng.n, 2) and one.dtype == np.int32
    k_dp = form[:, 0] == N.DP_FORM_K_DP
    tried = form[:, 2] != N.DP_START_NONE
    retried_k_dp = form[:, 2] == N.DP_START_RETRY_K_DP
    assert np.array_equal(one[:, 0], (k_dp & want_main).astype(np.int32)), (one.tolist(), form.tolist())
    assert np.array_equal(one[:, 1] & 1, (tried & want_start).astype(np.int32)), (one.tolist(), form.tolist())
    assert np.array_equal(one[:, 1] >> 1, (retried_k_dp & want_start).astype(np.int32)), (one.tolist(), form.tolist())
    return one, form


def run_standard(name):
    """the batch under its own model, once: the oracle's results in every stage, the two-operation division reported
    as before and k_dp_c1 by the new selector -> (forward products, oracles, engine reports)"""
    key = ('std', name)
    if key not in _cache:
        from tombo_amd import _native as N
        samp_name, mdl, params, reads = batch(name)
        eng, out, oracles = run_batch(mdl, params, samp_name, reads)
        assert eng.model_const_division()
        assert eng.last_dp_const_division() == (True, True)
        bad = compare_batch(eng, oracles, out, name)
        assert not bad, '\n'.join(bad[:40])
        check_dp_forms(eng, params, False, oracles)
        one, form = check_one_sd_report(eng, True, True)
        _cache[key] = (_forward_products(eng), oracles, dict(one=one, form=form, path=eng.get(N.GET_PATH),
                                                             bst=eng.get(N.GET_BAND_STARTS), start=eng.get(N.GET_START),
                                                             ref_off=np.array(eng.ref_off),
                                                             seg_off=np.array(eng.seg_off)))
    return _cache[key]


# ---- parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['dna_w500', 'dna_w300', 'dna_w100', 'rna_b400'])
def test_one_sd_batches_equal_the_oracle(name):
    """six reads per batch: statuses, boundaries, scale values, scores and every stage before them equal the oracle's;
    the batch holds a read whose first start discovery fails and is retried, a read on the static whole-read path
    and reads with a masked start (every adaptive read), and k_dp_c1 is reported for the reads it took"""
    from tombo_amd import _native as N
    snap, oracles, rep = run_standard(name)
    assert len(oracles) == 6
    d = [o['dbg'] for o in oracles]
    assert any(x['n_start_calls'] == 2 for x in d), [x['n_start_calls'] for x in d]
    assert any(x['used_static'] for x in d)
    masked = [i for i, x in enumerate(d) if oracles[i]['status'] == 0 and not x['used_static']]
    assert len(masked) >= 3 and all(d[i]['mask_seq_len'] >= 50 for i in masked)
    assert all(o['status'] == 0 for o in oracles), [o['status'] for o in oracles]
    for i, o in enumerate(oracles):     # (compare_batch holds these too: spelled out, they are what the issue names)
        s0, s1 = int(rep['seg_off'][i]), int(rep['seg_off'][i + 1])
        assert np.array_equal(snap['segs'][s0:s1], o['segs'])
        assert np.array_equal(_bits(snap['sv'][i][:2]), _bits(np.asarray(o['scale_values'][:2], np.float64)))
        assert _bits(np.float64(snap['score'][i])) == _bits(np.float64(o['sig_match_score']))
    bw = BATCHES[name][1]
    adaptive = rep['path'][:, 0] == 1
    if bw <= 128:       # narrow adaptive bands are k_dp_multi's: k_dp_c1 has the static read and start discovery
        assert np.all(rep['one'][adaptive, 0] == 0) and rep['one'][~adaptive, 0].sum() >= 1
    else:
        assert np.all(rep['one'][adaptive, 0] == 1) and np.all(rep['form'][adaptive, 1] == cpl_class(bw))
    assert np.all(rep['one'][:, 1] & 1 == (rep['form'][:, 2] != N.DP_START_NONE))


# ---- the same batch four ways -------------------------------------------------------------------------
FOUR_WAYS = 'dna_w500'


def _upload(name, mdl=None):
    """the batch uploaded to the default engine the way run_batch uploads it, not yet run"""
    from tombo_amd import tombo_stats as ts, _native as N
    from tombo_amd._default_parameters import SIG_MATCH_THRESH
    samp_name, std_model, params, reads = batch(name)
    mdl = mdl or std_model
    eng = _engine()
    eng.set_model(mdl.level_means, mdl.level_sds, mdl.kmer_width, mdl.central_pos)
    si = np.zeros((len(reads), 1000), np.int64)
    for i, r in enumerate(reads):
        if r[3] is not None:
            si[i] = r[3]
    eng.upload(N.make_params(params), N.make_opts(outlier_thresh=5.0, sig_match_thresh=SIG_MATCH_THRESH[samp_name]),
               [np.asarray(r[0], np.float64) for r in reads], [ts.encode_seq(r[1]) for r in reads], samp_ind=si)
    return eng


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), '%s differs between k_dp_c1 and %s' % (k, what)


def _two_sd_model():
    """the standard model with the sd of ONE k-mer that no read of the batch contains replaced by a second proven
    divisor: a proven table with two sds, and the same levels for every base of the batch"""
    from tombo_amd import tombo_stats as ts, _native
    _, mdl, _, reads = batch(FOUR_WAYS)
    K = mdl.kmer_width
    seen = set()
    for r in reads:
        codes = ts.encode_seq(r[1])
        for p in range(len(codes) - K + 1):
            seen.add(int(sum(int(c) << (2 * (K - 1 - j)) for j, c in enumerate(codes[p:p + K]))))
    kmer = next(k for k in range(4 ** K) if k not in seen)
    sd2 = RNA_SD
    assert sd2 != DNA_SD and model_math.proven(sd2) and _native.prove_const_division(np.array([sd2]))[0]
    m2 = copy.copy(mdl)
    m2.level_sds = np.array(mdl.level_sds, dtype=np.float64, copy=True)
    m2.level_sds[kmer] = sd2
    return m2


def test_two_sd_model_runs_the_lane_form_and_gives_the_same_bits():
    """a proven table with two sds: k_dp_cdiv (the reciprocal pair per row, from the lanes), not k_dp_c1"""
    std, oracles, _ = run_standard(FOUR_WAYS)
    eng = _upload(FOUR_WAYS, _two_sd_model())
    eng.run()
    assert eng.model_const_division()
    assert eng.last_dp_const_division() == (True, True)
    check_one_sd_report(eng, False, False)
    _assert_same(_forward_products(eng), std, 'k_dp_cdiv')


def test_sds_from_the_caller_run_the_general_form_and_give_the_same_bits():
    """TBA_PUT_REF_SDS with the model's own values between the stages: the general division, from the array"""
    from tombo_amd import _native as N
    std, oracles, _ = run_standard(FOUR_WAYS)
    eng = _upload(FOUR_WAYS)
    eng.run_stages(N.STAGE_SEGMENT, N.STAGE_REF_LEVELS)
    sds = eng.get(N.GET_REF_SDS)
    assert np.all(sds == DNA_SD)
    eng.put(N.PUT_REF_SDS, sds)
    eng.run_stages(N.STAGE_START, N.STAGE_RESCALE)
    assert eng.last_dp_const_division() == (False, False)
    check_one_sd_report(eng, False, False)
    _assert_same(_forward_products(eng), std, 'k_dp after TBA_PUT_REF_SDS')
    eng.run()                                   # the next run from the top is back on the one-sd form
    assert eng.last_dp_const_division() == (True, True)
    check_one_sd_report(eng, True, True)


def test_switch_off_runs_the_general_form_and_gives_the_same_bits():
    """tba_engine_set_dp_const_division(0): k_dp<CPL>"""
    std, oracles, _ = run_standard(FOUR_WAYS)
    eng = _upload(FOUR_WAYS)
    try:
        eng.set_dp_const_division(False)
        eng.run()
        assert eng.model_const_division()
        assert eng.last_dp_const_division() == (False, False)
        check_one_sd_report(eng, False, False)
        off = _forward_products(eng)
    finally:
        eng.set_dp_const_division(True)
    _assert_same(off, std, 'k_dp')
    eng.run()
    check_one_sd_report(eng, True, True)
    _assert_same(_forward_products(eng), std, 'its own second run')


# ---- row-count edges, static-row arg-max --------------------------------------------------------------
def test_row_counts_around_the_level_block():
    """reads of 63, 64, 65 and 129 rows past their static rows (and 113 .. 179 rows in all): the level registers are
    reloaded every 64 rows, the last block is partial, exactly full, one row into the next"""
    _, oracles, rep = run_standard('edges')
    assert all(o['status'] == 0 and not o['dbg']['used_static'] for o in oracles)
    past = tuple(len(o['dbg']['band_event_starts']) - o['dbg']['mask_seq_len'] for o in oracles)
    assert past == ROWS_PAST_STATIC, past
    assert np.all(rep['one'][:, 0] == 1) and np.all(rep['one'][:, 1] == 1)
    assert np.all(rep['form'][:, 1] == cpl_class(150))


@pytest.mark.parametrize('name', sorted(BOUNDARY))
def test_static_row_argmax_is_taken_where_it_is_read(name):
    """start discovery's result (its traceback starts at top_pos, the arg-max of the LAST of 250 static rows) and the
    band start of the first adaptive row of the main pass (placed by the arg-max of the last static row) equal the
    oracle's, with the boundary on row 50 -- the smallest a batch read has -- and on the block boundaries 64 and 128"""
    _, oracles, rep = run_standard(name)
    o = oracles[0]
    d = o['dbg']
    msl = int(d['mask_seq_len'])
    assert o['status'] == 0 and not d['used_static'] and msl == BOUNDARY[name], (o['status'], msl)
    assert d['n_start_calls'] == 1
    assert np.array_equal(_bits(rep['start'][0, :2]), _bits(np.asarray(d['start_calls'][:2], np.float64)))
    r0 = int(rep['ref_off'][0])
    assert rep['bst'][r0 + msl] == d['band_event_starts'][msl]
    assert np.array_equal(rep['bst'][r0:int(rep['ref_off'][1])], d['band_event_starts'])
    assert rep['one'][0, 0] == 1 and rep['one'][0, 1] == 1


def test_start_discovery_top_pos_in_a_full_batch():
    """... and for every read of the W = 500 batch that went through start discovery, first try and retry"""
    _, oracles, rep = run_standard(FOUR_WAYS)
    n = 0
    for i, o in enumerate(oracles):
        k = o['dbg']['n_start_calls']
        if k >= 1:
            n += 1
            assert np.array_equal(_bits(rep['start'][i, 2 * (k - 1):2 * k]),
                                  _bits(np.asarray(o['dbg']['start_calls'][2 * (k - 1):2 * k], np.float64))), i
    assert n >= 4

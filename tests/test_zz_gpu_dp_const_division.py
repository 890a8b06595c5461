"""k_dp_cdiv, the forward pass that divides by a PROVEN level sd in two float64 operations (csrc/k_dp.h,
div_const_proof.h): the division itself on the device against numpy's, dividend by dividend, and the forward passes
that take it against the oracle -- and against the general division, bit for bit -- with the engine's report of which
form ran.  Every comparison is exact.

(The file sorts behind every other test file on purpose: these tests allocate and free device memory of their own,
and tests/test_gpu_synth.py compares the unwritten tails of the output buffers of two fresh engines, which are
equal only as long as the allocations before it are the ones it has always seen.)"""
import copy

import numpy as np
import pytest

import div_const_model as model
from test_div_const_proof import DNA_SD, RNA_SD, BAD_SD, BAD_DIVIDEND
from test_gpu_parity import run_batch, compare_batch, _engine, _si

pytestmark = pytest.mark.gpu

Z_SHIFT, Z_CAP = 4.2, 5.0     # a z_shift / max_half_z_score pair of the order the resquiggle parameters have


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits_or_both_nan(a, b):
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


_cache = {}


def proven_divisors():
    """the two standard sds and three dozen random ones the prover accepts"""
    if 'sds' not in _cache:
        from tombo_amd import _native
        rng = np.random.RandomState(7)
        sds = rng.uniform(0.05, 1.0, 60)
        sds = sds[_native.prove_const_division(sds)][:36]
        assert sds.shape[0] == 36
        _cache['sds'] = np.concatenate([[DNA_SD, RNA_SD], sds])
    return _cache['sds']


def random_dividends():
    """10^6 values of both signs, significands uniform, exponents over 2^-60 .. 2^60"""
    if 'a' not in _cache:
        rng = np.random.RandomState(11)
        n = 1000000
        a = np.ldexp(rng.uniform(1.0, 2.0, n), rng.randint(-60, 61, n)) * rng.choice([-1.0, 1.0], n)
        _cache['a'] = a
    return _cache['a']


def test_two_operation_division_is_ieee_for_proven_divisors():
    """for each proven sd: the dividends nearest a rounding boundary (|rho| <= 64, at three exponents and both signs)
    and 10^6 random ones -- the device's quotient equals numpy's a / sd bit for bit"""
    eng = _engine()
    rnd = random_dividends()
    n_near = 0
    for sd in proven_divisors():
        near = np.array(model.candidates(float(sd), 64), dtype=np.float64)
        n_near += near.shape[0]
        near = np.concatenate([np.ldexp(near, e) for e in (-52, -45, -70)] + [-np.ldexp(near, -52)])
        a = np.concatenate([near, rnd])
        q = eng.selftest_const_division(a, np.full(a.shape[0], sd), Z_SHIFT, Z_CAP)[0]
        want = a / sd
        bad = np.flatnonzero(_bits(q) != _bits(want))
        assert bad.size == 0, (float(sd).hex(), [(float(a[i]).hex(), float(q[i]).hex(), float(want[i]).hex()) for i in bad[:5]])
    # (64 * 2^52 / S of them are expected per divisor, S its 53-bit significand: between 32 and 64)
    assert n_near >= 16 * len(proven_divisors())


def test_edge_dividends_give_the_cell_value_of_the_general_division():
    """0, tiny, NaN, infinite dividends and those whose quotient overflows or whose low product underflows: the
    cell's z_shift - min(|q|, cap) is the one the five-operation form gives (a finite cap: the DNA and RNA defaults
    winsorise)"""
    eng = _engine()
    tiny = [5e-324, 1e-320, 1e-310, 2.0 ** -1022, 2.0 ** -1000, 2.0 ** -970, 1e-290]
    huge = [1e300, 1e307, 8e307, 1.7e308, np.finfo(np.float64).max]
    a = np.array([0.0, -0.0, np.nan, np.inf, -np.inf] + tiny + [-x for x in tiny] + huge + [-x for x in huge] +
                 [1.0, -2.5, 123.456])
    for sd in proven_divisors()[:8]:
        q, z2, z5 = eng.selftest_const_division(a, np.full(a.shape[0], sd), Z_SHIFT, Z_CAP)
        ok = _same_bits_or_both_nan(z2, z5)
        assert ok.all(), (float(sd).hex(), a[~ok], z2[~ok], z5[~ok])
        assert not np.isnan(z2).any()                              # fmin drops a NaN quotient: the cell is capped
        fin = np.isfinite(a) & (np.abs(a) <= 1e290) & (np.abs(a) >= 1e-290)
        assert np.array_equal(_bits(q[fin]), _bits(a[fin] / sd))


def test_the_self_test_tells_a_wrong_quotient_from_a_right_one():
    """the unproven divisor with its dividend: the device's two-operation quotient is one ulp below a / sd (and a
    dividend next to it is divided correctly)"""
    eng = _engine()
    a = np.array([BAD_DIVIDEND, np.nextafter(BAD_DIVIDEND, np.inf), -BAD_DIVIDEND, np.ldexp(BAD_DIVIDEND, -50)])
    q = eng.selftest_const_division(a, np.full(4, BAD_SD), Z_SHIFT, Z_CAP)[0]
    want = a / BAD_SD
    assert q[0] == float.fromhex('0x1.d68e47d408cccp+52') and want[0] == float.fromhex('0x1.d68e47d408ccdp+52')
    assert q[0] == np.nextafter(want[0], 0.0) and q[2] == -q[0] and q[3] == np.nextafter(want[3], 0.0)
    assert q[1] == want[1]


# ---- the forward passes ------------------------------------------------------------------------------------
CASES = ('dna_b600_w300', 'dna_b2000_w500', 'rna_one_read')


def _case(name):
    """(samp name, model, params, reads) of a case; made once"""
    if name not in _cache:
        import oracle
        from tombo_amd import synth, tombo_stats as ts, tombo_helper as th
        samp_name = 'RNA' if name.startswith('rna') else 'DNA'
        samp = th.seqSampleType(samp_name, False)
        mdl = ts.TomboModel(seq_samp_type=samp)
        params = ts.load_resquiggle_parameters(samp)
        reads = []
        if samp_name == 'RNA':
            seq, raw, _ = synth.synth_read(mdl, 900, 71001, **synth.RNA_SYNTH)
            reads.append((raw, seq, oracle.identify_stalls(raw), _si(900, 0)))
        else:
            nb, bw = (600, 300) if name == 'dna_b600_w300' else (2000, 500)
            params = params._replace(bandwidth=bw)
            for k in range(8):
                seq, raw, _ = synth.synth_read(mdl, nb, 72000 + 10 * bw + k, **synth.DNA_SYNTH)
                reads.append((raw, seq, None, _si(nb, k)))
        _cache[name] = (samp_name, mdl, params, reads)
    return _cache[name]


def _forward_products(eng):
    from tombo_amd import _native as N
    gets = (N.GET_START, N.GET_BAND_STARTS, N.GET_LAST_ROW, N.GET_READ_TB, N.GET_DP_SEGS, N.GET_SEGS, N.GET_STATUS,
            N.GET_PATH, N.GET_THEIL_SEN)
    snap = dict(('get%d' % g, eng.get(g)) for g in gets)
    # (a last row is the read's W band cells; what lies behind them in the engine's buffer is older batches')
    last, width = snap['get%d' % N.GET_LAST_ROW], snap['get%d' % N.GET_PATH][:, 2]
    last[np.arange(last.shape[1])[None, :] >= width[:, None]] = 0.0
    out = eng.download()
    # (... and the normalised signal of a read ends at its norm_len)
    norm = out['norm']
    for i in range(eng.n):
        norm[int(eng.raw_off[i]) + int(out['norm_len'][i]):int(eng.raw_off[i + 1])] = 0.0
    snap.update(out)
    return snap


def _run_standard(name):
    """(a): the case under its own model, once -> (engine state snapshot, oracles)"""
    key = ('std', name)
    if key not in _cache:
        samp_name, mdl, params, reads = _case(name)
        eng, out, oracles = run_batch(mdl, params, samp_name, reads)
        assert eng.model_const_division()
        assert eng.last_dp_const_division() == (True, True)
        bad = compare_batch(eng, oracles, out, name)
        assert not bad, '\n'.join(bad[:40])
        assert all(o['status'] == 0 for o in oracles)
        _cache[key] = (_forward_products(eng), oracles)
    return _cache[key]


def _upload_case(name):
    """the case uploaded to the default engine the way run_batch uploads it, not yet run"""
    from tombo_amd import tombo_stats as ts, _native as N
    from tombo_amd._default_parameters import SIG_MATCH_THRESH
    samp_name, mdl, params, reads = _case(name)
    eng = _engine()
    eng.set_model(mdl.level_means, mdl.level_sds, mdl.kmer_width, mdl.central_pos)
    si = np.zeros((len(reads), 1000), np.int64)
    for i, r in enumerate(reads):
        if r[3] is not None:
            si[i] = r[3]
    stalls = [r[2] for r in reads]
    eng.upload(N.make_params(params), N.make_opts(outlier_thresh=5.0, sig_match_thresh=SIG_MATCH_THRESH[samp_name]),
               [np.asarray(r[0], np.float64) for r in reads], [ts.encode_seq(r[1]) for r in reads], samp_ind=si,
               stall_ints=stalls if any(s is not None for s in stalls) else None)
    return eng


@pytest.mark.parametrize('name', CASES)
def test_standard_model_takes_the_short_division_and_equals_the_oracle(name):
    """(a) band starts, start results, last rows, tracebacks and every output equal the oracle's; the engine reports
    k_dp_cdiv for the main pass and for start discovery"""
    _run_standard(name)


@pytest.mark.parametrize('name', CASES)
def test_model_with_an_unproven_sd_keeps_the_general_division(name):
    """(b) one k-mer's sd replaced by the unproven divisor (a k-mer the first read contains): the general form runs,
    and the results equal the oracle's under that model"""
    from tombo_amd import tombo_stats as ts
    samp_name, mdl, params, reads = _case(name)
    m2 = copy.copy(mdl)
    m2.level_sds = np.array(mdl.level_sds, dtype=np.float64, copy=True)
    codes = ts.encode_seq(reads[0][1])[40:40 + mdl.kmer_width]
    kmer = int(sum(int(c) << (2 * (mdl.kmer_width - 1 - j)) for j, c in enumerate(codes)))
    m2.level_sds[kmer] = BAD_SD
    eng, out, oracles = run_batch(m2, params, samp_name, reads)
    assert not eng.model_const_division()
    assert eng.last_dp_const_division() == (False, False)
    from tombo_amd import _native as N
    assert (eng.get(N.GET_REF_SDS) == BAD_SD).sum() >= 1         # the rows do meet it
    bad = compare_batch(eng, oracles, out, name + '-unproven')
    assert not bad, '\n'.join(bad[:40])
    assert all(o['status'] == 0 for o in oracles)


@pytest.mark.parametrize('name', CASES)
def test_sds_from_the_caller_keep_the_general_division(name):
    """(c) TBA_PUT_REF_SDS with the model's own values between the stages: the general form runs (the engine cannot
    know what it was given), the results are the oracle's; the next run from the top is back on the short form"""
    from tombo_amd import _native as N
    samp_name = _case(name)[0]
    std, oracles = _run_standard(name)
    eng = _upload_case(name)
    eng.run_stages(N.STAGE_SEGMENT, N.STAGE_REF_LEVELS)
    sds = eng.get(N.GET_REF_SDS)
    assert np.all(sds == (RNA_SD if samp_name == 'RNA' else DNA_SD))
    eng.put(N.PUT_REF_SDS, sds)
    eng.run_stages(N.STAGE_START, N.STAGE_RESCALE)
    assert eng.last_dp_const_division() == (False, False)
    out = eng.download()
    bad = compare_batch(eng, oracles, out, name + '-put')
    assert not bad, '\n'.join(bad[:40])
    eng.run()
    assert eng.last_dp_const_division() == (True, True)


@pytest.mark.parametrize('name', CASES)
def test_switch_off_gives_the_same_bits(name):
    """(d) tba_engine_set_dp_const_division(0): k_dp<CPL> runs, and every forward-pass product and every output
    equals the short form's bit for bit"""
    _run_standard(name)                         # (the short form's results are the oracle's)
    eng = _upload_case(name)
    eng.run()                                   # the same resident batch, first on the short form ...
    assert eng.last_dp_const_division() == (True, True)
    std = _forward_products(eng)
    try:
        eng.set_dp_const_division(False)        # ... then on the general one
        eng.run()
        assert eng.model_const_division()
        assert eng.last_dp_const_division() == (False, False)
        off = _forward_products(eng)
    finally:
        eng.set_dp_const_division(True)
    assert sorted(off) == sorted(std)
    for k in sorted(std):
        assert np.array_equal(_bits(off[k]), _bits(std[k])), '%s differs between k_dp_cdiv and k_dp' % k
    assert (std['status'] == 0).all()

"""k_normalize_hist (csrc/k_segment.h, block_hist_medians of csrc/k_select.h): the float medians of the normalisation
from one histogram pass and one list pass.  Reads just above NORM_WINDOW_MIN through the segmentation stage; shift,
scale and the two outlier limits bit for bit against the CPU oracle, the code that ran (TBA_GET_NORM_FORM) against
what the case is built for and against the numpy restatement's own decision (tests/norm_hist_model.py).

(The file is named to be collected after the test_gpu_* files: tests/test_gpu_synth.py compares two engines' whole
norm buffers, never-written tails included, and so depends on which freed blocks the allocator hands out again --
on the allocations of every test that ran before it.)"""
import numpy as np
import pytest

import oracle
import norm_hist_model as M

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _setup(samp_name):
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    samp = th.seqSampleType(samp_name, samp_name == 'RNA')
    model = ts.TomboModel(seq_samp_type=samp)
    return model, ts.load_resquiggle_parameters(samp)


def _segment(samp_name, model, params, raws, seq, raw_dtype=np.float64, const_scale=None, scale_values=None,
             rna_event_scale=True):
    """the batch through TBA_STAGE_SEGMENT and every read through the oracle.
    Returns (norm forms, statuses, scale values [n][4], normalised signals, oracle results)"""
    from tombo_amd import resquiggle as rq, tombo_stats as ts, _native as N
    from tombo_amd._default_parameters import SIG_MATCH_THRESH
    eng = rq.get_engine(0)
    eng.set_model(model.level_means, model.level_sds, model.kmer_width, model.central_pos)
    o = N.make_opts(outlier_thresh=5.0, const_scale=const_scale, sig_match_thresh=SIG_MATCH_THRESH[samp_name])
    o.use_rna_event_scale = int(rna_event_scale)
    sv_in = sv_flags = None
    if scale_values is not None:
        sv_in = np.array([[sv.shift, sv.scale, sv.lower_lim, sv.upper_lim] for sv in scale_values])
        sv_flags = np.full(len(raws), 3, np.int32)
    codes = ts.encode_seq(seq)
    up = [np.asarray(r, raw_dtype) for r in raws]
    eng.upload(N.make_params(params), o, up, [codes] * len(raws), sv_in=sv_in, sv_flags=sv_flags)
    eng.run_stages(N.STAGE_SEGMENT, N.STAGE_SEGMENT)
    form, status, sv = eng.get(N.GET_NORM_FORM), eng.get(N.GET_STATUS), eng.get(N.GET_SEG_SV)
    norm = eng.get(N.GET_SEG_NORM)
    norms = [norm[eng.raw_off[i]:eng.raw_off[i + 1]] for i in range(len(raws))]
    orcs = []
    for i, r in enumerate(up):
        oo = oracle.make_opts(model.kmer_width, model.central_pos, outlier_thresh=5.0, const_scale=const_scale,
                              scale_values=None if scale_values is None else scale_values[i],
                              sig_match_thresh=SIG_MATCH_THRESH[samp_name])
        oo.use_rna_event_scale = int(rna_event_scale)
        orcs.append(oracle.resquiggle_read(r.astype(np.float64), codes, model.level_means, model.level_sds,
                                           oracle.make_params(params), oo, debug=True))
    return form, status, sv, norms, orcs


def _check_against_oracle(names, status, sv, norms, orcs, n_sv=4):
    """scale values and normalised signal of the segmentation stage, bit for bit, wherever the oracle's
    segmentation went through; its failure status where it did not.  Returns the reads compared."""
    compared = 0
    for i, (name, o) in enumerate(zip(names, orcs)):
        d = o['dbg']
        if len(d['valid_cpts']) == 0:                 # the oracle's segmentation failed: the status is what compares
            assert o['status'] != 0 and int(status[i]) == o['status'], (name, int(status[i]), o['status'])
            continue
        assert int(status[i]) == 0, (name, int(status[i]))
        assert np.array_equal(_bits(sv[i][:n_sv]), _bits(d['seg_scale_values'][:n_sv])), \
            (name, sv[i].tolist(), d['seg_scale_values'].tolist())
        assert np.array_equal(_bits(norms[i]), _bits(d['seg_norm_signal'])), name
        compared += 1
    return compared


@pytest.fixture(scope='module')
def dna():
    from tombo_amd import synth
    model, params = _setup('DNA')
    seq, raw, _ = synth.synth_read(model, 2400, 31337, **synth.DNA_SYNTH)
    return model, params, seq, M.variants(raw)


def _want_form(N, x, want, want_mad=True):
    if want is None:
        want = 'hist' if M.hist_medians(x, want_mad) is not None else 'select'
    return N.NORM_FORM_HIST if want == 'hist' else N.NORM_FORM_SELECT


def test_case_list_float64_on_gpu(dna):
    """odd / even length, symmetric and asymmetric middle samples, a coarse grid, a middle bucket beyond the list,
    wild samples inside and outside the strided sample, a constant read, a NaN, a read below NORM_WINDOW_MIN"""
    from tombo_amd import _native as N
    model, params, seq, cases = dna
    names = list(cases)
    form, status, sv, norms, orcs = _segment('DNA', model, params, [cases[k][0] for k in names], seq)
    for i, k in enumerate(names):
        x, want = cases[k]
        print(k, 'form', int(form[i]), 'status', int(status[i]), 'oracle status', orcs[i]['status'], sv[i].tolist())
        # the kernel and its restatement take the same decision on every case
        assert (M.hist_medians(x) is not None) == (form[i] == N.NORM_FORM_HIST), k
        assert form[i] == _want_form(N, x, want), (k, int(form[i]))
    # (a NaN has no defined median -- np.median gives NaN, a sort puts it anywhere: no reference to compare with.  The
    # histogram kernel leaves such a read alone, asserted above; k_normalize's own code does not fail it)
    i_nan = names.index('nan')
    keep = [i for i in range(len(names)) if i != i_nan]
    assert _check_against_oracle([names[i] for i in keep], status[keep], sv[keep], [norms[i] for i in keep],
                                 [orcs[i] for i in keep]) >= 8
    assert int(status[i_nan]) == 0
    # ... and gives it the scale values it gave before the histogram kernel existed (recorded from the parent commit's
    # library on this very read: a change of k_normalize's behaviour on NaN shows here)
    assert sv[i_nan].tolist() == [90.5734472188457, 12.853471433985973, -4.999999999999999, 5.000000000000001]
    assert int(status[names.index('constant')]) == 100                    # zero MAD: TBA_INTERNAL
    assert M.hist_medians(cases['even_symmetric'][0])[2] == 0.0 and M.hist_medians(cases['even'][0])[2] != 0.0


def test_float32_input_on_gpu(dna):
    from tombo_amd import _native as N
    model, params, seq, cases = dna
    names = ['odd', 'even', 'coarse_grid', 'wild_outside_sample', 'short']
    raws = [cases[k][0].astype(np.float32) for k in names]
    form, status, sv, norms, orcs = _segment('DNA', model, params, raws, seq, raw_dtype=np.float32)
    for i, k in enumerate(names):
        x = raws[i].astype(np.float64)
        assert form[i] == _want_form(N, x, None), (k, int(form[i]))
    assert form[:2].tolist() == [N.NORM_FORM_HIST] * 2 and form[4] == N.NORM_FORM_SELECT
    assert _check_against_oracle(names, status, sv, norms, orcs) == len(names)


def test_given_scale_is_not_ranked_on_gpu(dna):
    """const_scale and scale_values: nothing for the histogram kernel to find, and it must not run"""
    from tombo_amd import tombo_helper as th, _native as N
    model, params, seq, cases = dna
    names = ['odd', 'even']
    raws = [cases[k][0] for k in names]
    form, status, sv, norms, orcs = _segment('DNA', model, params, raws, seq, const_scale=11.5)
    assert form.tolist() == [N.NORM_FORM_SELECT] * 2
    assert _check_against_oracle(names, status, sv, norms, orcs) == 2
    svs = [th.scaleValues(90.25, 11.75, -4.5, 5.5, 5.0)] * 2
    form, status, sv, norms, orcs = _segment('DNA', model, params, raws, seq, scale_values=svs)
    assert form.tolist() == [N.NORM_FORM_NONE] * 2
    assert _check_against_oracle(names, status, sv, norms, orcs) == 2


def test_rna_mode_1_on_gpu():
    """RNA normalises after event detection (k_normalize's mode 1): with the event scaling off its medians are
    taken over the raw signal, without outlier limits; with it on (the default) there is nothing to rank"""
    from tombo_amd import synth, _native as N
    model, params = _setup('RNA')
    seq, raw, _ = synth.synth_read(model, 520, 4242, **synth.RNA_SYNTH)
    assert raw.shape[0] >= 20001
    raws = [raw[:20000], raw[:17001], raw[:M.WINDOW_MIN - 1]]
    names = ['even', 'odd', 'short']
    form, status, sv, norms, orcs = _segment('RNA', model, params, raws, seq, rna_event_scale=False)
    assert form.tolist() == [N.NORM_FORM_HIST, N.NORM_FORM_HIST, N.NORM_FORM_SELECT]
    assert all(M.hist_medians(r, want_mad=False) is not None for r in raws[:2])
    assert _check_against_oracle(names, status, sv, norms, orcs, n_sv=2) == 3
    form, status, sv, norms, orcs = _segment('RNA', model, params, raws, seq, rna_event_scale=True)
    assert form.tolist() == [N.NORM_FORM_NONE] * 3
    assert _check_against_oracle(names, status, sv, norms, orcs) == 3

"""RNA adapter trimming inside the worker: resquiggle_batch_iters(device_prep=True, trim_rna_adapter=True) over reads
in acquisition order with a DNA-adapter-like head equals the same call on the reads cut beforehand at the ends the CPU
restatement of trim_rna gives (tests/trim_rna_reference.py over the oracle) -- every field; a read too short for the
windows fails once, without a pass and without the save-parameter retry; without the argument nothing changes."""
import numpy as np
import pytest

import trim_rna_cases as tc
import trim_rna_reference as tr

pytestmark = pytest.mark.gpu
N_READS = 24
SHORT = 9           # this read is too short for the windows


@pytest.fixture(scope='module')
def setup():
    from tombo_amd import synth, tombo_stats as ts, tombo_helper as th
    samp = th.seqSampleType('RNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)
    save = ts.load_resquiggle_parameters(samp, use_save_bandwidth=True)
    rng = np.random.default_rng(8800)
    mrs = []
    for k in range(N_READS):
        nb = 25 if k == SHORT else int(rng.integers(150, 320))
        mr = synth.synth_map_res(model, nb, 8800 + k, **synth.RNA_SYNTH)
        raw = mr.raw_signal[::-1]                                   # acquisition order, as the FAST5 holds it
        if k != SHORT:                                              # a head of events with little spread
            head = tc.signal(tc.Case('head', 100 + k, int(rng.integers(2000, 5000)), 1 << 30, False, None, None))
            raw = np.concatenate([head, raw])
        mrs.append(mr._replace(raw_signal=tc.dac(raw)))
    return samp, model, params, save, mrs


@pytest.fixture(scope='module')
def ends(setup):
    import oracle
    out = []
    for mr in setup[4]:
        try:
            out.append(tr.trim_rna(mr.raw_signal, tc.RNA_SEG, tc.DEFAULT_TRIM, oracle.valid_cpts, oracle.new_mean_stds))
        except ValueError as e:
            out.append(e)
    return out


def _run(setup, mrs, **kw):
    from tombo_amd import resquiggle as rq
    samp, model, params, save = setup[:4]
    st = np.random.get_state()
    np.random.seed(31)
    try:
        return rq.resquiggle_batch_iters(mrs, model, params, save, outlier_thresh=5.0, seq_samp_type=samp,
                                         return_passes=True, device_prep=True, **kw)
    finally:
        np.random.set_state(st)


def _same(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        assert type(a) is type(b) and str(a) == str(b), (a, b)
        return
    assert a._fields == b._fields
    for f, x, y in zip(a._fields, a, b):
        if f == 'scale_values':
            assert tuple(x) == tuple(y), f
        elif isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f
        elif f == 'stall_ints':
            assert np.array_equal(np.asarray(x), np.asarray(y)), f
        else:
            assert x == y, f


def test_trimming_in_the_worker_equals_presliced_reads(setup, ends):
    mrs = setup[4]
    assert isinstance(ends[SHORT], ValueError) and sum(isinstance(e, Exception) for e in ends) == 1
    assert sum(1 for e in ends if not isinstance(e, Exception) and e > 0) >= N_READS // 2
    got, passes = _run(setup, mrs, trim_rna_adapter=True)
    keep = [k for k in range(N_READS) if k != SHORT]
    cut = [mrs[k]._replace(raw_signal=mrs[k].raw_signal[ends[k]:]) for k in keep]
    want, want_passes = _run(setup, cut)
    for k, w, p in zip(keep, want, want_passes):
        _same(got[k], w)
        assert passes[k] == p >= 1
    assert sum(not isinstance(r, Exception) for r in got) >= N_READS // 2
    # the short read: numpy's error once, no pass, no retry with the save parameters
    assert isinstance(got[SHORT], ValueError) and str(got[SHORT]) == tr.TOO_FEW_EVENTS_MSG and passes[SHORT] == 0


def test_without_the_argument_nothing_changes(setup):
    mrs = setup[4][:8]
    off, off_passes = _run(setup, mrs, trim_rna_adapter=False)
    plain, plain_passes = _run(setup, mrs)
    assert off_passes == plain_passes
    for a, b in zip(off, plain):
        _same(a, b)

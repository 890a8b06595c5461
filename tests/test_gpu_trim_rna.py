"""ts.trim_rna and the medians of ts.estimate_global_scale on the device (csrc/k_trim_rna.h).

trim_rna: the engine equals what the live reference answered on the float64 signals (tests/golden/stats_trim_rna.npz) and
equals the restatement over the CPU oracle (tests/trim_rna_reference.py, pinned to the reference by
tests/test_trim_rna_reference.py) on float64 and on int16 DAC input, exactly -- every case alone and the cases of one
parameter set as one mixed batch, in both dispatch forms of event detection, the form reported asserted.
raw_med_mad: np.median and np.median(np.abs(x - median)), bit for bit."""
import numpy as np
import pytest

import trim_rna_cases as tc
from conftest import engine_dispatch, FORMS
from test_trim_rna_reference import expected, recorded, golden  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def signals():
    return dict((c.name, tc.signal(c)) for c in tc.CASES)


@pytest.fixture(scope='module')
def want(signals):
    """the restatement over the oracle, once: name -> (answer on float64, answer on the DAC rounding)"""
    return dict((c.name, (expected(signals[c.name], c), expected(tc.dac(signals[c.name]), c))) for c in tc.CASES)


def run(eng, raws, case):
    """Engine.trim_rna -> per read the adapter end, or 'Class: text' of the exception the host layer makes of it"""
    from tombo_amd import tombo_stats as ts
    ends, status = eng.trim_rna(raws, case.seg, case.trim)
    out = []
    for end, st in zip(ends.tolist(), status.tolist()):
        err = ts._trim_error(st)
        assert err is None or end == 0
        out.append(end if err is None else '%s: %s' % (type(err).__name__, err))
    return out


def check_form(eng, form, case, answers):
    """the kernels that produced the change points of the reads that have some: k_detect + k_pick in the throughput
    form at the parameters it is compiled for (a read it gives up goes to the kernels that keep the scores),
    else those kernels"""
    from tombo_amd import _native as N
    assert len(answers) == eng.last_trim_ed_form.shape[0]
    got = eng.last_trim_ed_form.tolist()
    fused = form == 'throughput' and 2 * case.seg[0] <= 32 and case.seg[1] == 3
    if fused:
        assert set(got) <= {N.ED_FORM_DETECT_PICK, N.ED_FORM_SCORES_PEAKS} and N.ED_FORM_DETECT_PICK in got, got
    else:
        assert set(got) == {N.ED_FORM_SCORES_PEAKS}, got


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', tc.CASES, ids=lambda c: c.name)
def test_each_case_alone(golden, signals, want, case, form):  # noqa: F811
    raw = signals[case.name]
    with engine_dispatch(form) as eng:
        got = run(eng, [raw], case)
        assert got == [recorded(golden, case)] == [want[case.name][0]]
        check_form(eng, form, case, got)
        got = run(eng, [tc.dac(raw)], case)
        assert got == [want[case.name][1]]
        check_form(eng, form, case, got)


def _groups():
    groups = {}
    for c in tc.CASES:
        groups.setdefault((c.seg, c.trim), []).append(c)
    return [g for g in groups.values() if len(g) > 1]


@pytest.mark.parametrize('form', FORMS)
def test_mixed_batches(signals, want, form):
    """the cases of one parameter set in one call: failing reads between good ones leave their neighbours' answers
    as they are alone"""
    groups = _groups()
    default = [g for g in groups if g[0].trim == tc.DEFAULT_TRIM and g[0].seg == tc.RNA_SEG][0]
    assert len(default) >= 10 and [isinstance(want[c.name][0], str) for c in default].count(True) == 2
    with engine_dispatch(form) as eng:
        for g in groups:
            names = [c.name for c in g]
            names = names[3:] + names[:3]       # (the default set: its two failing reads end up side by side inside)
            if g is default:
                assert all(isinstance(want[k][0], int) for k in (names[0], names[-1]))
            assert run(eng, [signals[k] for k in names], g[0]) == [want[k][0] for k in names]
            assert run(eng, [tc.dac(signals[k]) for k in names], g[0]) == [want[k][1] for k in names]


def test_empty_batch_and_argument_checks():
    from tombo_amd import resquiggle as rq
    eng = rq.get_engine(0)
    ends, status = eng.trim_rna([], tc.RNA_SEG, tc.DEFAULT_TRIM)
    assert ends.shape == status.shape == (0,) and eng.last_trim_kernel_ms == 0.0
    x = np.zeros(3000)
    for seg, trim in (((12, 6), tc.DEFAULT_TRIM), ((12, 0, 15), tc.DEFAULT_TRIM), (tc.RNA_SEG, (0, 100, 0.7, 40000)),
                      (tc.RNA_SEG, (50, 100, float('nan'), 40000)), (tc.RNA_SEG, (8193, 100, 0.7, 40000))):
        with pytest.raises(ValueError):
            eng.trim_rna([x], seg, trim)
    with pytest.raises(ValueError):
        eng.trim_rna([x.astype(np.float32)], tc.RNA_SEG, tc.DEFAULT_TRIM)
    with pytest.raises(ValueError):
        eng.trim_rna([x, x.astype(np.int16)], tc.RNA_SEG, tc.DEFAULT_TRIM)


def test_budget_cut_and_determinism(want):
    """40 reads under a sample budget that cuts them into several device passes: the uncut result, and the same bytes
    from a second call"""
    from tombo_amd import resquiggle as rq
    eng = rq.get_engine(0)
    base = [c for c in tc.CASES if c.trim == tc.DEFAULT_TRIM and c.seg == tc.RNA_SEG and c.n <= 12000]
    raws, exp = [], []
    for k in range(40):
        c = base[k % len(base)]
        raws.append(tc.dac(tc.signal(c)))
        exp.append(want[c.name][1])
    case = base[0]
    uncut = run(eng, raws, case)
    form_uncut = eng.last_trim_ed_form.copy()
    assert uncut == exp
    try:
        eng.set_trim_budget(30000)          # two or three of these reads per pass
        a = eng.trim_rna(raws, case.seg, case.trim)
        b = eng.trim_rna(raws, case.seg, case.trim)
        assert run(eng, raws, case) == uncut and np.array_equal(eng.last_trim_ed_form, form_uncut)
        eng.set_trim_budget(1)              # a pass per read
        assert run(eng, raws[:6], case) == uncut[:6]
    finally:
        eng.set_trim_budget(0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


MED_MAD_LENGTHS = (1, 2, 3, 64, 65, 4096, 4097, 100001)


@pytest.mark.parametrize('dtype', (np.int16, np.float64))
def test_raw_med_mad_is_np_median(dtype):
    from tombo_amd import resquiggle as rq
    eng = rq.get_engine(0)
    rng = np.random.default_rng(99)
    raws = [rng.normal(480.0, 70.0, size=n) for n in MED_MAD_LENGTHS]
    raws.append(np.full(777, 503.0))                                   # a constant read: MAD 0
    raws.append(np.array([-32768.0, 32767.0] * 50 + [-32768.0]))       # the extremes of int16 in one read
    raws.append(np.array([-32768.0, 32767.0]))                         # ... and a median between them
    raws = [np.round(r).astype(np.int16) if dtype is np.int16 else r for r in raws]
    med, mad = eng.raw_med_mad(raws)
    for i, r in enumerate(raws):
        m = np.median(r)
        assert med[i].tobytes() == np.float64(m).tobytes(), (i, med[i], m)
        assert mad[i].tobytes() == np.float64(np.median(np.abs(r - m))).tobytes(), i
    assert mad[len(MED_MAD_LENGTHS)] == 0.0
    one = eng.raw_med_mad(raws[3:4])
    assert one[0][0] == med[3] and one[1][0] == mad[3]
    assert eng.raw_med_mad([])[0].shape == (0,)
    with pytest.raises(ValueError):
        eng.raw_med_mad([raws[0][:0]])
    with pytest.raises(ValueError):
        eng.raw_med_mad([raws[0].astype(np.float32)])


def test_estimate_global_scale_on_the_device():
    """ts.estimate_global_scale over raw arrays: the shuffle of numpy's global RNG, one engine call, np.mean"""
    from tombo_amd import tombo_stats as ts
    rng = np.random.default_rng(5)
    reads = [np.round(rng.normal(500.0, 30.0 + 3 * i, size=3000 + 17 * i)).astype(np.int16) for i in range(12)]
    order = list(range(12))
    np.random.seed(11)
    np.random.shuffle(order)
    want = np.mean([np.median(np.abs(reads[i] - np.median(reads[i]))) for i in order[:8]])
    np.random.seed(11)
    assert ts.estimate_global_scale(list(reads), 8) == want

"""The counting argument of block_hist_medians (csrc/k_select.h), restated in numpy (norm_hist_model.py) and held
against np.median: wherever the restatement answers, its four medians are the reference's bit for bit; where
it declines, k_normalize's own selects run.  tests/test_normalize_hist_gpu.py holds the kernel to the same cases."""
import numpy as np
import pytest

import norm_hist_model as M


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


@pytest.fixture(scope='module')
def cases():
    return M.variants(M.model_signal(20001, 11))


@pytest.mark.parametrize('name', ['odd', 'even', 'even_symmetric', 'coarse_grid', 'median_bucket_over_cap',
                                  'wild_in_sample', 'wild_outside_sample', 'constant', 'nan', 'short'])
def test_case_list(cases, name):
    x, want = cases[name]
    got = M.hist_medians(x)
    if want is not None:
        assert (got is not None) == (want == 'hist'), name
    if got is not None:
        with np.errstate(all='ignore'):
            assert _same_bits(got[:4], M.reference_medians(x)), name
        if want == 'hist':                                                # continuous values: the list is a small part of the read
            assert got[4] <= 0.02 * x.size


def test_symmetric_and_asymmetric_middle(cases):
    """even length: the normalised median is exactly 0 when the middle samples sit symmetrically around the shift
    (the third median is then an image of the second), a few 1e-17 otherwise (it is ranked on its own)"""
    assert M.hist_medians(cases['even_symmetric'][0])[2] == 0.0
    assert M.hist_medians(cases['even'][0])[2] != 0.0
    assert M.hist_medians(cases['odd'][0])[2] == 0.0


def test_random_reads():
    """3 000 reads of random length, five kinds: never a wrong answer.  The plain, float32 and rescaled signals are
    always answered; quantised ones decline when the grid is coarse (empty brackets, ties around the middle), the
    ones with wild samples when a wild sample falls into the strided sample (the histogram's range is then theirs)"""
    rng = np.random.default_rng(5)
    kinds = ['plain', 'quantised', 'wild', 'float32', 'rescaled']
    declined = dict.fromkeys(kinds, 0)
    for i in range(3000):
        n = int(rng.integers(M.WINDOW_MIN, 24000))
        x = M.model_signal(n, 1000 + i)
        kind = kinds[i % 5]
        if kind == 'quantised':
            x = np.round(x * 2.0 ** int(rng.integers(0, 12))) / 2.0 ** int(rng.integers(0, 12))
        elif kind == 'wild':
            x[rng.integers(0, n, 5)] += rng.normal(0, 1e4, 5)
        elif kind == 'float32':
            x = x.astype(np.float32).astype(np.float64)
        elif kind == 'rescaled':
            x = x * 2.0 ** int(rng.integers(-40, 40)) + rng.normal(0, 50)
        got = M.hist_medians(x)
        if got is None:
            declined[kind] += 1
            continue
        assert _same_bits(got[:4], M.reference_medians(x)), (i, kind)
    print(declined)
    assert declined['plain'] == declined['float32'] == declined['rescaled'] == 0, declined
    assert declined['quantised'] + declined['wild'] <= 600, declined


def _shapes(rng, n):
    """signals that are nothing like a nanopore read"""
    two = rng.choice([-1.0, 1.0], n)
    return {
        'bimodal': np.where(rng.random(n) < 0.5, rng.normal(-40.0, 1.0, n), rng.normal(60.0, 3.0, n)),
        'bimodal_even_split': np.concatenate([rng.normal(-40.0, 1.0, n // 2), rng.normal(60.0, 3.0, n - n // 2)]),
        'exponential': rng.exponential(5.0, n),
        'cauchy': rng.standard_cauchy(n),
        'small_integers': rng.poisson(3.0, n).astype(np.float64),
        'two_point': two,
        'two_point_jitter': two + rng.normal(0.0, 1e-9, n),
        'uniform': rng.random(n),
        'ramp': np.arange(n, dtype=np.float64),
        'heavy_ties_one_side': np.where(rng.random(n) < 0.4, 7.0, rng.normal(0.0, 1.0, n)),
        'sign_flip': rng.normal(0.0, 1.0, n) * 1e-300,
    }


def test_adversarial_shapes():
    """bimodal, skewed, heavy-tailed, discrete and two-point signals, odd and even lengths: the restatement may decline
    (massive ties, empty brackets, a middle that straddles a gap) but every answer it gives is np.median's bit for bit;
    signals of few distinct values are always declined"""
    rng = np.random.default_rng(77)
    answered = dict()
    for rep in range(12):
        n = int(rng.integers(M.WINDOW_MIN, 22000)) | (rep & 1)
        for name, x in _shapes(rng, n).items():
            got = M.hist_medians(x)
            answered.setdefault(name, 0)
            if got is None:
                continue
            answered[name] += 1
            with np.errstate(all='ignore'):
                assert _same_bits(got[:4], M.reference_medians(x)), (name, n)
    print(answered)
    assert answered['two_point'] == 0 and answered['small_integers'] == 0, answered
    # (not a bound on how often it answers: only that the exactness above was exercised on the continuous shapes)
    assert min(answered[k] for k in ('uniform', 'exponential', 'ramp', 'heavy_ties_one_side')) >= 1, answered

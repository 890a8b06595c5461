"""The cases of tests/theil_cases.py on the CPU: from the reference alone, each has the property it is named for -- where
the median slope lies relative to the first bucket range (0.5, 1.5), the share of pairs with equal levels or equal
slopes, the parity of n (n - 1) / 2, twice the raw samples against the list's smallest and largest capacity, the
status -- and the forms SMALL and NO_SCRATCH follow from n and n_raw by the header's constants, which are read from the
source: a retuned constant fails here first, not as a path that silently goes untested on the GPU."""
import numpy as np
import pytest

import norm_api_cases as M
import theil_cases as TC

CASES = TC.cases()
BY_NAME = {c.name: c for c in CASES}
T = TC.constants()


def group(letter):
    return [c for c in CASES if c.name.startswith(letter + '_')]


def n_points(c):
    return min(c.means.shape[0], 1000)


def bits(x):
    return np.float64(x).tobytes()


def test_constants_are_the_ones_the_cases_were_built_for():
    assert (T['TSW_MIN_POINTS'], T['LIST_MIN'], T['LIST_MAX'], T['SEL_NT']) == (256, 4096, 65536, 512)
    assert (T['TSW_SAMPLE_MIN'], T['TSW_SAMPLE_DIST'], T['BS_NB'], T['BS_CAP'], T['BS_LEVELS']) == (48, 128, 4096, 2048, 4)
    assert T['TSW_REL'] == 1e-5
    assert len(BY_NAME) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_reference_status_and_second_statement(case):
    """the status the case expects, and norm_api_cases.theil_sen_fit -- the same statement in numpy, held to the
    reference's golden vectors -- gives the same bits"""
    ref = TC.reference_fit(case)
    assert ref.status == case.status
    assert ref.e.shape[0] == n_points(case) and case.norm.shape[0] == case.segs[-1]
    assert case.means.shape[0] <= 1001 or case.name == 'a_sub_2500'
    with np.errstate(over='ignore'):
        second = M.theil_sen_fit(0.0, 1.0, ref.e, ref.m)
    if case.status == TC.TBA_RESCALE_FAIL:
        assert second == 'zero_slope' and ref.slope == 0
    else:
        assert bits(second[2]) == bits(ref.shift_corr) and bits(second[3]) == bits(ref.scale_corr)


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_small_and_no_scratch_follow_from_the_sizes(case):
    n, cap = n_points(case), min(2 * case.norm.shape[0], T['LIST_MAX'])
    assert (case.form == 'SMALL') == (n < T['TSW_MIN_POINTS'])
    assert (case.form == 'NO_SCRATCH') == (n >= T['TSW_MIN_POINTS'] and cap < T['LIST_MIN'])
    assert case.form is None or case.form in TC.FORMS


def test_a_natural_points():
    a = group('a')
    assert sorted(n_points(c) for c in a if c.samp_ind is None) == [2, 3, 255, 256, 257, 511, 512, 513, 577, 999, 1000]
    assert sorted(c.means.shape[0] for c in a if c.samp_ind is not None) == [1001, 2500]
    for c in a:
        ref = TC.reference_fit(c)
        assert c.norm.shape[0] >= 32768 and 2 * c.norm.shape[0] >= T['LIST_MAX']
        assert n_points(c) < 256 or 0.5 < ref.slope < 1.5, c.name
        if c.samp_ind is not None:
            assert c.samp_ind.shape == (1000,) and np.unique(c.samp_ind).shape == (1000,)
            assert 0 <= c.samp_ind.min() and c.samp_ind.max() < c.means.shape[0]
    # odd and even numbers of slopes from TSW_MIN_POINTS on (below it the issue's sizes 2, 3 and 255 are all odd)
    par = {(n_points(c) >= 256, (n_points(c) * (n_points(c) - 1) // 2) % 2) for c in a}
    assert par == {(False, 1), (True, 0), (True, 1)}


def test_b_generic_enumerator_past_one_pass():
    b = group('b')
    assert sorted(n_points(c) for c in b) == [256, 511, 512, 513, 999, 1000]
    for c in b:
        assert c.norm.shape[0] == 2 * n_points(c) and 2 * c.norm.shape[0] < T['LIST_MIN']
        assert 0.5 < TC.reference_fit(c).slope < 1.5
    past = [n_points(c) for c in b if n_points(c) > T['SEL_NT']]
    assert {n % 2 for n in past} == {0, 1}              # the antipodal distance of an even n in the second trip of the loop
    assert {(n * (n - 1) // 2) % 2 for n in past} == {0, 1}


def test_c_no_window():
    c_ = group('c')
    assert sorted({n_points(c) for c in c_}) == [513, 1000] and len(c_) == 16
    for c in c_:
        ref = TC.reference_fit(c)
        assert not 0.5 < ref.slope < 1.5, c.name
        win, _ = TC.sampled_window(ref.e, ref.m, T['LIST_MAX'], T)
        assert win is None, c.name
    for n in (513, 1000):
        want = {'0.25': 0.25, '3': 3.0, 'neg1': -1.0, '2pm40': 2.0 ** -40, '2p40': 2.0 ** 40}
        base = TC.reference_fit(BY_NAME['c_3_%d' % n]).slope / 3.0
        assert 0.5 < base < 1.5
        for tag, s in want.items():                      # (powers of two scale every slope exactly, 3 and -1 nearly)
            got = TC.reference_fit(BY_NAME['c_%s_%d' % (tag, n)]).slope
            assert abs(got / s - base) < 1e-12
        for tag, s in (('0.5', 0.5), ('1.5', 1.5)):
            ref = TC.reference_fit(BY_NAME['c_exact%s_%d' % (tag, n)])
            assert ref.slope == s and 0.5 < (ref.slopes == s).mean() < 0.6
            assert (ref.slopes < s).any() and (ref.slopes > s).any()
        # the refinement levels run out: after every level the median's bucket still holds more than one gather
        ref = TC.reference_fit(BY_NAME['c_decades_%d' % n])
        ns = ref.slopes.shape[0]
        members = TC.refinement_members(ref.slopes, (ns - 1) // 2, T)
        assert len(members) == T['BS_LEVELS'] and min(members) > T['BS_CAP'], members
        pos = ref.slopes[ref.slopes > 0]
        assert pos.shape[0] == ns and np.log10(pos.max() / pos.min()) > 250


def test_d_exact_ties():
    ref = TC.reference_fit(BY_NAME['d_all_1.0'])
    assert (ref.slopes == 1.0).all() and ref.slopes.shape[0] == 499500 > T['LIST_MAX']
    assert (TC.reference_fit(BY_NAME['d_all_0.25']).slopes == 0.25).all()
    ref = TC.reference_fit(BY_NAME['d_bimodal'])
    ns = ref.slopes.shape[0]
    assert (ref.slopes == 0.9).sum() == (ref.slopes == 1.1).sum() == 500 * 499 // 2
    assert (ref.slopes < 0.9).sum() == 0 and (ref.slopes > 1.1).sum() == 0
    win, _ = TC.sampled_window(ref.e, ref.m, T['LIST_MAX'], T)
    assert win is not None and 0.9 < win[0] <= ref.slope < win[1] < 1.1
    listed = ((ref.slopes >= win[0] * (1 - 2e-5)) & (ref.slopes <= win[1] * (1 + 2e-5))).sum()
    assert listed < T['LIST_MAX'] // 2 and (ref.slopes < win[0]).sum() <= (ns - 1) // 2


def test_e_equal_levels():
    ref = TC.reference_fit(BY_NAME['e_equal_75'])
    assert (ref.slopes == 1000.0).mean() > 0.5 and ref.slope == 1000.0 and ref.status == TC.TBA_OK
    assert (ref.slopes == 1000.0).sum() == 750 * 749 // 2
    ref = TC.reference_fit(BY_NAME['e_equal_50'])
    assert (ref.slopes == 1000.0).sum() == 500 * 499 // 2 and 0.5 < ref.slope < 1.5


def test_f_zero_slope_of_either_sign():
    signs = {}
    for tag in ('pos', 'neg'):
        ref = TC.reference_fit(BY_NAME['f_zero_' + tag])
        zeros = ref.slopes[ref.slopes == 0]
        assert zeros.shape[0] == 750 * 749 // 2 > ref.slopes.shape[0] // 2 and ref.slope == 0
        assert np.unique(np.signbit(zeros)).shape[0] == 1       # every middle slope carries the same sign
        signs[tag] = bool(np.signbit(zeros[0]))
    assert signs == {'pos': False, 'neg': True}


def test_g_scratch_edges():
    g = group('g')
    n_raw = sorted(c.norm.shape[0] for c in g)
    assert n_raw[0] == 2048 and 3000 in n_raw and sum(2048 < v < 3000 for v in n_raw) >= 2
    assert 2 * n_raw[0] == T['LIST_MIN'] and 2 * n_raw[-1] < T['LIST_MAX']
    for c in g:
        assert n_points(c) == 1000 and c.form is None and np.diff(c.segs).min() >= 2
        assert bits(TC.reference_fit(c).slope) == bits(TC.reference_fit(g[0]).slope)   # the same points, other dwells


def test_h_intercepts():
    ref = TC.reference_fit(BY_NAME['h_far'])
    assert (ref.m - ref.slope * ref.e).max() < -2.0
    ref = TC.reference_fit(BY_NAME['h_collinear'])
    assert ref.slope == 1.0 and np.unique(ref.m - ref.slope * ref.e).tolist() == [-500.0]
    ref = TC.reference_fit(BY_NAME['h_even_512'])
    mid = np.sort(ref.m - ref.slope * ref.e)[255:257]
    assert mid[0] < mid[1] < -2.0 and bits(ref.inter) == bits((mid[0] + mid[1]) / 2.0)


def test_i_magnitudes():
    base = TC.reference_fit(BY_NAME['a_1000'])
    win, _ = TC.sampled_window(base.e, base.m, T['LIST_MAX'], T)
    ns = base.slopes.shape[0]
    assert win is not None and (base.slopes < win[0]).sum() <= (ns - 1) // 2 and (base.slopes < win[1]).sum() > ns // 2
    listed = {}
    for tag, s in (('2p100', 2.0 ** 100), ('2pm100', 2.0 ** -100), ('2pm140', 2.0 ** -140), ('2pm160', 2.0 ** -160),
                   ('2p200', 2.0 ** 200)):
        ref = TC.reference_fit(BY_NAME['i_' + tag])
        assert ref.slopes.tobytes() == base.slopes.tobytes()
        assert bits(ref.scale_corr) == bits(base.scale_corr) and bits(ref.shift_corr) == bits(base.shift_corr * s)
        listed[tag] = TC.listed_pairs(ref.e, ref.m, win, T)     # (the same slopes: the same window)
    # normal floats list what the unscaled points list; subnormal ones some more, still far below the list's capacity;
    # zeros and infinities list every pair
    assert listed['2p100'] == listed['2pm100'] == TC.listed_pairs(base.e, base.m, win, T) < T['LIST_MAX'] // 4
    assert listed['2pm100'] < listed['2pm140'] < T['LIST_MAX'] // 4
    assert listed['2pm160'] == ns and listed['2p200'] == ns + 24 * 1000      # (and 24 padding partners per row)
    f32 = np.finfo(np.float32)
    assert np.abs(TC.reference_fit(BY_NAME['i_2p100']).e).max() * 4 < f32.max
    assert np.abs(TC.reference_fit(BY_NAME['i_2pm100']).e).min() > f32.tiny
    ref = TC.reference_fit(BY_NAME['i_2pm140'])
    assert (np.abs(ref.m) + 3 * np.abs(ref.e)).max() < f32.tiny      # every float copy is subnormal or zero
    assert np.float32(2.0 ** -20 * (np.abs(ref.m) + 3 * np.abs(ref.e)).max()) == 0
    assert np.abs(TC.reference_fit(BY_NAME['i_2pm160']).e).max() * 4 < 2.0 ** -150
    assert np.abs(TC.reference_fit(BY_NAME['i_2p200']).e).min() * 2.0 ** -60 > f32.max
    # e + 2^20: the guard band tau = 2^-20 max(|m| + 3 |e|) exceeds every difference of the compared values u = m - t e
    ref = TC.reference_fit(BY_NAME['i_cancel'])
    win, _ = TC.sampled_window(ref.e, ref.m, T['LIST_MAX'], T)
    assert win is not None and 0.5 < ref.slope < 1.5
    tau = 2.0 ** -20 * (np.abs(ref.m) + 3 * np.abs(ref.e)).max()
    for t in (win[0] * (1 - T['TSW_REL']), win[1] * (1 + T['TSW_REL'])):
        u = (ref.m - t * ref.e).astype(np.float32).astype(np.float64)
        assert u.max() - u.min() < np.float64(np.float32(tau)) - 1.0
    assert TC.listed_pairs(ref.e, ref.m, win, T) == ref.slopes.shape[0]


def test_w_window_miss():
    c = BY_NAME['w_miss']
    ref = TC.reference_fit(c)
    ns = ref.slopes.shape[0]
    win, dist = TC.sampled_window(ref.e, ref.m, min(2 * c.norm.shape[0], T['LIST_MAX']), T)
    assert dist == list(range(1, 480, 10)) and win is not None
    assert ref.slope == 1.2 < win[0] and win[1] < 1.5
    assert (ref.slopes < win[0] * (1 - 2e-5)).sum() > (ns - 1) // 2          # the middle ranks lie below the window
    assert ((ref.slopes >= win[0] * (1 - 2e-5)) & (ref.slopes <= win[1] * (1 + 2e-5))).sum() < T['LIST_MAX'] // 2

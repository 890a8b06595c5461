"""TEST INFRASTRUCTURE: the cases of tests/golden/stats_norm_api.npz (gen_golden_norm_api.py records them from the
reference; test_norm_api_reference.py and test_gpu_norm_api.py read them) and a plain numpy restatement of the four
documented per-read functions of tombo_stats:

    normalize_raw_signal           tombo_stats.py:482-573
    calc_kmer_fitted_shift_scale   :370-450 ('mom' and 'theil_sen')
    get_read_seg_score             :2327-2338

The inputs are made from seeds here; the fixture keeps their SHA-256 only.  The restatement spells every median and
percentile out as order statistics of a sorted copy, which is the form the kernels of csrc/k_norm_api.h compute."""
import hashlib
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stats_norm_api.npz')

# the edges of the select forms of k_select.h (192: direct ranking, 2048: one bucket, 4096 / 16384: the pipeline's
# one-pass forms) and 201, where (n - 1) * 0.465 is a whole number
LENGTHS = (1, 2, 3, 63, 64, 65, 201, 4095, 4096, 16383, 16384, 16385, 50001)
NORM_TYPES = ('none', 'pA_raw', 'median', 'median_const_scale', 'robust_median')
THRESHES = (None, 5.0, 0.5)
CONST_SCALE = 37.25
CHANNEL = (-3.0, 1437.5, 8192.0)            # offset, range, digitisation
POINT_SIZES = (2, 9, 128, 129, 8192, 8193, 20000)       # every depth of numpy's pairwise summation tree
THEIL_SIZES = (2, 3, 1000, 1001)
MAX_FULL = 512      # a normalised signal of at most this many samples is stored whole

# sv: None, or (shift, scale, lower_lim or None, upper_lim or None)
NormCase = namedtuple('NormCase', 'name dtype kind seed n_sig start n norm_type thresh sv const_scale')


def make_signal(kind, dtype, n, seed):
    """'noise': a DAC-like signal (int16: rounded, so full of ties); 'runs': DAC values in runs of 50 equal samples;
    'flat': one value"""
    rng = np.random.default_rng(seed)
    if kind == 'flat':
        x = np.full(n, 517.0)
    elif kind == 'runs':
        x = np.repeat(rng.integers(400, 600, n // 50 + 1), 50)[:n].astype(np.float64)
    else:
        x = rng.standard_normal(n) * 80.0 + 500.0 + (rng.random(n) < 0.01) * rng.standard_normal(n) * 900.0
    if dtype == 'int16':
        return np.clip(np.rint(x), -2000, 8000).astype(np.int16)
    return x if kind != 'noise' else x + rng.random(n) * 1e-3


def norm_cases():
    cases = []

    def add(name, dtype, kind, seed, n_sig, start, n, norm_type, thresh, sv=None, const_scale=None):
        if norm_type == 'median_const_scale' and const_scale is None:
            const_scale = CONST_SCALE
        cases.append(NormCase('%s/%s' % (dtype, name), dtype, kind, seed, n_sig, start, n, norm_type, thresh, sv, const_scale))

    for dtype in ('int16', 'float64'):
        for li, n in enumerate(LENGTHS):
            for ti, norm_type in enumerate(NORM_TYPES):
                # the whole signal under every threshold; a window strictly inside a longer signal under one of them
                for thresh in THRESHES:
                    add('full/%d/%s/%s' % (n, norm_type, thresh), dtype, 'noise', 1000 + li, n, 0, n, norm_type, thresh)
                thresh = THRESHES[(li + ti) % 3]
                add('inside/%d/%s/%s' % (n, norm_type, thresh), dtype, 'noise', 2000 + li, n + 37, 11, n, norm_type, thresh)
        for n in (3, 65, 4096, 16385):
            for what, sv, thresh in (('lims', (497.5, 81.25, -2.5, 3.0), None), ('no_lims', (497.5, 81.25, None, None), None),
                                     ('lims_overridden', (497.5, 81.25, -2.5, 3.0), 5.0), ('negative_scale', (497.5, -81.25, -1.0, 1.0), None)):
                add('given/%d/%s' % (n, what), dtype, 'noise', 3000 + n, n + 5, 2, n, 'median', thresh, sv)
            add('given_invalid_type/%d' % n, dtype, 'noise', 3000 + n, n + 5, 2, n, 'no_such_type', None, (497.5, 81.25, None, None))
            for thresh in (None, 5.0):
                add('neg_const/%d/%s' % (n, thresh), dtype, 'noise', 3100 + n, n, 0, n, 'median_const_scale', thresh, None, -12.5)
        for n in (1000, 4096, 16385, 50001):
            for norm_type in ('median', 'robust_median'):
                for thresh in (None, 5.0):
                    add('runs/%d/%s/%s' % (n, norm_type, thresh), dtype, 'runs', 4000 + n, n, 0, n, norm_type, thresh)
        for n in (1, 200, 5000):        # a scale of exactly 0: the reference raises FloatingPointError
            for norm_type in ('median', 'robust_median'):
                add('flat/%d/%s' % (n, norm_type), dtype, 'flat', 0, n, 0, n, norm_type, None)
        add('flat/given_zero_scale', dtype, 'noise', 5000, 100, 0, 100, 'median', None, (1.0, 0.0, None, None))
        add('flat/zero_const_scale', dtype, 'noise', 5000, 100, 0, 100, 'median_const_scale', 5.0, None, 0.0)
    assert len(set(c.name for c in cases)) == len(cases)
    return cases


def case_signal(c):
    return make_signal(c.kind, c.dtype, c.n_sig, c.seed)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the restatement -------------------------------------------------------------------------------------------
def median(v):
    """np.median as order statistics: the middle one, or the two middle ones added and halved"""
    s = np.sort(np.asarray(v, dtype=np.float64))
    n = s.shape[0]
    return s[(n - 1) // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0


def percentile(v, pct):
    """np.percentile, linear: numpy's _lerp between the two order statistics around (n - 1) q; for an integer array
    numpy subtracts them in the array's own type"""
    s = np.sort(v)
    n = s.shape[0]
    vi = (n - 1) * (pct / 100.0)
    k = int(np.floor(vi))
    a, b = s[k], s[min(k + 1, n - 1)]
    t = vi - np.floor(vi)
    with np.errstate(over='ignore'):
        d = np.float64(b - a)
    a, b = np.float64(a), np.float64(b)
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def normalize(sig, start, n, norm_type, thresh, sv, const_scale):
    """-> (norm, shift, scale, lower, upper) with None limits where the reference returns None, or 'zero_scale'"""
    x = sig[start:start + n]
    xf = x.astype(np.float64)
    if sv is not None:
        shift, scale = sv[0], sv[1]
    elif norm_type == 'none':
        shift, scale = 0, 1
    elif norm_type == 'pA_raw':
        shift, scale = -1 * CHANNEL[0], CHANNEL[2] / CHANNEL[1]
    elif norm_type == 'robust_median':
        shift = (percentile(x, 46.5) + percentile(x, 53.5)) / 2.0
        scale = median(np.abs(xf - shift))
    else:
        shift = median(xf)
        scale = const_scale if norm_type == 'median_const_scale' else median(np.abs(xf - shift))
    if scale == 0:
        return 'zero_scale'
    norm = (xf - shift) / scale
    lower, upper = (None, None) if sv is None else (sv[2], sv[3])
    if thresh is not None:
        med = median(norm)
        mad = median(np.abs(norm - med))
        lower, upper = med - (mad * thresh), med + (mad * thresh)
    if lower is not None and upper is not None:
        norm = np.where(norm > upper, upper, np.where(norm < lower, lower, norm))       # c_apply_outlier_thresh
    return norm, shift, scale, lower, upper


def points(n, seed):
    """(event means, model means, model inverse variances) of n points: a line with noise"""
    rng = np.random.default_rng(seed)
    model = rng.standard_normal(n) * 1.2
    sds = 0.1 + rng.random(n) * 0.4
    events = 3.5 + 1.75 * model + rng.standard_normal(n) * 0.3
    return events, model, 1.0 / (sds * sds), sds


def mom_sums(e, m, iv):
    mv = m * iv
    ev = e * iv
    return np.array([iv.sum(), mv.sum(), (mv * m).sum(), ev.sum(), (ev * m).sum()])


def mom_fit(prev_shift, prev_scale, sums):
    coef_mat = np.array(((sums[0], sums[1]), (sums[1], sums[2])))
    shift_corr, scale_corr = np.linalg.solve(coef_mat, np.array((sums[3], sums[4])))
    return prev_shift + (shift_corr * prev_scale), prev_scale * scale_corr, shift_corr, scale_corr


def theil_sen_fit(prev_shift, prev_scale, e, m, max_points=1000):
    """after np.random.seed: the draw, the slopes of all pairs i < j (equal event means give c_compute_slopes'
    max_slope of 1000), both medians"""
    if m.shape[0] > max_points:
        ind = np.random.choice(m.shape[0], max_points, replace=False)
        m, e = m[ind], e[ind]
    i, j = np.triu_indices(e.shape[0], 1)
    de, dm = e[i] - e[j], m[i] - m[j]
    with np.errstate(divide='ignore', invalid='ignore'):
        slopes = np.where(de == 0, 1000.0, dm / de)
    slope = median(slopes)
    inter = median(m - (slope * e))
    if slope == 0:
        return 'zero_slope'
    scale_corr, shift_corr = 1 / slope, -inter / slope
    return prev_shift + (shift_corr * prev_scale), prev_scale * scale_corr, shift_corr, scale_corr


def seg_score(means, ref_means, ref_sds):
    return np.mean(np.abs((means - ref_means) / ref_sds))

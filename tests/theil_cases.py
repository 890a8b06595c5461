"""Reads that take k_theil_sen (csrc/k_tail.h) through every form it has and every reason its one-pass form declines
(helper module of test_theil_cases_reference.py and test_gpu_theil_sen_forms.py; no tests of its own).

A case is what the stage entry takes: a normalised signal, base boundaries, expected levels -- built from the POINTS of
the fit: base k gets L_k samples of one value e_k, so bases of the same value and length have bit-equal means, and m_k
is its expected level.  The reference (reference_fit) is plain float64 on the CPU: oracle.new_means over the boundaries
for e, oracle.compute_slopes(e, m), np.median of the slopes, np.median(m - slope * e); slope == 0 is TBA_RESCALE_FAIL,
otherwise the fit is (-inter / slope, 1 / slope).  The kernel has to give those two numbers bit for bit.

What decides the form (TBA_TS_FORM_*, TBA_GET_TS_FORM): n against TSW_MIN_POINTS, twice the read's raw samples against
4096 (the smallest list the one-pass form takes) and 65 536 (the largest), where the sampled median slope lies
relative to the first bucket range (0.5, 1.5), how many pairs the window lists, and whether the window holds the middle
ranks.  constants() reads the numbers out of the headers.

Groups (the letter in front of a case's name):
  a  natural points e = 0.02 + m + noise (norm_api_cases.points with slope 1) at the sizes where the kernel's loops
     change their trip counts, and two subsampled reads;
  b  the same points with two samples per base: 2 n_raw < 4096, the generic pair enumerator beyond one pass of the
     workgroup, odd and even n;
  c  the sampled median slope outside (0.5, 1.5) -- 0.25, exactly 0.5 and 1.5, 3, -1, 2^-40, 2^40 -- and slopes over
     300 decades, where the bucket select's refinement levels run out and the radix select finishes;
  d  massive exact ties: every slope 1.0 (all 499 500 pairs listed, past the list's cap), every slope 0.25 (the
     refinement meets a bucket of equal members), and two tie blocks beside the median.  Pairs of equal slope 0.9 are
     pairs on a common line of slope 0.9, an equivalence relation on the points, so two slopes can hold a quarter of
     the pairs each and no more (half the points on a line of each): d_bimodal has 25 % at exactly 0.9, 25 % at
     exactly 1.1 and the median among the cross pairs between;
  e  equal levels (the reference's max_slope = 1000): 75 % of the points share one e (median 1000.0), 50 % share one;
  f  slope exactly 0: 75 % of the points share one m; the zeros are +0.0 with e descending, -0.0 with e ascending;
  g  1000 points over 2048 .. 4200 raw samples: the list's cap is 2 n_raw, the short-dwell edge where the list crosses
     from the first scratch slice into the second or overflows.  No form is expected of a single read of this group;
  h  intercepts far outside [-2, 2], all equal, and an even n whose two middle intercepts differ;
  i  magnitudes: the points of a_1000 times 2^100 and 2^-100 (normal floats), 2^-140 (the float copies u the pair pass
     compares are subnormal, nine bits of them left, and the guard band tau rounds to zero: underflow is gradual on the
     device as in numpy, rounding is monotone and the compares are strict, so the pass stays right and lists some more
     pairs -- listed_pairs() restates it), 2^-160 (every u is zero) and 2^200 (every u is infinite, tau too: every
     compare is false or against NaN, the partners that pad the points to a multiple of 64 included) where everything
     is listed, and e + 2^20 (cancellation in e_i - e_j; tau
     exceeds every difference the pass compares: everything is listed);
  w  a window miss: 961 points, so that the sampled circular distances 1 + t0 * dmax / ds are 1, 11, 21, ...; the
     points lie on ten parallel lines of slope 1.2 by index modulo ten, ascending in e.  A sampled pair joins
     neighbouring lines and lies above 1.2 nine times out of ten; over all pairs the offsets cancel and the median is
     the tie at exactly 1.2, below the window."""
import collections
import os
import re

import numpy as np

TBA_OK, TBA_RESCALE_FAIL = 0, 19                                       # include/tombo_amd.h
FORMS = ('NONE', 'SMALL', 'FAST', 'NO_SCRATCH', 'NO_WINDOW', 'LIST_OVERFLOW', 'WINDOW_MISS')   # TBA_TS_FORM_*
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tombo_amd', 'csrc')

# form: the TBA_TS_FORM_* name expected, None where the group alone is held to a condition (g)
Case = collections.namedtuple('Case', 'name norm segs means sds samp_ind form status')


def constants():
    """what decides a read's form, out of the source: TSW_MIN_POINTS, the list's smallest and largest capacity, the
    sample's distances, the guard band, the workgroup's size, the bucket select's shape"""
    tail, sel = (open(os.path.join(CSRC, f)).read() for f in ('k_tail.h', 'k_select.h'))
    out = {}
    for text, names in ((tail, ('TSW_MIN_POINTS', 'TSW_SAMPLE_DIST', 'TSW_SAMPLE_MIN')),
                        (sel, ('SEL_NT', 'BS_NB', 'BS_CAP', 'BS_LEVELS'))):
        for nm in names:
            out[nm] = int(re.search(r'^#define[ \t]+%s[ \t]+(\d+)\b' % nm, text, re.M).group(1))
    out['TSW_REL'] = float(re.search(r'^#define[ \t]+TSW_REL[ \t]+([0-9.e+-]+)', tail, re.M).group(1))
    m = re.search(r'const i64 cap = cap1 \+ cap2 < (\d+) \? cap1 \+ cap2 : (\d+);', tail)
    assert m and m.group(1) == m.group(2)
    out['LIST_MAX'] = int(m.group(1))
    out['LIST_MIN'] = int(re.search(r'n >= TSW_MIN_POINTS && scratch != nullptr && cap >= (\d+)\)', tail).group(1))
    return out


def natural_points(n, seed, noise=0.3):
    """norm_api_cases.points with slope 1: m from the seed, e = 0.02 + m + noise"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal(n) * 1.2
    return 0.02 + m + rng.standard_normal(n) * noise, m


def _lens(n, n_raw):
    """n dwells that add up to n_raw, as even as they come"""
    return np.full(n, n_raw // n, np.int64) + (np.arange(n) < n_raw % n)


def _case(name, e, m, n_raw, form, status=TBA_OK, samp_ind=None):
    e, m = np.asarray(e, np.float64), np.asarray(m, np.float64)
    lens = _lens(e.shape[0], max(int(n_raw), e.shape[0]))
    segs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Case(name, np.repeat(e, lens), segs, m.copy(), np.ones(m.shape[0]),
                None if samp_ind is None else np.asarray(samp_ind, np.int64), form, status)


BIG = 33000         # raw samples of a read whose list has the largest capacity (2 n_raw >= 65 536)
G_NOISE = 0.3       # (group g: tuned together with G_N_RAW until the group holds both of its forms)
G_N_RAW = (2048, 2500, 2800, 3000, 3300, 3700, 4200)


def _build():
    cases = []
    add = lambda *a, **k: cases.append(_case(*a, **k))
    for n in (2, 3, 255, 256, 257, 511, 512, 513, 577, 999, 1000):
        e, m = natural_points(n, 100 + n)
        add('a_%d' % n, e, m, BIG, 'SMALL' if n < 256 else 'FAST')
    for nb in (1001, 2500):
        e, m = natural_points(nb, 100 + nb)
        samp = np.random.default_rng(nb).permutation(nb)[:1000]
        add('a_sub_%d' % nb, e, m, 35000, 'FAST', samp_ind=samp)
    for n in (256, 511, 512, 513, 999, 1000):
        e, m = natural_points(n, 200 + n)
        add('b_%d' % n, e, m, 2 * n, 'NO_SCRATCH')
    for n in (513, 1000):
        e, m = natural_points(n, 300 + n)
        for tag, s in (('0.25', 0.25), ('3', 3.0), ('neg1', -1.0), ('2pm40', 2.0 ** -40), ('2p40', 2.0 ** 40)):
            add('c_%s_%d' % (tag, n), e, s * m, BIG, 'NO_WINDOW')
        # exactly 0.5 / 1.5: three quarters of the points on the exact line through integer levels, the rest around it
        rng = np.random.default_rng(310 + n)
        ei = rng.permutation(4 * n)[:n].astype(np.float64) - 2 * n
        off = np.where(np.arange(n) % 4 == 0, np.round(rng.standard_normal(n) * 64), 0.0)
        add('c_exact0.5_%d' % n, 2 * ei, ei + off, BIG, 'NO_WINDOW')
        add('c_exact1.5_%d' % n, 2 * ei, 3 * ei + off, BIG, 'NO_WINDOW')
        # slopes over 300 decades: e positive and descending, m = e 2^(-1000 i / n), so slope(i, j > i) ~ 2^(-1000 i / n)
        ed = np.sort(rng.random(n) + 0.5)[::-1]
        add('c_decades_%d' % n, ed, ed * 2.0 ** -np.floor(1000.0 * np.arange(n) / n), BIG, 'NO_WINDOW')
    n = 1000
    rng = np.random.default_rng(400)
    ei = rng.permutation(4 * n)[:n].astype(np.float64) - 2 * n
    add('d_all_1.0', ei, ei, BIG, 'LIST_OVERFLOW')
    add('d_all_0.25', ei, ei / 4, BIG, 'NO_WINDOW')
    k = np.arange(1, n // 2 + 1, dtype=np.float64)
    p = rng.permutation(n)
    add('d_bimodal', np.concatenate([-10 * k, 10 * k])[p], np.concatenate([-9 * k, 11 * k])[p], BIG, 'FAST')
    for frac, form in ((0.75, 'NO_WINDOW'), (0.5, 'FAST')):
        e, m = natural_points(n, 500 + int(100 * frac))
        e[rng.permutation(n)[:int(frac * n)]] = 0.25
        add('e_equal_%d' % int(100 * frac), e, m, BIG, form)
    for tag, order in (('pos', -1), ('neg', 1)):       # (the reference divides by e_i - e_j, i < j)
        e, m = natural_points(n, 600)
        e = np.sort(e)[::order]
        m = np.sort(m)[::order]
        m[rng.permutation(n)[:3 * n // 4]] = 0.125
        add('f_zero_' + tag, e, m, BIG, 'NO_WINDOW', status=TBA_RESCALE_FAIL)
    e, m = natural_points(n, 700, G_NOISE)
    for n_raw in G_N_RAW:
        add('g_%d' % n_raw, e, m, n_raw, None)
    e, m = natural_points(n, 800)
    add('h_far', e, m - 500.0, BIG, 'FAST')
    add('h_collinear', ei, ei - 500.0, BIG, 'LIST_OVERFLOW')
    e, m = natural_points(512, 801)
    add('h_even_512', e, m - 500.0, BIG, 'FAST')
    e, m = natural_points(n, 100 + n)                                     # (the points of a_1000)
    for tag, s, form in (('2p100', 2.0 ** 100, 'FAST'), ('2pm100', 2.0 ** -100, 'FAST'), ('2pm140', 2.0 ** -140, 'FAST'),
                         ('2pm160', 2.0 ** -160, 'LIST_OVERFLOW'), ('2p200', 2.0 ** 200, 'LIST_OVERFLOW')):
        add('i_' + tag, e * s, m * s, BIG, form)
    add('i_cancel', e + 2.0 ** 20, m, BIG, 'LIST_OVERFLOW')
    i = np.arange(961, dtype=np.float64)
    add('w_miss', 10 * i, 12 * i + 50 * (i % 10), 961 * 35, 'WINDOW_MISS')
    return cases


_cases = []


def cases():
    """every case, built once and shared (callers leave the arrays alone)"""
    if not _cases:
        _cases.extend(_build())
        for c in _cases:
            for a in (c.norm, c.segs, c.means, c.sds) + (() if c.samp_ind is None else (c.samp_ind,)):
                a.setflags(write=False)
    return _cases


def by_name(name):
    return [c for c in cases() if c.name == name][0]


def points(case):
    """(e, m) of the fit: base means over the boundaries (oracle.new_means), expected levels, the subsample applied"""
    import oracle
    e, m = oracle.new_means(case.norm, case.segs), case.means
    return (e, m) if case.samp_ind is None else (e[case.samp_ind], m[case.samp_ind])


Ref = collections.namedtuple('Ref', 'status slope inter shift_corr scale_corr slopes e m')
_refs = {}


def reference_fit(case):
    """ts.calc_kmer_fitted_shift_scale(method='theil_sen') in float64 on the CPU, once per case"""
    if case.name not in _refs:
        import oracle
        e, m = points(case)
        slopes = oracle.compute_slopes(e, m)
        slope = np.median(slopes)
        inter = np.median(m - (slope * e))
        if slope == 0:
            _refs[case.name] = Ref(TBA_RESCALE_FAIL, slope, inter, np.nan, np.nan, slopes, e, m)
        else:
            _refs[case.name] = Ref(TBA_OK, slope, inter, -inter / slope, 1 / slope, slopes, e, m)
    return _refs[case.name]


def sampled_window(e, m, cap, T=None):
    """numpy restatement of the one-pass form's sampling step for n points in read order and a list of `cap` pairs:
    the circular distances 1 + t0 * dmax / ds, the histogram of their pairs' slopes over [0.5, 1.5), the buckets at the
    sample ranks (0.5 -/+ dq) m -> (t1, t2) or None (no window), and the distances.  Exact quotients where the kernel
    takes a reciprocal and a Newton step: a slope within an ulp of a bucket edge may land on its other side."""
    T = T or constants()
    n = e.shape[0]
    ns, dmax, nb = n * (n - 1) // 2, (n - 1) // 2, T['BS_NB']
    need = (4.0 * ns / (0.6 * cap)) ** 2 / n
    ds = T['TSW_SAMPLE_MIN'] if need < T['TSW_SAMPLE_MIN'] else T['TSW_SAMPLE_DIST'] if need > T['TSW_SAMPLE_DIST'] \
        else int(need) + 1
    ds = min(ds, dmax)
    dist = [1 + (t0 * dmax) // ds for t0 in range(ds)]
    i = np.arange(n)
    sl = []
    for d in dist:
        j = (i + d) % n
        de = e - e[j]
        with np.errstate(divide='ignore', invalid='ignore'):
            sl.append(np.where(de == 0, 1000.0, (m - m[j]) / de))
    t = (np.concatenate(sl) - 0.5) * float(nb)
    bucket = np.minimum(np.maximum(t, 0.0), nb - 1.0).astype(np.int64)
    cum = np.cumsum(np.bincount(bucket, minlength=nb))
    tot = float(n * ds)
    dq = 4.0 * np.sqrt(0.25 / tot) + 0.0005
    b1, b2 = (int(np.searchsorted(cum, int(q * tot), side='right')) for q in (0.5 - dq, 0.5 + dq))
    if not (b1 > 0 and b2 >= b1 and b2 < nb - 1):
        return None, dist
    return (0.5 + b1 / float(nb), 0.5 + (b2 + 1) / float(nb)), dist


def refinement_members(slopes, k, T=None):
    """numpy restatement of the bucket select's refinement (block_kth_fe): members of rank k's bucket after each of
    BS_LEVELS levels of BS_NB uniform buckets, the first over [0.5, 1.5], the next over the members' min / max"""
    T = T or constants()
    nb, lo, hi, v, out = T['BS_NB'], 0.5, 1.5, np.asarray(slopes), []
    for _ in range(T['BS_LEVELS']):
        if not hi > lo:
            break
        t = (v - lo) * (nb / (hi - lo))
        b = np.minimum(np.maximum(t, 0.0), nb - 1.0).astype(np.int64)
        cum = np.cumsum(np.bincount(b, minlength=nb))
        bk = int(np.searchsorted(cum, k, side='right'))
        k -= int(cum[bk - 1]) if bk else 0
        v = v[b == bk]
        out.append(v.shape[0])
        lo, hi = v.min(), v.max()
    return out


def listed_pairs(e, m, win, T=None):
    """numpy restatement of what the one-pass form lists for the window `win`: the points sorted by (level, expected
    level), u1 = m - A1 e and u2 = m - B2 e rounded to float for the edges moved outwards by TSW_REL, tau = 2^-20
    max(|m| + 3 |e|) as a float; the pair i < j is below the window if u1[j] < u1[i] - tau, above it if
    u2[j] > u2[i] + tau (float arithmetic, gradual underflow), and listed otherwise -> number of list entries.  The
    pass pads the points to a multiple of 64 with u = +inf, which is never below a row and always above it -- unless the
    row's own u2 + tau is +inf or NaN (float overflow): then the row lists its padding partners too, entries that
    the exact division of the listed pairs turns into NaN and drops"""
    T = T or constants()
    o = np.lexsort((m, e))
    e, m = e[o], m[o]
    a1, b2 = win[0] - win[0] * T['TSW_REL'], win[1] + win[1] * T['TSW_REL']
    with np.errstate(all='ignore'):
        u1, u2 = (m - a1 * e).astype(np.float32), (m - b2 * e).astype(np.float32)
        tau = np.float32(2.0 ** -20 * (np.abs(m) + 3.0 * np.abs(e)).max())
        pad = np.full(-e.shape[0] % 64, np.inf, np.float32)
        lo = np.concatenate([u1, pad])[None, :] < (u1 - tau)[:, None]
        hi = np.concatenate([u2, pad])[None, :] > (u2 + tau)[:, None]
    return int(np.triu(~(lo | hi), 1).sum())

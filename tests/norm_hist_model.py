"""numpy restatement of block_hist_medians (tombo_amd/csrc/k_select.h): the float medians of the
normalisation from one histogram of the samples and one list of a few buckets' members.  Same
bucket map, same bracket, same ranks and the same value checks as the kernel; only the selection
among the listed values is a sort here.  hist_medians returns None wherever the kernel declines the
read (k_normalize's own selects take it then)."""
import numpy as np

NB = 4096            # BS_NB
CAP = 4096           # NH_CAP
N_SAMPLE = 512 * 4   # SEL_NT * WS_PER
WINDOW_MIN = 16384   # NORM_WINDOW_MIN


def bucket(v, lo, scale):
    """bs_bucket: monotone non-decreasing in v; NaN -> 0"""
    with np.errstate(invalid='ignore', over='ignore'):
        t = (np.asarray(v, np.float64) - lo) * scale
        b = np.where(t >= NB - 1, NB - 1, np.where(t > 0.0, np.minimum(t, NB - 1), 0.0))
    return np.where(np.isnan(b), 0, b).astype(np.int64)


def sample_range(x):
    n = x.size
    idx = (n * np.arange(N_SAMPLE, dtype=np.int64)) // N_SAMPLE
    s = x[idx]
    s = s[~np.isnan(s)]
    return (np.inf, -np.inf) if s.size == 0 else (s.min(), s.max())


def hist_medians(x, want_mad=True):
    """(shift, scale, med, mad, n_listed) or None"""
    x = np.asarray(x, np.float64)
    n = x.size
    if n < WINDOW_MIN:
        return None
    smn, smx = sample_range(x)
    if not smx > smn:
        return None
    with np.errstate(over='ignore'):
        hsc = NB / (smx - smn)
    if not (hsc < 1e300 and hsc > 0.0):
        return None
    # pass A
    b = bucket(x, smn, hsc)
    if np.isnan(x).any():
        return None
    P = np.concatenate(([0], np.cumsum(np.bincount(b, minlength=NB))))  # P[i + 1]: count of buckets <= i

    def cum(i):
        return 0 if i < 0 else int(P[min(i, NB - 1) + 1])
    k_lo, k_hi = (n - 1) // 2, n // 2
    bl = int(np.searchsorted(P[1:], k_lo, side='right'))
    bh = int(np.searchsorted(P[1:], k_hi, side='right'))

    def first_s(k):
        for s in range(NB):
            if cum(bh + s) - cum(bl - s - 1) >= k + 1:
                return s
    s1, s1p = first_s(k_lo), first_s(k_hi)
    la, rb = bl - s1p - 1, bh + s1p + 1
    lb, ra = bh - s1 + 1, bl + s1 - 1
    if not (bh - bl <= 1 and lb < bl and ra > bh and lb >= 0 and ra <= NB - 1):
        return None
    la, rb = max(la, 0), min(rb, NB - 1)
    n_l, n_m, n_r = cum(lb) - cum(la - 1), cum(bh) - cum(bl - 1), cum(rb) - cum(ra - 1)
    if not (n_l > 0 and n_r > 0 and n_l + n_m + n_r <= CAP):
        return None
    c_below, c_inner = cum(bl - 1), cum(ra - 1) - cum(lb)
    c_outl, c_outr = cum(la - 1), n - cum(rb)
    # pass B
    left, mid, right = x[(b >= la) & (b <= lb)], x[(b >= bl) & (b <= bh)], x[(b >= ra) & (b <= rb)]
    assert (left.size, mid.size, right.size) == (n_l, n_m, n_r)
    o_l, m_l, m_r, o_r = left.min(), left.max(), right.min(), right.max()
    kk_lo, kk_hi = k_lo - c_inner, k_hi - c_inner
    if kk_lo < 0 or kk_hi >= n_l + n_r:
        return None
    # resolve
    ms = np.sort(mid)
    xlo, xhi = ms[k_lo - c_below], ms[k_hi - c_below]
    shift = xlo if n & 1 else (xlo + xhi) / 2.0
    brk = np.concatenate((left, right))

    def deviations(g):
        with np.errstate(invalid='ignore'):
            d = np.sort(np.abs(g(brk)))
            d_lo, d_hi = d[kk_lo], d[kk_hi]
            g_l, g_r = g(m_l), g(m_r)
            ok = g_l <= 0.0 and g_r >= 0.0 and abs(g_l) <= d_lo and abs(g_r) <= d_lo
            if c_outl > 0:
                ok = ok and abs(g(o_l)) >= d_hi
            if c_outr > 0:
                ok = ok and abs(g(o_r)) >= d_hi
        return ok, d_lo, d_hi
    ok, dlo, dhi = deviations(lambda v: v - shift)
    if not ok:
        return None
    scale = dlo if n & 1 else (dlo + dhi) / 2.0
    if not scale > 0.0:
        return None
    med = mad = 0.0
    if want_mad:
        ylo, yhi = (xlo - shift) / scale, (xhi - shift) / scale
        med = ylo if n & 1 else (ylo + yhi) / 2.0
        if med == 0.0:
            m_lo, m_hi = dlo / scale, dhi / scale
        else:
            ok, m_lo, m_hi = deviations(lambda v: (v - shift) / scale - med)
            if not ok:
                return None
        mad = m_lo if n & 1 else (m_lo + m_hi) / 2.0
    return shift, scale, med, mad, n_l + n_m + n_r


def reference_medians(x):
    """ts.normalize_raw_signal, 'median' with an outlier threshold: the four medians it takes"""
    x = np.asarray(x, np.float64)
    shift = np.median(x)
    scale = np.median(np.abs(x - shift))
    norm = (x - shift) / scale
    med = np.median(norm)
    mad = np.median(np.abs(norm - med))
    return shift, scale, med, mad


def model_signal(n, seed):
    """a nanopore-like signal: one level per event (about nine samples), noise on top"""
    rng = np.random.default_rng(seed)
    dwell = 2 + rng.geometric(1.0 / 7.0, n // 4)
    levels = np.repeat(rng.normal(0.0, 1.0, dwell.size), dwell)[:n]
    return 90.0 + 12.0 * (levels + rng.normal(0.0, 0.25, n))


def variants(raw):
    """name -> (signal, what must happen to it: 'hist', 'select', or None = whatever hist_medians says) for the
    cases of the histogram medians, cut from one signal of at least 20 001 samples"""
    raw = np.asarray(raw, np.float64)
    assert raw.size >= 20001
    med, spread = np.median(raw), np.median(np.abs(raw - np.median(raw)))
    sampled = (20000 * np.arange(N_SAMPLE, dtype=np.int64)) // N_SAMPLE
    unsampled = np.setdiff1d(np.arange(20000), sampled)
    out = {}
    out['odd'] = (raw[:16385].copy(), 'hist')
    # even length, middle samples NOT symmetric around the shift (about every second length: the first such)
    n_even = next(n for n in range(20000, 19000, -2) if reference_medians(raw[:n])[2] != 0.0)
    out['even'] = (raw[:n_even].copy(), 'hist')
    # values on a 2^-10 grid: sums and halves of the middle samples are exact, the normalised median is 0
    out['even_symmetric'] = (np.round(raw[:18000] * 1024.0) / 1024.0, 'hist')
    out['coarse_grid'] = (np.round(raw[:20000] * 2.0) / 2.0, None)       # a few hundred distinct values
    ties = raw[:20001].copy()
    ties[np.argsort(np.abs(ties - med))[:6000]] = med                       # 6 000 > NH_CAP equal to the median
    out['median_bucket_over_cap'] = (ties, 'select')
    wild = raw[:20000].copy()
    wild[sampled[[100, 900, 1500]]] = med + np.array([1e6, -1e6, 2e6]) * spread
    out['wild_in_sample'] = (wild, 'select')                                # the range of the histogram is theirs
    wild = raw[:20000].copy()
    wild[unsampled[[100, 9000, 15000]]] = med + np.array([1e6, -1e6, 2e6]) * spread
    out['wild_outside_sample'] = (wild, 'hist')                             # edge buckets
    out['constant'] = (np.full(16384, 431.0), 'select')
    nan = raw[:20000].copy()
    nan[unsampled[7777]] = np.nan
    out['nan'] = (nan, 'select')
    out['short'] = (raw[:WINDOW_MIN - 1].copy(), 'select')
    return out

"""Reads that take the skipped-base stage (rq.resolve_skipped_bases_with_raw: k_skip_plan, k_skip_dp<>, k_skip_dp_wave<>
of csrc/k_tail.h) through every form it has (helper module of test_skip_cases_reference.py and test_gpu_skip_paths.py;
no tests of its own).

A case is a synthetic dpResults -- base boundaries with skipped bases, expected levels, a normalised signal -- built as
tests/golden/gen_golden_skipwin.py builds its inputs: a dwell per base, dwell[skipped] = 0, norm = repeat(means, dwell)
+ noise, a fixed seed.  What decides the form is the planner's window (n bases over L samples, admissible interval
len = L - (n - 1) m) and the number of skipped bases of the read:

    planner   at most SKP_LDS_DELS skipped bases: windows planned out of LDS; more: in the read's slice of global memory
    column    m == 1, len <= SKL_LEN, n <= SKL_N: k_skip_dp<true>, every lane its window in a column of LDS
    flat      m == 1, len <= SKL_FLAT_LEN, n ceil(len / 64) <= SKL_FLAT_WORDS: the same kernel, SKL_FLAT_N at a time
    S, M, B   m > 1, n len >= SKIP_WAVE_MIN: the three queues of k_skip_dp_wave<>
    arena     everything else: raw_window_dp over global scratch

get_deletion_windows() restates the planner in plain Python and window_class() the class decision, with the thresholds
read from the #defines of k_tail.h: a moved threshold changes what the cases reach, and test_skip_cases_reference.py
then fails on the CPU instead of a path silently going untested on the GPU.  The expected answer of every case is
oracle.resolve_skipped_bases (integers, exact).

The constructions are those of the issue that asked for these tests; the seeds are this module's own, so the counts
differ a little from the issue's table (widening: 295 windows, n from 5 to 21, three in the flat form, where the table
has 298, up to 23, one; RNA with 300 skipped bases: 292 arena + 8 S where it has 288 + 12).  The classes reached are
the same."""
import collections
import os
import re

import numpy as np

TBA_OK, TBA_NOT_ENOUGH_DEL_SIGNAL, TBA_TOO_MANY_DELS = 0, 13, 14      # include/tombo_amd.h
K_TAIL = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tombo_amd', 'csrc', 'k_tail.h')
CLASSES = ('column', 'flat', 'S', 'M', 'B', 'arena')

# kw: keyword arguments of resolve_skipped_bases_with_raw that are not the defaults; status / classes: what the oracle
# and the planner must give (classes: {class: windows}, empty for a read that fails or has no window)
Case = collections.namedtuple('Case', 'name samp segs means sds norm kw status classes')


def thresholds():
    """the integer #defines of k_tail.h that decide a window's class, expressions in other defines evaluated"""
    text = open(K_TAIL).read()
    raw = dict(re.findall(r'^#define[ \t]+((?:SKL|SKIP|SKP)_\w+)[ \t]+(\([^\n]*?\)|\d+)[ \t]*(?://.*)?$', text, re.M))
    out = {}

    def value(name):
        if name not in out:
            expr = re.sub(r'[A-Z_]{3,}\w*', lambda m: str(value(m.group(0))), raw[name])
            assert re.fullmatch(r'[\d\s()+\-*/]+', expr), (name, expr)
            out[name] = int(eval(expr.replace('/', '//')))      # (C integer division of positive values)
        return out[name]
    for name in raw:
        value(name)
    return out


def get_deletion_windows(segs, m, max_raw_cpts=200, del_fix_window=2, max_del_fix_window=10, extra_sig_factor=1.1):
    """get_deletion_windows and the checks behind it (resquiggle.py:462-498) -> (status, [(n, len)] in window order)"""
    segs = [int(x) for x in segs]
    n_segs = len(segs)
    dfw = del_fix_window

    def merged(ws):
        out = []
        for s, e in ws:
            if out and s < out[-1][1]:
                out[-1][1] = e
            else:
                out.append([s, e])
        out[0][0], out[-1][1] = max(out[0][0], 0), min(out[-1][1], n_segs - 1)
        return out

    def too_small(w):
        return segs[w[1]] - segs[w[0]] <= ((w[1] - w[0]) + 1) * m * extra_sig_factor
    ws = []
    for d in range(n_segs - 1):
        if segs[d + 1] != segs[d]:
            continue
        if ws and d < ws[-1][1] + dfw:
            ws[-1][1] = d + dfw + 1
        else:
            ws.append([d - dfw, d + dfw + 1])
    if not ws:
        return TBA_OK, []
    ws = merged(ws)
    expanded = False
    for _ in range(max_del_fix_window - dfw):
        small = [too_small(w) for w in ws]
        expanded = any(small)
        if not expanded:
            break
        ws = merged([[s - 1, e + 1] if t else [s, e] for (s, e), t in zip(ws, small)])
    if expanded and any(too_small(w) for w in ws):
        return TBA_NOT_ENOUGH_DEL_SIGNAL, []
    if max_raw_cpts is not None and max(e - s for s, e in ws) > max_raw_cpts:
        return TBA_TOO_MANY_DELS, []
    return TBA_OK, [(e - s, segs[e] - segs[s] - (e - s - 1) * m) for s, e in ws]


def window_class(n, length, m, T=None):
    """the form k_skip_plan must pick for a window of n bases over an admissible interval of `length` samples"""
    T = T or thresholds()
    words = n * ((length + 63) // 64)
    if m == 1 and length <= T['SKL_LEN'] and n <= T['SKL_N']:
        return 'column'
    if m == 1 and length <= T['SKL_FLAT_LEN'] and words <= T['SKL_FLAT_WORDS']:
        return 'flat'
    if m > 1 and n * length >= T['SKIP_WAVE_MIN'] and (n - 1) * m <= 512 and n <= 256:   # (the staged signal / levels)
        for c in 'SMB':
            if length <= T['SKIP_LEN_' + c] and words <= T['SKIP_BITS_' + c]:
                return c
    return 'arena'


def n_skipped(case):
    return int((np.diff(case.segs) == 0).sum())


def windows(case):
    """-> (status, [(n, len, class)]) of the planner's restatement under the case's own keyword arguments"""
    m = raw_min_obs(case.samp)
    status, ws = get_deletion_windows(case.segs, m, **dict(dict(max_raw_cpts=200), **case.kw))
    T = thresholds()
    return status, [(n, ln, window_class(n, ln, m, T)) for n, ln in ws]


_params = {}


def rsqgl_params(samp):
    if samp not in _params:
        from tombo_amd import tombo_stats as ts, tombo_helper as th
        _params[samp] = ts.load_resquiggle_parameters(th.seqSampleType(samp, samp == 'RNA'))
    return _params[samp]


def raw_min_obs(samp):
    return int(rsqgl_params(samp).raw_min_obs_per_base)


def oracle_result(case, **kw):
    """(status, boundaries) of oracle.resolve_skipped_bases under the case's keyword arguments, or under `kw`"""
    import oracle
    return oracle.resolve_skipped_bases(case.segs, case.norm, case.means, case.sds, oracle.make_params(rsqgl_params(case.samp)),
                                        **dict(dict(max_raw_cpts=200), **(kw or case.kw)))


def dp_results(case):
    from tombo_amd import tombo_helper as th
    return th.dpResults(read_start_rel_to_raw=0, segs=case.segs, ref_means=case.means, ref_sds=case.sds,
                        genome_seq='A' * case.means.shape[0])


def _case(name, samp, seed, nb, lo, hi, skipped, edits=(), kw=None, status=TBA_OK, classes=None):
    """dwells lo..hi - 1 per base, `edits` = ((base, dwell), ...) on top, dwell[skipped] = 0"""
    rng = np.random.default_rng(seed)
    dwell = rng.integers(lo, hi, size=nb)
    for base, d in edits:
        dwell[base] = d
    dwell[np.asarray(skipped, np.int64)] = 0
    segs = np.concatenate([[0], np.cumsum(dwell)]).astype(np.int64)
    means, sds = rng.normal(0, 1, nb), rng.uniform(0.1, 0.4, nb)
    norm = np.repeat(means, dwell) + rng.normal(0, 0.25, int(segs[-1]))
    return Case(name, samp, segs, means, sds, norm, kw or {}, status, classes or {})


def _every_8th(n_del):
    """(bases, skipped): n_del skipped bases eight apart, a window of five bases each at the default del_fix_window"""
    return 8 * n_del + 8, 4 + 8 * np.arange(n_del)


def _runs(starts, length):
    return np.concatenate([np.arange(s, s + length) for s in starts])


def _build():
    cases = []
    # DNA on both sides of SKP_LDS_DELS: one column-form window per skipped base
    for n_del in (256, 257, 300):
        nb, sk = _every_8th(n_del)
        cases.append(_case('dna_%d' % n_del, 'DNA', 100 + n_del, nb, 3, 15, sk, classes={'column': n_del}))
    nb, sk = _every_8th(300)
    # too little signal per window at first: the windows widen, some merge, three outgrow the column form (n up to 21)
    cases.append(_case('dna_300_widening', 'DNA', 11, nb, 1, 4, sk, classes={'column': 292, 'flat': 3}))
    cases.append(_case('dna_300_too_many', 'DNA', 12, nb, 3, 15, sk, kw=dict(max_raw_cpts=4), status=TBA_TOO_MANY_DELS))
    cases.append(_case('dna_300_starved', 'DNA', 13, nb, 1, 2, sk, kw=dict(max_del_fix_window=3, extra_sig_factor=4.0),
                       status=TBA_NOT_ENOUGH_DEL_SIGNAL))
    # six windows of 14 bases over about 110 samples: more than SKL_FLAT_N, a second round of the flat phase
    cases.append(_case('dna_flat_rounds', 'DNA', 14, 200, 25, 35, _runs(range(20, 200, 30), 10), classes={'flat': 6}))
    # past the flat form by flag words (64 bases x 4 words) and by length
    cases.append(_case('dna_arena_words', 'DNA', 15, 120, 70, 90, np.arange(30, 90), kw=dict(max_raw_cpts=None),
                       classes={'arena': 1}))
    cases.append(_case('dna_arena_len', 'DNA', 16, 40, 3, 15, [20], edits=[(21, 1100)], classes={'arena': 1}))
    cases.append(_case('dna_none', 'DNA', 17, 60, 3, 15, []))
    # RNA (m = 2), every form in one read: a lone skipped base between short bases (under SKIP_WAVE_MIN positions); four
    # skipped bases before long ones (S); one skipped base beside a dwell of 500 (M), 1500 (B), 2500 (past SKIP_LEN_B)
    edits = [(b, 8) for b in (18, 19, 21, 22)] + [(54, 60), (55, 60), (56, 60), (91, 500), (121, 1500), (151, 2500)]
    cases.append(_case('rna_every_form', 'RNA', 18, 200, 6, 18, [20, 50, 51, 52, 53, 90, 120, 150], edits=edits,
                       classes={'arena': 2, 'S': 1, 'M': 1, 'B': 1}))
    cases.append(_case('rna_300', 'RNA', 19, nb, 6, 18, sk, classes={'arena': 292, 'S': 8}))
    # (for the batches: a read that fails at the default arguments as well)
    cases.append(_case('rna_starved', 'RNA', 21, 400, 1, 3, 4 + 8 * np.arange(48), status=TBA_NOT_ENOUGH_DEL_SIGNAL))
    # (the same edits under another seed: in a batch each of the three queues then holds windows of more than one read)
    cases.append(_case('rna_every_form_2', 'RNA', 22, 200, 6, 18, [20, 50, 51, 52, 53, 90, 120, 150], edits=edits,
                       classes={'arena': 2, 'S': 1, 'M': 1, 'B': 1}))
    cases.append(_case('rna_none', 'RNA', 20, 60, 6, 18, []))
    return cases


_cases = []


def cases():
    """every case, built once and shared (callers leave the arrays alone)"""
    if not _cases:
        _cases.extend(_build())
        for c in _cases:
            for a in (c.segs, c.means, c.sds, c.norm):
                a.setflags(write=False)
    return _cases

"""TEST INFRASTRUCTURE: the read filters restated in numpy on plain index tuples, and the loader of the fixture
tests/golden/stats_filters.npz (gen_golden_filters.py: the live reference's outputs).  Nothing here imports
tombo_amd.filter_reads; test_filter_reference.py pins these functions to the fixture, the host-layer and GPU tests
use them and the fixture as their references.

An index here is [[chrm, strand, [record, ...]], ...] in key order, a record the tuple of the index file:
(fn, start, end, read_start_rel_to_raw, corr_grp, sub_grp, filtered, rna, sig_match_score, mean_q_score, read_id)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stats_filters.npz')
FN, START, END, RSRTR, CGRP, SGRP, FILT, RNA, SMS, MQ, RID = range(11)
PHRED_BASE = 33

_cache = {}


def fixture():
    """-> (doc, lens): the JSON document of the fixture and one uint32 array of base lengths per read (by the
    number in the read's file name)"""
    if not _cache:
        z = np.load(GOLDEN)
        off = z['lens_off']
        _cache['doc'] = json.loads(str(z['doc']))
        _cache['lens'] = [z['lens'][off[i]:off[i + 1]] for i in range(off.shape[0] - 1)]
    return _cache['doc'], _cache['lens']


def read_no(rec):
    return int(os.path.basename(rec[FN])[1:4])


def copy_index(index, all_filtered=False):
    return [[c, s, [list(r[:FILT]) + [bool(r[FILT] or all_filtered)] + list(r[FILT + 1:]) for r in recs]]
            for c, s, recs in index]


def case_index(doc, case):
    """the input index of a case, its keys in the order the reference iterated them when it recorded the case (it
    merges the indices of its directories through a set of the keys, so that order changes from run to run; the
    coverage filter's draw numbers the reads in it) -- the order of the keys of the case's output"""
    by_key = dict(((c, s), recs) for c, s, recs in doc['index'])
    return copy_index([[c, s, by_key[(c, s)]] for c, s, _ in case['out']], case['all_filtered'])


def counts_message(num_filt, prev_unfilt, total, filter_text):
    return ('Filtered {:d} reads ({:.1%} of previously filtered and '.format(num_filt, float(num_filt) / prev_unfilt) +
            '{:.1%} of all valid reads)'.format(float(num_filt) / total) +
            ' reads due to ' + filter_text + ' filter from <DIR>.')


def dwell_pctl_flags(segs, seg_off, pairs):
    """np.percentile of np.diff of every read's boundaries and the strict comparison -> (vals, flags); a read
    without lengths: NaN and True"""
    n = len(seg_off) - 1
    vals, flags = np.full((n, len(pairs)), np.nan), np.ones(n, dtype=bool)
    for i in range(n):
        lens = np.diff(np.asarray(segs[seg_off[i]:seg_off[i + 1]]))
        if lens.shape[0]:
            vals[i] = [np.percentile(lens, p) for p, _ in pairs]
            flags[i] = any(v > t for v, (_, t) in zip(vals[i], pairs))
    return vals, flags


def _flag_loop(index, is_filtered):
    out, num, prev, total = copy_index(index), 0, 0, 0
    for c, s, recs in out:
        for r in recs:
            total += 1
            if not r[FILT]:
                prev += 1
                if is_filtered(c, r):
                    num += 1
                    r[FILT] = True
    return out, (num, prev, total)


def clear(index):
    out = copy_index(index)
    for _, _, recs in out:
        for r in recs:
            r[FILT] = False
    return out


def stuck(index, obs_filter, lens, kind):
    def is_stuck(c, r):
        i = read_no(r)
        if kind[i] != 0:        # an empty table, no table, no file
            return True
        return any(np.percentile(lens[i], p) > t for p, t in obs_filter)
    return _flag_loop(index, is_stuck)


def coverage(index, frac, seed):
    out = [[c, s, [list(r) for r in recs if r[FILT]]] for c, s, recs in index]
    unfilt, cov_at, total = [], [], 0
    for k, (c, s, recs) in enumerate(index):
        cov = np.zeros(max(r[END] for r in recs), dtype=np.int64)
        for r in recs:
            total += 1
            cov[r[START]:r[END]] += 1
        for r in recs:
            if not r[FILT]:
                cov_at.append(cov[r[START] + (r[END] - r[START]) // 2])
                unfilt.append((k, r))
    prev = len(unfilt)
    num = int(frac * prev)
    cov_at = np.array(cov_at, dtype=np.float64)
    np.random.seed(seed)
    chosen = set(np.random.choice(prev, size=num, replace=False, p=cov_at / cov_at.sum()))
    for i, (k, r) in enumerate(unfilt):
        r = list(r)
        r[FILT] = i in chosen
        out[k][2].append(r)
    return out, (num, prev, total)


def qscore(index, thresh, fastq_q):
    def fails(c, r):
        if r[MQ] is not None:
            return r[MQ] < thresh
        q = fastq_q[read_no(r)]
        return True if q is None else np.mean([x - PHRED_BASE for x in q.encode('ASCII')]) < thresh
    return _flag_loop(index, fails)


def sigmatch(index, thresh, sms_attr):
    def fails(c, r):
        if r[SMS] is not None:
            return r[SMS] > thresh
        a = sms_attr[read_no(r)]
        return True if a is None else a > thresh
    return _flag_loop(index, fails)


def genome_pos(index, regs, partial):
    def outside(c, r):
        if c not in regs:
            return True
        if regs[c] is None:
            return False
        if partial:
            return not any(not (r[START] > e or r[END] < s) for s, e in regs[c])
        return not any(r[START] >= s and r[END] <= e for s, e in regs[c])
    return _flag_loop(index, outside)


def run_case(case, doc, lens):
    """the restatement of one fixture case -> (out index, counts, filter text)"""
    index = case_index(doc, case)
    f, a = case['func'], case['args']
    if f == 'clear_filters':
        return clear(index), None, None
    if f == 'filter_reads_for_stuck':
        return stuck(index, a[1], lens, doc['kind']) + ('observations per base',)
    if f == 'filter_reads_for_coverage':
        return coverage(index, a[1], case['seed']) + ('even coverage',)
    if f == 'filter_reads_for_qscore':
        return qscore(index, a[2], doc['fastq_q']) + ('q-score',)
    if f == 'filter_reads_for_signal_matching':
        return sigmatch(index, a[1], doc['sms_attr']) + ('signal matching',)
    if f == 'filter_reads_for_genome_pos':
        return genome_pos(index, a[1], a[2]) + ('genomic position',)
    raise ValueError(f)

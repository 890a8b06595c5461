"""TEST INFRASTRUCTURE: the recorded ROC computations of tests/golden/stats_roc.npz (written by
tests/golden/gen_golden_roc.py from the live reference), this project's containers holding the recorded blocks, and
the comparisons the CPU and GPU tests share.  No tolerance anywhere; NaN (the 0 / 0 rates of an all-True or all-False
set) is compared as NaN."""
import os
import json

import numpy as np

from store_memh5 import StoreGroup
from tombo_amd import tombo_stats as ts, tombo_helper as th, _native

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN = os.path.join(GOLDEN_DIR, 'stats_roc.npz')
FASTA, MOD_BED, UNMOD_BED = (os.path.join(GOLDEN_DIR, f) for f in ('roc_genome.fa', 'roc_mod.bed', 'roc_unmod.bed'))
_CACHE = {}


def gold():
    if 'g' not in _CACHE:
        with np.load(GOLDEN) as z:
            _CACHE['g'] = dict((k, z[k]) for k in z.files)
        _CACHE['meta'] = json.loads(str(_CACHE['g']['meta']))
    return _CACHE['g']


def meta():
    gold()
    return _CACHE['meta']


def js(key):
    return json.loads(str(gold()[key]))


def genome():
    if 'genome' not in _CACHE:
        _CACHE['genome'] = th.Fasta(FASTA, force_in_mem=True)
    return _CACHE['genome']


def motif_descs(key):
    return th.parse_motif_descs(meta()['motif_sets'][key])


def _store(fn):
    """a closed file of this project's containers holding the recorded blocks of `fn` -> the group"""
    if fn in _CACHE:
        return _CACHE[fn]
    g, m, grp = gold(), meta(), StoreGroup()
    layout = m['ctrl_blocks'] if fn.endswith('_ctrl') else m['blocks']
    if fn.startswith('pr'):
        pr = ts.PerReadStats(grp, 'model_compare', m['region_size'])
        for i, (chrm, strand, start, _) in enumerate(layout):
            lookup = dict(zip(g['%s_ids|%d' % (fn, i)].tolist(), g['%s_id_vals|%d' % (fn, i)].tolist()))
            pr._write_per_read_block(g['%s_block|%d' % (fn, i)], lookup, chrm, strand, start)
        pr.close()
    else:
        stat_type, region, damp, cov_thresh, n_signif = m['model_stats_args']
        ms = ts.ModelStats(grp, stat_type, region, tuple(damp), cov_thresh, n_signif)
        for i, (chrm, strand, start, _) in enumerate(layout):
            frac, poss, cov, valid = (g['%s_%s|%d' % (fn, k, i)] for k in ('frac', 'poss', 'cov', 'valid'))
            with np.errstate(invalid='ignore'):
                ms._write_stat_block(th.regionStats(frac, poss, chrm, strand, start, cov, [0] * poss.shape[0], valid))
        ms.close()
    _CACHE[fn] = grp
    return grp


def open_store(fn):
    """the container `fn` ('pr', 'pr_ctrl', 'ms', 'ms_ctrl') opened for reading"""
    return ts.PerReadStats(_store(fn)) if fn.startswith('pr') else ts.TomboStats(_store(fn))


def ground_truth():
    return th.parse_locs_file(MOD_BED), th.parse_locs_file(UNMOD_BED), 'gt'


def run_case(case, engine):
    """the recorded computation `case` through this project's method on `engine` -> {name: MotifStats}"""
    c = meta()['cases'][case]
    stats = open_store(c['store'])
    if c['kind'] == 'truth':
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            truth = ground_truth()
        return stats.compute_ground_truth_stats(truth, engine=engine)
    np.random.seed(meta()['seed'])
    if c['kind'] == 'motif':
        return stats.compute_motif_stats(motif_descs(c['motifs']), genome(), engine=engine, **c['kwargs'])
    return stats.compute_ctrl_motif_stats(open_store(c['ctrl']), motif_descs(c['motifs']), genome(), engine=engine,
                                          **c['kwargs'])


def same(a, b):
    """equal dtype-for-dtype and value-for-value, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def same_signed(a, b):
    """same() and the same sign bits (-0.0 is not 0.0)"""
    return same(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def check_case(case, res):
    g, c = gold(), meta()['cases'][case]
    assert list(res) == c['names']
    for name in c['names']:
        assert isinstance(res[name], ts.MotifStats)
        assert same_signed(res[name].stats, g['%s|%s|stat' % (case, name)]), (case, name)
        assert same(res[name].has_mod, g['%s|%s|has_mod' % (case, name)]), (case, name)


def recorded(case):
    """the recorded {name: MotifStats} of `case`"""
    g = gold()
    return dict((name, ts.MotifStats(g['%s|%s|stat' % (case, name)], g['%s|%s|has_mod' % (case, name)]))
                for name in meta()['cases'][case]['names'])


def check_rates(case, engine):
    """prep_accuracy_rates of the recorded lists of `case` (names without entries dropped, as the reference's callers
    do) against the recorded lists, AUC and mean average precision"""
    g, r = gold(), meta()['rates'][case]
    res = dict((k, v) for k, v in recorded(case).items() if len(v) > 0)
    summary = {}
    tp, fp, prec, names = ts.prep_accuracy_rates(res, engine=engine, summary=summary)
    assert same(np.array(tp, dtype=np.float64), g['rates|%s|tp' % case])
    assert same(np.array(fp, dtype=np.float64), g['rates|%s|fp' % case])
    assert same(np.array(prec, dtype=np.float64), g['rates|%s|precision' % case])
    assert names == [n for n in r['names'] for _ in range(1000)]
    assert list(summary) == list(r['summary'])
    for name, (auc, mean_ap) in r['summary'].items():
        assert same(np.float64(summary[name][0]), np.float64(float.fromhex(auc))), (case, name)
        assert same(np.float64(summary[name][1]), np.float64(float.fromhex(mean_ap))), (case, name)


def pr_store(blocks):
    grp = StoreGroup()
    pr = ts.PerReadStats(grp, 'model_compare', 100)
    for chrm, strand, start, pos, stat in blocks:
        block = np.zeros(len(pos), dtype=_native.PER_READ_DTYPE)
        block['pos'], block['stat'] = pos, stat
        pr._write_per_read_block(block, {'r': 0}, chrm, strand, start)
    pr.close()
    return ts.PerReadStats(grp)


def check_edge_rule(engine, tmp_path):
    """a motif whose window leaves the sequence does not match; the base test still applies"""
    fn = tmp_path / 'edge.fa'
    fn.write_text('>c\nGATCAAAACCAGG\n>d\nCCTGGTTTTGATC\n')       # d is the reverse complement of c
    genome = th.Fasta(str(fn))
    descs = th.parse_motif_descs('GATC:2:b::CCWGG:2:a::ATC:1:e::NGATC:3:n')
    pos = [0, 1, 2, 9, 10, 12]
    stat = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    res = pr_store([('c', '+', 0, pos, stat)]).compute_motif_stats(descs, genome, engine=engine)
    assert list(res['b']) == [(2.0, True), (5.0, False)]        # the A at 1: GATC from base 0 on, all inside
    assert list(res['a']) == [(4.0, True)]                      # the second C of CCAGG
    assert list(res['e']) == [(2.0, True), (5.0, False)]
    assert list(res['n']) == [(2.0, False), (5.0, False)]       # at 1 NGATC would start at base -1
    # the same records on the minus strand of the reverse complement: position p -> 12 - p
    res = pr_store([('d', '-', 0, [12 - p for p in pos], stat)]).compute_motif_stats(descs, genome,
                                                                                      engine=engine)
    assert list(res['b']) == [(2.0, True), (5.0, False)] and list(res['a']) == [(4.0, True)]
    assert list(res['n']) == [(2.0, False), (5.0, False)]       # NGATC would end past the last base
    # a motif that ends on the last base matches; one base longer does not
    descs = th.parse_motif_descs('CAGG:1:k::CAGGN:1:l')
    res = pr_store([('c', '+', 0, [9], [7.0])]).compute_motif_stats(descs, genome, engine=engine)
    assert list(res['k']) == [(7.0, True)] and list(res['l']) == [(7.0, False)]
    # the control form keeps matches only; AA over AAAA (bases 4-7): the sites of finditer are 4 and 6
    res = pr_store([('c', '+', 0, [1, 4, 5], [2.0, 3.0, 4.0])]).compute_ctrl_motif_stats(
        pr_store([('c', '+', 0, [1, 5, 6], [8.0, 9.0, 10.0])]), th.parse_motif_descs('GATC:2:b::AA:1:c'), genome,
        engine=engine)
    assert list(res['b']) == [(2.0, True), (8.0, False)]
    assert list(res['c']) == [(3.0, True), (10.0, False)]

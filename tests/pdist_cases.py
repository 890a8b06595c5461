"""TEST INFRASTRUCTURE: the recorded most-significant-sites computations of tests/golden/stats_pdist.npz (written by
tests/golden/gen_golden_pdist.py from the live reference), this project's containers and reads holding the recorded
inputs, and the comparisons the CPU and GPU tests share.  No tolerance anywhere."""
import io
import os
import json
import warnings

import numpy as np

import pdist_reference as ref
from store_memh5 import StoreGroup
from tombo_amd import tombo_stats as ts, tombo_helper as th, text_output

FASTA = os.path.join(os.path.dirname(ref.GOLDEN), 'roc_genome.fa')
_CACHE = {}
WINDOW_CASES = [('w27', 0), ('w27', 1), ('w27', 3), ('w140', 0), ('w140', 1), ('w140', 3), ('wbig', 0), ('wbig', 1)]


def gold():
    if 'g' not in _CACHE:
        with np.load(ref.GOLDEN) as z:
            _CACHE['g'] = dict((k, z[k]) for k in z.files)
        _CACHE['meta'] = json.loads(str(_CACHE['g']['meta']))
    return _CACHE['g']


def meta():
    gold()
    return _CACHE['meta']


def genome():
    if 'genome' not in _CACHE:
        _CACHE['genome'] = th.Fasta(FASTA, force_in_mem=True)
    return _CACHE['genome']


def open_stats(empty=False):
    """this project's ModelStats over the recorded blocks (or over none), opened for reading"""
    key = 'empty' if empty else 'ms'
    if key not in _CACHE:
        g, m, grp = gold(), meta(), StoreGroup()
        stat_type, region, damp, cov_thresh, n_signif = m['model_stats_args']
        ms = ts.ModelStats(grp, stat_type, region, tuple(damp), cov_thresh, n_signif)
        for i, (chrm, strand, start) in enumerate([] if empty else m['blocks']):
            frac, poss, cov, valid = (g['ms_%s|%d' % (k, i)] for k in ('frac', 'poss', 'cov', 'valid'))
            ms._write_stat_block(th.regionStats(frac, poss, chrm, strand, start, cov, [0] * poss.shape[0], valid))
        ms.close()
        _CACHE[key] = grp
    return ts.TomboStats(_CACHE[key])


class Read(object):
    def __init__(self, chrm, strand, start, end, seq):
        self.chrm, self.strand, self.start, self.end, self.seq = chrm, strand, start, end, seq


def reads_index():
    index = {}
    for chrm, strand, start, end, seq in meta()['reads']:
        index.setdefault((chrm, strand), []).append(Read(chrm, strand, start, end, seq))
    return index


def most_signif_text(source, num_regions, num_bases):
    fp = io.StringIO()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')   # (fewer unique locations than asked for)
        text_output.write_most_signif(open_stats(), fp, num_regions, num_bases,
                                      reads_index=reads_index() if source == 'reads' else None,
                                      genome_index=genome() if source == 'fasta' else None)
    return fp.getvalue()


def check_window_case(engine, name, slide_span):
    g = gold()
    rows = g['%s_rows' % name]
    with np.errstate(all='ignore'):
        got = ts.get_pairwise_dists(list(rows), slide_span, engine=engine)
    ref.same_bits(got, g['%s_dists_s%d' % (name, slide_span)])


def check_order_reads(engine, name):
    """the distances handed to the linkage and the leaf order of order_reads on the recorded trimmed statistics"""
    g = gold()
    stats = g['%s_trimmed' % name]
    ref.same_bits(engine.pairwise_nanmean_dists(np.ascontiguousarray(stats)), g['%s_raw_dists' % name])
    leaves = ts.order_reads(stats.copy(), engine=engine)
    assert np.array_equal(np.asarray(leaves), g['%s_leaves' % name])

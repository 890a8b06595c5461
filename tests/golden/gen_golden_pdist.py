"""Golden vectors of the most-significant-sites family from the REFERENCE (build container only).

    python tests/golden/gen_golden_pdist.py   # writes tests/golden/stats_pdist.npz

(The `stats_` prefix keeps the npz out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference, `h5py.File` pointed at the dict-backed group of tests/store_memh5.py, the Events accessor
(`th.get_single_slot_read_centric`) at in-memory arrays, `th.TomboReads` objects made around a ready index:
  get_pairwise_dists (its queues are queue.Queue)         tombo/tombo_stats.py:171-196, slide_span 0, 1 and 3
  transform_and_trim_stats                                :130-140, p-values and likelihood ratios
  order_reads                                             :142-156: the distances handed to `single` and the leaves
  ModelStats.iter_stat_seqs                               :2811-2848, both strands, windows that leave a chromosome
  th.get_unique_intervals                                 tombo/tombo_helper.py:2045-2064
  write_most_signif                                       tombo/_text_output_commands.py:395-420, reads and FASTA
Only data is written: the input matrices, the statistics blocks, the reads and the outputs.

Left out: _plot_commands.cluster_most_signif as a whole.  It hands its matrix to R through rpy2, which this image
lacks, and its statements before that are calls of the pieces recorded here (get_most_signif_regions,
get_unique_intervals over sets of covered positions, get_signal_differences, get_pairwise_dists); its column names
are therefore not recorded.

Matrices: full-mantissa random doubles (a changed summation order shows in the last bit) and rows of multiples of
1/64 that repeat with a shift, so that several window pairs tie for the minimum; a row of NaN in first and in later
windows (Python's min keeps a NaN only when it comes first).  The genome is tests/golden/roc_genome.fa."""
import io
import os
import sys
import json
import queue
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_oracle  # noqa: E402
import store_memh5  # noqa: E402

rq, ts, th = ref_oracle.load()

REGION = 100
CHRM_LENS = {'chrA': 1250, 'chrB': 830}
MODEL_STATS_ARGS = ['model_compare', REGION, [2, 1], 1, 60]
# (chrm, strand, start, positions that must be among the sites)
BLOCKS = [('chrA', '+', 0, [0, 1, 2, 7]), ('chrA', '+', 1200, [1249, 1247, 1244]), ('chrB', '-', 800, [829, 827, 822]),
          ('chrB', '-', 0, [1, 3, 6]), ('chrA', '-', 500, []), ('chrB', '+', 300, []), ('chrA', '+', 500, [])]
STORES, READ_BASES = {}, {}


def h5_file(fn, mode='r'):
    if mode == 'w':
        STORES[fn] = store_memh5.StoreGroup()
    return STORES[fn]


def install():
    ts.h5py.File = h5_file
    ts.h5py.special_dtype = lambda vlen=None: object
    ts.VERBOSE = False
    np.NAN = np.float64(np.nan)
    np.seterr(invalid='ignore')
    isfile = os.path.isfile
    os.path.isfile = lambda fn: fn in STORES or isfile(fn)
    th.get_single_slot_read_centric = lambda r, name, grp=None: READ_BASES[r.fn]


def load_text_output_commands():
    import types
    for name, attrs in (('future', {}), ('future.utils', dict(native=lambda x: x)), ('tqdm', dict(tqdm=lambda x, **kw: x)),
                        ('pkg_resources', dict(resource_string=lambda *a: b''))):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            mod.__dict__.update(attrs)
            sys.modules[name] = mod
    from tombo import _text_output_commands as toc
    toc.VERBOSE = False
    return toc


TOMBO_READS = th.TomboReads


def tombo_reads(index):
    tr = object.__new__(TOMBO_READS)
    tr.reads_index = index
    tr.coverage = None
    return tr


def ref_pairwise(rows, slide_span):
    index_q, dists_q = queue.Queue(), queue.Queue()
    for i in range(len(rows)):
        index_q.put(i)
    with np.errstate(all='ignore'):   # (squares that overflow or underflow)
        ts.get_pairwise_dists(list(rows), index_q, dists_q, slide_span)
    got = {}
    while not dists_q.empty():
        i, row = dists_q.get(block=False)
        got[i] = np.asarray(row, dtype=np.float64)
    return np.stack([got[i] for i in range(len(rows))])


def window_matrix(rng, n, row_len):
    rows = rng.standard_normal((n, row_len)) + rng.random((n, row_len)) * 1e-3
    base = rng.integers(-96, 97, row_len + 8) / 64.0
    base[row_len // 2:] = base[row_len // 2]                 # a flat stretch: many equal window sums
    for k, r in enumerate(range(2, n, 5)):
        rows[r] = base[k % 7:k % 7 + row_len]                # shifted copies: ties for the minimum, exact zeros
    rows[1] = rows[0]                                        # identical rows: distance 0
    rows[n - 1, 0] = np.nan                                  # NaN in the first window of this row only
    rows[n - 2, row_len - 1] = np.nan                        # NaN in the last windows only
    rows[n - 3, :] = 0.0
    return rows


def site_block(rng, chrm, strand, start, forced):
    hi = min(start + REGION, CHRM_LENS[chrm])
    free = np.setdiff1d(np.arange(start, hi), forced)
    poss = np.sort(np.concatenate([rng.choice(free, 14, replace=False), forced]).astype(np.int64))
    valid = rng.integers(2, 9, poss.shape[0])
    cov = valid + rng.integers(0, 3, poss.shape[0])
    frac = rng.integers(0, 9, poss.shape[0]) % (valid + 1) / valid
    frac[np.isin(poss, forced)] = 0.0                        # the forced positions are among the most significant
    return frac, poss, chrm, strand, start, cov, [0] * poss.shape[0], valid


def make_reads(rng, genome):
    """reads over parts of both chromosomes; [600, 700) of chrA and chrB '-' below 20 stay uncovered"""
    reads = []
    for chrm, n in CHRM_LENS.items():
        for strand in '+-':
            for _ in range(40):
                a = int(rng.integers(0, n - 30))
                b = int(min(n, a + rng.integers(25, 160)))
                if chrm == 'chrA' and a < 700 and b > 600:
                    continue
                if chrm == 'chrB' and strand == '-' and a < 20:
                    continue
                reads.append((chrm, strand, a, b))
    reads += [('chrA', '+', 0, 90), ('chrA', '+', 1180, 1250), ('chrB', '-', 780, 830)]
    out = []
    for chrm, strand, a, b in reads:
        fwd = genome.get_seq(chrm, a, b)
        out.append((chrm, strand, a, b, fwd if strand == '+' else th.rev_comp(fwd)))
    return out


def signed_positions(stats):
    """The stored position is a uint32.  The reference subtracts Python ints from it (:2831-2837, :2883); under the
    numpy it was written for that gave a negative int64 near a chromosome start, under numpy 2 it wraps.  The sites
    are handed to the reference's code with the position as int64, which restores the arithmetic it was written
    for; nothing else changes."""
    sites = stats.most_signif_stats
    dtype = [(n, 'i8' if n == 'pos' else sites.dtype[n]) for n in sites.dtype.names]
    stats.most_signif_stats = sites.astype(dtype)
    return stats


def main():
    install()
    toc = load_text_output_commands()
    rng = np.random.default_rng(20241020)
    out, meta = {}, {}
    # ---- get_pairwise_dists
    for name, n, row_len in (('w27', 35, 27), ('w140', 19, 140)):
        rows = window_matrix(rng, n, row_len)
        out['%s_rows' % name] = rows
        for s in (0, 1, 3):
            out['%s_dists_s%d' % (name, s)] = ref_pairwise(rows, s)
    big = rng.standard_normal((4, 9))
    big[0, :3], big[1, :3], big[2, 4] = 1e160, -1e160, 1e-170
    big[3] = 1e-170
    out['wbig_rows'] = big
    for s in (0, 1):
        out['wbig_dists_s%d' % s] = ref_pairwise(big, s)
    # ---- transform_and_trim_stats
    pvals = rng.random((12, 17)) ** 8
    pvals[rng.random(pvals.shape) < 0.15] = np.nan
    pvals[0, 0], pvals[3, 5], pvals[4, :] = 0.0, 1.0, np.nan
    llrs = rng.standard_normal((12, 17)) * 6
    llrs[rng.random(llrs.shape) < 0.15] = np.nan
    llrs[2, 2], llrs[2, 3], llrs[7, :9], llrs[8, 9:], llrs[9, :] = 25.0, -25.0, np.nan, np.nan, np.nan
    out['pvals'], out['llrs'] = pvals.copy(), llrs.copy()
    meta['pval_trim'], meta['llr_trim'] = 4.0, 10.0
    p_in, l_in = pvals.copy(), llrs.copy()
    out['pvals_trimmed'] = ts.transform_and_trim_stats(p_in, True, meta['pval_trim'])
    out['pvals_after'] = p_in
    out['llrs_trimmed'] = ts.transform_and_trim_stats(l_in, False, meta['llr_trim'])
    out['llrs_after'] = l_in
    assert out['llrs_trimmed'] is l_in and out['pvals_trimmed'] is not p_in
    # ---- order_reads: the distances before linkage, the leaves
    real_single = ts.single
    seen = []

    def recording_single(d):
        seen.append(np.array(d, dtype=np.float64))
        return real_single(d)
    ts.single = recording_single
    for name in ('pvals', 'llrs'):
        stats = out['%s_trimmed' % name]
        real_nanmax = np.nanmax
        raw = []
        ts.np.nanmax = lambda d: (raw.append(np.array(d, dtype=np.float64)), real_nanmax(d))[1]
        try:
            leaves = ts.order_reads(stats.copy())
        finally:
            ts.np.nanmax = real_nanmax
        out['%s_raw_dists' % name] = raw[0]            # pdist's result, NaN where two reads share no position
        out['%s_dists' % name] = seen.pop()
        out['%s_leaves' % name] = np.asarray(leaves, dtype=np.int64)
        assert np.isnan(raw[0]).any() and not np.isnan(out['%s_dists' % name]).any()
    out['one_read_leaves'] = np.asarray(ts.order_reads(out['llrs_trimmed'][:1].copy()), dtype=np.int64)
    ts.single = real_single
    # ---- a statistics file and its most significant sites
    genome = th.Fasta(os.path.join(HERE, 'roc_genome.fa'), force_in_mem=True)
    ms = ts.ModelStats('ms', *MODEL_STATS_ARGS)
    for i, (chrm, strand, start, forced) in enumerate(BLOCKS):
        rs = site_block(rng, chrm, strand, start, np.array(forced, dtype=np.int64))
        for k, v in zip(('frac', 'poss', 'cov', 'valid'), (rs[0], rs[1], rs[5], rs[7])):
            out['ms_%s|%d' % (k, i)] = np.asarray(v)
        ms._write_stat_block(th.regionStats(*rs))
    ms.close()
    stats = signed_positions(ts.TomboStats('ms'))
    out['most_signif_pos'] = np.array([int(p['pos']) for p in stats.most_signif_stats], dtype=np.int64)
    # ---- iter_stat_seqs
    seq_cases = {}
    for before, after in ((3, 5), (0, 0), (8, 1)):
        with_pos = [[str(s), str(c), str(st), int(a), int(b)] for s, c, st, a, b in
                    stats.iter_stat_seqs(genome, before, after)]
        seqs = [str(s) for s in stats.iter_stat_seqs(genome, before, after, include_pos=False)]
        seq_cases['%d_%d' % (before, after)] = dict(with_pos=with_pos, seqs=seqs)
        assert len(with_pos) < len(stats.most_signif_stats) or (before, after) == (0, 0)
        assert set(r[2] for r in with_pos) == {'+', '-'}
    meta['iter_stat_seqs'] = seq_cases
    # ---- get_unique_intervals
    def as_rows(intervals):
        return [[str(r.chrm), int(r.start), int(r.end), str(r.strand), str(r.reg_id), str(r.reg_text)] for r in intervals]
    uniq = {}
    regions = stats.get_most_signif_regions(11, 40)
    covered = {}
    for chrm, n in CHRM_LENS.items():
        for strand in '+-':
            c = rng.random(n) < 0.97
            c[:4] = False
            covered[(chrm, strand)] = set(int(p) for p in np.flatnonzero(c))
            out['covered|%s|%s' % (chrm, strand)] = c
    uniq['regions'] = as_rows(regions)
    uniq['plain'] = as_rows(th.get_unique_intervals(regions))
    uniq['covered'] = as_rows(th.get_unique_intervals(regions, covered))
    uniq['covered_5'] = as_rows(th.get_unique_intervals(regions, covered, 5))
    uniq['plain_3'] = as_rows(th.get_unique_intervals(regions, None, 3))
    not_unique = stats.get_most_signif_regions(11, 40, unique_pos=False)
    uniq['overlapping_regions'] = as_rows(not_unique)
    uniq['overlapping_plain'] = as_rows(th.get_unique_intervals(not_unique))
    assert len(uniq['overlapping_plain']) < len(not_unique) and len(uniq['covered']) < len(uniq['plain'])
    meta['unique_intervals'] = uniq
    # ---- write_most_signif
    reads = make_reads(rng, genome)
    index = {}
    for i, (chrm, strand, a, b, seq) in enumerate(reads):
        fn = 'read%d' % i
        READ_BASES[fn] = np.frombuffer(seq.encode(), dtype='S1')
        index.setdefault((chrm, strand), []).append(
            th.readData(a, b, False, 0, strand, fn, 'grp', False, 0.0, 10.0, fn))
    meta['reads'] = [list(r) for r in reads]
    real_reads, real_stats = th.TomboReads, ts.TomboStats
    th.TomboReads = lambda *a, **k: tombo_reads(index)
    ts.TomboStats = lambda fn: signed_positions(real_stats(fn))
    texts = {}
    try:
        for num_regions, num_bases in ((40, 9), (6, 30)):
            for source, fasta_fn in (('reads', None), ('fasta', os.path.join(HERE, 'roc_genome.fa'))):
                with tempfile.TemporaryDirectory() as td:
                    fn = os.path.join(td, 'seqs.fa')
                    toc.write_most_signif(None, fasta_fn, num_regions, 'grp', None, fn, num_bases, 'ms')
                    with io.open(fn) as fp:
                        texts['%s_%d_%d' % (source, num_regions, num_bases)] = fp.read()
    finally:
        th.TomboReads, ts.TomboStats = real_reads, real_stats
    assert '-' in texts['reads_40_9'].replace(':-', '') and texts['reads_40_9'] != texts['fasta_40_9']
    meta['most_signif_text'] = texts
    # the reference's words for an empty statistics file
    empty = ts.ModelStats('empty', *MODEL_STATS_ARGS)
    empty.close()
    err = io.StringIO()
    import contextlib
    with contextlib.redirect_stderr(err):
        try:
            ts.TomboStats('empty').get_most_signif_regions(9, 5)
            raise AssertionError('accepted')
        except SystemExit:
            pass
    meta['empty_text'] = err.getvalue()
    meta.update(region_size=REGION, chrm_lens=CHRM_LENS, blocks=[list(b[:3]) for b in BLOCKS],
                model_stats_args=MODEL_STATS_ARGS)
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'stats_pdist.npz')
    np.savez_compressed(path, **out)
    print('stats_pdist.npz %.1f KB, %d arrays' % (os.path.getsize(path) / 1024., len(out)))
    print(' sites', len(stats.most_signif_stats), 'unique', dict((k, len(v)) for k, v in uniq.items()))
    print(' iter_stat_seqs', dict((k, len(v['seqs'])) for k, v in seq_cases.items()))
    print(' leaves', out['pvals_leaves'].tolist(), out['llrs_leaves'].tolist())


if __name__ == '__main__':
    main()

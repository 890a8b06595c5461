"""Golden vectors of the statistics files from the REFERENCE (build container only).

    python tests/golden/gen_golden_stat_store.py   # writes tests/golden/stats_store.npz

(The `stats_` prefix keeps the file out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference's containers and aggregation on synthetic per-read blocks, with `h5py.File` pointed at
the dict-backed group of tests/store_memh5.py and plain list queues in place of the multiprocessing ones:
  PerReadStats._write_per_read_block                         (tombo/tombo_stats.py:3335-3366)
  _agg_stats_worker + _write_stats, run one after the other  (:4664-4725), under the three validity rules
  ModelStats / LevelStats _write_stat_block and close        (:2737-2804, :3194-3224)
  __iter__, get_pos_stat, get_reg_stats, get_most_signif_regions, PerReadStats.get_region_per_read_stats /
  get_reg_stats
  write_frac_wigs                                            (tombo/_text_output_commands.py:95-228)
Only data is written: the blocks, the flattened trees, the accessor results and the file texts.

Two places where the reference's accessors cannot be recorded: iter_most_signif_sites (:2850-2859) indexes the
statistic's value with the slot name and raises, and get_reg_stats (:3060) stacks blocks with np.vstack, which
raises for blocks of different lengths; the requests recorded here each lie inside one block.

All statistics are multiples of 1/64, some of them exactly a threshold: every comparison and every count is
exact, a fraction is one division, so the recorded outputs are compared without a tolerance."""
import os
import sys
import json
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
from tombo import _text_output_commands as toc  # noqa: E402

REGION = 100
PER_READ_DTYPE = [('pos', 'u4'), ('stat', 'f8'), ('read_id', 'u4')]
# per-read blocks in the order they are stored: (chrm, strand, start, kind).  Three (chrm, strand) keys; the
# first stored key's blocks are out of start order.
# (Starts from 1000 on: get_most_signif_regions subtracts half a window from the stored uint32 position, :2883, which
# under this numpy wraps below 0 instead of going negative.)
BLOCKS = [('chr2', '+', 1300, 'mixed'), ('chr2', '+', 1100, 'edges'), ('chr1', '+', 1200, 'mixed'),
          ('chr1', '+', 1000, 'deep'), ('chr1', '-', 1100, 'empty'), ('chr1', '-', 1000, 'mixed'),
          ('chr1', '+', 1100, 'sorted'), ('chr2', '+', 1000, 'thin')]
# aggregations: name -> (stat type, single_read_thresh, lower_thresh, cov_damp_counts, num_most_signif)
AGGS = {'lower': ('de_novo', 0.5, 0.15625, (0, 0), 60),      # valid coverage 0 -> NaN damp_frac, row dropped
        'abs': ('model_compare', 2.0, None, (2, 0), 45),
        'all': ('de_novo', 0.5, None, (2, 0), 100000),       # fewer sites than num_most_signif
        'lower_damp': ('model_compare', 2.5, -1.5, (1, 3), 45)}
STORES = {}


class ListQueue(list):
    put = list.append

    def get(self, block=True):
        if not self:
            raise ts.queue.Empty
        return self.pop(0)


def h5_file(fn, mode='r'):
    if mode == 'w':
        STORES[fn] = store_memh5.StoreGroup()
    return STORES[fn]


def install():
    ts.h5py.File = h5_file
    ts.h5py.special_dtype = lambda vlen=None: object
    ts.VERBOSE = toc.VERBOSE = False
    # `running_most_signif_sites[:] = np.NAN` (:2625) fills unsigned fields too: this numpy refuses the Python
    # float there and takes the numpy scalar (with a warning), as the numpy of the reference's time did
    np.NAN = np.float64(np.nan)
    np.seterr(invalid='ignore')
    isfile = os.path.isfile
    os.path.isfile = lambda fn: fn in STORES or isfile(fn)


def make_block(rng, start, kind, llr):
    """records of one block; stats multiples of 1/64: p-value-like in [0, 1] or log-likelihood-ratio-like"""
    def stats(n):
        v = rng.integers(0, 65, n) / 64.0
        return (v * 10 - 5) if llr else v
    if kind == 'empty':
        pos = np.zeros(0, dtype=np.int64)
    elif kind == 'edges':      # a record at the first and at the last position, coverage 1 there
        pos = np.concatenate([[start, start + REGION - 1], rng.integers(start + 1, start + REGION - 1, 300)])
    elif kind == 'deep':       # coverage 70 at one site, coverage 1 at another
        inner = rng.integers(start, start + REGION, 250)
        inner = inner[(inner != start + 40) & (inner != start + 41)]
        pos = np.concatenate([np.full(70, start + 40), [start + 41], inner])
    elif kind == 'thin':       # coverage 1-2: many equal fractions
        pos = rng.choice(np.arange(start, start + REGION), 60, replace=False)
        pos = np.concatenate([pos, pos[:25]])
    else:
        pos = rng.integers(start, start + REGION, 400)
    if kind == 'sorted':
        pos = np.sort(pos)
    elif kind != 'empty':
        pos = rng.permutation(pos)
    block = np.empty(pos.shape[0], dtype=PER_READ_DTYPE)
    block['pos'], block['stat'] = pos, stats(pos.shape[0])
    n_reads = 12
    block['read_id'] = rng.integers(0, n_reads, pos.shape[0])
    # exact threshold values (the three thresholds of AGGS for this statistic)
    for k, v in enumerate((2.0, 2.5, -1.5) if llr else (0.5, 0.15625)):
        if block.shape[0] > 10:
            block['stat'][3 + k::37] = v
    lookup = dict(('read_%s_%d_%02d' % (kind, start, i), i) for i in range(n_reads))
    return block, lookup


def put_tree(out, name, group):
    t = store_memh5.flat_tree(group)
    out[name + '_keys'] = np.array(json.dumps(list(t)))
    for k, v in t.items():
        out['%s|%s' % (name, k)] = v


def read_texts(td, base):
    return dict((f, open(os.path.join(td, f)).read()) for f in sorted(os.listdir(td)) if f.startswith(base + '.'))


def record_accessors(out, name, stats, requests):
    """the reference's read accessors of an open (read mode) ModelStats / LevelStats"""
    blocks = list(stats)
    out[name + '_iter'] = np.array(json.dumps([[c, s, int(a), int(b)] for c, s, a, b, _ in blocks]))
    for i, blk in enumerate(blocks):
        out['%s_iter|%d' % (name, i)] = blk[4]
    out[name + '_pos_stat_req'] = np.array(json.dumps(requests['pos']))
    out[name + '_pos_stat'] = np.array([stats.get_pos_stat(c, s, p, missing_value=-7.0) for c, s, p in requests['pos']],
                                       dtype=np.float64)
    out[name + '_reg_req'] = np.array(json.dumps(requests['reg']))
    for i, (c, s, a, b) in enumerate(requests['reg']):
        r = stats.get_reg_stats(c, s, a, b)
        out['%s_reg|%d' % (name, i)] = np.zeros(0) if r is None else r
        out['%s_reg_none|%d' % (name, i)] = np.array(r is None)
    regs = {}
    for key, (nb, nr, uniq, prep) in requests['signif'].items():
        regs[key] = [[r.chrm, int(r.start), int(r.end), r.strand, r.reg_id, r.reg_text] for r in
                     stats.get_most_signif_regions(nb, nr, unique_pos=uniq, prepend_loc_to_text=prep)]
    out[name + '_signif_req'] = np.array(json.dumps(requests['signif']))
    out[name + '_signif'] = np.array(json.dumps(regs))


REQUESTS = {
    'pos': [['chr1', '+', 1040], ['chr1', '+', 1041], ['chr2', '+', 1100], ['chr2', '+', 1199], ['chr1', '-', 1150],
            ['chr3', '+', 1005], ['chr1', '+', 1950]],
    'reg': [['chr1', '+', 1010, 1060], ['chr2', '+', 1150, 1200], ['chr1', '-', 1100, 1200], ['chr3', '+', 1000, 1050],
            ['chr1', '+', 1900, 1950], ['chr2', '+', 1300, 1400]],
    'signif': {'a': [20, 8, True, False], 'b': [7, 1000, True, True], 'c': [10, 5, False, True]},
}


def main():
    install()
    rng = np.random.default_rng(20240611)
    out = {}
    meta = dict(region_size=REGION, blocks=BLOCKS, aggs=AGGS, min_test_reads=1)
    # ---- per-read files, one per statistic type
    pr_blocks = {}
    for stat_type in ('de_novo', 'model_compare'):
        fn = 'pr_' + stat_type
        pr = ts.PerReadStats(fn, stat_type, REGION)
        for i, (chrm, strand, start, kind) in enumerate(BLOCKS):
            block, lookup = make_block(rng, start, kind, stat_type == 'model_compare')
            out['%s_block|%d' % (fn, i)] = block
            out['%s_ids|%d' % (fn, i)] = np.array(list(lookup.keys()))
            out['%s_id_vals|%d' % (fn, i)] = np.array(list(lookup.values()))
            pr._write_per_read_block(block, lookup, chrm, strand, start)
        pr.close()
        put_tree(out, fn, STORES[fn])
        pr = ts.PerReadStats(fn)
        blocks = list(pr)
        out[fn + '_iter'] = np.array(json.dumps([[c, s, int(a), int(b)] for c, s, a, b, _ in blocks]))
        for i, blk in enumerate(blocks):
            out['%s_iter|%d' % (fn, i)] = blk[4]
        out[fn + '_reg_req'] = np.array(json.dumps(REQUESTS['reg']))
        for i, (c, s, a, b) in enumerate(REQUESTS['reg']):
            r = pr.get_reg_stats(c, s, a, b)
            out['%s_reg|%d' % (fn, i)] = np.zeros(0) if r is None else r
            out['%s_reg_none|%d' % (fn, i)] = np.array(r is None)
            r = pr.get_region_per_read_stats(th.intervalData(chrm=c, start=a, end=b, strand=s))
            out['%s_region_none|%d' % (fn, i)] = np.array(r is None)
            if r is not None:
                out['%s_region_pos|%d' % (fn, i)] = r['pos']
                out['%s_region_stat|%d' % (fn, i)] = r['stat']
                out['%s_region_id|%d' % (fn, i)] = r['read_id'].astype(str)
        pr_blocks[stat_type] = blocks
        pr.close()
    # ---- aggregation under the three validity rules: the worker's raw outputs, then the written file
    sizes = {}
    for name, (stat_type, single, lower, damp, n_signif) in AGGS.items():
        pr_q, stats_q = ListQueue(), ListQueue()
        for c, s, a, b, blk in pr_blocks[stat_type]:
            pr_q.put((c, s, a, b, blk.copy()))
        pr_q.put(None)
        ts._agg_stats_worker(pr_q, stats_q, stat_type, single, lower)
        for i, item in enumerate(stats_q[:-1]):
            (frac, cov, ctrl_cov, valid), c, s, start, poss = item
            out['agg_%s_frac|%d' % (name, i)], out['agg_%s_cov|%d' % (name, i)] = frac, cov
            out['agg_%s_valid|%d' % (name, i)], out['agg_%s_poss|%d' % (name, i)] = valid, poss
            with np.errstate(invalid='ignore'):
                out['agg_%s_damp|%d' % (name, i)] = ts.calc_damp_fraction(
                    dict(zip(('unmod', 'mod'), damp)), frac, valid)
            out['agg_%s_n_ctrl|%d' % (name, i)] = np.array(len(ctrl_cov))
        fn = 'agg_' + name
        with np.errstate(invalid='ignore'):
            ts._write_stats(stats_q, fn, stat_type, REGION, damp, 1, n_signif, len(BLOCKS), 1)
        put_tree(out, fn, STORES[fn])
        signif = STORES[fn]['Most_Significant_Stats']['Most_Significant_Stats'][:]
        every = np.sort(np.concatenate([b['block_stats'][:]['damp_frac'] for b in STORES[fn]['Statistic_Blocks'].values()]))
        sizes[name] = (int(signif.shape[0]), int(every.shape[0]))
        if n_signif < every.shape[0]:
            assert every[n_signif - 1] == every[n_signif], ('the cut must lie inside a tie', name)
        if name == 'lower':
            raw = sum(out['agg_lower_poss|%d' % i].shape[0] for i in range(len(BLOCKS)))
            assert every.shape[0] < raw, 'no site without valid coverage'
        stats = ts.TomboStats(fn)
        assert stats.is_model_stats
        record_accessors(out, fn, stats, REQUESTS)
        with tempfile.TemporaryDirectory() as td:
            cwd = os.getcwd()
            os.chdir(td)
            try:
                toc.write_frac_wigs(ts.TomboStats(fn), 'st', True, True, False, True, None, None)
            finally:
                os.chdir(cwd)
            out[fn + '_wigs'] = np.array(json.dumps(read_texts(td, 'st')))
    assert sizes['all'][0] == sizes['all'][1] < AGGS['all'][4]
    # ---- ModelStats written directly, blocks of the first sorted key out of start order, in several batch sizes
    direct = [('chr1', '+', 1200), ('chr1', '+', 1000), ('chr2', '-', 1000), ('chr1', '+', 1100), ('chr1', '-', 1300)]
    reg_stats = []
    for i, (c, s, start) in enumerate(direct):
        n = (30, 45, 0, 25, 38)[i]
        poss = np.sort(rng.choice(np.arange(start, start + REGION), n, replace=False))
        valid = rng.integers(0, 5, n)
        cov = valid + rng.integers(0, 3, n)
        with np.errstate(invalid='ignore'):
            frac = np.where(valid > 0, rng.integers(0, 5, n) % (valid + 1) / np.maximum(valid, 1), np.nan)
        ctrl = rng.integers(0, 9, n + 3).tolist()
        reg_stats.append((frac, poss, c, s, start, cov, ctrl, valid))
        for k, v in zip(('frac', 'poss', 'cov', 'ctrl', 'valid'), (frac, poss, cov, np.array(ctrl), valid)):
            out['direct_%s|%d' % (k, i)] = v
    meta['direct'] = direct
    meta['direct_args'] = dict(stat_type='sample_compare', cov_damp_counts=(2, 1), cov_thresh=3, num_most_signif=50)
    for n_batches in (1, 2, 10):
        fn = 'direct_b%d' % n_batches
        ms = ts.ModelStats(fn, 'sample_compare', REGION, (2, 1), 3, 50, most_signif_num_batches=n_batches)
        for r in reg_stats:
            with np.errstate(invalid='ignore'):
                ms._write_stat_block(th.regionStats(*r))
        ms.close()
        put_tree(out, fn, STORES[fn])
    assert all(store_memh5.same_array(out['direct_b1|' + k[len('direct_b2|'):]], out[k])
               for k in out if k.startswith('direct_b2|'))
    stats = ts.TomboStats('direct_b10')
    record_accessors(out, 'direct_b10', stats, REQUESTS)
    with tempfile.TemporaryDirectory() as td:
        cwd = os.getcwd()
        os.chdir(td)
        try:
            toc.write_frac_wigs(ts.TomboStats('direct_b10'), 'st', True, True, False, True, None, None)
        finally:
            os.chdir(cwd)
        out['direct_b10_wigs'] = np.array(json.dumps(read_texts(td, 'st')))
    # ---- LevelStats
    level = [('chr1', '+', 1100), ('chr1', '+', 1000), ('chr1', '-', 1000)]
    meta['level'] = level
    meta['level_args'] = dict(region_size=REGION, cov_thresh=2, num_most_signif=40)
    grp_stats = []
    for i, (c, s, start) in enumerate(level):
        n = (40, 35, 20)[i]
        poss = np.sort(rng.choice(np.arange(start, start + REGION), n, replace=False))
        st = rng.integers(0, 9, n) / 8.0           # many ties, some exact zeros (-log10 -> inf)
        st[rng.integers(0, n, 4)] = np.nan
        cov, ctrl = rng.integers(2, 30, n), rng.integers(2, 30, n)
        grp_stats.append((st, poss, c, s, start, cov, ctrl))
        for k, v in zip(('stat', 'poss', 'cov', 'ctrl'), (st, poss, cov, ctrl)):
            out['level_%s|%d' % (k, i)] = v
    for stat_type in ('ks_test', 'u_stat_test', 'ks_stat_test'):
        fn = 'level_' + stat_type
        ls = ts.LevelStats(fn, stat_type, REGION, 2, 40)
        for g in grp_stats:
            ls._write_stat_block(th.groupStats(*g))
        ls.close()
        put_tree(out, fn, STORES[fn])
        stats = ts.TomboStats(fn)
        assert not stats.is_model_stats
        with np.errstate(divide='ignore'):
            record_accessors(out, fn, stats, REQUESTS)
            with tempfile.TemporaryDirectory() as td:
                cwd = os.getcwd()
                os.chdir(td)
                try:
                    toc.write_frac_wigs(ts.TomboStats(fn), 'st', False, False, True, False, None, None)
                finally:
                    os.chdir(cwd)
                out[fn + '_wigs'] = np.array(json.dumps(read_texts(td, 'st')))
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'stats_store.npz')
    np.savez_compressed(path, **out)
    n_rec = sum(v.shape[0] for k, v in out.items() if k.startswith('pr_') and '_block|' in k)
    print('stats_store.npz %.1f KB, %d arrays, %d records, most significant / sites: %s' % (
        os.path.getsize(path) / 1024., len(out), n_rec, sizes))


if __name__ == '__main__':
    main()

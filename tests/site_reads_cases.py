"""TEST INFRASTRUCTURE: the inputs and comparisons that tests/test_site_reads_host_layer.py (numpy stand-in
engine) and tests/test_gpu_site_reads.py (device) share for `compute_reg_stats_reads_batch` and
`test_significance`.  The oracle throughout is the route that exists without them: `compute_reg_stats_batch`
(per-read preparation in Python) and `write_stats_from_regions`."""
import numpy as np

from tombo_amd import tombo_stats as ts, tombo_helper as th
from tombo_amd import _native
import site_stats_reference as ssr
from stats_cases import site_key, check_site_region
from store_memh5 import StoreGroup, flat_tree, same_array

REGION = 100
DAMP = (2, 0)


def make_read(genome, model, rng, start, end, strand, read_id, shift_frac=0.3, means=True):
    """a read over genome[start:end]: levels of the model under its own sequence plus noise (a shift on some)"""
    seq = genome[start:end]
    seq = th.rev_comp(seq) if strand == '-' else seq
    n, K, cp = end - start, model.kmer_width, model.central_pos
    m = rng.normal(0.0, 1.0, n)
    codes = ts.encode_seq(seq).astype(np.int64)
    for i in range(cp, n - (K - cp - 1)):
        w = codes[i - cp:i - cp + K]
        if (w < 4).all():
            km = int(sum(int(c) * 4 ** (K - 1 - j) for j, c in enumerate(w)))
            m[i] = model.level_means[km] + rng.normal(0.0, 1.2) * model.level_sds[km] + 1.5 * (rng.random() < shift_frac)
    return th.resquiggledRead(start, end, False, 0, strand, None, None, False, read_id=read_id,
                              means=m if means else None, seq=seq)


def seeded_index(model, seed=7, per_strand=20, shift_frac=0.3, tag='s'):
    """{('chr1', strand): reads}: per strand `per_strand` reads of 150-400 bases inside [1000, 1600), each spanning
    2-4 regions of REGION positions"""
    rng = np.random.default_rng(seed)
    genome = ''.join(rng.choice(list('ACGT'), 1700))
    index = {}
    for strand in '+-':
        reads = []
        while len(reads) < per_strand:
            n = int(rng.integers(150, 401))
            s = int(rng.integers(1000, 1600 - n + 1))
            if not 2 <= (s + n - 1) // REGION - s // REGION + 1 <= 4:
                continue
            reads.append(make_read(genome, model, rng, s, s + n, strand, '%s%s%d' % (tag, strand, len(reads)), shift_frac))
        index[('chr1', strand)] = reads
    return index


def index_regions(index, starts, ctrl_index=None, size=REGION):
    """regions [start, start + size) of (chrm, strand, start) triples with the reads add_reads selects"""
    regs = [th.intervalData(c, s, s + size, st).add_reads(index) for c, st, s in starts]
    if ctrl_index is None:
        return regs, None
    return regs, [r.copy(include_reads=False).add_reads(ctrl_index) for r in regs]


def failing_index(model, fm):
    """reads index, control index and region triples of the failing-pair cases (see test_failing_pairs)"""
    rng = np.random.default_rng(11)
    K, cp = model.kmer_width, model.central_pos
    dn = K - cp - 1
    g = list(''.join(rng.choice(list('ACGT'), 1500)))
    g[1150] = 'N'
    g1 = ''.join(g)
    g2 = list(''.join(rng.choice(list('ACGT'), 1200)))
    g2[1060] = 'N'
    g2 = ''.join(g2)
    g3 = ''.join(rng.choice(list('ACGT'), 1200))
    mk = lambda gen, s, e, st, rid, **kw: make_read(gen, model, rng, s, e, st, rid, **kw)   # noqa: E731
    a_b = 1100                                   # start of region B
    plus = [mk(g1, 990, 1410, '+', 'G1'), mk(g1, 1005, 1395, '+', 'G2'), mk(g1, 1050, 1350, '+', 'G3'),
            mk(g1, 1050, 1190, '+', 'N1'),                                   # N at 1150: inside B's clip only
            mk(g1, 1010, a_b + 1, '+', 'K1'),                                # one base of B: shorter than K there
            mk(g1, 1020, a_b - fm + dn + 2 * fm, '+', 'F4'),                 # de_novo: 2 fm statistics in B
            mk(g1, 1020, a_b - fm + dn + 2 * fm + 1, '+', 'F5'),             # de_novo: 2 fm + 1
            mk(g1, 1020, a_b - fm + 2 * fm, '+', 'S4'),                      # sample_compare: 2 fm in B
            mk(g1, 1020, a_b - fm + 2 * fm + 1, '+', 'S5'),                  # sample_compare: 2 fm + 1
            mk(g1, 1030, 1180, '+', 'M1', means=False),
            mk(g1, 1375, 1420, '+', 'X1')]                                   # control ends at 1370
    minus = [mk(g1, 990, 1210, '-', 'GM1'), mk(g1, 1000, 1200, '-', 'GM2'), mk(g1, 1050, 1190, '-', 'NM'),
             mk(g1, 1020, a_b - fm + cp + 2 * fm, '-', 'FM4'), mk(g1, 1020, a_b - fm + cp + 2 * fm + 1, '-', 'FM5')]
    index = {('c1', '+'): plus, ('c1', '-'): minus,
             ('c2', '+'): [mk(g2, 1040, 1090, '+', 'P1')],                   # the only read of its region, N at 1060
             ('c3', '+'): [mk(g3, 1010, 1090, '+', 'Q1')]}                   # no control reads on c3
    ctrl = {('c1', '+'): [mk(g1, 980 + i, 1370 - i, '+', 'C%d' % i, shift_frac=0.0) for i in range(3)],
            ('c1', '-'): [mk(g1, 980 + i, 1220, '-', 'CM%d' % i, shift_frac=0.0) for i in range(3)],
            ('c2', '+'): [mk(g2, 1000, 1035 - i, '+', 'CP%d' % i, shift_frac=0.0) for i in range(3)]}
    starts = [('c1', '+', s) for s in (1000, 1100, 1200, 1300)] + [('c1', '-', 1000), ('c1', '-', 1100),
                                                                   ('c2', '+', 1000), ('c3', '+', 1000)]
    return index, ctrl, starts


def oracle_pair_errors(regions, stat_type, model, fm, levels=None):
    """per region [(read, None or the TomboError message of the oracle's per-read preparation)]"""
    out = []
    for r, reg in enumerate(regions):
        rows = []
        for rd in reg.reads:
            try:
                if stat_type == ts.DE_NOVO_TXT:
                    ts._prep_de_novo_read(rd, model, fm, reg)
                elif levels[r] is None:
                    continue
                else:
                    ts._prep_sample_compare_read(rd, *levels[r], fm, reg)
                rows.append((rd, None))
            except th.TomboError as e:
                rows.append((rd, str(e)))
        out.append(rows)
    return out


class Capture(object):
    """wraps an engine's site_fractions_reads: keeps the arguments and what came back of every call"""

    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def site_fractions_reads(self, *args, **kw):
        out = self.eng.site_fractions_reads(*args, **kw)
        self.calls.append((args, out))
        return out


def run_both(regions, ctrl_regions, fm, stat_type, model, engine, min_test_reads=2, single=0.3, lower=0.05,
             prior_weights=None, use_ref=False):
    """-> ((results, per-read blocks) of the oracle route, the same of compute_reg_stats_reads_batch)"""
    std_ref = model if stat_type == ts.DE_NOVO_TXT or use_ref else None
    args = (regions, fm, min_test_reads, single, lower, ctrl_regions, std_ref, None, False, stat_type, prior_weights)
    want = ts.compute_reg_stats_batch(*args, cov_damp_counts=DAMP, return_per_read=True, engine=engine)
    got = ts.compute_reg_stats_reads_batch(*args, cov_damp_counts=DAMP, return_per_read=True, engine=engine)
    return want, got


def _same_bytes(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def check_same(want, got):
    """results and per-read blocks of two routes: the same errors, the same bytes -> regions with statistics"""
    (w_res, w_pr), (g_res, g_pr) = want, got
    assert len(w_res) == len(g_res) == len(w_pr) == len(g_pr)
    n = 0
    for w, g in zip(w_res, g_res):
        if isinstance(w, Exception):
            assert type(g) is type(w) and str(g) == str(w)
            continue
        assert not isinstance(g, Exception), g
        assert [k for k, _ in g] == [k for k, _ in w]
        for (_, a), (_, b) in zip(w, g):
            assert (a.chrm, a.strand, a.start) == (b.chrm, b.strand, b.start)
            assert list(a.ctrl_cov) == list(b.ctrl_cov)
            for x, y in zip((a.reg_frac_standard_base, a.reg_poss, a.reg_cov, a.valid_cov, a.damp_frac),
                            (b.reg_frac_standard_base, b.reg_poss, b.reg_cov, b.valid_cov, b.damp_frac)):
                assert _same_bytes(x, y)
        n += 1
    for w, g in zip(w_pr, g_pr):
        assert len(w) == len(g)
        for (wn, (wb, wl, *wrest)), (gn, (gb, gl, *grest)) in zip(w, g):
            assert wn == gn and wrest == grest and list(wl.items()) == list(gl.items())
            assert _same_bytes(wb, gb)
    return n


# ---- test_significance -------------------------------------------------------------------------
def oracle_signif(index, stat_type, fm, model, engine, ctrl_index=None, alt_refs=None, per_read=False, max_stats=None,
                  min_test_reads=2, single=0.3, lower=0.05, use_ref=False):
    """today's route over the batches of `iter_signif_region_batches`: compute_reg_stats_batch (the group tests:
    compute_group_reg_stats_batch) and write_stats_from_regions -> {file name: StoreGroup}"""
    std_ref = model if stat_type != ts.SAMP_COMP_TXT or use_ref else None
    kw = {} if max_stats is None else dict(max_stats_per_call=max_stats)
    level = stat_type in ts.LEVEL_STATS_TXTS
    stat_fns, pr_fns = ts.signif_store_names(stat_type, 'out', 'out' if per_read else None, alt_refs)
    stores = dict((fn, StoreGroup()) for fn in list(stat_fns.values()) + list(pr_fns.values()))
    if level:
        stats = dict((n, ts.LevelStats(stores[fn], stat_type, REGION, min_test_reads, 50)) for n, fn in stat_fns.items())
    else:
        stats = dict((n, ts.ModelStats(stores[fn], stat_type, REGION, DAMP, min_test_reads, 50)) for n, fn in stat_fns.items())
    prs = dict((n, ts.PerReadStats(stores[fn], stat_type, REGION)) for n, fn in pr_fns.items())
    n_batches = 0
    for regs, ctrls in ts.iter_signif_region_batches(index, stat_type, REGION, fm, ctrl_index, std_ref, alt_refs,
                                                     engine=engine, **kw):
        n_batches += 1
        if level:
            for res in ts.compute_group_reg_stats_batch(regs, ctrls, fm, min_test_reads, stat_type, engine):
                for name, gs in res:
                    stats[name]._write_stat_block(gs)
            continue
        res, blocks = ts.compute_reg_stats_batch(regs, fm, min_test_reads, single, lower, ctrls, std_ref, alt_refs, False,
                                                 stat_type, None, return_per_read=True, engine=engine)
        for name in stat_fns:   # one statistic name per file
            ts.write_stats_from_regions(
                [r if isinstance(r, Exception) else [x for x in r if x[0] == name] for r in res],
                [[b for b in bl if b[0] == name] for bl in blocks], stats[name], prs.get(name))
    for c in list(stats.values()) + list(prs.values()):
        c.close()
    return stores, n_batches


def run_signif(index, stat_type, fm, model, engine, ctrl_index=None, alt_refs=None, per_read=False, max_stats=None,
               min_test_reads=2, single=0.3, lower=0.05, use_ref=False):
    std_ref = model if stat_type != ts.SAMP_COMP_TXT or use_ref else None
    kw = {} if max_stats is None else dict(max_stats_per_call=max_stats)
    stat_fns, pr_fns = ts.signif_store_names(stat_type, 'out', 'out' if per_read else None, alt_refs)
    stores = dict((fn, StoreGroup()) for fn in list(stat_fns.values()) + list(pr_fns.values()))
    ts.test_significance(index, stat_type, 'out', REGION, 4, min_test_reads, 50, 'out' if per_read else None, single,
                         lower, DAMP, fm, ctrl_index, std_ref, alt_refs, False, None, engine=engine, stores=stores, **kw)
    return stores


def check_same_stores(want, got):
    """two {file name: StoreGroup}: the same files, every file closed, the same tree (paths in order, dtypes, values)
    -> number of blocks"""
    assert list(want) == list(got)
    n = 0
    for fn in want:
        assert got[fn].closed
        a, b = flat_tree(want[fn]), flat_tree(got[fn])
        assert list(a) == list(b), fn
        assert all(same_array(a[k], b[k]) for k in a), fn
        n += sum(1 for k in a if k.endswith('/block_stats'))
    return n


# ---- the checks both test files run, on their engine ---------------------------------------------
Z_TYPES = (ts.DE_NOVO_TXT, ts.SAMP_COMP_TXT)


_GOLDEN_REGIONS = {}


def golden_case_args(gold, meta, model, c, which=None):
    if c['fm'] not in _GOLDEN_REGIONS:   # (built once per fm_offset: nothing below changes a region)
        _GOLDEN_REGIONS[c['fm']] = ssr.golden_regions(gold, th, c['fm'], model.kmer_width)
    samp, ctrl = _GOLDEN_REGIONS[c['fm']]
    if which is not None:
        samp, ctrl = [samp[i] for i in which], [ctrl[i] for i in which]
    return (samp, c['fm'], meta['min_test_reads'], c['single'], c['lower'], ctrl, model if c['use_ref'] else None,
            None, False, c['stat_type'], None)


def check_golden(gold, meta, model, engine, stat_type, at_once):
    """every case of `stat_type` in stats_site.npz against the live reference's results, all regions at once (then
    the per-read blocks against compute_reg_stats_batch byte for byte, too) or one at a time -> names checked"""
    n = 0
    for c in meta['cases']:
        if c['stat_type'] != stat_type:
            continue
        key = lambda ri: (site_key(c, ri), int(gold['reg_start'][ri]), '-' if gold['reg_minus'][ri] else '+')   # noqa: E731
        if not at_once:
            for ri in range(gold['reg_start'].shape[0]):
                one = ts.compute_reg_stats_reads_batch(*golden_case_args(gold, meta, model, c, [ri]), engine=engine)
                k, start, strand = key(ri)
                n += check_site_region(gold, k, one[0], start, strand)
            continue
        args = golden_case_args(gold, meta, model, c)
        got = ts.compute_reg_stats_reads_batch(*args, cov_damp_counts=meta['cov_damp_counts'], return_per_read=True,
                                               engine=engine)
        want = ts.compute_reg_stats_batch(*args, cov_damp_counts=meta['cov_damp_counts'], return_per_read=True,
                                          engine=engine)
        check_same(want, got)
        for ri, res in enumerate(got[0]):
            k, start, strand = key(ri)
            n += check_site_region(gold, k, res, start, strand, damp=True)
    return n


def check_shared_reads(model, engine, fm):
    index, ctrl = seeded_index(model), seeded_index(model, seed=8, shift_frac=0.0, tag='c')
    starts = [('chr1', st, s) for st in '+-' for s in range(1000, 1600, REGION)]
    regs, ctrls = index_regions(index, starts, ctrl)
    n_reads = sum(len(v) for v in index.values())
    n = 0
    for stat_type in Z_TYPES:
        cap = Capture(engine)
        n += check_same(*run_both(regs, ctrls, fm, stat_type, model, cap))
        (args, _), = cap.calls                          # one call, and its reads table holds every read once
        assert args[3].shape[0] == n_reads and args[9].shape[0] == sum(len(r.reads) for r in regs) > 2 * n_reads
        assert np.unique(args[9]).shape[0] == n_reads
        assert args[6].shape[0] == int(args[5][-1]) == sum(rd.end - rd.start for v in index.values() for rd in v)
    return n


def check_failing_pairs(model, engine):
    """Every way a pair fails, each shown to fail in the oracle's per-read preparation too; the pair_ok the
    engine returns against the oracle pair by pair; results and per-read blocks against the oracle route."""
    fm, min_reads = 2, 2
    index, ctrl, starts = failing_index(model, fm)
    regs, ctrls = index_regions(index, starts, ctrl)
    need = {ts.DE_NOVO_TXT: ['Invalid sequence encountered', 'does not contain information in this region',
                             'too short for Fisher', 'valid re-squiggled data'],
            ts.SAMP_COMP_TXT: ['No valid z-scores in read', 'too short for Fisher', 're-squiggled level means']}
    for stat_type in Z_TYPES:
        cap = Capture(engine)
        want, got = run_both(regs, ctrls, fm, stat_type, model, cap, min_test_reads=min_reads)
        check_same(want, got)
        levels = None
        if stat_type == ts.SAMP_COMP_TXT:
            levels = ts._ctrl_levels(ctrls, min_reads, fm, None, None, engine)[0]
        rows = oracle_pair_errors(regs, stat_type, model, fm, levels)
        msgs = [m for reg_rows in rows for _, m in reg_rows]
        for text in need[stat_type]:
            assert any(m is not None and text in m for m in msgs), (stat_type, text)
        (args, (res, pair_ok, pair_pos, pair_off)), = cap.calls
        # the pairs are the oracle's pairs without the reads that have no levels, in order
        oracle_ok = [m is None for reg_rows in rows for rd, m in reg_rows if rd.means is not None]
        assert pair_ok.astype(bool).tolist() == oracle_ok
        assert sum(oracle_ok) >= (len(oracle_ok) + 1) // 2 and sum(oracle_ok) < len(oracle_ok)
        # the Fisher guard exactly: a pair of 2 fm statistics failed, one of 2 fm + 1 did not
        pair_ids = [rd.read_id for reg_rows in rows for rd, _ in reg_rows if rd.means is not None]
        pair_reg = [r for r, reg_rows in enumerate(rows) for rd, _ in reg_rows if rd.means is not None]
        short, enough = ('F4', 'F5') if stat_type == ts.DE_NOVO_TXT else ('S4', 'S5')
        p4, p5 = (next(p for p, (i, r) in enumerate(zip(pair_ids, pair_reg)) if i == rid and r == 1) for rid in (short, enough))
        t = _native._check_site_reads_args(0 if stat_type == ts.DE_NOVO_TXT else 1, *args[1:13])
        bound = _native.site_reads_stat_bound(0 if stat_type == ts.DE_NOVO_TXT else 1, t, model.kmer_width, model.central_pos)
        assert (bound[p4], pair_ok[p4]) == (2 * fm, 0) and (bound[p5], pair_ok[p5]) == (2 * fm + 1, 1)
        assert np.array_equal(np.diff(pair_off), np.where(pair_ok == 1, bound, 0))
        # N1: inside the clip in region B, outside it in region A -> the read counts in A only
        if stat_type == ts.DE_NOVO_TXT:
            n1 = [pair_ok[p] for p, i in enumerate(pair_ids) if i == 'N1']
            assert n1 == [1, 0]
        # whole regions: all pairs failed / a control region without reads
        errs = [str(r) for r in got[0] if isinstance(r, Exception)]
        assert 'Reads contains no statistics in this region.' in errs
        assert (ts._NO_READS_MSG in errs) == (stat_type == ts.SAMP_COMP_TXT)


DRIVER_CASES = [(ts.DE_NOVO_TXT, False, False), (ts.DE_NOVO_TXT, True, False), (ts.SAMP_COMP_TXT, True, True),
                (ts.ALT_MODEL_TXT, True, False), (ts.KS_TEST_TXT, False, False)]


def check_driver(model, alt_refs, engine, stat_type, per_read, use_ref, fm=1):
    index, ctrl = seeded_index(model), seeded_index(model, seed=8, shift_frac=0.0, tag='c')
    needs_ctrl = stat_type == ts.SAMP_COMP_TXT or stat_type in ts.LEVEL_STATS_TXTS
    kw = dict(ctrl_index=ctrl if needs_ctrl else None, alt_refs=alt_refs if stat_type == ts.ALT_MODEL_TXT else None,
              per_read=per_read, use_ref=use_ref)
    want, n_batches = oracle_signif(index, stat_type, fm, model, engine, **kw)
    got = run_signif(index, stat_type, fm, model, engine, **kw)
    n = check_same_stores(want, got)
    want_1, n_single = oracle_signif(index, stat_type, fm, model, engine, max_stats=1, **kw)
    assert n_batches == 1 and n_single >= 12       # one region per call
    check_same_stores(want, want_1)
    check_same_stores(want, run_signif(index, stat_type, fm, model, engine, max_stats=1, **kw))
    names = ts.signif_store_names(stat_type, 'out', 'out' if per_read else None, kw['alt_refs'])
    assert list(got) == list(names[0].values()) + list(names[1].values())
    return n


def base_args():
    """a small valid (form 0) argument set of site_fractions_reads in the order of _check_site_reads_args"""
    return dict(form=0, reg_start=np.array([100, 200], dtype=np.int64), reg_end=np.array([200, 300], dtype=np.int64),
                read_start=np.array([90, 150], dtype=np.int64), read_strand=np.array([0, 1], dtype=np.int8),
                read_off=np.array([0, 60, 260], dtype=np.int64), means=np.zeros(260), seq=np.zeros(260, dtype=np.uint8),
                reg_pair_off=np.array([0, 2, 3], dtype=np.int64), pair_read=np.array([0, 1, 1], dtype=np.int64),
                pos_means=None, pos_sds=None, fm_offset=1)


BAD_ARGS = [dict(form=2), dict(fm_offset=65), dict(fm_offset=-1), dict(reg_end=np.array([200, 200], dtype=np.int64)),
            dict(read_off=np.array([1, 60, 260], dtype=np.int64)), dict(read_off=np.array([0, 270, 260], dtype=np.int64)),
            dict(reg_pair_off=np.array([0, 3, 2], dtype=np.int64)), dict(pair_read=np.array([0, 1, 2], dtype=np.int64)),
            dict(pair_read=np.array([0, -1, 1], dtype=np.int64)), dict(read_strand=np.array([0, 2], dtype=np.int8)),
            dict(pair_read=np.array([0, 1, 0], dtype=np.int64)),       # read 0 ends at 150: not in region [200, 300)
            dict(seq=None), dict(means=np.zeros(259)), dict(means=np.zeros(260, dtype=np.float32)),
            dict(reg_start=np.array([100, 200 - 2 ** 31], dtype=np.int64)), dict(form=1)]

"""Golden vectors of the ROC / precision-recall computations from the REFERENCE (build container only).

    python tests/golden/gen_golden_roc.py   # writes tests/golden/stats_roc.npz, roc_genome.fa, roc_mod.bed, roc_unmod.bed

(The `stats_` prefix keeps the npz out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference on a synthetic genome and synthetic statistics files, with `h5py.File` pointed at the
dict-backed group of tests/store_memh5.py:
  ModelStats / PerReadStats .compute_motif_stats, .compute_ground_truth_stats, .compute_ctrl_motif_stats
                                                              (tombo/tombo_stats.py:2406-2535)
  compute_accuracy_rates, compute_auc, compute_mean_avg_precison   (:2377-2404)
  prep_accuracy_rates                                         (tombo/_plot_commands.py:60-82)
  parse_locs_file, parse_motif_descs, Fasta.get_seq           (tombo/tombo_helper.py:475-506, 710-730, 813-850)
Only data is written: the blocks, the (statistic, has_mod) lists, the sampled rates, the parsed locations, the
sequences and the message texts.

Per-read statistics are multiples of 1/64 with many ties, 0.0 and -0.0 among them and values shared by modified and
unmodified records; per-site fractions are single divisions.  Nothing is compared with a tolerance.

No record lies within max(before_bases, after_bases) of a chromosome start, and no minus-strand record that close to
a chromosome end: there the reference slices its window with a negative offset, or reverse-complements a
truncated one, and reads bases that are not the record's (checked below)."""
import io
import os
import sys
import json
import contextlib
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
PER_READ_DTYPE = [('pos', 'u4'), ('stat', 'f8'), ('read_id', 'u4')]
CHRM_LENS = {'chrA': 1250, 'chrB': 830}
MARGIN = 4      # at least max(before_bases, after_bases) of every motif set below
# blocks in stored order: (chrm, strand, start, records).  The first stored key's blocks are out of start order;
# one block is empty; chrB + 800 reaches the chromosome end (830) and holds a record on its last base.
BLOCKS = [('chrA', '+', 300, 260), ('chrA', '+', 100, 240), ('chrA', '-', 200, 250), ('chrB', '-', 100, 0),
          ('chrB', '+', 800, 90), ('chrA', '-', 1100, 230), ('chrB', '+', 700, 220), ('chrA', '+', 0, 150)]
# control blocks: some of the sample's blocks have none
CTRL_BLOCKS = [('chrA', '+', 100, 200), ('chrA', '+', 300, 180), ('chrA', '-', 200, 210), ('chrB', '+', 800, 60),
               ('chrA', '-', 1100, 150), ('chrA', '+', 0, 100)]
# ('dup': two motifs under one name share a list)
MOTIF_SETS = {'cg': 'CG:1:x', 'two': 'CCWGG:2:a::GATC:2:b', 'self': 'AA:1:c', 'dup': 'CG:1:x::GC:2:x::AA:1:x'}
SEED, PER_BLOCK, LIMIT, CTRL_LIMIT = 7, 50, 700, 60
STORES = {}


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


def make_genome(rng):
    seqs = {}
    for chrm, n in CHRM_LENS.items():
        s = rng.choice(list('ACGT'), n)
        for at, word in ((130, 'CCAGG'), (160, 'GATC'), (225, 'CCTGGATC'), (330, 'AAAAAAA'), (352, 'CCAGGG'),
                         (420, 'NNNNNN'), (470, 'GATCGATC'), (731, 'AAAAA'), (760, 'CCTGG'), (815, 'CGCGATCCAGG'),
                         (1150, 'GATCCWGGNCG'), (1190, 'AAAAAAAAAA')):
            if at + len(word) <= n:
                s[at:at + len(word)] = list(word)
        s[n - 3:] = list('CGA')        # a CG whose G is the second last base, an A on the last
        s = ''.join(s)
        seqs[chrm] = s[:250] + s[250:290].lower() + s[290:600] + s[600:640].lower() + s[640:]
    return seqs


def write_fasta(path, seqs):
    with open(path, 'w') as fp:
        for chrm, s in seqs.items():
            fp.write('>%s synthetic\n' % chrm)
            for a in range(0, len(s), 60):
                fp.write(s[a:a + 60] + '\n')


def block_positions(rng, chrm, strand, start, n):
    lo = max(start, MARGIN)
    hi = min(start + REGION, CHRM_LENS[chrm] - (MARGIN if strand == '-' else 0))
    pos = rng.integers(lo, hi, n)
    if n and strand == '+' and start + REGION > CHRM_LENS[chrm]:
        pos[:3] = CHRM_LENS[chrm] - 1, CHRM_LENS[chrm] - 2, CHRM_LENS[chrm] - 3
    return pos


def per_read_block(rng, chrm, strand, start, n):
    block = np.empty(n, dtype=PER_READ_DTYPE)
    block['pos'] = block_positions(rng, chrm, strand, start, n)
    block['stat'] = rng.integers(-40, 41, n) / 64.0 * rng.choice([1, 8], n)
    block['stat'][5::17] = 0.0
    block['stat'][9::23] = -0.0
    block['read_id'] = rng.integers(0, 9, n)
    return block, dict(('read_%s_%s_%d_%d' % (chrm, strand, start, i), i) for i in range(9))


def site_block(rng, chrm, strand, start, n):
    """regionStats inputs of one ModelStats block: distinct positions"""
    lo = max(start, MARGIN)
    hi = min(start + REGION, CHRM_LENS[chrm] - (MARGIN if strand == '-' else 0))
    n = min(n // 4, hi - lo)
    poss = np.sort(rng.choice(np.arange(lo, hi), n, replace=False))
    if n and strand == '+' and start + REGION > CHRM_LENS[chrm]:
        poss = np.unique(np.concatenate([poss, [CHRM_LENS[chrm] - 1, CHRM_LENS[chrm] - 2]]))
    valid = rng.integers(1, 6, poss.shape[0])
    cov = valid + rng.integers(0, 3, poss.shape[0])
    frac = rng.integers(0, 6, poss.shape[0]) % (valid + 1) / valid
    return frac, poss, chrm, strand, start, cov, [0] * poss.shape[0], valid


def check_margins(blocks, pos_of):
    for (chrm, strand, start, _), blk in blocks:
        pos = pos_of(blk).astype(np.int64)
        assert np.all(pos >= MARGIN), 'record at a chromosome start'
        if strand == '-':
            assert np.all(pos < CHRM_LENS[chrm] - MARGIN), 'minus-strand record at a chromosome end'


def put_result(out, case, res):
    """the reference's {name: [(stat, bool), ...]}"""
    for name, pairs in res.items():
        out['%s|%s|stat' % (case, name)] = np.array([float(p[0]) for p in pairs], dtype=np.float64)
        out['%s|%s|has_mod' % (case, name)] = np.array([bool(p[1]) for p in pairs], dtype=np.bool_)
    return list(res)


def load_plot_commands():
    """tombo._plot_commands with stand-ins for the modules it imports and this image lacks (none is used by
    prep_accuracy_rates)"""
    import types
    for name, attrs in (('future', {}), ('future.utils', dict(native=lambda x: x)), ('tqdm', dict(tqdm=lambda x, **kw: x)),
                        ('pkg_resources', dict(resource_string=lambda *a: b''))):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            mod.__dict__.update(attrs)
            sys.modules[name] = mod
    from tombo import _plot_commands as pc
    return pc


def main():
    install()
    pc = load_plot_commands()
    pc.VERBOSE = False
    rng = np.random.default_rng(20241019)
    out, cases = {}, {}
    seqs = make_genome(rng)
    fasta_fn = os.path.join(HERE, 'roc_genome.fa')
    write_fasta(fasta_fn, seqs)
    genome = th.Fasta(fasta_fn, force_in_mem=True)
    descs = dict((k, th.parse_motif_descs(v)) for k, v in MOTIF_SETS.items())
    for d in descs.values():
        motifs = [m for m, _ in d]
        assert max(max(m.mod_pos - 1, m.motif_len - m.mod_pos) for m in motifs) <= MARGIN
    # ---- BED files: one location in both lists, a repeated line, two malformed lines
    bed = {'mod': [], 'unmod': []}
    for chrm, strand, start, _ in BLOCKS:
        for k in range(12):
            bed['mod' if k % 3 == 0 else 'unmod'].append((chrm, start + 5 + 7 * k, strand))
    bed['unmod'].append(bed['mod'][2])
    bed['mod'].append(bed['mod'][0])
    for key, rows in bed.items():
        with open(os.path.join(HERE, 'roc_%s.bed' % key), 'w') as fp:
            for i, (chrm, pos, strand) in enumerate(rows):
                fp.write('%s\t%d\t%d\tloc%d\t0\t%s\n' % (chrm, pos, pos + 1, i, strand))
            if key == 'mod':
                fp.write('chrA\tnot_a_number\t5\tbad\t0\t+\nchrA\t12\n')
    locs, warn_text = {}, {}
    for key in bed:
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            locs[key] = th.parse_locs_file(os.path.join(HERE, 'roc_%s.bed' % key))
        warn_text[key] = err.getvalue()
        out['locs_%s_keys' % key] = np.array(json.dumps([list(cs) for cs in locs[key]]))
        for cs, v in locs[key].items():
            out['locs_%s|%s|%s' % ((key,) + cs)] = np.asarray(v)
    bad_fn = os.path.join(HERE, 'roc_bad.bed')
    with open(bad_fn, 'w') as fp:
        fp.write('chrA\tx\n')
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        assert th.parse_locs_file(bad_fn) == {}
    warn_text['all_bad'] = err.getvalue()
    os.remove(bad_fn)
    ground_truth = (locs['mod'], locs['unmod'], 'gt')
    # ---- containers: per-read sample / control, per-site sample / control
    blocks = {}
    for fn, layout in (('pr', BLOCKS), ('pr_ctrl', CTRL_BLOCKS)):
        pr = ts.PerReadStats(fn, 'model_compare', REGION)
        blocks[fn] = []
        for i, (chrm, strand, start, n) in enumerate(layout):
            block, lookup = per_read_block(rng, chrm, strand, start, n)
            blocks[fn].append(((chrm, strand, start, n), block))
            out['%s_block|%d' % (fn, i)] = block
            out['%s_ids|%d' % (fn, i)] = np.array(list(lookup.keys()))
            out['%s_id_vals|%d' % (fn, i)] = np.array(list(lookup.values()))
            pr._write_per_read_block(block, lookup, chrm, strand, start)
        pr.close()
        check_margins(blocks[fn], lambda b: b['pos'])
    for fn, layout in (('ms', BLOCKS), ('ms_ctrl', CTRL_BLOCKS)):
        ms = ts.ModelStats(fn, 'model_compare', REGION, (2, 1), 1, 50)
        blocks[fn] = []
        for i, (chrm, strand, start, n) in enumerate(layout):
            rs = site_block(rng, chrm, strand, start, n)
            blocks[fn].append(((chrm, strand, start, n), rs))
            for k, v in zip(('frac', 'poss', 'cov', 'valid'), (rs[0], rs[1], rs[5], rs[7])):
                out['%s_%s|%d' % (fn, k, i)] = np.asarray(v)
            ms._write_stat_block(th.regionStats(*rs))
        ms.close()
        check_margins(blocks[fn], lambda rs: rs[1])
    # ---- the three computations
    results = {}
    for fn, ctrl_fn, opener in (('pr', 'pr_ctrl', ts.PerReadStats), ('ms', 'ms_ctrl', ts.TomboStats)):
        for key, d in descs.items():
            variants = {'plain': {}}
            if fn == 'pr':
                variants.update(sub=dict(stats_per_block=PER_BLOCK), limit=dict(total_stats_limit=LIMIT),
                                sub_limit=dict(stats_per_block=PER_BLOCK, total_stats_limit=200))
            for vname, kw in variants.items():
                case = 'motif_%s_%s_%s' % (fn, key, vname)
                np.random.seed(SEED)
                res = opener(fn).compute_motif_stats(d, genome, **kw)
                cases[case] = dict(kind='motif', store=fn, motifs=key, kwargs=kw, names=put_result(out, case, res))
                results[case] = res
            for vname, kw in (('plain', {}), ('limit', dict(total_stats_limit=CTRL_LIMIT))):
                case = 'ctrl_%s_%s_%s' % (fn, key, vname)
                res = opener(fn).compute_ctrl_motif_stats(opener(ctrl_fn), d, genome, **kw)
                cases[case] = dict(kind='ctrl', store=fn, ctrl=ctrl_fn, motifs=key, kwargs=kw,
                                   names=put_result(out, case, res))
                results[case] = res
        case = 'truth_%s' % fn
        res = opener(fn).compute_ground_truth_stats(ground_truth)
        cases[case] = dict(kind='truth', store=fn, names=put_result(out, case, res))
        results[case] = res
    n_plain = sum(len(v) for v in results['motif_pr_cg_plain'].values())
    assert sum(len(v) for v in results['motif_pr_cg_limit'].values()) < n_plain, 'the limit must stop mid-file'
    assert len(results['ctrl_pr_cg_limit']['x']) < len(results['ctrl_pr_cg_plain']['x'])
    assert any(p[1] for p in results['truth_pr']['gt']) and not all(p[1] for p in results['truth_pr']['gt'])
    # ---- the numbers that go into the plots
    rates = {}
    for case, res in results.items():
        res = dict((k, v) for k, v in res.items() if len(v) > 0)     # (as the reference's callers do)
        if not res:
            continue
        tp, fp, prec, names = pc.prep_accuracy_rates(res)
        out['rates|%s|tp' % case], out['rates|%s|fp' % case] = np.array(tp, dtype=np.float64), np.array(fp, dtype=np.float64)
        out['rates|%s|precision' % case] = np.array(prec, dtype=np.float64)
        summary = {}
        for name, pairs in res.items():
            ordered = list(zip(*sorted(pairs)))[1]
            t, f, p = ts.compute_accuracy_rates(ordered)
            summary[name] = [float(ts.compute_auc(t, f)).hex(), float(ts.compute_mean_avg_precison(t, p)).hex()]
        rates[case] = dict(names=[str(n) for n in names[::ts.ROC_PLOT_POINTS]], summary=summary)
    ordered = np.array(list(zip(*sorted(results['motif_pr_cg_plain']['x'])))[1])
    for n, points in ((ordered.shape[0], 1000), (37, 1000), (37, 10), (1, 5)):
        t, f, p = ts.compute_accuracy_rates(ordered[:n], points)
        for k, v in zip('tfp', (t, f, p)):
            out['acc|%d|%d|%s' % (n, points, k)] = v
    out['acc_ordered'] = ordered
    # ---- host pieces
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        try:
            th.parse_motif_descs('CG:1')
            raise AssertionError('accepted')
        except SystemExit:
            pass
    seq_reqs = [['chrA', 0, 10], ['chrA', 240, 300], ['chrA', 1240, 1300], ['chrB', 415, 430], ['chrB', 830, 840],
                ['chrA', None, None]]
    seq_errs = [['chrA', -1, 5, True], ['chrA', 1251, 1260, False], ['chrA', 1240, 1251, True]]
    for c, a, b, e in seq_errs:
        try:
            genome.get_seq(c, a, b, error_end=e)
            raise AssertionError('accepted')
        except th.TomboError as exc:
            seq_err_text = str(exc)
    meta = dict(region_size=REGION, chrm_lens=CHRM_LENS, blocks=BLOCKS, ctrl_blocks=CTRL_BLOCKS, motif_sets=MOTIF_SETS,
                seed=SEED, cases=cases, rates=rates, warn_text=warn_text, motif_err_text=err.getvalue(),
                parsed_motifs=dict((k, [[m.raw_motif, m.mod_pos, m.mod_base, n] for m, n in d]) for k, d in descs.items()),
                seq_reqs=seq_reqs, seqs=[genome.get_seq(c, a, b, error_end=False) for c, a, b in seq_reqs],
                seq_errs=seq_errs, seq_err_text=seq_err_text, chrms=list(genome.iter_chrms()),
                has_rna_bases=bool(genome.has_rna_bases), model_stats_args=['model_compare', REGION, [2, 1], 1, 50])
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'stats_roc.npz')
    np.savez_compressed(path, **out)
    print('stats_roc.npz %.1f KB, %d arrays, %d cases, %d rate sets' % (
        os.path.getsize(path) / 1024., len(out), len(cases), len(rates)))
    for case in sorted(results):
        print(' ', case, dict((k, (len(v), sum(p[1] for p in v))) for k, v in results[case].items()))


if __name__ == '__main__':
    main()

"""Golden vectors of `tombo plot kmer` and of the model overlay / per-read statistic frames from the REFERENCE (build
container only).

    python tests/golden/gen_golden_kmer_dist.py   # writes tests/golden/stats_kmer_dist.npz

(The `stats_` prefix keeps the npz out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference (tools/ref_oracle.py) with
  th.TomboReads                           a list of in-memory reads
  th.get_multiple_slots_read_centric      pointed at their arrays (norm_mean, base)
  np.random.shuffle                       the identity: the reads are taken in the order given
  _plot_commands.r                        a stand-in whose DataFrame returns a dict of numpy columns and which records
                                          factor levels and r.r(...) / r.globalenv[...](...) calls
  _plot_commands.importr                  succeeds, so that baseDat is built
  th.error_message_and_exit / warning_message   recorded
and records what plot_kmer_dist (_plot_commands.py:451-559) hands to R for every case of kmer_dist_cases().

The model overlay and per-read statistic frames run on the scenario of gen_golden_plot_data.py (same seed, so the
same reads bit for bit; th.is_sample_rna answers False, _R_DF.rbind concatenates columns) plus three reads over an
N: get_reg_kmers :1435 and get_model_r_data :1034 for models whose central_pos is below, equal to and above the
downstream bases, with and without an alternate model and min_reg_overlap; what plot_model_single_sample :1592,
plot_motif_centered_with_stats :1526 and plot_per_read_modification :1638 hand to R.

Only data is written: the reads (levels, sequences, raw values, segments), the model tables, the cases and the
recorded frames."""
import os
import sys
import json
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_oracle  # noqa: E402
import gen_golden_plot_data as gpd  # noqa: E402  (load_plot_commands: the reference module with its imports shimmed)

rq, ts, th = gpd.rq, gpd.ts, gpd.th


class Exit(Exception):
    pass


class Recorder(object):
    """the stand-in `r`: frames become dicts of numpy arrays; factor levels, r.r / r.globalenv calls are kept"""
    NA_Character = 'NA_character_'

    def __init__(self):
        self.calls, self.messages, self.factor_levels = [], [], []
        self.globalenv = self

    DataFrame = staticmethod(lambda d: d)
    FloatVector = staticmethod(lambda v: np.array([float(x) for x in v], dtype=np.float64))
    IntVector = staticmethod(lambda v: np.array([int(x) for x in v], dtype=np.int64))
    StrVector = staticmethod(lambda v: np.array([str(x) for x in v], dtype='U'))
    BoolVector = staticmethod(lambda v: [bool(x) for x in v])

    def FactorVector(self, v, ordered=True, levels=None):
        assert ordered
        self.factor_levels.append([str(x) for x in levels])
        return np.array([str(x) for x in v], dtype='U')

    def r(self, text):
        self.calls.append(('r', text))

    def __getitem__(self, name):
        return lambda *args: self.calls.append((name, args))


class FrameBinder(object):
    """_R_DF.rbind of two recorded frames"""
    @staticmethod
    def rbind(f1, f2):
        return dict((k, np.concatenate([f1[k], f2[k]])) for k in f1)


def random_seq(rng, n):
    return ''.join('ACGT'[i] for i in rng.integers(0, 4, n))


def counts_of(seq, K):
    out = {}
    for i in range(len(seq) - K + 1):
        out[seq[i:i + K]] = out.get(seq[i:i + K], 0) + 1
    return out


def rare_cg_read(rng, n_cg):
    """a read that shows all 16 2-mers, CG exactly n_cg times and every other one more often than 8 times"""
    body = list(random_seq(rng, 420))
    for i in range(1, len(body)):
        if body[i - 1] == 'C' and body[i] == 'G':
            body[i] = 'A'
    seq = ''.join(body) + 'A' + 'CGA' * n_cg
    c = counts_of(seq, 2)
    assert len(c) == 16 and c['CG'] == n_cg and min(v for k, v in c.items() if k != 'CG') > 8
    return seq


def make_pool(rng):
    """-> [(name, levels or None, sequence)]"""
    full = (lambda n: rng.standard_normal(n) + rng.random(n) * 1e-3)
    pool = []
    for i in range(6):
        seq = random_seq(rng, 400 + 13 * i)
        assert len(counts_of(seq, 2)) == 16 and min(counts_of(seq, 2).values()) > 6
        pool.append(('rand%d' % i, full(len(seq)), seq))
    body = list(random_seq(rng, 300))
    for i in range(1, len(body)):
        if body[i - 1] == 'T' and body[i] == 'T':
            body[i] = 'C'
    assert len(counts_of(''.join(body), 2)) == 15
    pool.append(('no_tt', full(300), ''.join(body)))
    for n in (1, 2, 3, 4):
        pool.append(('short%d' % n, full(n), random_seq(rng, n)))
    for n_cg in (2, 3, 5, 6):
        seq = rare_cg_read(rng, n_cg)
        pool.append(('cg%d' % n_cg, full(len(seq)), seq))
    # about 8 300 bases, all but 40 of them A: one segment of more than 8192 levels at K = 1 and K = 2
    body = ['A'] * 8300
    for i in rng.choice(np.arange(5, 8290, 7), 40, replace=False):
        body[i] = 'CGT'[int(rng.integers(0, 3))]
    seq = ''.join(body)
    assert counts_of(seq, 1)['A'] > 8192 and counts_of(seq, 2)['AA'] > 8192
    pool.append(('homopolymer', full(8300), seq))
    # equal means: every A and every C level of the two reads is a multiple of 1/64 with mean 0.5 exactly
    for i in range(2):
        seq = 'ACGT' * 12
        lv = rng.integers(-40, 41, len(seq)) / 64.0
        lv[0::4] = np.tile([0.25, 0.75], 6)
        lv[1::4] = np.tile([0.75, 0.25, 0.5], 4)
        pool.append(('tie%d' % i, lv, seq))
    for i in range(2):
        seq = random_seq(rng, 2600)
        assert len(counts_of(seq, 4)) == 256 and len(counts_of(seq, 3)) == 64 and min(counts_of(seq, 3).values()) > 5
        pool.append(('long%d' % i, full(2600), seq))
    pool.append(('no_levels', None, random_seq(rng, 50)))
    return pool


def kmer_dist_cases(names):
    """[(case name, read names, read_mean, upstrm_bases, dnstrm_bases, kmer_thresh, num_reads)]"""
    rand = ['rand%d' % i for i in range(6)]
    cases = []
    for rm in (True, False):
        t = 'mean' if rm else 'raw'
        cases += [
            ('k1_%s' % t, rand[:3], rm, 0, 0, 1, 3),
            ('k2_up0_%s' % t, rand[:3], rm, 0, 1, 2, 3),
            ('k2_up1_%s' % t, rand[:3] + ['no_levels'], rm, 1, 0, 5, 3),
            ('k3_up1_%s' % t, rand[:2], rm, 1, 1, 0, 2),
            ('tie_%s' % t, ['tie0', 'tie1'], rm, 0, 0, 1, 2),
            ('short_k2_%s' % t, ['short1', 'rand0', 'short2', 'short3', 'rand1'], rm, 0, 1, 0, 5),
            ('num_reads_reached_%s' % t, [rand[0], 'no_tt', rand[1], rand[2], rand[3]], rm, 1, 0, 1, 2),
        ]
    cases += [
        ('k3_up0', ['long0', 'long1'], True, 0, 2, 1, 2), ('k3_up2', ['long0', 'long1', rand[0]], True, 2, 0, 5, 2),
        ('k4_up0', ['long0', 'long1'], True, 0, 3, 1, 2), ('k4_up2', ['long0', 'short3', 'short4', 'long1'], True, 2, 1, 0, 4),
        ('k4_up3_thresh1', ['long0', rand[0], 'long1'], True, 3, 0, 1, 3),
        ('k4_up1_raw', ['short4', rand[0], rand[1]], False, 1, 2, 0, 3),
        ('short_k3', ['short2', 'short3', 'rand0', 'short4', 'rand1'], True, 1, 1, 0, 9),
        ('short_k4', ['short3', 'short4', 'rand0', 'rand1'], False, 3, 0, 0, 4),
        # the rarest 2-mer exactly kmer_thresh times: rejected; kmer_thresh + 1 times: accepted
        ('rare_thresh2', ['cg2', 'cg3', rand[0], 'cg5'], True, 0, 1, 2, 4),
        ('rare_thresh5', ['cg5', 'cg6', 'cg3', rand[0], 'cg2'], True, 1, 0, 5, 5),
        ('rare_thresh1', ['cg2', 'no_tt', 'cg3'], False, 0, 1, 1, 2),
        ('missing_kmer_warns', [rand[0], 'no_tt', rand[1]], True, 0, 1, 1, 5),
        ('no_valid_read', ['no_tt', 'short1', 'no_levels'], True, 0, 1, 1, 3),
        ('one_valid_read', [rand[0], 'no_tt'], False, 0, 1, 1, 3),
        ('one_read_asked', rand[:3], True, 0, 1, 1, 1),
        ('num_reads_zero', rand[:3], True, 0, 1, 1, 0),
        ('homopolymer_k1', ['homopolymer', rand[0]], True, 0, 0, 0, 2),
        ('homopolymer_k2', [rand[0], 'homopolymer'], True, 1, 0, 0, 2),
        ('homopolymer_k2_raw_order', ['homopolymer', rand[1]], True, 0, 1, 0, 2),
    ]
    for c in cases:
        assert all(n in names for n in c[1]), c
    return cases


def run_kmer_dist(pc, pool, case):
    name, read_names, read_mean, up, dn, thresh, num_reads = case
    by_name = {n: (lv, seq) for n, lv, seq in pool}
    rec = Recorder()
    pc.r = rec
    pc.importr = lambda pkg: None

    class Reads(object):
        def __init__(self, *a):
            pass

        def iter_reads(self):
            return iter(read_names)

    def slots(r_data, slot_names):
        lv, seq = by_name[r_data]
        assert slot_names == ['norm_mean', 'base']
        return (None, None) if lv is None else (lv, np.frombuffer(seq.encode(), dtype='S1'))

    def exit_(msg):
        raise Exit(msg)

    pc.th.TomboReads, pc.th.get_multiple_slots_read_centric = Reads, slots
    pc.th.error_message_and_exit, pc.th.warning_message = exit_, rec.messages.append
    shuffle, pc.np.random.shuffle = pc.np.random.shuffle, (lambda x: None)
    out = dict(name=name, reads=read_names, read_mean=read_mean, upstrm_bases=up, dnstrm_bases=dn, kmer_thresh=thresh,
               num_reads=num_reads, exit=None)
    arrays = {}
    try:
        pc.plot_kmer_dist(['dir'], 'grp', ['sub'], 'out.pdf', read_mean, up, dn, thresh, num_reads, None, False)
    except Exit as e:
        out['exit'] = str(e)
    except Exception as e:           # (one valid read asked for and found passes the exit test only with num_reads 1)
        out['exit'] = 'raised %s' % type(e).__name__
    finally:
        pc.np.random.shuffle = shuffle
    out['warnings'] = list(rec.messages)
    if out['exit'] is None:
        (fn_name, (kmerDat, baseDat, r_struct, dont_plot)), = [c for c in rec.calls if c[0] != 'r']
        assert fn_name == ('plotKmerDistWReadPath' if read_mean else 'plotKmerDist')
        assert rec.factor_levels[0] == rec.factor_levels[1] and len(rec.factor_levels) == 2
        out['r_function'] = fn_name
        arrays = {'levels': np.array(rec.factor_levels[0]), 'Kmer': kmerDat['Kmer'], 'Base': kmerDat['Base'],
                  'Signal': kmerDat['Signal'], 'Read': kmerDat['Read'], 'base_Kmer': baseDat['Kmer'],
                  'base_Base': baseDat['Base'], 'base_Position': baseDat['Position']}
        assert arrays['Signal'].dtype == np.float64 and arrays['base_Position'].dtype == np.int64
    return out, arrays


# ---- model overlays and per-read statistic frames: the scenario of gen_golden_plot_data.py (same seed, same reads)
# plus two reads with an N and a region over them
EXTRA_REGIONS = [(250, 263, None, 'r11', 'with N'), (252, 261, '-', 'r12', 'with N minus')]
# name -> (kmer_width, central_pos): central_pos equal to, below and above the downstream bases
MODELS = {'k3_cp1': (3, 1), 'k4_cp1': (4, 1), 'k4_cp2': (4, 2), 'k1_cp0': (1, 0)}
# (case, model, with alt model, regions, min_reg_overlap)
KMERS_CASES = [
    ('equal', 'k3_cp1', True, [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12], None),
    ('below', 'k4_cp1', True, [0, 1, 2, 3, 5, 7, 8, 11, 12], None),
    ('above', 'k4_cp2', True, [0, 1, 2, 3, 5, 7, 8, 11, 12], None),
    ('overlap_4', 'k4_cp2', False, [0, 1, 2, 3, 7], 4),
    ('overlap_9', 'k3_cp1', True, [0, 1, 2, 3, 7], 9),
    ('width_1', 'k1_cp0', False, [0, 1, 2, 11], None),      # expand_width 0: seq[0:-0] is ''
]


class Model(object):
    def __init__(self, kmer_width, central_pos, means, sds):
        self.kmer_width, self.central_pos, self.means, self.sds = kmer_width, central_pos, means, sds


def make_models(rng):
    """-> {name: (std Model, alt Model, std mean / sd arrays by k-mer code, alt rows)}; the alternate models know the
    k-mers with an A or a C at the position, so that windows with and without an entry occur"""
    from itertools import product
    out = {}
    for name, (K, cp) in sorted(MODELS.items()):
        kmers = [''.join(p) for p in product('ACGT', repeat=K)]
        means, sds = rng.standard_normal(4 ** K) * 1.5, 0.1 + rng.random(4 ** K) * 0.4
        alt_rows = [(kmer, pos, float(rng.standard_normal()), float(0.1 + rng.random()))
                    for kmer in kmers for pos in range(K) if kmer[pos] in 'AC']
        alt = Model(K, cp, dict(((k, p), m) for k, p, m, s in alt_rows), dict(((k, p), s) for k, p, m, s in alt_rows))
        out[name] = (Model(K, cp, dict(zip(kmers, means.tolist())), dict(zip(kmers, sds.tolist()))), alt, means, sds,
                     alt_rows)
    return out


def extra_reads(rng, genome, first_i):
    with_n = genome[:255] + 'N' + genome[256:]
    reads = []
    for i, (a, b, strand) in enumerate(((244, 270, '+'), (246, 272, '-'), (249, 262, '+'))):
        n = b - a
        segs = np.concatenate([[0], np.cumsum(rng.integers(3, 9, n))]).astype(np.int64)
        rsrtr = int(rng.integers(0, 20))
        raw = np.clip(np.rint(rng.standard_normal(rsrtr + int(segs[-1]) + 7) * 80 + 500), 0, 2000).astype(np.int16)
        fwd = with_n[a:b]
        reads.append(dict(start=a, end=b, strand=strand, rna=False, group=0, means=rng.standard_normal(n), segs=segs,
                          rsrtr=rsrtr, raw=raw, shift=float(500 + rng.standard_normal()), scale=float(80 + rng.random()),
                          lower=-1.5, upper=1.6, seq=fwd if strand == '+' else th.rev_comp(fwd), fn='read%d' % (first_i + i)))
    return reads


def all_intervals(which):
    regions = gpd.REGIONS + EXTRA_REGIONS
    return [th.intervalData(gpd.CHRM, a, b, strand, reg_id, text) for a, b, strand, reg_id, text in (regions[i] for i in which)]


def put_frame(store, prefix, frame):
    for col, values in frame.items():
        store['%s/%s' % (prefix, col)] = np.asarray(values)
    return list(frame)


def put_model_data(store, prefix, data):
    """[(reg_id, strand, fwd rows, rev rows)] -> arrays; -> [(reg_id, strand, fwd count, rev count)]"""
    rows = [(pos, m, s) for _, _, fwd, rev in data for pos, m, s in list(fwd) + list(rev)]
    store[prefix + '/pos'] = np.array([r[0] for r in rows], dtype=np.int64)
    store[prefix + '/mean'] = np.array([r[1] for r in rows], dtype=np.float64)
    store[prefix + '/sd'] = np.array([r[2] for r in rows], dtype=np.float64)
    return [(reg_id, strand, len(fwd), len(rev)) for reg_id, strand, fwd, rev in data]


def run_overlays(pc, store):
    gpd.install()
    rng = np.random.default_rng(20261020)                     # the scenario of stats_plot_data.npz, bit for bit
    genome = ''.join(rng.choice(list('ACGT'), gpd.CHRM_LEN))
    reads = gpd.make_reads(rng, genome)
    rng = np.random.default_rng(20240612)
    extras = extra_reads(rng, genome, len(reads))
    sample, control = gpd.register(reads + extras)
    models = make_models(rng)
    warned = []
    rec = Recorder()
    pc.r, pc._R_DF = rec, FrameBinder

    def exit_(msg):
        raise Exit(msg)
    th.warning_message, th.error_message_and_exit = warned.append, exit_
    th.is_sample_rna = lambda **kw: False
    meta = dict(extra_regions=[list(r) for r in EXTRA_REGIONS], models={}, kmers_cases=[], body_cases=[],
                extra_reads=[dict((k, r[k]) for k in ('start', 'end', 'strand', 'rna', 'group', 'fn', 'rsrtr', 'shift',
                                                      'scale', 'lower', 'upper', 'seq')) for r in extras])
    for i, r in enumerate(extras):
        store['extra/%d/means' % i], store['extra/%d/raw' % i], store['extra/%d/segs' % i] = r['means'], r['raw'], r['segs']
    for name, (std, alt, means, sds, alt_rows) in models.items():
        store['model/%s/means' % name], store['model/%s/sds' % name] = means, sds
        store['model/%s/alt_mean' % name] = np.array([r[2] for r in alt_rows])
        store['model/%s/alt_sd' % name] = np.array([r[3] for r in alt_rows])
        meta['models'][name] = dict(kmer_width=std.kmer_width, central_pos=std.central_pos,
                                    alt_keys=[[r[0], r[1]] for r in alt_rows])

    # get_reg_kmers and get_model_r_data
    n_alt = [0, 0]
    for case, model, with_alt, which, overlap in KMERS_CASES:
        std, alt = models[model][:2]
        regs = all_intervals(which)
        model_data, alt_data = pc.get_reg_kmers(std, regs, sample, min_reg_overlap=overlap, alt_ref=alt if with_alt else None)
        info = dict(name=case, model=model, with_alt=with_alt, regions=which, min_reg_overlap=overlap,
                    model_data=put_model_data(store, 'kmers/%s/std' % case, model_data),
                    alt_data=put_model_data(store, 'kmers/%s/alt' % case, alt_data),
                    intervals=[dict(start=int(p.start), end=int(p.end), seq=p.seq, reads=[r.fn for r in p.reads]) for p in regs])
        for d in alt_data:
            n_alt[0] += (len(d[2]) > 0) + (len(d[3]) > 0)
            n_alt[1] += (len(d[2]) == 0) + (len(d[3]) == 0)
        info['ModelData'] = put_frame(store, 'kmers/%s/ModelData' % case, pc.get_model_r_data(model_data))
        # read-centric: the reference indexes the minus strand's first entry, so only regions that have one
        ok = [d for d in model_data if d[1] == '+' or len(d[3]) > 0]
        info['read_centric_regions'] = [d[0] for d in ok]
        put_frame(store, 'kmers/%s/ModelDataReadCentric' % case, pc.get_model_r_data(ok, genome_centric=False))
        if with_alt:
            put_frame(store, 'kmers/%s/AltModelData' % case, pc.get_model_r_data(alt_data))
        meta['kmers_cases'].append(info)
    assert n_alt[0] > 3 and n_alt[1] > 3, n_alt
    assert any('N' in p['seq'] for c in meta['kmers_cases'] for p in c['intervals'])
    try:
        pc.get_reg_kmers(models['k4_cp1'][0], all_intervals([0]), sample, alt_ref=models['k4_cp2'][1])
        raise AssertionError('accepted')
    except Exit as e:
        meta['kmer_pos_error'] = str(e)
    # a model of another width passes the reference's check (it compares alt_ref.kmer_width with itself)
    pc.get_reg_kmers(models['k4_cp1'][0], all_intervals([0]), sample, alt_ref=models['k3_cp1'][1])

    def body(name, run, **info):
        del rec.calls[:], warned[:]
        np.random.seed(info['seed'])
        run()
        (fn_name, args), = [c for c in rec.calls if c[0] != 'r']
        frames = []
        for i, a in enumerate(args):
            if isinstance(a, dict):
                frames.append(put_frame(store, 'body/%s/%d' % (name, i), a))
            else:
                frames.append(None if a is None else a)
        meta['body_cases'].append(dict(info, name=name, r_function=fn_name, args=frames, warned=list(warned)))

    k3, k4 = models['k3_cp1'], models['k4_cp2']
    body('model_single', lambda: pc.plot_model_single_sample(all_intervals([0, 1, 2, 4, 8, 11]), sample, k3[0], 'Quantile', 4, 'x.pdf'),
         kind='model_single', regions=[0, 1, 2, 4, 8, 11], model='k3_cp1', with_alt=False, overplot_type='Quantile',
         overplot_thresh=4, seed=21, opts={})
    body('model_single_alt', lambda: pc.plot_model_single_sample(
        all_intervals([0, 2, 3, 5, 7, 12]), sample, k4[0], 'Downsample', 5, 'x.pdf', alt_ref=k4[1], title_include_chrm=False),
         kind='model_single', regions=[0, 2, 3, 5, 7, 12], model='k4_cp2', with_alt=True, overplot_type='Downsample',
         overplot_thresh=5, seed=22, opts={'title_include_chrm': False})
    stat_locs = [(float(p), float(s)) for p, s in zip(range(-3, 4), np.random.default_rng(5).random(7))]
    body('motif_no_model', lambda: pc.plot_motif_centered_with_stats(sample, None, all_intervals([0, 1, 2]), stat_locs, 5, 'x.pdf', None),
         kind='motif', regions=[0, 1, 2], model=None, with_alt=False, ctrl=False, overplot_thresh=5, seed=23, stat_locs=stat_locs)
    # read-centric alternate model data: the reference indexes the minus strand's first entry, so of the candidates
    # only regions whose minus-strand window is in the alternate model (or that are plus-strand regions)
    cand = [0, 1, 2, 3, 4, 5, 12]
    trial = pc.get_reg_kmers(k3[0], all_intervals(cand), sample, alt_ref=k3[1])[1]
    alt_regs = [i for i, d in zip(cand, trial) if d[1] == '+' or len(d[3]) > 0]
    assert any(d[1] != '+' for i, d in zip(cand, trial) if i in alt_regs) and len(alt_regs) >= 3, alt_regs
    body('motif_model_alt', lambda: pc.plot_motif_centered_with_stats(
        sample, None, all_intervals(alt_regs), stat_locs, 6, 'x.pdf', k3[0], alt_ref=k3[1]),
         kind='motif', regions=alt_regs, model='k3_cp1', with_alt=True, ctrl=False, overplot_thresh=6, seed=24, stat_locs=stat_locs)
    body('motif_model', lambda: pc.plot_motif_centered_with_stats(sample, None, all_intervals([1, 3]), stat_locs, 6, 'x.pdf', k4[0]),
         kind='motif', regions=[1, 3], model='k4_cp2', with_alt=False, ctrl=False, overplot_thresh=6, seed=25, stat_locs=stat_locs)
    body('motif_ctrl', lambda: pc.plot_motif_centered_with_stats(sample, control, all_intervals([0, 1, 2, 8]), stat_locs, 4, 'x.pdf', None),
         kind='motif', regions=[0, 1, 2, 8], model=None, with_alt=False, ctrl=True, overplot_thresh=4, seed=26, stat_locs=stat_locs)

    # per-read statistics: p-values (zeros, tiny ones, NaN) and likelihood ratios (beyond +-4, NaN); a region of one
    # read; two reads of three that share no position
    srng = np.random.default_rng(77)
    for name, are_pvals, box_center in (('per_read_pvals', True, True), ('per_read_llrs', False, False)):
        regs = [p.add_reads(sample).add_seq() for p in all_intervals([0, 1, 2, 3])]
        stats = []
        for j, (p, n_reads) in enumerate(zip(regs, (6, 5, 1, 3))):
            n_pos = p.end - p.start
            m = srng.random((n_reads, n_pos)) ** 4 if are_pvals else srng.standard_normal((n_reads, n_pos)) * 3
            m[srng.random(m.shape) < 0.15] = np.nan
            if are_pvals:
                m[0, :3] = [0.0, 1e-7, 1.0]
            if n_reads == 3:
                m[0, n_pos // 2:], m[1, :n_pos // 2] = np.nan, np.nan
            stats.append((p.reg_id, p.strand, m))
            store['body/%s/in/%d' % (name, j)] = m.copy()
        body(name, lambda: pc.plot_per_read_modification(regs, stats, are_pvals, box_center, 'x.pdf'),
             kind='per_read', regions=[0, 1, 2, 3], are_pvals=are_pvals, box_center=box_center, seed=27,
             strands=[p.strand for p in regs])
    for c in meta['body_cases']:
        print('%-18s %s %s' % (c['name'], c['r_function'], [a if not isinstance(a, list) else len(a) for a in c['args']]))
    return meta


def main():
    rng = np.random.default_rng(20240611)
    pc = gpd.load_plot_commands()
    pool = make_pool(rng)
    store = {}
    for n, lv, seq in pool:
        if lv is not None:
            store['pool/%s/means' % n] = np.asarray(lv, dtype=np.float64)
    cases = []
    for case in kmer_dist_cases([n for n, _, _ in pool]):
        out, arrays = run_kmer_dist(pc, pool, case)
        cases.append(out)
        for k, v in arrays.items():
            store['kmer/%s/%s' % (out['name'], k)] = v
        print('%-28s exit=%r warnings=%d rows=%d' % (out['name'], out['exit'] and out['exit'][:20], len(out['warnings']),
                                                      arrays['Signal'].shape[0] if arrays else 0))
    overlays = run_overlays(pc, store)
    store['meta'] = np.array(json.dumps(dict(
        pool=[dict(name=n, seq=seq, has_levels=lv is not None) for n, lv, seq in pool], kmer_cases=cases,
        overlays=overlays)))
    path = os.path.join(HERE, 'stats_kmer_dist.npz')
    np.savez_compressed(path, **store)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()

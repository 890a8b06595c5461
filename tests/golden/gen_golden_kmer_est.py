"""Golden vectors of the canonical and motif k-mer model estimation from the REFERENCE (build container only).

    python tests/golden/gen_golden_kmer_est.py   # writes tests/golden/stats_kmer_est.npz

Runs the live reference's extract_kmer_levels (tombo/tombo_stats.py:1398-1452, its worker processes run
in-process) with get_region_kmer_levels (:1242-1359), tabulate_kmer_levels (:1454-1501),
tabulate_mod_kmer_levels (:2108-2158), TomboModel / AltModel with _make_constant_sd and write_model (against the
dict-backed HDF5 stand-in of tests/memh5.py) on synthetic reads.  The Events accessor
(`th.get_single_slot_read_centric`) is pointed at in-memory arrays, `Process` / `Queue` at in-process stand-ins
and the TomboReads objects are made with object.__new__ around a ready `reads_index` -- everything after that is
the reference's own code.  Only data is written: the reads, the cases and the outputs.

Every case is run TWICE on the same seeded inputs: as the reference is, and with the `np.argsort` inside
th.get_reads_events forced to kind='stable'.  The default argsort is not stable, so the order of the levels of
a position -- and with it the last bits of np.std and of both values of c_mean_std -- depends on the sort
implementation; a stable sort leaves them in read order, which is the order the device uses.  Medians and counts
do not depend on it (asserted here).  Per case and column the largest absolute difference between the two runs
is recorded (`spread`): the as-is run is compared within four times that figure, the stable run bit for bit.

Centring: the live center_model_to_median_norm (:1599-1705; `h5py.File`, `th.get_raw_read_slot` and
`th.get_multiple_slots_read_centric` pointed at in-memory arrays) on eight DNA reads of 150-400 bases, one of 1200
(its Theil-Sen points are drawn with np.random.choice) and a homopolymer read whose slope is 0, with max_reads below,
at and above the number of successes and on the failing read alone; the factors handed to _center_model and the
centred levels are recorded.  The end-to-end models are the lines of estimate_kmer_model (:1727-1740) in order --
tabulate, TomboModel, centre on those reads, _make_constant_sd -- on the reads without a NaN level.

Reads: a 600-base genome (all xyCGz 5-mers, CCWGG sites, random bases), both strands, reads of 20-120 bases kept
out of [400, 500) where exactly cov_thresh short reads lie (a region with no interval); reads ending at 400 and
600 (intervals that end with their region, '-' in the flank); reads with an N, a NaN level, fewer levels than
bases, no Events table.  Deep pile: 8-base reads over a 12-base stretch, 4100 on '+' (positions with 4095, 4096,
4097 and 4100 reads) and 65 on '-' (63, 64, 65): both sides of each sorter class; its levels are multiples of
1/256 stored as int16.
"""
import os
import re
import sys
import json
import queue
from itertools import product

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_oracle  # noqa: E402
import memh5  # noqa: E402
import kmer_est_reference as kr  # noqa: E402

rq, ts, th = ref_oracle.load()
STORE = {}
REGION_SIZE, COV_THRESH = 100, 3
CHRM = 'chr1'


class FakeQueue(object):
    def __init__(self):
        self.items = []

    def put(self, x):
        self.items.append(x)

    def get(self, block=True):
        if not self.items:
            raise queue.Empty
        return self.items.pop(0)

    def empty(self):
        return not self.items


class FakeProcess(object):   # runs its target in-process on start()
    def __init__(self, target, args):
        self.target, self.args = target, args

    def start(self):
        self.target(*self.args)

    def is_alive(self):
        return False


class RefExit(Exception):
    pass


def _exit(msg):
    raise RefExit(msg)


class StableNumpy(object):
    """numpy with argsort forced stable, for th.get_reads_events"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kw):
        return np.argsort(a, kind='stable')


CENTER = {}     # the centring reads: id -> {'raw', 'start', 'base'}
MESSAGES = []
FACTORS = []


class FakeFile(object):
    def __init__(self, fn, mode='r'):
        self.fn = fn

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class ReadsIndex(object):
    def __init__(self, reads):
        self.reads = reads

    def iter_reads(self):
        return iter(self.reads)


def install():
    ts.Process, ts.Queue, ts.sleep = FakeProcess, FakeQueue, lambda s: None
    ts.h5py.File = FakeFile
    th.get_raw_read_slot = lambda f: {'Signal': CENTER[f.fn]['raw']}
    th.get_multiple_slots_read_centric = lambda f, names, grp=None: [CENTER[f.fn][n] for n in names]
    real_center = ts.TomboModel._center_model

    def recording_center(self, shift, scale):
        FACTORS.append((float(shift), float(scale)))
        return real_center(self, shift, scale)
    ts.TomboModel._center_model = recording_center
    th.get_single_slot_read_centric = lambda r, name, grp=None: (None if STORE[r.fn] is None else STORE[r.fn][name])
    th.error_message_and_exit = _exit
    th.warning_message = MESSAGES.append


def tombo_reads(index):
    tr = object.__new__(th.TomboReads)
    tr.reads_index = index
    tr.coverage = None
    return tr


ROWS = {}   # set name -> [(minus, start, end, has, seq, means)]


def add_read(index, which, strand, start, end, seq, means):
    fn = 'r%d' % len(STORE)
    STORE[fn] = None if seq is None else {'norm_mean': means, 'base': np.frombuffer(seq.encode(), dtype='S1')}
    index.setdefault((CHRM, strand), []).append(th.readData(start, end, False, 0, strand, fn, 'grp', False, 0.0, 10.0, fn))
    ROWS.setdefault(which, []).append((strand == '-', start, end, seq is not None, seq or '', means if seq is not None else np.empty(0)))


def make_genome(rng):
    parts = [x + y + 'CG' + z for x in 'ACGT' for y in 'ACGT' for z in 'ACGT']
    rng.shuffle(parts)
    g = ''.join(parts) + 'TCCAGGA' + 'ACCTGGT' + 'GCCAGGC'
    g += ''.join(rng.choice(list('ACGT'), 600 - len(g) - 14)) + 'ACCTGGA' + 'TCCAGGT'
    assert len(g) == 600
    return g


def read_of(rng, genome, level, strand, start, end):
    """(seq, means) of a read over [start, end), read-centric"""
    seq = genome[start:end]
    lv = np.array([level.get(genome[max(i - 1, 0):i + 2], 0.0) if strand == '+' else
                   level.get(th.rev_comp(genome[max(i - 1, 0):i + 2]), 0.0) for i in range(start, end)])
    lv = lv + rng.normal(0.0, 0.15, end - start)
    if strand == '-':
        seq, lv = th.rev_comp(seq), lv[::-1].copy()
    return seq, lv


def make_main(rng, genome, level):
    idx = {}
    for strand in '+-':
        spans = [(0, int(n)) for n in rng.integers(20, 121, 5)] + [(400 - int(n), 400) for n in rng.integers(20, 121, 5)] + \
            [(500, 500 + int(n)) for n in rng.integers(20, 100, 5)] + [(600 - int(n), 600) for n in rng.integers(20, 100, 5)]
        for lo, hi, count in ((0, 400, 70), (500, 600, 20)):
            for _ in range(count):
                n = int(rng.integers(20, min(120, hi - lo) + 1))
                s = int(rng.integers(lo, hi - n + 1))
                spans.append((s, s + n))
        spans += [(420, 450), (430, 470), (445, 480)]     # exactly COV_THRESH reads in [400, 500)
        order = rng.permutation(len(spans))
        for j, i in enumerate(order.tolist()):
            s, e = spans[i]
            seq, lv = read_of(rng, genome, level, strand, s, e)
            if j % 17 == 3:      # an N in the read
                p = int(rng.integers(2, len(seq) - 2))
                seq = seq[:p] + 'N' + seq[p + 1:]
            if j % 23 == 5:      # a NaN level
                lv[int(rng.integers(0, len(lv)))] = np.nan
            if j % 29 == 7:      # fewer levels (and bases) than the mapping says
                seq, lv = seq[:-3], lv[:-3].copy()
            if j % 31 == 11:     # no Events table
                seq, lv = None, None
            add_read(idx, 'main', strand, s, e, seq, lv)
    return idx


def make_deep(rng, genome):
    idx = {}
    base = 30
    for strand, per_start in (('+', (3, 1, 1, 4031, 64)), ('-', (63, 1, 1, 0, 0))):
        starts = np.repeat(np.arange(5), per_start)
        rng.shuffle(starts)
        for s in starts.tolist():
            seq = genome[base + s:base + s + 8]
            q = rng.integers(-700, 700, 8).astype(np.int16)
            add_read(idx, 'deep', strand, base + s, base + s + 8, th.rev_comp(seq) if strand == '-' else seq, q / 256.0)
    return idx


def make_center_reads(rng, level):
    """eight DNA reads of 150-400 bases, one of 1200 (its Theil-Sen points are drawn), one homopolymer (every
    expected level equal: the slope is 0 and the read fails): raw DAC-like integers, 5-12 samples a base"""
    reads = []
    seqs = [''.join(rng.choice(list('ACGT'), int(n))) for n in list(rng.integers(150, 401, 8)) + [1200]] + ['A' * 200]
    for i, seq in enumerate(seqs):
        n, rsr = len(seq), int(rng.integers(20, 60))
        dwell = rng.integers(5, 13, n)
        lv = np.array([level.get(seq[max(j - 1, 0):j + 2], 0.0) for j in range(n)])
        body = np.repeat(lv * 12.0 + 90.0 + rng.normal(0, 0.6, n), dwell) + rng.normal(0, 1.5, int(dwell.sum()))
        raw = np.round(np.concatenate([rng.normal(95, 6, rsr), body, rng.normal(95, 6, 25)])).astype(np.int16)
        start = np.concatenate([[0], np.cumsum(dwell)[:-1]]).astype(np.uint32)
        rid = 'c%d' % i
        CENTER[rid] = {'raw': raw, 'start': start, 'base': np.frombuffer(seq.encode(), dtype='S1')}
        reads.append(th.readData(0, n, False, rsr, '+', rid, 'grp', False, 0.0, 10.0, rid))
    return reads


def pack_center_reads(out, reads):
    rows = [CENTER[r.fn] for r in reads]
    out['center_rsr'] = np.array([r.read_start_rel_to_raw for r in reads], dtype=np.int32)
    out['center_raw_off'] = np.concatenate([[0], np.cumsum([len(c['raw']) for c in rows])]).astype(np.int32)
    out['center_raw'] = np.concatenate([c['raw'] for c in rows])
    out['center_off'] = np.concatenate([[0], np.cumsum([len(c['start']) for c in rows])]).astype(np.int32)
    out['center_start'] = np.concatenate([c['start'] for c in rows])
    out['center_seq'] = np.frombuffer(b''.join(c['base'].tobytes() for c in rows), dtype=np.uint8)


def run_centring(meta, out, level, kmers3, reads):
    """center_model_to_median_norm of the live reference on a 3-mer model without the reads' scale"""
    meta['center_runs'] = []
    out['center_init'] = np.array([(level[k], 0.2) for k in kmers3])
    for name, sel, seed, max_reads in (('all_reads', list(range(10)), 5, 50), ('first_three', list(range(10)), 5, 3),
                                       ('only_the_failing_read', [9], 5, 50), ('max_equals_successes', list(range(10)), 6, 9)):
        del MESSAGES[:], FACTORS[:]
        model = ts.TomboModel(kmer_ref=[(k, level[k], 0.2) for k in kmers3], central_pos=1)
        np.random.seed(seed)
        run = dict(name=name, reads=sel, seed=seed, max_reads=max_reads, error=None)
        try:
            ts.center_model_to_median_norm(ReadsIndex([reads[i] for i in sel]), model, max_reads)
            run['factors'] = list(FACTORS[0])
            out['center_' + name + '_means'] = np.array([model.means[k] for k in kmers3])
        except RefExit as e:
            run['error'] = str(e)
        run['warning'] = MESSAGES[0] if MESSAGES else None
        print('centring %-22s factors %s warning %s error %s' % (name, run.get('factors'), bool(run['warning']), run['error']))
        meta['center_runs'].append(run)
    runs = dict((r['name'], r) for r in meta['center_runs'])
    assert runs['all_reads']['warning'] and not runs['first_three']['warning'] and not runs['max_equals_successes']['warning']
    assert runs['only_the_failing_read']['error'] and runs['all_reads']['factors'] != runs['first_three']['factors']


def pack_reads(out, name):
    rows = ROWS[name]
    out[name + '_minus'] = np.array([r[0] for r in rows], dtype=np.uint8)
    out[name + '_start'] = np.array([r[1] for r in rows], dtype=np.int32)
    out[name + '_end'] = np.array([r[2] for r in rows], dtype=np.int32)
    out[name + '_has'] = np.array([r[3] for r in rows], dtype=np.uint8)
    out[name + '_off'] = np.concatenate([[0], np.cumsum([len(r[4]) for r in rows])]).astype(np.int32)
    out[name + '_seq'] = np.frombuffer(''.join(r[4] for r in rows).encode(), dtype=np.uint8)
    means = np.concatenate([r[5] for r in rows])
    if name == 'deep':
        q = np.round(means * 256.0).astype(np.int16)
        assert np.array_equal(q / 256.0, means)
        out[name + '_means_q256'] = q
    else:
        out[name + '_means'] = means


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def nan_absdiff(a, b):
    both = ~(np.isnan(a) & np.isnan(b))
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def run_case(out, meta, indices, case):
    name = case['name']
    motif = None
    if case.get('motif'):
        raw, pos = case['motif'].split(':')
        motif = th.TomboMotif(raw, int(pos))
    K = case['upstrm'] + case['dnstrm'] + 1
    keys = [''.join(p) for p in product('ACGT', repeat=K)] if motif is None else \
        [(''.join(k), o - 1) for k in product('ACGT', repeat=K) for o in motif.find_mod_poss(''.join(k))]
    valid = None
    if case.get('valid_poss') is not None:
        valid = {(CHRM, '+'): np.array(case['valid_poss'], dtype=np.int64)}
    runs = {}
    for run in ('stable', 'asis'):
        th.np = StableNumpy() if run == 'stable' else np
        if case.get('seed') is not None:
            np.random.seed(case['seed'])
        regs = ts.extract_kmer_levels(tombo_reads(indices[case['reads']]), REGION_SIZE, case['cov_thresh'], case['upstrm'],
                                      case['dnstrm'], case.get('cs_cov_thresh'), case['est_mean'], 1, motif, valid)
        th.np = np
        counts, lv, sd = kr.flatten(regs, keys)
        tab = err = None
        try:
            tab = ts.tabulate_kmer_levels(regs, case['min_kmer_obs']) if motif is None else \
                ts.tabulate_mod_kmer_levels(regs, case['min_kmer_obs'], motif)
        except RefExit as e:
            err = str(e)
        except NameError:    # tabulate_kmer_levels' too-few-observations branch names an undefined `motif`
            err = 'NameError'
        runs[run] = (regs, counts, lv, sd, tab, err)
    (regs, counts, lv, sd, tab, err), (_, counts2, lv2, sd2, tab2, err2) = runs['stable'], runs['asis']
    assert np.array_equal(counts, counts2) and err == err2
    if not case['est_mean']:
        assert same(lv, lv2), 'medians must not depend on the sort'
    out[name + '_reg_counts'] = counts.astype(np.int32)
    out[name + '_levels'], out[name + '_sds'] = lv, sd
    out[name + '_asis_levels'], out[name + '_asis_sds'] = lv2, sd2
    case['spread'] = [nan_absdiff(lv, lv2), nan_absdiff(sd, sd2)]
    case['error'] = err
    case['n_regions'] = len(regs)
    if tab is not None:
        out[name + '_tab'] = np.array([t[-2:] for t in tab], dtype=np.float64)
        out[name + '_asis_tab'] = np.array([t[-2:] for t in tab2], dtype=np.float64)
        case['tab_spread'] = [nan_absdiff(out[name + '_tab'][:, j], out[name + '_asis_tab'][:, j]) for j in (0, 1)]
    print('%-18s regions %2d entries %5d  spread %.3g / %.3g  %s' % (
        name, len(regs), lv.shape[0], case['spread'][0], case['spread'][1], 'ERROR: ' + err.split('.')[0] if err else ''))
    meta['cases'].append(case)
    return regs, tab, motif


def written(model, out, meta, name):
    grp = memh5.MemGroup()

    class _Opened(object):
        def __init__(self, fn, mode='r'):
            pass

        def __enter__(self):
            return grp

        def __exit__(self, *a):
            return False
    real = getattr(ts.h5py, 'File', None)
    ts.h5py.File = _Opened
    model.write_model('unused.model')
    ts.h5py.File = real
    tree = memh5.tree(grp)
    out[name + '_written_model'] = tree.pop('/model')
    meta[name + '_written_attrs'] = dict((k, v if isinstance(v, (int, str)) or v is None else int(v)) for k, v in tree.items())
    meta[name + '_written_dataset_kw'] = grp.items['model'].kw


def main():
    install()
    rng = np.random.default_rng(2108)
    genome = make_genome(rng)
    kmers3 = [''.join(p) for p in product('ACGT', repeat=3)]
    level = dict(zip(kmers3, (rng.permutation(np.linspace(-2.4, 2.4, 64)) + rng.normal(0, 0.02, 64)).tolist()))
    indices = {'main': make_main(rng, genome, level), 'deep': make_deep(rng, genome)}
    # the reads of 'main' without those that hold a NaN level: every k-mer of the tabulated model is a number
    indices['clean'] = dict((cs, [r for r in rds if STORE[r.fn] is None or not np.isnan(STORE[r.fn]['norm_mean']).any()])
                            for cs, rds in indices['main'].items())
    center_reads = make_center_reads(rng, level)
    out = {'genome': np.frombuffer(genome.encode(), dtype=np.uint8)}
    pack_reads(out, 'main')
    pack_reads(out, 'deep')
    ccwgg = [m.start() + 1 for m in re.finditer('CC[AT]GG', genome)]
    valid = [ccwgg[2], ccwgg[0]] + ccwgg[3:] + [ccwgg[1], 7, 455, 599, 433]   # unsorted, with positions off any site
    base = dict(reads='main', cov_thresh=COV_THRESH, upstrm=1, dnstrm=1, est_mean=False, min_kmer_obs=1)
    cases = [
        dict(base, name='canon_med'),
        dict(base, name='canon_mean', est_mean=True),
        dict(base, name='canon_cs', cs_cov_thresh=14, seed=11),
        dict(base, name='canon_clean', reads='clean'),
        dict(base, name='canon_few', min_kmer_obs=40),
        dict(base, name='fourmer', dnstrm=2),
        dict(base, name='motif_cg', motif='CG:1'),
        dict(base, name='motif_cg_few', motif='CG:1', min_kmer_obs=30),
        dict(base, name='motif_ccwgg_valid', motif='CCWGG:2', valid_poss=valid),
        dict(base, name='deep_med', reads='deep', cov_thresh=2),
        dict(base, name='deep_mean', reads='deep', cov_thresh=2, est_mean=True),
    ]
    meta = {'region_size': REGION_SIZE, 'chrm': CHRM, 'cases': []}
    got = {}
    for case in cases:
        got[case['name']] = run_case(out, meta, indices, case)
    by = dict((c['name'], c) for c in meta['cases'])
    assert by['canon_med']['error'] is None and by['motif_cg']['error'] is None and by['canon_cs']['error'] is None
    assert by['motif_cg_few']['error'] and 'fewer observations' in by['motif_cg_few']['error']
    assert by['deep_mean']['spread'][0] > 0 or by['deep_mean']['spread'][1] > 0 or by['deep_med']['spread'][1] > 0, \
        'the deep pile should tell the two sort orders apart'
    pack_center_reads(out, center_reads)
    run_centring(meta, out, level, kmers3, center_reads)
    # the models: estimate_kmer_model (tombo_stats.py:1727-1740) and estimate_motif_alt_model (:2180-2189) after the
    # file access, line by line: tabulate, TomboModel, center_model_to_median_norm, _make_constant_sd
    _, tab, _ = got['canon_clean']
    assert not np.isnan(np.array([t[1:] for t in tab])).any()
    for name, kmer_specific_sd in (('model_kmer_sd', True), ('model_const_sd', False)):
        del MESSAGES[:], FACTORS[:]
        np.random.seed(7)
        model = ts.center_model_to_median_norm(ReadsIndex(center_reads), ts.TomboModel(kmer_ref=tab, central_pos=1))
        if not kmer_specific_sd:
            model._make_constant_sd()
        out[name] = np.array([(model.means[k], model.sds[k]) for k in kmers3])
        meta[name + '_factors'] = list(FACTORS[0])
    meta['model_center_seed'] = 7
    written(model, out, meta, 'model_const_sd')
    _, tab, motif = got['motif_cg']
    alt = ts.AltModel(kmer_ref=tab, central_pos=1, alt_base=motif.mod_base, motif=motif)
    alt._make_constant_sd()
    out['alt_model'] = np.array([(k, p, alt.means[(k, p)], alt.sds[(k, p)]) for k, p in alt.means],
                                dtype=[('kmer', 'S3'), ('pos', 'u4'), ('mean', 'f8'), ('sd', 'f8')])
    written(alt, out, meta, 'alt_model')
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'stats_kmer_est.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()

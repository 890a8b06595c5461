"""Golden vectors of the alternate-base model estimation from the REFERENCE (build container only).

    python tests/golden/gen_golden_alt_est.py   # writes tests/golden/stats_alt_est.npz

Runs the live reference's parse_base_levels (tombo/tombo_stats.py:1811-1884, its worker processes run
in-process), est_kernel_density (:1914-1939, i.e. scipy.stats.gaussian_kde), write / parse of the
density files, isolate_alt_density (:1991-2071) and AltModel.write_model (:929-953, against the
dict-backed HDF5 stand-in of tests/memh5.py) on synthetic reads of a made-up 3-mer model.  The file
accessors (`h5py.File`, `th.get_multiple_slots_read_centric`) are pointed at in-memory arrays and
`Process` / `Queue` at in-process stand-ins -- everything after them is the reference's own code.
Only data is written: the model table, the reads, and the outputs.

The reference's worker indexes its per-k-mer dict with every window of a read, so a read with an N
ends it with a KeyError; the engine skips such windows instead.  The read with an N is therefore
given to the reference as its ACGT pieces (consecutive reads with the matching slices of the
levels), which pairs exactly the windows without an N with the same levels in the same order.

Conditions on the inputs (asserted here): no density-shift offset lies within 1e-9 of an integer
before truncation; the arg-max of every standard density and the matched alternate peak win over
their neighbours by more than 1e-9 relative; std_frac < 1.  Under them the discrete steps of
isolate_alt_density cannot flip between densities that agree to 1e-12.  A direct float64 evaluation
of the density formula is recorded next to scipy's (their spread is asserted under 1e-13 relative
where the density is at least 1e-10).
"""
import os
import sys
import json
import queue
import hashlib
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_oracle  # noqa: E402
import memh5  # noqa: E402

rq, ts, th = ref_oracle.load()
STORE = {}
MESSAGES = []
K, CP, G_EST, BW, BW_EST = 3, 1, 150, 0.05, 0.08
ALT_BASE, PCTL = 'A', 5
MARGIN = 1e-9


class FakeFile(object):
    def __init__(self, fn, mode='r'):
        self.fn = fn

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


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


class ReadsIndex(object):
    def __init__(self, reads):
        self.reads = reads

    def iter_reads(self):
        return iter(self.reads)


def _exit(msg):
    raise RefExit(msg)


def install():
    ts.h5py.File = FakeFile
    ts.Process, ts.Queue, ts.sleep = FakeProcess, FakeQueue, lambda s: None
    th.get_multiple_slots_read_centric = lambda f, names, grp=None: [STORE[f.fn][n] for n in names]
    th.error_message_and_exit = _exit
    th.warning_message = MESSAGES.append
    ts.np.random.shuffle = lambda x: None   # (the order of the reads is part of the recorded case)


def ref_reads(seqs, means):
    """reference readData of the reads; a read with non-ACGT bases as its ACGT pieces (see above)"""
    out = []
    for seq, m in zip(seqs, means):
        pieces, a = [], 0
        if all(c in 'ACGT' for c in seq):
            pieces = [(0, len(seq))]
        else:
            for i, c in enumerate(seq + 'N'):
                if c not in 'ACGT':
                    if i > a:
                        pieces.append((a, i))
                    a = i + 1
        for a, b in pieces:
            rid = 'r%d' % len(STORE)
            STORE[rid] = {'norm_mean': m[a:b], 'base': np.frombuffer(seq[a:b].encode(), dtype='S1')}
            out.append(th.readData(0, b - a, False, 0, '+', rid, 'grp', False, 0.0, 10.0, rid))
    return out


def make_sample(rng, kmers, level, shift, n_reads, length, frac_mod):
    """reads of a sample in which every ALT_BASE is modified with probability frac_mod; a k-mer with a
    modified base sits `shift[kmer]` above its canonical level"""
    seqs, means = [], []
    for _ in range(n_reads):
        n = int(length + rng.integers(-20, 20))
        seq = ''.join(rng.choice(list('ACGT'), n))
        mod = (np.array(list(seq)) == ALT_BASE) & (rng.random(n) < frac_mod)
        m = rng.normal(0.0, 0.5, n)
        for i in range(n - K + 1):
            km = seq[i:i + K]
            m[i + CP] = level[km] + (shift[km] if mod[i:i + K].any() else 0.0) + rng.normal(0.0, 0.2)
        seqs.append(seq)
        means.append(m)
    return seqs, means


def pack(out, name, seqs, means):
    out[name + '_off'] = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    out[name + '_seq'] = np.frombuffer(''.join(seqs).encode(), dtype=np.uint8)
    out[name + '_means'] = np.concatenate(means) if means else np.empty(0)


def flat(kmers, levels_dict):
    counts = [len(levels_dict[k]) for k in kmers]
    return (np.array([x for k in kmers for x in levels_dict[k]], dtype=np.float64),
            np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))


def direct_density(levels, x, h):
    lv = np.sort(np.asarray(levels, dtype=np.float64))
    acc = np.zeros(x.shape[0])
    with np.errstate(under='ignore'):
        for c in range(0, lv.shape[0], 2048):
            t = (x[:, None] - lv[None, c:c + 2048]) / h
            acc += np.exp(-0.5 * (t * t)).sum(axis=1)
        return acc / (lv.shape[0] * h * 2.50662827463100050242)


def check_isolation_margins(alt_dens, std_dens, std_ref, save_x):
    """the conditions of the module docstring, from the reference's own expressions"""
    def calc_mean(dens):
        return np.average(save_x[dens > 1e-10], weights=dens[dens > 1e-10])
    xs, ds = [], []
    for kmer in std_dens:
        if ALT_BASE in kmer:
            continue
        xs.append(calc_mean(std_dens[kmer]))
        ds.append(calc_mean(alt_dens[kmer]) - xs[-1])
    calc_offset = np.poly1d(np.polyfit(xs, ds, 2))
    unit = save_x[1] - save_x[0]
    fracs = []
    for kmer, ad in alt_dens.items():
        v = calc_offset(calc_mean(std_dens[kmer])) / unit
        assert abs(v - round(v)) > MARGIN, (kmer, v)
        off = int(v)
        sh = np.concatenate([np.zeros(-off), ad[:off]]) if off < 0 else np.concatenate([ad[off:], np.zeros(off)])
        if kmer.count(ALT_BASE) != 1:
            continue
        sd = std_dens[kmer]
        p = int(np.argmax(sd))
        assert (sd[p] - np.delete(sd, p).max()) / sd[p] > MARGIN, kmer
        peaks = np.flatnonzero((sh[1:-1] > sh[:-2]) & (sh[1:-1] > sh[2:])) + 1
        dist = np.abs(peaks - p)
        q = int(peaks[np.argmin(dist)])
        for t in peaks[dist == dist.min()].tolist():   # (equidistant peaks: np.argmin takes the first in both)
            assert sh[t] > 1e-10 and min(sh[t] - sh[t - 1], sh[t] - sh[t + 1]) / sh[t] > MARGIN, kmer
        fracs.append(sh[q] / sd[p])
    std_frac = np.percentile(fracs, PCTL)
    assert std_frac < 1, std_frac
    return float(std_frac)


def model_table(alt_ref):
    return np.array([(k, p, alt_ref.means[(k, p)], alt_ref.sds[(k, p)]) for k, p in alt_ref.means],
                    dtype=[('kmer', 'S%d' % K), ('pos', 'u4'), ('mean', 'f8'), ('sd', 'f8')])


def main():
    install()
    rng = np.random.default_rng(1747)
    from itertools import product
    kmers = [''.join(p) for p in product('ACGT', repeat=K)]
    lv = rng.permutation(np.linspace(-2.6, 2.6, len(kmers))) + rng.normal(0, 0.02, len(kmers))
    level = dict(zip(kmers, lv.tolist()))
    shift = dict((k, float(rng.uniform(0.7, 1.1))) for k in kmers)
    sds = np.full(len(kmers), 0.2)
    std_ref = ts.TomboModel(kmer_ref=[(k, level[k], 0.2) for k in kmers], central_pos=CP,
                            seq_samp_type=th.seqSampleType('DNA', False))
    out = {'model_means': lv, 'model_sds': sds}
    meta = {'kmer_width': K, 'central_pos': CP, 'alt_base': ALT_BASE, 'alt_frac_pctl': PCTL,
            'bw': BW, 'bw_est': BW_EST, 'g_est': G_EST, 'parse_cases': []}

    alt_seqs, alt_means = make_sample(rng, kmers, level, shift, 40, 300, 0.5)
    ctl_seqs, ctl_means = make_sample(rng, kmers, level, shift, 40, 300, 0.0)
    # (d): a read shorter than K, one of exactly K, one with Ns (an N window at either end and inside),
    # one with a NaN level, among ordinary short reads
    edge_seqs, edge_means = make_sample(rng, kmers, level, shift, 10, 120, 0.5)
    edge_seqs[2:2] = ['AC', 'GAT', 'NACGTANNCGATTNACAGN' + edge_seqs[0][:40] + 'N']
    edge_means[2:2] = [rng.normal(0, 1, 2), rng.normal(0, 1, 3), rng.normal(0, 1, 19 + 41)]
    edge_means[7] = edge_means[7].copy()
    edge_means[7][5] = np.nan
    pack(out, 'alt', alt_seqs, alt_means)
    pack(out, 'ctrl', ctl_seqs, ctl_means)
    pack(out, 'edge', edge_seqs, edge_means)
    sets = {'alt': ref_reads(alt_seqs, alt_means), 'ctrl': ref_reads(ctl_seqs, ctl_means),
            'edge': ref_reads(edge_seqs, edge_means)}

    # (a) (b) (c): parse_base_levels(reads, std_ref, batch, kmer_obs_thresh, max_kmer_obs, min_kmer_obs_to_est)
    for name, rset, bs, thresh, max_obs, min_obs in (
            ('a_overshoot', 'alt', 20, 85, 90, 50), ('b_reads_run_out', 'edge', 4, 1000, 10000, 3),
            ('c_too_few', 'edge', 4, 1000, 10000, 1000), ('a2_batch_of_7', 'ctrl', 7, 60, 75, 50)):
        del MESSAGES[:]
        case = dict(name=name, reads=rset, batch=bs, kmer_obs_thresh=thresh, max_kmer_obs=max_obs,
                    min_kmer_obs_to_est=min_obs, error='', warning='')
        try:
            res = ts.parse_base_levels(sets[rset], std_ref, bs, thresh, max_obs, min_obs, 1)
            out[name + '_levels'], out[name + '_lv_off'] = flat(kmers, res)
            n = np.diff(out[name + '_lv_off'])
            print(name, 'levels per k-mer: min %d max %d' % (n.min(), n.max()), MESSAGES)
            if name == 'a_overshoot':
                # k-mers complete after the first batch (past the cap by less than a batch) and after the second
                assert ((n > max_obs) & (n < max_obs + 40)).any() and (n >= max_obs + 40).any()
        except RefExit as e:
            case['error'] = str(e)
        case['warning'] = MESSAGES[0] if MESSAGES else ''
        meta['parse_cases'].append(case)
    assert [c['error'] != '' for c in meta['parse_cases']] == [False, False, True, False]
    assert [c['warning'] != '' for c in meta['parse_cases']] == [False, True, False, False]

    # (e) (f): densities of segments of every sorter class, through the reference's est_kernel_density
    # (its parse_base_levels replaced by the prepared segments)
    segs = [rng.normal(rng.uniform(-2, 2), rng.uniform(0.15, 0.5), n)
            for n in (2, 63, 64, 65, 4095, 4096, 4097, 12003)]
    segs.append(np.concatenate([rng.normal(5.6, 0.5, 300), rng.normal(-7.0, 0.3, 40), [9.5, -11.0]]))   # outside [-5, 5]
    ident = np.full(200, 0.3)
    ident[57] = 0.35
    segs.append(ident)   # identical apart from one
    save_x = np.linspace(-5, 5, 500)
    real_parse = ts.parse_base_levels
    ts.parse_base_levels = lambda *a: dict(('s%02d' % i, list(s)) for i, s in enumerate(segs))
    dens = ts.est_kernel_density(ReadsIndex([]), std_ref, 0, None, save_x, BW, 1)
    ts.parse_base_levels = real_parse
    dens = np.array([dens['s%02d' % i] for i in range(len(segs))])
    direct = np.array([direct_density(s, save_x, BW) for s in segs])
    big = dens >= 1e-10
    spread = float(np.max(np.abs(direct[big] - dens[big]) / dens[big]))
    spread_abs = float(np.max(np.abs(direct[~big] - dens[~big])))
    print('direct evaluation vs scipy: %.3g relative above the cut, %.3g absolute below' % (spread, spread_abs))
    assert spread < 1e-13 and spread_abs < 1e-20
    out['dens_levels'] = np.concatenate(segs)
    out['dens_lv_off'] = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    out['dens_scipy'] = dens
    meta['dens_direct_spread'] = spread
    meta['dens_direct_spread_abs'] = spread_abs

    # (g): the full estimation, from the reads and from the density files the first run wrote
    save_g = np.linspace(-5, 5, G_EST)
    with tempfile.TemporaryDirectory() as td:
        base = os.path.join(td, 'dens')
        est = dict(parse_levels_batch_size=20, max_kmer_obs=10000, min_kmer_obs_to_est=50)
        del MESSAGES[:]
        alt_dens = ts.est_kernel_density(ReadsIndex(sets['alt']), std_ref, 100, base, save_g, BW_EST, 1, 'alternate', **est)
        std_dens = ts.est_kernel_density(ReadsIndex(sets['ctrl']), std_ref, 100, base, save_g, BW_EST, 1, 'control', **est)
        assert not MESSAGES, MESSAGES
        meta['std_frac'] = check_isolation_margins(alt_dens, std_dens, std_ref, save_g)
        alt_ref = ts.isolate_alt_density(alt_dens, std_dens, ALT_BASE, PCTL, std_ref, save_g)
        files = {}
        for nm in ('alternate', 'control'):
            text = open(base + '.' + nm + '_density.txt').read()
            files[nm] = dict(sha256=hashlib.sha256(text.encode()).hexdigest(), head=text.split('\n')[:3],
                             n_lines=text.count('\n'))
        f_alt = ts.parse_kmer_densities_file(base + '.alternate_density.txt')
        f_std = ts.parse_kmer_densities_file(base + '.control_density.txt')
        check_isolation_margins(f_alt, f_std, std_ref, save_g)
        alt_ref_files = ts.isolate_alt_density(f_alt, f_std, ALT_BASE, PCTL, std_ref, save_g)
    assert not MESSAGES, MESSAGES
    out['g_alt_dens'] = np.array([alt_dens[k] for k in kmers])
    out['g_std_dens'] = np.array([std_dens[k] for k in kmers])
    out['g_model'] = model_table(alt_ref)
    out['g_model_from_files'] = model_table(alt_ref_files)
    assert sorted(set(k.decode().count(ALT_BASE) for k in out['g_model']['kmer'])) == [1, 2, 3]
    meta['density_files'] = files
    meta['est_kernel_density'] = dict(kmer_obs_thresh=100, **est)
    # write_model against the HDF5 stand-in: `h5py.File(fn, 'w')` hands out the MemGroup
    grp = memh5.MemGroup()
    grp.__enter__ = lambda: grp

    class _Opened(object):
        def __init__(self, fn, mode='r'):
            pass

        def __enter__(self):
            return grp

        def __exit__(self, *a):
            return False
    ts.h5py.File = _Opened
    alt_ref.write_model('unused.model')
    ts.h5py.File = FakeFile
    tree = memh5.tree(grp)
    out['g_written_model'] = tree.pop('/model')
    meta['written_attrs'] = dict((k, v if isinstance(v, (int, str)) or v is None else int(v)) for k, v in tree.items())
    meta['written_dataset_kw'] = grp.items['model'].kw

    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'stats_alt_est.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays; std_frac', meta['std_frac'])


if __name__ == '__main__':
    main()

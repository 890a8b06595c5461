"""Golden vectors of the genome tracks from the REFERENCE (build container only).

    python tests/golden/gen_golden_tracks.py   # writes tests/golden/stats_tracks.npz

(The `stats_` prefix keeps the file out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference's get_mean_slot_genome_centric, TomboReads.iter_coverage_regions / iter_cov_regs,
get_chrm_sizes, get_signal_differences, get_largest_signal_differences (tombo/tombo_helper.py) and the three
writers write_cov_wig, write_slot_mean_wig, write_signal_and_diff_wigs (tombo/_text_output_commands.py), called
in the order write_all_browser_files calls them, on synthetic reads.  The reference loads an Events column of a
read from its FAST5 file; here that accessor (`th.get_single_slot_read_centric`) is pointed at in-memory arrays,
and the TomboReads objects are made with object.__new__ around a ready `reads_index` -- everything after that is
the reference's own code.  Only data is written: the reads and the outputs.

T below is the tile of the device pileup (tombo_amd._native.TRK_TILE); the reads are placed on its edges.
Values are normal * 10**randint(-6, 9): sums of such values depend on the order of the adds in most bits, and the
generator asserts that the deep stack tells a reversed read list from the recorded one.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import ref_oracle  # noqa: E402
from tombo_amd._native import TRK_TILE as T  # noqa: E402

rq, ts, th = ref_oracle.load()
from tombo import _text_output_commands as toc  # noqa: E402

STORE = {}
SLOTS = ('norm_mean', 'norm_stdev', 'length')
CHRMS = ['chrA', 'chrC', 'chrD', 'chrS']
WIG_TYPES = ('coverage', 'signal', 'signal_sd', 'dwell', 'difference')
ROWS = []   # (set, chrm, minus, start, end, has, columns)


def install():
    th.get_single_slot_read_centric = lambda r, name, grp=None: (
        None if STORE[r.fn] is None else STORE[r.fn][name])


def add_read(rng, index, which, chrm, strand, start, n, events=True, end=None):
    cols = None
    if events:
        mag = 10.0 ** rng.integers(-6, 10, n)
        sd = np.abs(rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-6, 10, n))
        sd[rng.random(n) < 0.06] = np.nan
        cols = {'norm_mean': rng.normal(0.0, 1.0, n) * mag, 'norm_stdev': sd,
                'length': rng.integers(1, 400, n).astype(np.uint32)}
    fn = 'r%d' % len(STORE)
    STORE[fn] = cols
    end = start + n if end is None else end
    index.setdefault((chrm, strand), []).append(
        th.readData(start, end, False, 0, strand, fn, 'grp', False, 0.0, 10.0, fn))
    ROWS.append((which, CHRMS.index(chrm), strand == '-', start, end, events, cols))


def rand_reads(rng, index, which, chrm, strand, count, lo, hi, max_len):
    """`count` reads of 1..max_len bases inside [lo, hi)"""
    for _ in range(count):
        n = int(rng.integers(1, min(max_len, hi - lo) + 1))
        add_read(rng, index, which, chrm, strand, int(rng.integers(lo, hi - n + 1)), n)


def make_sample(rng):
    idx = {}
    # case 1, '+': tile 0 holds no read at all; one read covers the tiles 1..3 exactly; the last, partial tile
    for s, n in ((T, 3 * T), (T, 50), (2 * T, 300), (2 * T - 40, 40), (3 * T - 100, 100), (T, 1), (2 * T - 1, 1),
                 (2 * T, 1), (3 * T - 1, 1), (3 * T, 1), (4 * T + 5, 12), (4 * T - 1, 1), (4 * T, 1)):
        add_read(rng, idx, 0, 'chrA', '+', s, n)
    add_read(rng, idx, 0, 'chrA', '+', 2 * T + 7, 90, events=False)    # no Events table: read coverage only
    rand_reads(rng, idx, 0, 'chrA', '+', 4, T, 4 * T + 17, 3 * T)
    rand_reads(rng, idx, 0, 'chrA', '+', 12, T, 4 * T + 17, T // 2)
    # case 1, '-': an uncovered gap [2T - 20, 2T + 30) across a tile edge; this strand ends at 4T + 3
    for s, n in ((0, T), (T - 1, 1), (T, 1), (T, T - 20), (2 * T + 30, T - 30), (3 * T, T + 3), (T - 60, 60),
                 (2 * T - 21, 1), (2 * T + 30, 1)):
        add_read(rng, idx, 0, 'chrA', '-', s, n)
    add_read(rng, idx, 0, 'chrA', '-', 40, 70, events=False)
    rand_reads(rng, idx, 0, 'chrA', '-', 10, 0, 2 * T - 20, T // 2)
    rand_reads(rng, idx, 0, 'chrA', '-', 10, 2 * T + 30, 4 * T + 3, T // 2)
    # case 2: 300 reads of 8..40 bases over the 64 positions around the first tile edge
    for _ in range(300):
        n = int(rng.integers(8, 41))
        add_read(rng, idx, 0, 'chrD', '+', int(rng.integers(T - 32, T + 32 - n + 1)), n)
    rand_reads(rng, idx, 0, 'chrS', '+', 6, 0, 300, 120)               # only in the sample
    return idx


def make_control(rng):
    idx = {}
    rand_reads(rng, idx, 1, 'chrA', '+', 14, 0, 3 * T + 50, T)    # shorter than the sample's chrA
    rand_reads(rng, idx, 1, 'chrA', '-', 14, 0, 3 * T + 50, T)
    add_read(rng, idx, 1, 'chrA', '-', 500, 60, events=False)
    rand_reads(rng, idx, 1, 'chrD', '+', 8, T - 60, T + 80, 90)       # longer than the sample's chrD
    rand_reads(rng, idx, 1, 'chrC', '-', 6, 0, 280, 100)               # only in the control
    return idx


def tombo_reads(index):
    tr = object.__new__(th.TomboReads)
    tr.reads_index = index
    tr.coverage = None
    return tr


def cov_rows(it, with_end):
    rows = [(CHRMS.index(r[0]), r[1] == '-') + tuple(int(x) for x in r[2:]) for r in it]
    return np.array(rows, dtype=np.int64).reshape(len(rows), 4 if with_end else 3)


def record_files(out, tag, samp, ctrl):
    """the reference writers in write_all_browser_files' order, for all five types"""
    with tempfile.TemporaryDirectory() as td:
        cwd = os.getcwd()
        os.chdir(td)
        try:
            group = '' if ctrl is None else toc.GROUP_NAME
            if ctrl is not None:
                sizes = th.get_chrm_sizes(samp, ctrl)
                toc.write_cov_wig(ctrl, 'trk', toc.CTRL_NAME)
                toc.write_slot_mean_wig(ctrl, sizes, 'trk', toc.CTRL_NAME, toc.SD_WIG_TYPE, toc.SD_SLOT)
                toc.write_slot_mean_wig(ctrl, sizes, 'trk', toc.CTRL_NAME, toc.DWELL_WIG_TYPE, toc.DWELL_SLOT)
                toc.write_signal_and_diff_wigs(samp, ctrl, sizes, 'trk', group, True, True)
            else:
                sizes = th.get_chrm_sizes(samp)
                toc.write_signal_and_diff_wigs(samp, None, sizes, 'trk', group, True, False)
            toc.write_cov_wig(samp, 'trk', group)
            toc.write_slot_mean_wig(samp, sizes, 'trk', group, toc.SD_WIG_TYPE, toc.SD_SLOT)
            toc.write_slot_mean_wig(samp, sizes, 'trk', group, toc.DWELL_WIG_TYPE, toc.DWELL_SLOT)
            import gc
            gc.collect()    # (write_signal_and_diff_wigs leaves its files to the collector)
            names = sorted(os.listdir('.'))
            out['files_%s_names' % tag] = np.array(names)
            for i, name in enumerate(names):
                out['files_%s_%d' % (tag, i)] = np.frombuffer(open(name, 'rb').read(), dtype=np.uint8)
        finally:
            os.chdir(cwd)


def main():
    install()
    rng = np.random.default_rng(5150)
    samp_idx, ctrl_idx = make_sample(rng), make_control(rng)
    samp, ctrl = tombo_reads(samp_idx), tombo_reads(ctrl_idx)
    out = {'T': np.array(T), 'chrm_names': np.array(CHRMS)}
    lens = [0 if r[6] is None else r[6]['norm_mean'].shape[0] for r in ROWS]
    out.update(rd_set=np.array([r[0] for r in ROWS]), rd_chrm=np.array([r[1] for r in ROWS]),
               rd_minus=np.array([r[2] for r in ROWS]), rd_start=np.array([r[3] for r in ROWS]),
               rd_end=np.array([r[4] for r in ROWS]), rd_has=np.array([r[5] for r in ROWS]),
               rd_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    for key, slot in (('rd_mean', 'norm_mean'), ('rd_sd', 'norm_stdev'), ('rd_len', 'length')):
        out[key] = np.concatenate([r[6][slot] for r in ROWS if r[6] is not None])

    for tag, sizes in (('s', th.get_chrm_sizes(samp)), ('sc', th.get_chrm_sizes(samp, ctrl))):
        out['sizes_%s_chrm' % tag] = np.array([CHRMS.index(c) for c in sorted(sizes)])
        out['sizes_%s' % tag] = np.array([sizes[c] for c in sorted(sizes)], dtype=np.int64)
    sizes = th.get_chrm_sizes(samp, ctrl)
    with np.errstate(all='ignore'):
        for which, index in ((0, samp_idx), (1, ctrl_idx)):
            for (chrm, strand), reads in index.items():
                for slot in SLOTS:
                    out['mean_%d_%s_%s_%s' % (which, chrm, strand, slot)] = th.get_mean_slot_genome_centric(
                        reads, sizes[chrm], slot)
        # case 2 can tell a reordered sum: reversing the read list changes at least a third of the covered means
        deep = samp_idx[('chrD', '+')]
        fwd = th.get_mean_slot_genome_centric(deep, sizes['chrD'], 'norm_mean')
        rev = th.get_mean_slot_genome_centric(deep[::-1], sizes['chrD'], 'norm_mean')
    covered = ~np.isnan(fwd)
    changed = int((fwd[covered] != rev[covered]).sum())
    print('deep stack: %d of %d covered means change when the reads are reversed' % (changed, int(covered.sum())))
    assert 3 * changed >= int(covered.sum())

    max_cov = 0
    for tag, c in (('s', None), ('sc', ctrl)):
        regs = list(samp.iter_coverage_regions(c))
        out['covreg_%s_cs' % tag] = np.array([[CHRMS.index(r[0]), r[1] == '-'] for r in regs], dtype=np.int64)
        for i, r in enumerate(regs):
            out['covreg_%s_%d_cov' % (tag, i)] = r[2]
            out['covreg_%s_%d_starts' % (tag, i)] = r[3]
            max_cov = max(max_cov, int(r[2].max()))
    out['max_cov'] = np.array(max_cov)
    for thresh in (1, 5, max_cov + 1):
        for rs in (100, None):
            for tag, c in (('s', None), ('sc', ctrl)):
                out['covregs_%s_t%d_r%s' % (tag, thresh, rs)] = cov_rows(samp.iter_cov_regs(thresh, rs, c), rs is None)

    diffs = th.get_signal_differences(samp, ctrl)
    out['diff_cs'] = np.array([[CHRMS.index(c), s == '-'] for c, s in diffs], dtype=np.int64)
    nz = []
    for i, d in enumerate(diffs.values()):
        out['diff_%d' % i] = d
        nz.append(np.abs(d[d != 0]))
    nz = np.concatenate(nz)
    assert np.unique(nz).shape[0] == nz.shape[0], 'two nonzero |differences| are equal'
    out['n_nonzero'], out['num_bases'] = np.array(nz.shape[0]), np.array(21)
    for n in (1, 5, int(nz.shape[0])):
        res = th.get_largest_signal_differences(samp, ctrl, n, 21)
        out['largest_%d_val' % n] = np.array([r[0] for r in res], dtype=np.float64)
        out['largest_%d_rest' % n] = np.array([[r[1], CHRMS.index(r[2]), r[3] == '-'] for r in res], dtype=np.int64)

    record_files(out, 's', samp, None)
    record_files(out, 'sc', samp, ctrl)
    path = os.path.join(HERE, 'stats_tracks.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

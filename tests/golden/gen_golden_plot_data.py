"""Golden vectors of the region plot data frames from the REFERENCE (build container only).

    python tests/golden/gen_golden_plot_data.py   # writes tests/golden/stats_plot_data.npz

(The `stats_` prefix keeps the npz out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference (tools/ref_oracle.py) with
  h5py.File                          pointed at dict-backed groups (tests/store_memh5.py) that hold Raw/Reads/Read_0/Signal,
                                     the Events table and the shift / scale / lower_lim / upper_lim / outlier_threshold
                                     attributes of the corrected group
  th.get_single_slot_read_centric    pointed at in-memory arrays (norm_mean, base)
  _plot_commands.r                   a stand-in whose DataFrame / FloatVector / IntVector / StrVector / FactorVector
                                     return plain dicts and lists
  np.NAN restored, the `interpolation=` deprecation warning silenced
and records, for every case below, what tombo/_plot_commands.py computes before it calls R:
  get_plots_titles :1256   get_base_r_data :986   get_r_raw_signal_data :907   get_r_quant_data :865
  get_r_boxplot_data :823  get_r_event_data :784  get_plot_types_data :978
  the bodies of plot_single_sample :1336-1351 and plot_two_samples :1384-1409 (group frames concatenated where the
  reference rbinds them, quantile offsets 0.1 and 0.5)
Only data is written: the reads (levels, raw DAC values, segments, scale values, sequences), the regions, the cases
and the recorded frames.

The Events `start` / `length` columns are stored as int64.  A FAST5 file holds them as uint32, and the reference
negates the segments of a minus-strand read (`segs[::-1] * -1`, tombo_helper.py:2113): under the numpy it was
written for that promoted to int64, under numpy 2 it raises OverflowError, which its bare `except` would turn
into the "could not be retrieved" warning for every minus-strand read.  int64 columns restore the arithmetic it
was written for; nothing else changes.

Reads (chromosome chrP): zone S [20, 70) about 8 DNA reads per strand with raw signal in every layout towards
the regions (contained, hanging over the start, the end, both, starting / ending exactly at a region's start /
end, ending exactly at a region's start and starting exactly at its end: no overlap), bases of a single sample, a
read without raw signal, reads without winsorising limits; zone Q [100, 121) 151 plus-strand reads over
[100, 111) of which 51 go on to 121 (piles of 151 and 51: (n - 1) * 0.01 is 1.5 and 0.5, where round-half-even
shows), levels multiples of 1/64 with ties and full-mantissa levels, and 5 minus-strand reads; zone L [150, 185)
coverages 1, 2 and 3, NaN levels inside reads and a position whose every level is NaN; zone R [200, 240) RNA
reads.  A control group of reads lies over parts of zones S and Q."""
import os
import sys
import json
import types
import warnings
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_oracle  # noqa: E402
import store_memh5  # noqa: E402

rq, ts, th = ref_oracle.load()

CHRM, CHRM_LEN, CORR_GROUP = 'chrP', 300, 'RawGenomeCorrected_000/BaseCalled_template'
STORES, READ_SLOTS = {}, {}
# (start, end, strand, reg_id, reg_text)
REGIONS = [(30, 51, '+', 'r00', 'plus'), (30, 51, '-', 'r01', 'minus'), (25, 66, None, 'r02', 'both wide'),
           (40, 51, None, 'r03', 'both narrow'), (100, 121, '+', 'r04', 'deep plus'), (105, 116, None, 'r05', 'deep both'),
           (200, 231, '+', 'r06', 'rna'), (150, 171, None, 'r07', 'low'), (280, 291, None, 'r08', 'empty'),
           (160, 181, None, 'r09', 'nan'), (205, 236, None, 'r10', 'rna both')]
# name -> (kind, regions, overplot_type, overplot_thresh, seed, options)
CASES = [
    ('signal', 'single', [0, 1, 2, 3, 7, 8, 9], 'Quantile', 50, 1, {}),
    ('downsample_5', 'single', [0, 1, 2, 3, 4, 5, 7], 'Downsample', 5, 2, {}),
    ('downsample_200', 'single', [2, 5, 6], 'Downsample', 200, 3, {}),
    ('quantile', 'single', [0, 2, 4, 5, 7, 9, 10], 'Quantile', 4, 4, {}),
    ('boxplot', 'single', [1, 2, 4, 5, 7, 9, 6], 'Boxplot', 4, 5, {}),
    ('density', 'single', [0, 2, 3, 4, 5, 7, 9, 10], 'Density', 4, 6, {}),
    ('rna', 'single', [6, 10], 'Boxplot', 50, 7, {'is_rna': True}),
    ('no_titles', 'single', [0, 2, 5], 'Density', 8, 8, {'title_include_chrm': False, 'title_include_cov': False}),
    ('read_centric', 'frames', [0, 1, 2, 3, 6, 10], 'Downsample', 6, 9, {'genome_centric': False}),
    ('two_signal', 'two', [0, 1, 2, 3, 8], 'Boxplot', 50, 10, {}),
    ('two_quantile', 'two', [2, 4, 5], 'Quantile', 4, 11, {}),
    ('two_density', 'two', [2, 3, 4, 5], 'Density', 4, 12, {}),
    ('two_downsample', 'two', [1, 2, 5], 'Downsample', 4, 13, {}),
    ('two_boxplot', 'two', [2, 4, 5, 7], 'Boxplot', 4, 14, {}),
]


class H5Stub(object):
    def __init__(self, group):
        self.group = group

    def __enter__(self):
        return self.group

    def __exit__(self, *exc):
        return False


class StandInR(object):
    DataFrame = staticmethod(lambda d: d)
    FloatVector = staticmethod(lambda v: [float(x) for x in v])
    IntVector = staticmethod(lambda v: [int(x) for x in v])
    StrVector = staticmethod(lambda v: [str(x) for x in v])

    @staticmethod
    def FactorVector(v, ordered=True, levels=None):
        assert ordered and list(levels) == ['Forward Strand', 'Reverse Strand']
        return list(v)


def load_plot_commands():
    for name, attrs in (('future', {}), ('future.utils', dict(native=lambda x: x)), ('tqdm', dict(tqdm=lambda x, **kw: x)),
                        ('pkg_resources', dict(resource_string=lambda *a: b''))):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            mod.__dict__.update(attrs)
            sys.modules[name] = mod
    from tombo import _plot_commands as pc
    pc.r = StandInR
    pc.VERBOSE = False
    return pc


def install():
    th.h5py.File = lambda fn, mode='r': H5Stub(STORES[fn])     # (a read without a file: KeyError, the reference's except)
    np.NAN = np.float64(np.nan)
    warnings.filterwarnings('ignore', message='.*interpolation=.*')
    th.get_single_slot_read_centric = lambda r, name, grp=None: READ_SLOTS[r.fn].get(name)


TOMBO_READS = th.TomboReads


def tombo_reads(index):
    tr = object.__new__(TOMBO_READS)
    tr.reads_index = index
    tr.coverage = None
    return tr


def make_reads(rng, genome):
    """-> list of dicts: start, end, strand, rna, group, means (read-centric), raw, segs, rsrtr, scale values"""
    specs = []     # (start, end, strand, rna, group, flags)
    # zone S: every layout towards [30, 51), [25, 66) and [40, 51)
    for strand in '+-':
        for a, b in ((33, 47), (22, 40), (45, 68), (20, 70), (30, 51), (26, 30), (51, 60), (30, 44), (41, 51), (24, 67)):
            specs.append((a, b, strand, False, 0, set()))
    specs[2][5].add('no_raw')
    specs[4][5].add('no_limits')
    specs[13][5].add('no_limits')
    specs[1][5].add('one_sample_bases')
    specs[14][5].add('one_sample_bases')
    for strand in '+-':
        for a, b in ((28, 55), (35, 52), (21, 45), (38, 69)):
            specs.append((a, b, strand, False, 1, set()))
    # zone Q
    for i in range(151):
        specs.append((100 - i % 3, 121 + i % 2 if i < 51 else 111, '+', False, 0, {'q'} if i % 4 else {'q', 'sixtyfourths'}))
    for i in range(5):
        specs.append((98 + i, 119 + i, '-', False, 0, {'q'}))
    for i in range(9):
        specs.append((99, 113 + i, '+', False, 1, {'q', 'sixtyfourths'}))
    for i in range(4):
        specs.append((101 + i, 121, '-', False, 1, {'q'}))
    # zone L: coverage 1, 2, 3; NaN levels
    for a, b, strand in ((150, 158, '+'), (154, 166, '+'), (156, 185, '+'), (160, 178, '+'), (162, 180, '-'),
                         (152, 175, '-'), (165, 184, '-')):
        specs.append((a, b, strand, False, 0, {'nan'}))
    # zone R: RNA
    for a, b, strand in ((198, 233, '+'), (203, 225, '+'), (210, 240, '+'), (200, 231, '+'), (207, 229, '-'),
                         (201, 238, '-'), (212, 236, '+')):
        specs.append((a, b, strand, True, 0, set()))
    reads = []
    for i, (a, b, strand, rna, group, flags) in enumerate(specs):
        n = b - a
        means = rng.standard_normal(n) + rng.random(n) * 1e-3
        if 'sixtyfourths' in flags:
            means = rng.integers(-40, 41, n) / 64.0
        if 'nan' in flags:
            means[rng.random(n) < 0.2] = np.nan
            g = np.arange(a, b)[::-1] if strand == '-' else np.arange(a, b)
            means[g == 168] = np.nan                       # a position whose every level is NaN
        dwell = rng.integers(3, 15, n) if 'q' not in flags else rng.integers(2, 7, n)
        if 'one_sample_bases' in flags:
            dwell[::3] = 1
        segs = np.concatenate([[0], np.cumsum(dwell)]).astype(np.int64)
        rsrtr = int(rng.integers(0, 40))
        raw = np.clip(np.rint(rng.standard_normal(rsrtr + int(segs[-1]) + int(rng.integers(0, 25))) * 80 + 500),
                      0, 2000).astype(np.int16)
        fwd = genome[a:b]
        reads.append(dict(
            start=a, end=b, strand=strand, rna=rna, group=group, means=means, segs=segs, rsrtr=rsrtr,
            raw=None if 'no_raw' in flags else raw, shift=float(500 + rng.standard_normal() * 7),
            scale=float(80 + rng.random() * 9), lower=None if 'no_limits' in flags else float(-1.4 - rng.random() * 0.3),
            upper=None if 'no_limits' in flags else float(1.5 + rng.random() * 0.3),
            seq=fwd if strand == '+' else th.rev_comp(fwd), fn='read%d' % i))
    return reads


def register(reads):
    """the reference's view of the reads: files, Events slots, index per group"""
    index = {0: {}, 1: {}}
    for rd in reads:
        fn = rd['fn']
        READ_SLOTS[fn] = dict(norm_mean=rd['means'], base=np.frombuffer(rd['seq'].encode(), dtype='S1'))
        if rd['raw'] is not None:
            f5 = store_memh5.StoreGroup()
            grp = f5.create_group('Analyses').create_group('RawGenomeCorrected_000').create_group('BaseCalled_template')
            ev = np.zeros(rd['segs'].shape[0] - 1, dtype=[('start', 'i8'), ('length', 'i8')])
            ev['start'], ev['length'] = rd['segs'][:-1], np.diff(rd['segs'])
            grp.create_dataset('Events', data=ev)
            grp.attrs.update(shift=np.float64(rd['shift']), scale=np.float64(rd['scale']), outlier_threshold=np.float64(5.0))
            if rd['lower'] is not None:
                grp.attrs.update(lower_lim=np.float64(rd['lower']), upper_lim=np.float64(rd['upper']))
            f5.create_group('Raw').create_group('Reads').create_group('Read_0').create_dataset('Signal', data=rd['raw'])
            STORES[fn] = f5
        index[rd['group']].setdefault((CHRM, rd['strand']), []).append(
            th.readData(rd['start'], rd['end'], False, rd['rsrtr'], rd['strand'], fn, CORR_GROUP, rd['rna'], 0.0, 10.0, fn))
    return tombo_reads(index[0]), tombo_reads(index[1])


def intervals(which):
    return [th.intervalData(CHRM, a, b, strand, reg_id, text) for a, b, strand, reg_id, text in (REGIONS[i] for i in which)]


def record(out, case, name, frame):
    for col, values in frame.items():
        kind = 'U' if col in ('Read', 'Strand', 'Region', 'Group', 'Base', 'Title') else \
            'i8' if (col == 'Position' and name in ('Box', 'Event')) else 'f8'
        out['%s|%s|%s' % (case, name, col)] = np.array(values, dtype=kind) if len(values) else np.empty(0, dtype=kind)


def rbind(f1, f2):
    return dict((k, list(f1[k]) + list(f2[k])) for k in f1)


def main():
    install()
    pc = load_plot_commands()
    rng = np.random.default_rng(20261020)
    genome = ''.join(rng.choice(list('ACGT'), CHRM_LEN))
    reads = make_reads(rng, genome)
    sample, control = register(reads)
    out, meta = {}, {'cases': {}}
    warned = []
    th.warning_message = lambda msg: warned.append(msg)
    for case, kind, which, overplot_type, thresh, seed, opts in CASES:
        np.random.seed(seed)
        del warned[:]
        info = dict(kind=kind, regions=which, overplot_type=overplot_type, overplot_thresh=thresh, seed=seed, opts=opts)
        if kind == 'single':
            # the body of plot_single_sample (:1340-1351); is_rna is what th.is_sample_rna reads from the files
            plot_intervals = intervals(which)
            for p_int in plot_intervals:
                p_int.add_reads(sample).add_seq()
            plot_intervals = th.filter_empty_regions(plot_intervals)
            Titles, plot_types = pc.get_plots_titles(
                plot_intervals, None, overplot_type, thresh, include_chrm=opts.get('title_include_chrm', True),
                include_cov=opts.get('title_include_cov', True))
            Bases = pc.get_base_r_data(plot_intervals, is_rna=opts.get('is_rna', False))
            frames = pc.get_plot_types_data((plot_intervals, plot_types, thresh, 'Group1'))
        elif kind == 'frames':
            # the frame functions called one by one, read-centric; titles with model_plot
            plot_intervals = [p.add_reads(sample).add_seq() for p in intervals(which)]
            Titles, plot_types = pc.get_plots_titles(plot_intervals, None, overplot_type, thresh, model_plot=True)
            info['titles_density_model'] = pc.get_plots_titles(plot_intervals, None, 'Density', thresh, model_plot=True)[0]['Title']
            Bases = pc.get_base_r_data(plot_intervals, zero_start=True, is_rna=True, genome_centric=False)
            record(out, case, 'BasesNotZero', pc.get_base_r_data(plot_intervals, genome_centric=False))
            args = (plot_intervals, plot_types, thresh, 'GroupX')
            frames = (pc.get_r_raw_signal_data(*args, genome_centric=False),
                      pc.get_r_quant_data(*args, pos_offest=0.25, pcntls=[5, 25, 45]), pc.get_r_boxplot_data(*args),
                      pc.get_r_event_data(*args))
        else:
            # the body of plot_two_samples (:1390-1409)
            plot_intervals = intervals(which)
            all1 = [p.copy().add_reads(sample) for p in plot_intervals]
            all2 = [p.copy().add_reads(control) for p in plot_intervals]
            merged, all1, all2 = pc.filter_and_merge_regs(all1, all2)
            Titles, plot_types = pc.get_plots_titles(all1, all2, overplot_type, thresh)
            Bases = pc.get_base_r_data(merged)
            f1 = pc.get_plot_types_data((all1, plot_types, thresh, 'Group1'), 0.1)
            f2 = pc.get_plot_types_data((all2, plot_types, thresh, 'Group2'), 0.5)
            frames = tuple(rbind(a, b) for a, b in zip(f1, f2))
        for name, frame in zip(('Signal', 'Quant', 'Box', 'Event'), frames):
            record(out, case, name, frame)
        record(out, case, 'Bases', Bases)
        record(out, case, 'Titles', Titles)
        info.update(plot_types=list(plot_types), warned=list(warned),
                    rows=dict((n, len(f[next(iter(f))])) for n, f in zip(('Signal', 'Quant', 'Box', 'Event'), frames)))
        meta['cases'][case] = info
    # every plot type and the warning occur
    seen = set(t for c in meta['cases'].values() for t in c['plot_types'])
    assert seen == {'Signal', 'Downsample', 'Quantile', 'Boxplot', 'Density'}, seen
    assert any(c['warned'] for c in meta['cases'].values())
    for n in ('Signal', 'Quant', 'Box', 'Event'):
        assert all(any(c['rows'][n] > 0 for c in meta['cases'].values() if c['kind'] == k) for k in ('single', 'two')), n
    # get_base_levels: matrices, the shuffle under a seed, the error text
    lv_reg = intervals([2])[0].add_reads(sample)
    out['base_levels|all'] = lv_reg.get_base_levels()
    out['base_levels|rows'] = intervals([1])[0].add_reads(sample).get_base_levels(read_rows=True)
    np.random.seed(77)
    out['base_levels|num_reads_5'] = lv_reg.get_base_levels(num_reads=5)
    meta['base_levels_order_after_shuffle'] = [r.fn for r in lv_reg.reads]
    try:
        intervals([8])[0].add_reads(sample).get_base_levels()
        raise AssertionError('accepted')
    except th.TomboError as e:
        meta['no_reads_error'] = str(e)
    meta['full_span'] = [r.fn for r in intervals([2])[0].add_reads(sample, require_full_span=True).reads]
    # the scenario
    meta.update(chrm=CHRM, genome=genome, regions=[list(r) for r in REGIONS],
                reads=[dict(start=r['start'], end=r['end'], strand=r['strand'], rna=r['rna'], group=r['group'], fn=r['fn'],
                            rsrtr=r['rsrtr'], shift=r['shift'], scale=r['scale'], lower=r['lower'], upper=r['upper'],
                            seq=r['seq'], has_raw=r['raw'] is not None) for r in reads])
    csr = (lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64))
    out['means'], out['means_off'] = np.concatenate([r['means'] for r in reads]), csr([r['means'] for r in reads])
    raws = [r['raw'] if r['raw'] is not None else np.empty(0, dtype=np.int16) for r in reads]
    out['raw'], out['raw_off'] = np.concatenate(raws), csr(raws)
    out['segs'], out['segs_off'] = np.concatenate([r['segs'] for r in reads]), csr([r['segs'] for r in reads])
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'stats_plot_data.npz')
    np.savez_compressed(path, **out)
    print('stats_plot_data.npz %.1f KB, %d arrays, %d reads' % (os.path.getsize(path) / 1024., len(out), len(reads)))
    for case, info in meta['cases'].items():
        print(' %-15s %s %s' % (case, info['plot_types'], info['rows']))


if __name__ == '__main__':
    main()

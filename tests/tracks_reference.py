"""TEST INFRASTRUCTURE: the genome-track functions of the reference restated in numpy, in this project's own words
(tombo_helper.py:396-421, 1394-1485, 1661-1742; _text_output_commands.py:64-93, 230-320), pinned to the reference's
recorded output by tests/test_tracks_reference.py.  The sums are numpy's own slice adds, read after read, as in the
reference: they are what the device kernels have to reproduce bit for bit.

A read here is any object with start, end, strand; its Events columns come from `cols`, a list parallel to the reads
of {slot name: read-centric array} or None (no Events table)."""
import io
import os

import numpy as np

SLOT_OF_TYPE = {'signal': 'norm_mean', 'signal_sd': 'norm_stdev', 'dwell': 'length'}


class Read(object):
    def __init__(self, start, end, strand, read_id=None, means=None):
        self.start, self.end, self.strand, self.read_id, self.means = start, end, strand, read_id, means


def chrm_sizes(index, ctrl_index=None):
    sizes = {}
    for idx in (index, ctrl_index):
        for (chrm, _), reads in ([] if idx is None else idx.items()):
            if reads:
                sizes[chrm] = max(sizes.get(chrm, 0), max(r.end for r in reads))
    return sizes


def slot_sums(reads, cols, chrm_len, slot):
    """(sums, coverage) of one slot over one read list, reads added in list order"""
    sums, cov = np.zeros(chrm_len), np.zeros(chrm_len, dtype=np.int64)
    for r, c in zip(reads, cols):
        if c is None or c.get(slot) is None:
            continue
        v = c[slot][::-1] if r.strand == '-' else c[slot]
        sums[r.start:r.start + len(v)] += v
        cov[r.start:r.start + len(v)] += 1
    return sums, cov


def slot_mean(reads, cols, chrm_len, slot):
    sums, cov = slot_sums(reads, cols, chrm_len, slot)
    with np.errstate(all='ignore'):
        return sums / cov


def coverage(index):
    out = {}
    for cs, reads in index.items():
        if reads:
            c = np.zeros(max(r.end for r in reads), dtype=np.int64)
            for r in reads:
                c[r.start:r.end] += 1
            out[cs] = c
    return out


def merged_coverage(index, ctrl_index):
    cov, out = coverage(index), {}
    for cs, c in coverage(ctrl_index).items():
        if cs in cov:
            a, b = (cov[cs], c) if cov[cs].shape[0] > c.shape[0] else (c, cov[cs])
            out[cs] = a.copy()
            out[cs][:b.shape[0]] += b
        else:
            out[cs] = c.copy()
    return out


def run_lengths(cov):
    """-> (run starts followed by len(cov), run values)"""
    starts = np.concatenate([[0], np.flatnonzero(np.diff(cov)) + 1, [cov.shape[0]]])
    return starts, cov[starts[:-1]]


def coverage_regions(index, ctrl_index=None):
    cov = coverage(index) if ctrl_index is None else merged_coverage(index, ctrl_index)
    return [(cs[0], cs[1]) + run_lengths(c)[::-1] for cs, c in cov.items()]


def cov_regs(index, thresh, region_size=None, ctrl_index=None):
    out = []
    for chrm, strand, cov, starts in coverage_regions(index, ctrl_index):
        last = -1
        cross = np.flatnonzero(np.diff(np.concatenate([[False], cov >= thresh, [False]])))
        for i, j in zip(cross[:-1], cross[1:]):
            if region_size is None:
                out.append((chrm, strand, int(starts[i]), int(starts[j])))
                continue
            lo = int(region_size * np.floor(starts[i] / float(region_size)))
            hi = int(region_size * np.ceil(starts[j] / float(region_size)))
            for s in range(lo, hi, region_size):
                if s != last:
                    out.append((chrm, strand, s))
                    last = s
    return out


def mean_slot_values(index, cols, sizes, slot, ctrl_index=None, ctrl_cols=None):
    """[(chrm, strand, sample means or None, control means or None)]"""
    out = []
    for chrm in sorted(sizes):
        for strand in '+-':
            cs = (chrm, strand)
            a = slot_mean(index[cs], cols[cs], sizes[chrm], slot) if cs in index else None
            b = None
            if ctrl_index is not None and cs in ctrl_index:
                b = slot_mean(ctrl_index[cs], ctrl_cols[cs], sizes[chrm], slot)
            if a is not None or b is not None:
                if ctrl_index is not None or a is not None:
                    out.append((chrm, strand, a, b))
    return out


def signal_differences(index, cols, ctrl_index, ctrl_cols):
    sizes = chrm_sizes(index, ctrl_index)
    return dict(((c, s), np.nan_to_num(a - b))
                for c, s, a, b in mean_slot_values(index, cols, sizes, 'norm_mean', ctrl_index, ctrl_cols)
                if a is not None and b is not None)


def top_n(a, b, n):
    """(values, positions) of the n largest nan_to_num(|a - b|), largest first, equal values: higher position first"""
    d = np.nan_to_num(np.abs(a - b))
    order = np.lexsort((np.arange(d.shape[0]), d))[::-1][:n]
    return d[order], order


def largest_signal_differences(index, cols, ctrl_index, ctrl_cols, num_regions, num_bases):
    sizes, found = chrm_sizes(index, ctrl_index), []
    for c, s, a, b in mean_slot_values(index, cols, sizes, 'norm_mean', ctrl_index, ctrl_cols):
        if a is None or b is None:
            continue
        vals, poss = top_n(a, b, num_regions)
        found.extend((v, max(int(p) - int(num_bases / 2.0), 0), c, s) for v, p in zip(vals, poss))
    return sorted(found, reverse=True)[:num_regions]


# ---- the browser files ---------------------------------------------------------------------------
def _header(kind, base, type_name, strand_name, group):
    return 'track type=%s name="%s_%s_%s%s" description="%s %s %s%s"\n' % (
        kind, base, type_name, strand_name, '_' + group if group else '', base, type_name, strand_name,
        ' ' + group if group else '')


class Files(object):
    """the files of one run as {name: text}"""

    def __init__(self):
        self.text = {}

    def open_pair(self, base, group, type_name, ext='wig'):
        names = []
        for strand_file, strand_name in (('plus', 'fwd_strand'), ('minus', 'rev_strand')):
            name = '%s.%s%s.%s.%s' % (base, type_name, '.' + group if group else '', strand_file, ext)
            self.text[name] = _header('wiggle_0' if ext == 'wig' else 'bedGraph', base, type_name, strand_name, group)
            names.append(name)
        return dict(zip('+-', names))

    def values(self, name, chrm, poss, vals):
        self.text[name] += 'variableStep chrom=%s span=1\n' % chrm
        self.text[name] += '\n'.join('%d %.4f' % (p + 1, v) for p, v in zip(poss, vals)) + '\n'


def not_nan(v):
    keep = np.flatnonzero(~np.isnan(v))
    return keep, v[keep]


def browser_files(base, wig_types, index, cols, ctrl_index=None, ctrl_cols=None):
    """what write_all_browser_files leaves behind for the five in-scope types -> {file name: text}"""
    f = Files()
    group = 'sample' if ctrl_index is not None else ''
    sizes = chrm_sizes(index, ctrl_index)

    def cov_file(idx, grp):
        names = f.open_pair(base, grp, 'coverage', 'bedgraph')
        for chrm, strand, cov, starts in coverage_regions(idx):
            f.text[names[strand]] += '\n'.join(
                '%s\t%d\t%d\t%d' % (chrm, starts[i], starts[i + 1], cov[i]) for i in range(cov.shape[0])) + '\n'

    def slot_file(idx, cl, grp, wig_type):
        names = f.open_pair(base, grp, wig_type)
        for chrm, strand, a, _ in mean_slot_values(idx, cl, sizes, SLOT_OF_TYPE[wig_type]):
            f.values(names[strand], chrm, *not_nan(a))

    def signal_files():
        sig, diff = 'signal' in wig_types, 'difference' in wig_types and ctrl_index is not None
        n1 = f.open_pair(base, group, 'signal') if sig else None
        n2 = f.open_pair(base, 'control', 'signal') if sig and ctrl_index is not None else None
        nd = f.open_pair(base, '', 'difference') if diff else None
        for chrm, strand, a, b in mean_slot_values(index, cols, sizes, 'norm_mean', ctrl_index, ctrl_cols):
            if a is not None:
                p1, v1 = not_nan(a)
                if sig:
                    f.values(n1[strand], chrm, p1, v1)
            if b is not None:
                p2, v2 = not_nan(b)
                if sig:
                    f.values(n2[strand], chrm, p2, v2)
                if a is not None and diff:
                    both = np.intersect1d(p1, p2, assume_unique=True)
                    f.values(nd[strand], chrm, both, a[both] - b[both])

    if ctrl_index is not None:
        if 'coverage' in wig_types:
            cov_file(ctrl_index, 'control')
        for t in ('signal_sd', 'dwell'):
            if t in wig_types:
                slot_file(ctrl_index, ctrl_cols, 'control', t)
        if 'signal' in wig_types or 'difference' in wig_types:
            signal_files()
    elif 'signal' in wig_types:
        signal_files()
    if 'coverage' in wig_types:
        cov_file(index, group)
    for t in ('signal_sd', 'dwell'):
        if t in wig_types:
            slot_file(index, cols, group, t)
    return f.text


# ---- the recorded cases (tests/golden/stats_tracks.npz) ------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stats_tracks.npz')
WIG_TYPES = ('coverage', 'signal', 'signal_sd', 'dwell', 'difference')


def load_reads(g, which):
    """the recorded reads of set `which` (0 sample, 1 control) -> (index {(chrm, strand): [Read]} in the generator's
    order, cols {(chrm, strand): [columns or None]})"""
    names = [str(x) for x in g['chrm_names']]
    index, cols = {}, {}
    off = g['rd_off']
    for q in np.flatnonzero(g['rd_set'] == which):
        cs = (names[g['rd_chrm'][q]], '-' if g['rd_minus'][q] else '+')
        c = None
        if g['rd_has'][q]:
            a, b = int(off[q]), int(off[q + 1])
            c = {'norm_mean': g['rd_mean'][a:b], 'norm_stdev': g['rd_sd'][a:b], 'length': g['rd_len'][a:b]}
        index.setdefault(cs, []).append(Read(int(g['rd_start'][q]), int(g['rd_end'][q]), cs[1], 'r%d' % q,
                                             None if c is None else c['norm_mean']))
        cols.setdefault(cs, []).append(c)
    return index, cols


def slot_maps(cols):
    """cols -> {slot name: {(chrm, strand): [column or None per read]}}: the `slots` of the public functions"""
    return dict((slot, dict((cs, [None if c is None else c[slot] for c in cl]) for cs, cl in cols.items()))
                for slot in ('norm_mean', 'norm_stdev', 'length'))

"""The data frames of the region plots (`tombo plot genome_locations`, `max_coverage`, `motif_centered`,
`max_difference`, `most_significant`, `per_read`): what tombo/_plot_commands.py hands to R, for reads held in
memory.  Names, arguments and defaults are the reference's (get_plots_titles :1256, get_base_r_data :986,
get_r_raw_signal_data :907, get_r_quant_data :865, get_r_boxplot_data :823, get_r_event_data :784,
get_plot_types_data :978, plot_single_sample / plot_two_samples :1336 / :1384 up to their R calls).  Drawing (R,
rpy2) is not built: the product is the frames.

A frame is an ordered dict of column name -> numpy array where the reference builds an `r.DataFrame`: float64 for
FloatVector, int64 for IntVector, an object array of str for StrVector; the strand factor is a str column whose
levels are STRAND_LEVELS.  The numbers come from the device (csrc/k_plot.h): each frame function makes ONE engine
call for all regions of its plot type.

Regions are `th.intervalData`.  Reads carry `start`, `end`, `strand`, read-centric `means`; for the signal frame
also `raw_signal` (the stored DAC integers, int16 or int32), `segs` (the Events start column plus the end),
`read_start_rel_to_raw`, `rna` and `scale_values` (th.scaleValues; None limits: no clip).  PlotRead is one such
type; any object with the attributes is accepted."""
import warnings
from collections import OrderedDict, namedtuple

import numpy as np

from . import tombo_helper as th
from . import _native

# quantiles and especially density plots need at least 3 values to be meaningful (_plot_commands.py:35-37)
QUANT_MIN = 3
FWD_STRAND = 'Forward Strand'
REV_STRAND = 'Reverse Strand'
STRAND_LEVELS = (FWD_STRAND, REV_STRAND)

RAW_SIGNAL_WARNING = ('Genome resolved raw signal could not be retrieved for some reads. Ensure that reads have been '
                      're-squiggled with the specified [--corrected-group].')

PlotRead = namedtuple('PlotRead', ('start', 'end', 'strand', 'means', 'raw_signal', 'segs', 'read_start_rel_to_raw',
                                   'rna', 'scale_values', 'seq'))
PlotRead.__new__.__defaults__ = (None,) * 6


def _engine(engine=None):
    if engine is not None:
        return engine
    from . import resquiggle as rq
    return rq.get_engine()


def _strs(values):
    out = np.empty(len(values), dtype=object)
    out[:] = values
    return out


def _cat(parts, dtype):
    return np.concatenate(parts).astype(dtype, copy=False) if parts else np.empty(0, dtype=dtype)


def _strand_name(strand):
    return FWD_STRAND if strand == '+' else REV_STRAND


def get_plots_titles(all_reg_data, all_reg_data2, overplot_type, overplot_thresh, model_plot=False,
                     include_chrm=True, include_cov=True):
    """-> (Titles frame, plot_types): the title and the plot type of every region (_plot_commands.py:1256-1334)"""
    strand_cov = []
    for reg_i in range(len(all_reg_data)):
        reg_cov1 = [sum(r_data.strand == '+' for r_data in all_reg_data[reg_i].reads),
                    sum(r_data.strand == '-' for r_data in all_reg_data[reg_i].reads)]
        reg_cov2 = [] if all_reg_data2 is None else [
            sum(r_data.strand == '+' for r_data in all_reg_data2[reg_i].reads),
            sum(r_data.strand == '-' for r_data in all_reg_data2[reg_i].reads)]
        strand_cov.append(reg_cov1 + reg_cov2)
    # downsample can be plotted with any number of reads on either strand
    if overplot_type == "Downsample":
        plot_types = ["Downsample" for _ in strand_cov]
        dnspl_stars = [['*' if grp_r_ovr_cov > overplot_thresh else '' for grp_r_ovr_cov in r_cov]
                       for r_cov in strand_cov]
    else:
        # need to remove 0 cov as might be plotting on just one strand
        gt0_strand_cov = [[x for x in covs if x > 0] for covs in strand_cov]
        plot_types = ['Signal' if (max(covs) < overplot_thresh or min(covs) < QUANT_MIN) else overplot_type
                      for covs in gt0_strand_cov]
        dnspl_stars = [['' for _ in r_cov] for r_cov in strand_cov]

    titles = []
    for int_i, r_cov, r_ovp in zip(all_reg_data, strand_cov, dnspl_stars):
        reg_title = int_i.chrm if include_chrm else ''
        if all_reg_data2 is None:
            if int_i.strand is None:
                reg_title += '  ' + int_i.reg_text
                if include_cov:
                    reg_title += ("  Coverage: " + str(r_cov[0]) + r_ovp[0] + " + " + str(r_cov[1]) + r_ovp[1] + " -")
            else:
                if include_chrm:
                    reg_title += ':' + int_i.strand
                reg_title += '  ' + int_i.reg_text
                if include_cov:
                    cov_str = (str(r_cov[0]) + r_ovp[0] if int_i.strand == '+' else str(r_cov[1]) + r_ovp[1])
                    reg_title += "  Coverage: " + cov_str
            if model_plot and overplot_type in ('Density', 'Quantile', 'Boxplot'):
                reg_title += '  (Model in Black)'
        else:
            if int_i.strand is None:
                reg_title += '  ' + int_i.reg_text
                if include_cov:
                    reg_title += ("  Coverage: Sample (Red): " + str(r_cov[0]) + r_ovp[0] + " + " +
                                  str(r_cov[1]) + r_ovp[1] + " -; Control (Black): " +
                                  str(r_cov[2]) + r_ovp[2] + " + " + str(r_cov[3]) + r_ovp[3] + " -")
            else:
                if include_chrm:
                    reg_title += ":" + int_i.strand
                reg_title += '  ' + int_i.reg_text
                if include_cov:
                    cov_str = ('Sample (Red): ' + str(r_cov[0]) + r_ovp[0] + '; Control (Black): ' +
                               str(r_cov[2]) + r_ovp[2]) if int_i.strand == '+' else (
                                   'Sample (Red): ' + str(r_cov[1]) + r_ovp[1] + '; Control (Black): ' +
                                   str(r_cov[3]) + r_ovp[3])
                    reg_title += "  Coverage: " + cov_str
        titles.append(reg_title)

    Titles = OrderedDict([('Title', _strs(titles)), ('Region', _strs([int_i.reg_id for int_i in all_reg_data]))])
    return Titles, plot_types


def get_base_r_data(all_reg_data, zero_start=False, is_rna=False, genome_centric=True):
    """the bases under the plots (_plot_commands.py:986-1031).  The reference builds the positions as strings and
    hands them to FloatVector: the column is float64."""
    BaseStart, Bases, BaseRegion, BaseStrand = [], [], [], []
    for reg_data in all_reg_data:
        # skip regions without sequence data
        if reg_data.seq is None:
            continue
        if reg_data.strand == '+' or reg_data.strand is None:
            for i, base in enumerate(reg_data.seq):
                if is_rna and base == 'T':
                    base = 'U'
                BaseStart.append(i if zero_start else i + reg_data.start)
                Bases.append(base)
                BaseRegion.append(reg_data.reg_id)
                BaseStrand.append(FWD_STRAND)
        if reg_data.strand == '-' or reg_data.strand is None:
            for i, base in enumerate(reg_data.seq):
                base = th.comp_seq(base)
                if is_rna and base == 'T':
                    base = 'U'
                if genome_centric:
                    BaseStart.append(i if zero_start else i + reg_data.start)
                else:
                    BaseStart.append(reg_data.end - reg_data.start - i - 1 if zero_start else reg_data.end - i - 1)
                Bases.append(base)
                BaseRegion.append(reg_data.reg_id)
                BaseStrand.append(REV_STRAND)

    return OrderedDict([('Position', np.array(BaseStart, dtype=np.float64)), ('Base', _strs(Bases)),
                        ('Region', _strs(BaseRegion)), ('Strand', _strs(BaseStrand))])


class _LevelBatch(object):
    """the regions of one `region_level_piles` call: every read once, regions by read index"""

    def __init__(self):
        self.read_idx, self.reads, self.reg_reads, self.reg_read_off, self.starts, self.ends = {}, [], [], [0], [], []

    def add(self, reg_data, reads):
        for rd in reads:
            if id(rd) not in self.read_idx:
                self.read_idx[id(rd)] = len(self.reads)
                self.reads.append(rd)
            self.reg_reads.append(self.read_idx[id(rd)])
        self.reg_read_off.append(len(self.reg_reads))
        self.starts.append(reg_data.start)
        self.ends.append(reg_data.end)

    def run(self, engine, q_linear=None, q_nearest=None, want_levels=False):
        means = [np.asarray(rd.means, dtype=np.float64) for rd in self.reads]
        return _engine(engine).region_level_piles(
            np.array([rd.start for rd in self.reads], dtype=np.int64),
            np.array([rd.strand == '-' for rd in self.reads], dtype=np.uint8),
            np.concatenate([[0], np.cumsum([m.shape[0] for m in means])]).astype(np.int64), _cat(means, np.float64),
            np.array(self.reg_read_off, dtype=np.int64), np.array(self.reg_reads, dtype=np.int64),
            np.array(self.starts, dtype=np.int64), np.array(self.ends, dtype=np.int64), q_linear, q_nearest,
            want_levels)


def _base_level_reads(reg_data):
    """the reads whose levels reg_data.get_base_levels() stacks, with its errors"""
    if reg_data.reads is None or len(reg_data.reads) == 0:
        raise th.TomboError('Must annotate region with reads (see `TomboInterval.add_reads`) to extract base levels.')
    reads = reg_data.level_reads()
    if len(reads) == 0:
        raise ValueError('need at least one array to concatenate')      # (np.column_stack of no column)
    return reads


def _pile_rows(all_reg_data, plot_types, plot_type, engine, q_linear=None, q_nearest=None):
    """The box and quantile frames' walk: per region of plot_type and strand that has reads, the positions with
    a level.  The reference takes get_base_levels() of the WHOLE region inside its strand loop, so a region
    without a strand and with reads on both strands yields the same numbers twice, once per strand label.
    -> (lin, near, rows): rows = [(region, strand, kept position indices of the call, their genomic positions)]"""
    batch, regs = _LevelBatch(), []
    for reg_plot_sig, reg_data in zip(plot_types, all_reg_data):
        if reg_plot_sig != plot_type:
            continue
        strands = [s for s in ('+', '-') if sum(r_data.strand == s for r_data in reg_data.reads) > 0]
        if strands:
            batch.add(reg_data, _base_level_reads(reg_data))
            regs.append((reg_data, strands))
    if not regs:
        return None, None, []
    off, _, lin, near = batch.run(engine, q_linear, q_nearest)
    rows, first = [], 0
    for reg_data, strands in regs:
        n_pos = reg_data.end - reg_data.start
        kept = np.flatnonzero(np.diff(off[first:first + n_pos + 1]) > 0)     # skip positions with no coverage
        rows.extend((reg_data, strand, kept + first, kept + reg_data.start) for strand in strands)
        first += n_pos
    return lin, near, rows


def _label_columns(rows, repeat=1):
    """Strand and Region columns of the rows of _pile_rows, every position `repeat` times"""
    strand = [np.full(idx.shape[0] * repeat, _strand_name(s), dtype=object) for _, s, idx, _ in rows]
    region = [np.full(idx.shape[0] * repeat, reg.reg_id, dtype=object) for reg, _, idx, _ in rows]
    return _cat(strand, object), _cat(region, object)


def get_r_event_data(all_reg_data, plot_types, overplot_thresh, group_num='Group1', engine=None):
    """the Density frame (_plot_commands.py:784-821): per region, strand and position with at least two levels, the
    levels of that strand's reads in read order"""
    batch, parts = _LevelBatch(), []
    for reg_plot_sig, reg_data in zip(plot_types, all_reg_data):
        if reg_plot_sig != 'Density':
            continue
        for strand in ('+', '-'):
            strand_reads = [r_data for r_data in reg_data.reads if r_data.strand == strand]
            if len(strand_reads) == 0:
                continue
            batch.add(reg_data, _base_level_reads(reg_data.copy(include_reads=False).update(reads=strand_reads)))
            parts.append((reg_data, strand))
    Position, Signal, Strand, Region = [], [], [], []
    if parts:
        off, levels, _, _ = batch.run(engine, want_levels=True)
        first = 0
        for reg_data, strand in parts:
            n_pos = reg_data.end - reg_data.start
            sizes = np.diff(off[first:first + n_pos + 1])
            # skip bases with zero or 1 read as ggplot won't be able to estimate the density
            for pos in np.flatnonzero(sizes >= 2).tolist():
                Position.append(np.full(sizes[pos], pos + reg_data.start, dtype=np.int64))
                Signal.append(levels[off[first + pos]:off[first + pos + 1]])
                Strand.append(np.full(sizes[pos], _strand_name(strand), dtype=object))
                Region.append(np.full(sizes[pos], reg_data.reg_id, dtype=object))
            first += n_pos
    Position = _cat(Position, np.int64)
    return OrderedDict([('Position', Position), ('Signal', _cat(Signal, np.float64)), ('Strand', _cat(Strand, object)),
                        ('Region', _cat(Region, object)), ('Group', _strs([group_num] * Position.shape[0]))])


def get_r_boxplot_data(all_reg_data, plot_types, overplot_thresh, group_num='Group1', engine=None):
    """the Boxplot frame (_plot_commands.py:823-863): np.percentile 0, 25, 50, 75, 100 of every covered position"""
    lin, _, rows = _pile_rows(all_reg_data, plot_types, 'Boxplot', engine,
                              q_linear=np.true_divide([0, 25, 50, 75, 100], 100))
    idx = _cat([i for _, _, i, _ in rows], np.int64)
    stats = lin[idx] if rows else np.empty((0, 5), dtype=np.float64)
    Strand, Region = _label_columns(rows)
    return OrderedDict(
        [('Position', _cat([g for _, _, _, g in rows], np.int64))] +
        [(name, np.ascontiguousarray(stats[:, j])) for j, name in enumerate(('SigMin', 'Sig25', 'SigMed', 'Sig75', 'SigMax'))] +
        [('Strand', Strand), ('Region', Region), ('Group', _strs([group_num] * idx.shape[0]))])


def get_r_quant_data(all_reg_data, plot_types, overplot_thresh, group_num='Group1', pos_offest=0,
                     pcntls=[1, 10, 20, 30, 40, 49], engine=None):
    """the Quantile frame (_plot_commands.py:865-905): the 'nearest' percentiles pcntls and 100 - pcntls of every
    covered position, one row per percentile pair"""
    upper_pcntls = [100 - pcntl for pcntl in pcntls]
    n_q = len(pcntls)
    _, near, rows = _pile_rows(
        all_reg_data, plot_types, 'Quantile', engine,
        q_nearest=np.concatenate([np.true_divide(pcntls, 100), np.true_divide(upper_pcntls, 100)]).astype(np.float64))
    idx = _cat([i for _, _, i, _ in rows], np.int64)
    stats = near[idx] if rows else np.empty((0, 2 * n_q), dtype=np.float64)
    Strand, Region = _label_columns(rows, n_q)
    Position = np.repeat(_cat([g + pos_offest for _, _, _, g in rows], np.float64), n_q)
    return OrderedDict([('Position', Position), ('Lower', stats[:, :n_q].reshape(-1)),
                        ('Upper', stats[:, n_q:].reshape(-1)), ('Strand', Strand), ('Region', Region),
                        ('Group', _strs([group_num] * Position.shape[0]))])


def _raw_signal_usable(r_data):
    """whether get_raw_signal and the normalisation can run for the read (the reference's try / except)"""
    try:
        if r_data.raw_signal is None or r_data.segs is None or r_data.scale_values is None:
            return False
        raw = np.asarray(r_data.raw_signal)
        return raw.ndim == 1 and raw.dtype in (np.dtype(np.int16), np.dtype(np.int32)) and _native.raw_signal_fits(
            r_data.segs, int(r_data.read_start_rel_to_raw), raw.shape[0])
    except (AttributeError, TypeError, ValueError):
        return False


def get_r_raw_signal_data(all_reg_data, plot_types, overplot_thresh, group_num='Group1', genome_centric=True,
                          engine=None):
    """the Signal / Downsample frame (_plot_commands.py:907-976): the normalised raw signal of every read over
    every region, each base's samples spread over [position, position + 1).  Downsample shuffles the plus, then
    the minus reads (np.random.shuffle), each only when longer than overplot_thresh.  `Read` counts the reads
    tried, not the reads kept.  A read whose raw signal cannot be had is skipped, with one warning per call."""
    not_warned = True
    read_idx, reads, pairs = {}, [], []       # pairs: (read index, region, r_num, strand)
    for reg_plot_sig, reg_data in zip(plot_types, all_reg_data):
        if reg_plot_sig not in ('Signal', 'Downsample'):
            continue
        reg_reads = reg_data.reads
        if reg_plot_sig == 'Downsample':
            plus_reads = [r_data for r_data in reg_data.reads if r_data.strand == '+']
            minus_reads = [r_data for r_data in reg_data.reads if r_data.strand == '-']
            # randomly select reads to plot if too many
            if len(plus_reads) > overplot_thresh:
                np.random.shuffle(plus_reads)
                plus_reads = plus_reads[:overplot_thresh]
            if len(minus_reads) > overplot_thresh:
                np.random.shuffle(minus_reads)
                minus_reads = minus_reads[:overplot_thresh]
            reg_reads = plus_reads + minus_reads
        for r_num, r_data in enumerate(reg_reads):
            if not _raw_signal_usable(r_data):
                if not_warned:
                    not_warned = False
                    warnings.warn(RAW_SIGNAL_WARNING)
                continue
            if id(r_data) not in read_idx:
                read_idx[id(r_data)] = len(reads)
                reads.append(r_data)
            pairs.append((read_idx[id(r_data)], reg_data, r_num, r_data.strand))
    if not pairs:
        empty = np.empty(0, dtype=np.float64)
        return OrderedDict([('Position', empty), ('Signal', empty.copy())] +
                           [(name, _strs([])) for name in ('Read', 'Strand', 'Region', 'Group')])
    raws = [np.asarray(rd.raw_signal) for rd in reads]
    raw_dtype = np.int32 if any(r.dtype == np.int32 for r in raws) else np.int16      # (int16 widens without loss)
    segs = [np.asarray(rd.segs, dtype=np.int64) for rd in reads]
    limit = (lambda v: np.nan if v is None else v)
    sig_off, position, signal, _ = _engine(engine).region_raw_signal(
        _cat(raws, raw_dtype), np.concatenate([[0], np.cumsum([r.shape[0] for r in raws])]).astype(np.int64),
        _cat(segs, np.int64), np.concatenate([[0], np.cumsum([s.shape[0] for s in segs])]).astype(np.int64),
        np.array([rd.start for rd in reads], dtype=np.int64),
        np.array([rd.read_start_rel_to_raw for rd in reads], dtype=np.int64),
        np.array([rd.strand == '-' for rd in reads], dtype=np.uint8),
        np.array([bool(rd.rna) for rd in reads], dtype=np.uint8),
        np.array([rd.scale_values.shift for rd in reads], dtype=np.float64),
        np.array([rd.scale_values.scale for rd in reads], dtype=np.float64),
        np.array([limit(rd.scale_values.lower_lim) for rd in reads], dtype=np.float64),
        np.array([limit(rd.scale_values.upper_lim) for rd in reads], dtype=np.float64),
        np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1].start for p in pairs], dtype=np.int64),
        np.array([p[1].end for p in pairs], dtype=np.int64), genome_centric)
    sizes = np.diff(sig_off)
    rep = (lambda values: np.repeat(_strs(values), sizes))
    return OrderedDict([
        ('Position', position), ('Signal', signal),
        ('Read', rep(['%d_%s' % (r_num, group_num) for _, _, r_num, _ in pairs])),
        ('Strand', rep([_strand_name(strand) for _, _, _, strand in pairs])),
        ('Region', rep([reg.reg_id for _, reg, _, _ in pairs])),
        ('Group', _strs([group_num] * position.shape[0]))])


def get_plot_types_data(plot_args, quant_offset=0, engine=None):
    SignalData = get_r_raw_signal_data(*plot_args, engine=engine)
    QuantData = get_r_quant_data(*plot_args, pos_offest=quant_offset, engine=engine)
    BoxData = get_r_boxplot_data(*plot_args, engine=engine)
    EventData = get_r_event_data(*plot_args, engine=engine)

    return SignalData, QuantData, BoxData, EventData


def filter_and_merge_regs(g1_data, g2_data):
    """-> (merged regions with sequence, group 1 regions, group 2 regions) of the regions that have a read in either
    group (_plot_commands.py:1362-1382)"""
    filt_g1, filt_g2, merged_reg_data = [], [], []
    for r1, r2 in zip(g1_data, g2_data):
        merged_reg = r1.merge(r2)
        if len(merged_reg.reads) > 0:
            merged_reg_data.append(merged_reg.add_seq())
            filt_g1.append(r1)
            filt_g2.append(r2)
    if len(merged_reg_data) == 0:
        raise th.TomboError('No reads in any selected regions.')
    return merged_reg_data, filt_g1, filt_g2


def single_sample_plot_data(plot_intervals, reads_index, overplot_thresh, overplot_type, title_include_chrm=True,
                            title_include_cov=True, is_rna=False, engine=None):
    """plot_single_sample up to its R calls (_plot_commands.py:1336-1351) -> the frames it hands to plotSingleRun:
    (SignalData, QuantData, BoxData, EventData, BasesData, Titles).  is_rna: what th.is_sample_rna reads from the
    files."""
    for p_int in plot_intervals:
        p_int.add_reads(reads_index).add_seq()
    plot_intervals = th.filter_empty_regions(plot_intervals)
    Titles, plot_types = get_plots_titles(plot_intervals, None, overplot_type, overplot_thresh,
                                          include_chrm=title_include_chrm, include_cov=title_include_cov)
    BasesData = get_base_r_data(plot_intervals, is_rna=is_rna)
    SignalData, QuantData, BoxData, EventData = get_plot_types_data(
        (plot_intervals, plot_types, overplot_thresh, 'Group1'), engine=engine)
    return SignalData, QuantData, BoxData, EventData, BasesData, Titles


def _rbind(frame1, frame2):
    return OrderedDict((name, np.concatenate([frame1[name], frame2[name]])) for name in frame1)


def two_samples_plot_data(plot_intervals, reads_index, ctrl_reads_index, overplot_thresh, overplot_type,
                          title_include_chrm=True, title_include_cov=True, engine=None):
    """plot_two_samples up to its R calls (_plot_commands.py:1384-1419) -> the frames it hands to plotGroupComp, the
    two groups' frames concatenated where it `rbind`s them: (SignalData, QuantData, BoxData, EventData, BasesData,
    Titles).  The quantile positions of the groups are offset by 0.1 and 0.5."""
    all_reg_data1 = [p_int.copy().add_reads(reads_index) for p_int in plot_intervals]
    all_reg_data2 = [p_int.copy().add_reads(ctrl_reads_index) for p_int in plot_intervals]
    # filter regions with no coverage in either read group
    merged_reg_data, all_reg_data1, all_reg_data2 = filter_and_merge_regs(all_reg_data1, all_reg_data2)
    Titles, plot_types = get_plots_titles(all_reg_data1, all_reg_data2, overplot_type, overplot_thresh,
                                          include_chrm=title_include_chrm, include_cov=title_include_cov)
    BasesData = get_base_r_data(merged_reg_data)
    frames1 = get_plot_types_data((all_reg_data1, plot_types, overplot_thresh, 'Group1'), 0.1, engine=engine)
    frames2 = get_plot_types_data((all_reg_data2, plot_types, overplot_thresh, 'Group2'), 0.5, engine=engine)
    return tuple(_rbind(f1, f2) for f1, f2 in zip(frames1, frames2)) + (BasesData, Titles)


# ---------------------------------------------------------------------------------------------
# K-mer level distributions: `tombo plot kmer` (plot_kmer_dist, _plot_commands.py:451-559)
KMER_DIST_NO_READS_ERROR = (
    'No valid reads present.\n\t\tCheck that [--corrected-group] matches value used in resquiggle.\n\t\tAlso consider '
    'lowering [--num-kmer-threshold] especially for k-mer lengths greater than 4.')
KMER_DIST_FEW_READS_WARNING = (
    'Fewer valid reads present than requested.\n\tConsider lowering [--num-kmer-threshold] especially for k-mer '
    'lengths greater than 4.')


def kmer_dist_plot_data(reads, read_mean, upstrm_bases, dnstrm_bases, kmer_thresh, num_reads, engine=None):
    """plot_kmer_dist up to its R calls -> (kmerDat, baseDat, kmer_levels).  `reads`: objects with `means` and `seq`
    (th.resquiggledRead), taken in the order given (the reference shuffles them first); a read whose `means` is None
    is skipped.  kmerDat: Kmer, Base (kmer[upstrm_bases]), Signal, Read (the label of the entry's read, as a str);
    baseDat: Kmer, Base, Position, the frame the reference builds when R has gridExtra; kmer_levels: the k-mers in
    plot order, the levels of the Kmer factor.

    All numbers come from ONE `Engine.kmer_dist` call (csrc/k_kmer_dist.h): which reads are taken, the levels of
    every (k-mer, read) in position order, np.mean of each in numpy's summation order and the mean of every k-mer.
    Ordering the at most 4**K k-mer means by (mean, k-mer) and putting the k-mers' runs of entries into that order are
    copies without arithmetic and stay on the host.

    Raises th.TomboError where the reference exits (no or one valid read) and warns where it warns (fewer valid reads
    than asked).  ValueError: options outside 0..4, levels and bases that differ in number, a base outside ACGT or a
    NaN level (the reference's result for those is a by-product of dict keys and of sorting NaNs), a batch whose
    4**K * reads is above the engine's table limit of 2**27 entries."""
    from .tombo_stats import encode_seq
    for name, v in (('upstrm_bases', upstrm_bases), ('dnstrm_bases', dnstrm_bases)):
        if int(v) != v or not 0 <= v <= 4:
            raise ValueError('%s must be an integer in [0, 4]' % name)
    upstrm_bases, dnstrm_bases = int(upstrm_bases), int(dnstrm_bases)
    K = upstrm_bases + dnstrm_bases + 1
    reads = [rd for rd in reads if rd.means is not None]
    means = [np.asarray(rd.means, dtype=np.float64) for rd in reads]
    codes = [encode_seq(rd.seq) for rd in reads]
    for rd, m, c in zip(reads, means, codes):
        if m.shape[0] != c.shape[0]:
            raise ValueError('read %r: levels and bases differ in number' % (getattr(rd, 'read_id', None),))
        if (c > 3).any():
            raise ValueError('read %r: a base outside ACGT' % (getattr(rd, 'read_id', None),))
        if np.isnan(m).any():
            raise ValueError('read %r: a NaN level' % (getattr(rd, 'read_id', None),))
    if 4 ** K * len(reads) > _native.KMER_DIST_TABLE_MAX:
        raise ValueError('%d reads at k-mer width %d are above the table limit of 2**27 (4**K * reads) entries' % (
            len(reads), K))
    n_sel = 0
    if reads:
        _, n_sel, _, counts, off, values, vlabel, kmer_mean = _engine(engine).kmer_dist(
            _cat(means, np.float64), _cat(codes, np.uint8),
            np.concatenate([[0], np.cumsum([m.shape[0] for m in means])]).astype(np.int64),
            K, upstrm_bases, kmer_thresh, num_reads, read_mean)
    if n_sel in (0, 1):
        raise th.TomboError(KMER_DIST_NO_READS_ERROR)
    if n_sel < num_reads:
        warnings.warn(KMER_DIST_FEW_READS_WARNING)

    have = np.flatnonzero(counts)
    order = have[np.lexsort((have, kmer_mean[have]))]     # (mean, k-mer string): index order is string order
    kmer_levels = [''.join('ACGT'[(q >> (2 * (K - 1 - j))) & 3] for j in range(K)) for q in order.tolist()]
    rows = _cat([np.arange(off[q], off[q + 1]) for q in order.tolist()], np.int64)
    row_kmers = np.repeat(_strs(kmer_levels), counts[order])
    kmerDat = OrderedDict([
        ('Kmer', row_kmers), ('Base', np.repeat(_strs([kmer[upstrm_bases] for kmer in kmer_levels]), counts[order])),
        ('Signal', values[rows]), ('Read', _strs([str(x) for x in vlabel[rows].tolist()]))])
    baseDat = OrderedDict([
        ('Kmer', np.repeat(_strs(kmer_levels), K)),
        ('Base', _strs([kmer[i] for kmer in kmer_levels for i in range(K)])),
        ('Position', np.tile(np.arange(K, dtype=np.int64) - upstrm_bases, len(kmer_levels)))])
    return kmerDat, baseDat, kmer_levels


# ---------------------------------------------------------------------------------------------
# Model overlays and per-read statistic frames (_plot_commands.py:1034-1096, :1435-1652).  Host code only: k-mer
# look-ups, slices and copies; the one computation, the read order of the per-read plots, is ts.order_reads, which
# runs on the device.
PLOT_PVAL_MAX, PLOT_LLR_MAX = 4, 4        # _default_parameters.py:197
MODEL_KMER_POS_ERROR = 'Standard model not based on the same kmer position as alternative model.'


def get_reg_kmers(std_ref, plot_intervals, reads_index, min_reg_overlap=None, alt_ref=None):
    """-> (all_reg_model_data, all_reg_alt_model_data): per region (reg_id, strand, [(pos, mean, sd)] of the plus
    strand, the same of the minus strand) from the standard model, and the alternate model's window round the plot
    centre (_plot_commands.py:1435-1524).  The intervals get their reads and sequence as a side effect, as in the
    reference.  std_ref is a ts.TomboModel (arrays by k-mer code), alt_ref a ts.AltModel.  Kept as they are: only
    central_pos of the two models is compared (the reference compares alt_ref.kmer_width with itself), and
    `seq[expand_width:-expand_width]` is '' when expand_width is 0."""
    def get_reg_reads(reads, int_start, int_end):
        return [r_data for r_data in reads if not (r_data.start >= int_end or r_data.end <= int_start)]

    def std_levels(kmer):
        code = std_ref._kmer_code(kmer)
        return float(std_ref.level_means[code]), float(std_ref.level_sds[code])
    # compute kmer values to make strand specific calculations easier
    dnstrm_bases = std_ref.kmer_width - std_ref.central_pos - 1
    expand_width = max(std_ref.central_pos, dnstrm_bases)
    filt_width = expand_width if min_reg_overlap is None else expand_width + min_reg_overlap
    if alt_ref is not None:
        if alt_ref.central_pos != std_ref.central_pos or alt_ref.kmer_width != alt_ref.kmer_width:
            raise th.TomboError(MODEL_KMER_POS_ERROR)

    # expand regions to get kmers at first and last positions, add reads and region sequence
    for p_int in plot_intervals:
        p_int.expand_interval(expand_width).add_reads(reads_index).add_seq()
    expand_seqs = [p_int.seq for p_int in plot_intervals]
    rev_expand_seqs = [th.rev_comp(p_int.seq) for p_int in plot_intervals]
    # convert back to original plot_intervals with seq from expanded intervals
    for p_int in plot_intervals:
        p_int.expand_interval(-expand_width)
        p_int.update(reads=get_reg_reads(p_int.reads, p_int.start + filt_width, p_int.end - filt_width),
                     seq=p_int.seq[expand_width:-expand_width])

    K = std_ref.kmer_width
    all_reg_model_data, all_reg_alt_model_data = [], []
    for reg_data, reg_seq, rev_seq in zip(plot_intervals, expand_seqs, rev_expand_seqs):
        clipped_reg_seq, clipped_rev_seq = reg_seq, rev_seq
        if std_ref.central_pos > dnstrm_bases:
            clipped_reg_seq = reg_seq[:dnstrm_bases - std_ref.central_pos]
            clipped_rev_seq = rev_seq[:dnstrm_bases - std_ref.central_pos]
        elif dnstrm_bases > std_ref.central_pos:
            clipped_reg_seq = reg_seq[dnstrm_bases - std_ref.central_pos:]
            clipped_rev_seq = rev_seq[dnstrm_bases - std_ref.central_pos:]
        fwd_kmers = [clipped_reg_seq[i:i + K] for i in range(len(clipped_reg_seq) - K + 1)]
        rev_kmers = [clipped_rev_seq[i:i + K] for i in range(len(clipped_rev_seq) - K + 1)]
        all_reg_model_data.append((
            reg_data.reg_id, reg_data.strand,
            [(reg_data.start + pos,) + std_levels(kmer) for pos, kmer in enumerate(fwd_kmers)
             if not th.invalid_seq(kmer)],
            [(reg_data.end - pos - 1,) + std_levels(kmer) for pos, kmer in enumerate(rev_kmers)
             if not th.invalid_seq(kmer)]))
        # if alternative model is supplied add info
        if alt_ref is not None and len(fwd_kmers) >= alt_ref.kmer_width:
            plot_center = len(fwd_kmers) // 2
            window = slice(plot_center - alt_ref.central_pos - 1, plot_center + alt_ref.kmer_width - alt_ref.central_pos)
            fwd_kmer_poss = list(zip(fwd_kmers[window], range(alt_ref.kmer_width - 1, -1, -1)))
            reg_fwd_alt_data = [
                (reg_data.start + (plot_center - pos + alt_ref.central_pos), alt_ref.means[(kmer, pos)],
                 alt_ref.sds[(kmer, pos)])
                for kmer, pos in fwd_kmer_poss] if all(kmer_pos in alt_ref.means for kmer_pos in fwd_kmer_poss) else []
            rev_kmer_poss = list(zip(rev_kmers[window], range(alt_ref.kmer_width - 1, -1, -1)))
            reg_rev_alt_data = [
                (reg_data.end - (plot_center - pos + alt_ref.central_pos) - 1, alt_ref.means[(kmer, pos)],
                 alt_ref.sds[(kmer, pos)])
                for kmer, pos in rev_kmer_poss] if all(kmer_pos in alt_ref.means for kmer_pos in rev_kmer_poss) else []
            all_reg_alt_model_data.append((reg_data.reg_id, reg_data.strand, reg_fwd_alt_data, reg_rev_alt_data))

    return all_reg_model_data, all_reg_alt_model_data


def get_model_r_data(all_reg_model_data, genome_centric=True):
    """the model levels under the plots (_plot_commands.py:1034-1068): Position, Strand, Mean, SD, Region.  Not
    genome-centric, the minus strand's positions are mirrored between its first and last entry."""
    Position, Strand, Mean, SD, Region = [], [], [], [], []
    for reg_id, strand, fwd_model_data, rev_model_data in all_reg_model_data:
        if strand == '+' or strand is None:
            for pos, base_model_mean, base_model_sd in fwd_model_data:
                Position.append(pos)
                Strand.append(FWD_STRAND)
                Mean.append(base_model_mean)
                SD.append(base_model_sd)
                Region.append(reg_id)
        if strand == '-' or strand is None:
            if not genome_centric:
                start_pos, end_pos = rev_model_data[0][0], rev_model_data[-1][0]
            for pos, base_model_mean, base_model_sd in rev_model_data:
                Position.append(pos if genome_centric else start_pos + end_pos - pos)
                Strand.append(REV_STRAND)
                Mean.append(base_model_mean)
                SD.append(base_model_sd)
                Region.append(reg_id)

    return OrderedDict([('Position', np.array(Position, dtype=np.float64)), ('Strand', _strs(Strand)),
                        ('Mean', np.array(Mean, dtype=np.float64)), ('SD', np.array(SD, dtype=np.float64)),
                        ('Region', _strs(Region))])


def get_reg_r_stats(all_reg_stats, are_pvals=False, engine=None):
    """-> (StatsData, OrdData) of the per-read statistic plots (_plot_commands.py:1070-1096).  all_reg_stats:
    (reg_id, strand, float64[reads, positions]) per region.  StatsData: Stats, Position, Read (all float64), Region,
    read by read; a minus-strand region's positions are reversed.  OrdData: Read (float64), Region: the reads in
    ts.order_reads order, taken before the reversal.  ts.transform_and_trim_stats trims likelihood ratios in the
    array that was passed, as in the reference."""
    from . import tombo_stats as ts
    Stats, Position, Read, Region, OrdRead, OrdRegion = [], [], [], [], [], []
    for reg_id, reg_strand, reg_stats in all_reg_stats:
        # -log if p-values and trim/winsorize stats before clustering here
        reg_stats = ts.transform_and_trim_stats(reg_stats, are_pvals, PLOT_PVAL_MAX if are_pvals else PLOT_LLR_MAX)
        OrdRead.append(np.asarray(ts.order_reads(reg_stats, engine=engine), dtype=np.float64))
        OrdRegion.extend([reg_id] * reg_stats.shape[0])
        if reg_strand == '-':
            reg_stats = reg_stats[:, ::-1]
        n_reads, n_pos = reg_stats.shape
        Stats.append(np.ascontiguousarray(reg_stats, dtype=np.float64).ravel())
        Position.append(np.tile(np.arange(n_pos, dtype=np.float64), n_reads))
        Read.append(np.repeat(np.arange(n_reads, dtype=np.float64), n_pos))
        Region.extend([reg_id] * (n_reads * n_pos))

    StatsData = OrderedDict([('Stats', _cat(Stats, np.float64)), ('Position', _cat(Position, np.float64)),
                             ('Read', _cat(Read, np.float64)), ('Region', _strs(Region))])
    OrdData = OrderedDict([('Read', _cat(OrdRead, np.float64)), ('Region', _strs(OrdRegion))])
    return StatsData, OrdData


def model_single_sample_plot_data(plot_intervals, reads_index, std_ref, overplot_type, overplot_thresh, alt_ref=None,
                                  title_include_chrm=True, title_include_cov=True, is_rna=False, engine=None):
    """plot_model_single_sample up to its R calls (_plot_commands.py:1592-1623) -> the frames it hands to
    plotModelComp: (SignalData, QuantData, BoxData, EventData, BasesData, Titles, ModelData) and, with alt_ref,
    AltModelData behind them.  is_rna: what th.is_sample_rna reads from the files."""
    # get reads overlapping each region along with all kmers
    all_reg_model_data, all_reg_alt_model_data = get_reg_kmers(std_ref, plot_intervals, reads_index, alt_ref=alt_ref)
    plot_intervals = th.filter_empty_regions(plot_intervals)
    Titles, plot_types = get_plots_titles(plot_intervals, None, overplot_type, overplot_thresh, True,
                                          include_chrm=title_include_chrm, include_cov=title_include_cov)
    ModelData = get_model_r_data(all_reg_model_data)
    BasesData = get_base_r_data(plot_intervals, is_rna=is_rna)
    SignalData, QuantData, BoxData, EventData = get_plot_types_data(
        (plot_intervals, plot_types, overplot_thresh, 'Group1'), engine=engine)
    frames = (SignalData, QuantData, BoxData, EventData, BasesData, Titles, ModelData)
    return frames if alt_ref is None else frames + (get_model_r_data(all_reg_alt_model_data),)


def motif_with_stats_plot_data(reads_index, ctrl_reads_index, plot_intervals, stat_locs, overplot_thresh, std_ref,
                               alt_ref=None, engine=None):
    """plot_motif_centered_with_stats up to its R calls (_plot_commands.py:1526-1587) -> the frames it hands to
    plotMotifStats: (SignalData, BasesData, StatsData, ModelData) and, with alt_ref, AltModelData behind them.  All
    frames are read direction-centric.  ModelData is None where the reference passes R's NULL (no std_ref, or a
    control sample).  alt_ref with a control sample or without std_ref is a ValueError: the reference then names
    an AltModelData it never made."""
    if alt_ref is not None and (ctrl_reads_index is not None or std_ref is None):
        raise ValueError('alt_ref needs std_ref and no control sample: the reference makes no AltModelData otherwise')
    ModelData = AltModelData = None
    plot_types = ['Downsample' for _ in plot_intervals]
    if ctrl_reads_index is None:
        if std_ref is None:
            for p_int in plot_intervals:
                p_int.add_reads(reads_index).add_seq()
            SignalData = get_r_raw_signal_data(plot_intervals, plot_types, overplot_thresh, 'Group1',
                                               genome_centric=False, engine=engine)
        else:
            all_reg_model_data, all_reg_alt_model_data = get_reg_kmers(std_ref, plot_intervals, reads_index,
                                                                       alt_ref=alt_ref)
            SignalData = get_r_raw_signal_data(plot_intervals, plot_types, overplot_thresh, 'Group1',
                                               genome_centric=False, engine=engine)
            ModelData = get_model_r_data(all_reg_model_data, genome_centric=False)
            if alt_ref is not None:
                AltModelData = get_model_r_data(all_reg_alt_model_data, genome_centric=False)
    else:
        all_reg_data = [p_int.copy().add_reads(reads_index) for p_int in plot_intervals]
        ctrl_reg_data = [p_int.copy().add_reads(ctrl_reads_index) for p_int in plot_intervals]
        plot_intervals, all_reg_data, ctrl_reg_data = filter_and_merge_regs(all_reg_data, ctrl_reg_data)
        plot_types = ['Downsample' for _ in plot_intervals]
        SignalData = _rbind(
            get_r_raw_signal_data(all_reg_data, plot_types, overplot_thresh, 'Group1', genome_centric=False,
                                  engine=engine),
            get_r_raw_signal_data(ctrl_reg_data, plot_types, overplot_thresh, 'Group2', genome_centric=False,
                                  engine=engine))

    BasesData = get_base_r_data(plot_intervals, genome_centric=False)
    plot_poss, plot_stats = zip(*stat_locs)
    StatsData = OrderedDict([('Position', np.array(plot_poss, dtype=np.float64)),
                             ('Stat', np.array(plot_stats, dtype=np.float64))])
    frames = (SignalData, BasesData, StatsData, ModelData)
    return frames if alt_ref is None else frames + (AltModelData,)


def per_read_modification_plot_data(plot_intervals, all_reg_stats, are_pvals, box_center, engine=None):
    """plot_per_read_modification up to its R calls (_plot_commands.py:1638-1649) -> what it hands to
    plotPerReadStats: (StatData, OrdData, BasesData, box_center, are_pvals)"""
    StatData, OrdData = get_reg_r_stats(all_reg_stats, are_pvals, engine=engine)
    BasesData = get_base_r_data(plot_intervals, zero_start=True, genome_centric=False)
    return StatData, OrdData, BasesData, box_center, are_pvals

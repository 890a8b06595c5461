"""Host-side model / parameter helpers of the resquiggle path (own implementation).

Mirrors the part of /root/reference/tombo/tombo_stats.py the hot path touches:
  TomboModel.get_exp_levels_from_seq   tombo_stats.py:834-862  (P3)
  load_resquiggle_parameters           tombo_stats.py:1505-1556
  compute_num_events                   tombo_stats.py:1558-1574
  get_dynamic_prog_params              tombo_stats.py:2364-2370
  identify_stalls (mean-window method) tombo_stats.py:269-368  (P10, caller-side, RNA only)
  remove_stall_cpts                    tombo_stats.py:1576-1597
  normalize_raw_signal, compute_base_means, get_read_seg_score, calc_kmer_fitted_shift_scale
                                       tombo_stats.py:482-573, 203-215, 2327-2338, 370-450 (csrc/k_norm_api.h)
  trim_rna, estimate_global_scale      tombo_stats.py:235-267, 452-480 (csrc/k_trim_rna.h)
The numeric kernels (normalisation, event detection, DP ...) live in csrc/ and are reached
through tombo_amd.resquiggle.
"""
import io
import os
import re
import warnings
from collections import namedtuple

import numpy as np

from . import tombo_helper as th, _native, errors
from ._c_helper import llh_ratio_windows
from ._default_parameters import (
    ALGN_PARAMS_TABLE, SEG_PARAMS_TABLE, RNA_SAMP_TYPE, DNA_SAMP_TYPE, STANDARD_MODELS,
    HALF_NORM_EXPECTED_VAL, MIN_EVENT_TO_SEQ_RATIO, STALL_PARAMS, OUTLIER_THRESH, COLLAPSE_RNA_STALLS, SMALLEST_PVAL, FM_OFFSET_DEFAULT,
    SAMP_COMP_TXT, DE_NOVO_TXT, ALT_MODEL_TXT, CONST_SD_MODEL, OCLLHR_SCALE, OCLLHR_HEIGHT,
    OCLLHR_POWER, MEAN_PRIOR_CONST, SD_PRIOR_CONST, ALT_EST_BATCH, MAX_KMER_OBS, MIN_KMER_OBS_TO_EST,
    KERNEL_DENSITY_RANGE, NUM_DENS_POINTS, ROC_PLOT_POINTS, NUM_READS_FOR_SCALE)

_MODEL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tombo_models')
_BASE_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _b in enumerate(b'ACGT'):
    _BASE_CODE[_b] = _i


def encode_seq(seq):
    """ACGT string -> uint8 codes 0..3 (255 for anything else)."""
    if isinstance(seq, str):
        seq = seq.encode()
    return _BASE_CODE[np.frombuffer(seq, dtype=np.uint8)]


class TomboModel(object):
    """Canonical k-mer level table: `means[4**K]`, `sds[4**K]` in lexicographic k-mer order.

    Constructed from a sample type (loads the extracted canonical table), or from
    `kmer_ref=[(kmer, mean, sd), ...]` + `central_pos` like the reference
    (tombo_stats.py:746-813).
    """

    def __init__(self, ref_fn=None, kmer_ref=None, central_pos=None, seq_samp_type=None):
        if kmer_ref is not None:
            assert central_pos is not None, 'central_pos must be provided with kmer_ref'
            kmers = [k for k, _, _ in kmer_ref]
            self.kmer_width = len(kmers[0])
            self.central_pos = int(central_pos)
            self.level_means = np.full(4 ** self.kmer_width, np.nan)
            self.level_sds = np.full(4 ** self.kmer_width, np.nan)
            for k, m, s in kmer_ref:
                if isinstance(k, bytes):
                    k = k.decode()
                c = self._kmer_code(k)
                self.level_means[c] = m
                self.level_sds[c] = s
        else:
            if ref_fn is None:
                if seq_samp_type is None:
                    seq_samp_type = th.seqSampleType(DNA_SAMP_TYPE, False)
                ref_fn = os.path.join(_MODEL_DIR, STANDARD_MODELS[seq_samp_type.name] + '.npz')
            tab = np.load(ref_fn)
            self.kmer_width = len(tab['kmer'][0])
            self.central_pos = int(tab['central_pos'])
            self.level_means = np.ascontiguousarray(tab['mean'], dtype=np.float64)
            self.level_sds = np.ascontiguousarray(tab['sd'], dtype=np.float64)
        self.seq_samp_type = seq_samp_type
        self._dicts = None

    @staticmethod
    def _kmer_code(kmer):
        c = 0
        for b in encode_seq(kmer):
            c = c * 4 + int(b)
        return c

    def _kmer_dicts(self):
        if self._dicts is None:
            from itertools import product
            kmers = [''.join(p) for p in product('ACGT', repeat=self.kmer_width)]
            self._dicts = (dict(zip(kmers, self.level_means.tolist())),
                           dict(zip(kmers, self.level_sds.tolist())))
        return self._dicts

    @property
    def means(self):
        return self._kmer_dicts()[0]

    @property
    def sds(self):
        return self._kmer_dicts()[1]

    def kmer_codes(self, seq):
        """int64 table index of every k-mer window of `seq`."""
        codes = encode_seq(seq).astype(np.int64)
        if (codes > 3).any():
            raise th.TomboError('Invalid sequence encountered from genome sequence.')
        n = codes.shape[0] - self.kmer_width + 1
        if n <= 0:
            return np.empty(0, dtype=np.int64)
        idx = np.zeros(n, dtype=np.int64)
        for j in range(self.kmer_width):
            idx = idx * 4 + codes[j:j + n]
        return idx

    def get_exp_levels_from_seq(self, seq, rev_strand=False):
        idx = self.kmer_codes(seq)
        if rev_strand:
            idx = idx[::-1]
        return self.level_means[idx], self.level_sds[idx]

    def _center_model(self, shift_corr_factor, scale_corr_factor):
        """tombo_stats.py:587-595: every level times the scale factor, plus the shift factor"""
        self.level_means = (self.level_means * scale_corr_factor) + shift_corr_factor
        self._dicts = None

    def _make_constant_sd(self):
        """tombo_stats.py:597-600: every spread becomes the median spread"""
        self.level_sds = np.full(self.level_sds.shape[0], np.median(self.level_sds))
        self._dicts = None

    def write_model(self, ref_fp):
        """tombo_stats.py:602-621 into `ref_fp`, any object with the h5py group interface (an open
        h5py.File): the record array `model` (kmer, mean, sd) in lexicographic k-mer order and the
        attributes central_pos and model_name"""
        kmers = _all_kmers(self.kmer_width)
        tab = np.array(list(zip(kmers, self.level_means.tolist(), self.level_sds.tolist())),
                       dtype=[(str('kmer'), 'S%d' % self.kmer_width), (str('mean'), 'f8'), (str('sd'), 'f8')])
        ref_fp.create_dataset('model', data=tab, compression='gzip')
        ref_fp.attrs['central_pos'] = self.central_pos
        ref_fp.attrs['model_name'] = STANDARD_MODEL_NAME

    def get_exp_levels_from_seq_with_gaps(self, reg_seq, rev_strand):
        """tombo_stats.py:886-915: levels of every k-mer of reg_seq, NaN for k-mers that touch a
        non-ACGT run"""
        K = self.kmer_width
        means, sds = np.full(len(reg_seq) - K + 1, np.nan), np.full(len(reg_seq) - K + 1, np.nan)
        prev = 0
        for m in th.INVALID_BASE_RUNS.finditer(reg_seq):
            if m.start() - prev >= K:
                means[prev:m.start() - K + 1], sds[prev:m.start() - K + 1] = \
                    self.get_exp_levels_from_seq(reg_seq[prev:m.start()])
            prev = m.end()
        if prev <= len(reg_seq) - K:
            means[prev:], sds[prev:] = self.get_exp_levels_from_seq(reg_seq[prev:])
        if rev_strand:
            means, sds = means[::-1], sds[::-1]
        return means, sds


def _engine(engine=None):
    """the engine a statistics call runs on: the given one, else the process-wide engine"""
    if engine is not None:
        return engine
    from . import resquiggle as rq   # (resquiggle imports this module)
    return rq.get_engine()


# ---- pair-wise distance and clustering (tombo_stats.py:126-196; the kernels are csrc/k_pdist.h) ----
def transform_and_trim_stats(reg_stats, are_pvals, trim_value):
    """:130-140, statement for statement: p-values become -log10 in a new array, likelihood ratios are trimmed in
    the array that was passed"""
    if are_pvals:
        with np.errstate(divide='ignore'):
            reg_stats = -np.log10(reg_stats)
        nan_r_stats = np.nan_to_num(reg_stats)
        reg_stats[nan_r_stats > trim_value] = trim_value
    else:
        nan_r_stats = np.nan_to_num(reg_stats)
        reg_stats[nan_r_stats > trim_value] = trim_value
        reg_stats[nan_r_stats < -trim_value] = -trim_value
    return reg_stats


def order_reads(reg_stats, engine=None):
    """The order of the reads (rows) of a per-read statistics matrix in the per-read plots (:142-156): single
    linkage over the NaN-aware mean absolute difference of every pair of rows, leaves in dendrogram order.  The
    distances come from the device (Engine.pairwise_nanmean_dists); a pair of reads that share no position gets the
    largest distance + 1, as in the reference."""
    reg_stats = np.asarray(reg_stats)
    if reg_stats.shape[0] == 1:
        return [0]
    try:
        from scipy.cluster.hierarchy import single, leaves_list
    except ImportError:
        raise th.TomboError('order_reads needs scipy (scipy.cluster.hierarchy), which is not installed.')
    r_dists = _engine(engine).pairwise_nanmean_dists(np.ascontiguousarray(reg_stats, dtype=np.float64))
    with warnings.catch_warnings():   # (all pairs NaN: nanmax warns and gives NaN, as in the reference)
        warnings.simplefilter('ignore', category=RuntimeWarning)
        r_dists[np.isnan(r_dists)] = np.nanmax(r_dists) + 1
    return leaves_list(single(r_dists))


def sliding_window_dist(sig_diffs1, sig_diffs2, slide_span, num_bases):
    """one pair of get_pairwise_dists with slide_span > 0, in numpy (:158-164)"""
    return np.sqrt(min(np.sum(np.square(sig_diffs1[i1:i1 + num_bases] - sig_diffs2[i2:i2 + num_bases]))
                       for i1 in range((slide_span * 2) + 1) for i2 in range((slide_span * 2) + 1)))


def euclidian_dist(sig_diffs1, sig_diffs2):
    """one pair of get_pairwise_dists with slide_span 0, in numpy (:166-169)"""
    return np.sqrt(np.sum(np.square(sig_diffs1 - sig_diffs2)))


def get_pairwise_dists(reg_sig_diffs, slide_span=0, engine=None):
    """The distances between the signal-shift profiles of regions (:171-196) -> float64[R, R], row i holding the
    distances to the regions j <= i and 0 beyond: the rows the reference's workers put on their queue, all from one
    engine call.  slide_span None counts as 0.  Profiles of unequal length (a region cut by a chromosome end) raise
    th.TomboError; the reference fails there with a broadcast error."""
    slide_span = int(slide_span) if slide_span else 0
    profiles = [np.asarray(v, dtype=np.float64) for v in reg_sig_diffs]
    if len(profiles) == 0:
        raise th.TomboError('No regions to compute distances between.')
    row_len = profiles[0].shape[0]
    for i, v in enumerate(profiles):
        if v.ndim != 1 or v.shape[0] != row_len:
            raise th.TomboError('Region %d holds %s signal differences where the first region holds %d: a region cut '
                                'by the end of its chromosome cannot be compared.' % (
                                    i, 'x'.join(str(d) for d in v.shape), row_len))
    if slide_span < 0 or row_len - 2 * slide_span < 1:
        raise th.TomboError('Regions of %d bases leave no window with a slide span of %d.' % (row_len, slide_span))
    return _engine(engine).pairwise_window_dists(np.ascontiguousarray(np.stack(profiles)), slide_span)


class _CoveredPositions(object):
    """`pos in covered` over a boolean track, where the reference builds a set of every covered position"""
    def __init__(self, covered=None):
        self.covered = np.zeros(0, dtype=np.bool_) if covered is None else covered

    def __contains__(self, pos):
        return 0 <= pos < self.covered.shape[0] and bool(self.covered[pos])


class _CoveredByBoth(dict):
    """{(chrm, strand): _CoveredPositions}; a (chrm, strand) that one of the two indices lacks covers nothing (the
    reference's plain dict raises KeyError for a significant region there)"""
    def __missing__(self, key):
        return _CoveredPositions()


def cluster_most_signif_dists(stats, reads_index, ctrl_reads_index, num_regions, num_bases, slide_span=0,
                              genome_index=None, with_seqs=False, engine=None):
    """The data half of `tombo plot cluster_most_significant` (_plot_commands.py:2122-2214) -> (dists float64[R, R],
    intervals, column names or None): the most significant regions of num_bases + 2 slide_span bases, those kept
    that are covered by both sets of reads at every position and do not start inside an earlier one, the pairwise
    distances of their sample - control signal differences.  with_seqs: the reference's column names
    `seq::chrm::strand::start + 1`, the sequence over the region widened by two bases on either side, from
    genome_index or else from the sample's reads (each listed twice, as the reference merges the region with
    itself).  As in the reference, the genome index refuses (th.TomboError) the widened form of a region that starts
    within two bases of its chromosome's start or ends within two of its end."""
    eng = _engine(engine)
    slide_span = int(slide_span) if slide_span else 0
    width = num_bases + 2 * slide_span
    plot_intervals = stats.get_most_signif_regions(width, num_regions)
    cov, ctrl_cov = th.compute_coverage(reads_index, engine=eng), th.compute_coverage(ctrl_reads_index, engine=eng)
    covered_poss = _CoveredByBoth()
    for cs in set(cov).intersection(ctrl_cov):
        n = min(cov[cs].shape[0], ctrl_cov[cs].shape[0])
        covered_poss[cs] = _CoveredPositions((cov[cs][:n] > 0) & (ctrl_cov[cs][:n] > 0))
    plot_intervals = th.get_unique_intervals(plot_intervals, covered_poss)
    if len(plot_intervals) == 0:
        raise th.TomboError('No significant region is covered by both sets of reads.')
    col_names = None
    if with_seqs:
        col_names = []
        for chrm, start, _, strand, _, _ in plot_intervals:
            seq_start, seq_end = start - 2, start + 2 + width
            if genome_index is not None:
                seq = genome_index.get_seq(chrm, seq_start, seq_end)
            else:
                reads = [rd for rd in reads_index.get((chrm, strand), ())
                         if not (rd.start >= seq_end or rd.end <= seq_start)]
                seq = th.get_region_seq(reads + reads, seq_start, seq_end)
            col_names.append('::'.join((seq, chrm, strand, str(start + 1))))
    signal_diffs = th.get_signal_differences(reads_index, ctrl_reads_index, engine=eng)
    reg_sig_diffs = [signal_diffs[(chrm, strand)][start:start + width] for chrm, start, _, strand, _, _ in plot_intervals]
    return get_pairwise_dists(reg_sig_diffs, slide_span, engine=eng), plot_intervals, col_names


def get_dynamic_prog_params(match_evalue):
    return HALF_NORM_EXPECTED_VAL + match_evalue, match_evalue


def load_resquiggle_parameters(seq_samp_type, sig_aln_params=None, seg_params=None,
                               use_save_bandwidth=False):
    if sig_aln_params is None:
        (match_evalue, skip_pen, bandwidth, save_bandwidth, max_half_z_score,
         band_bound_thresh, start_bw, start_save_bw,
         start_n_bases) = ALGN_PARAMS_TABLE[seq_samp_type.name]
    else:
        (match_evalue, skip_pen, bandwidth, save_bandwidth, max_half_z_score,
         band_bound_thresh, start_bw, start_save_bw, start_n_bases) = sig_aln_params
        bandwidth, save_bandwidth, band_bound_thresh = (
            int(bandwidth), int(save_bandwidth), int(band_bound_thresh))
        start_bw, start_save_bw, start_n_bases = (
            int(start_bw), int(start_save_bw), int(start_n_bases))
    if use_save_bandwidth:
        bandwidth = save_bandwidth
    if seg_params is None:
        seg_params = SEG_PARAMS_TABLE[seq_samp_type.name]
    running_stat_width, min_obs_per_base, raw_min_obs_per_base, mean_obs_per_event = seg_params
    z_shift, stay_pen = get_dynamic_prog_params(match_evalue)
    return th.resquiggleParams(
        match_evalue, skip_pen, bandwidth, max_half_z_score, running_stat_width,
        min_obs_per_base, raw_min_obs_per_base, mean_obs_per_event, z_shift, stay_pen,
        seq_samp_type.name == RNA_SAMP_TYPE, band_bound_thresh, start_bw, start_save_bw,
        start_n_bases)


def compute_num_events(signal_len, seq_len, mean_obs_per_event,
                       min_event_to_seq_ratio=MIN_EVENT_TO_SEQ_RATIO):
    return max(signal_len // mean_obs_per_event, int(seq_len * min_event_to_seq_ratio))


def identify_stalls(all_raw_signal, stall_params=None, return_metric=False):
    """Stall intervals of one read (caller-side RNA preparation, tombo_stats.py:269-368, the
    running-window-mean method): computed on the device (`tba_identify_stalls`; kernels in
    csrc/k_prep_raw.h, the same ones a batch runs under `tba_opts.detect_stalls`).  Returns a list
    of [start, end] int64 pairs like the reference.  int16 DAC, float32 and float64 samples are
    taken as they are (DAC sums are exact, float sums keep np.cumsum's order)."""
    if return_metric:
        raise NotImplementedError('the per-sample stall metric stays on the device')
    sp = th.stallParams(**STALL_PARAMS) if stall_params is None else stall_params
    if sp.lower_pctl is not None and sp.upper_pctl is not None:
        raise NotImplementedError('the percentile stall detector (PCTL_STALL_PARAMS) is not the '
                                  'reference default and not part of this engine')
    return list(_native.identify_stalls(_engine(), all_raw_signal, sp))


def remove_stall_cpts(stall_ints, valid_cpts):
    """Drop change points strictly inside a stall interval (same walk as the reference,
    including its behaviour once the interval iterator is exhausted)."""
    if len(stall_ints) == 0:
        return valid_cpts
    it = iter(stall_ints)
    cur = next(it)
    keep = []
    for i, cpt in enumerate(valid_cpts):
        while cpt > cur[1]:
            try:
                cur = next(it)
            except StopIteration:
                break
        if not (cur[0] < cpt < cur[1]):
            keep.append(i)
    return valid_cpts[keep]


# ---- RNA adapter trimming and the global scale estimate (tombo_stats.py:235-267, :452-480; csrc/k_trim_rna.h) ----
DEFAULT_TRIM_RNA_PARAMS = th.trimRnaParams(moving_window_size=50, min_running_values=100, thresh_scale=0.7,
                                           max_raw_obs=40000)     # tombo_stats.py:98-100
_TRIM_TOO_FEW_MSG = 'negative dimensions are not allowed'          # numpy's, from as_strided's shape
_NO_SCALE_READS_MSG = 'No reads contain raw signal for global scale parameter estimation.'
_FEW_SCALE_READS_MSG = ('Few reads contain raw signal for global scale parameter estimation. Results may not be '
                        'optimal.')


def _trim_error(status):
    """the exception the reference's trim_rna ends in for a read of this status, or None"""
    status = int(status)
    if status == 0:
        return None
    if status == _native.TRIM_TOO_FEW_EVENTS:
        return ValueError(_TRIM_TOO_FEW_MSG)
    try:
        errors.raise_for_status(status)
    except Exception as e:
        return e


def _raw_for_device(raws):
    """the reads as the raw-signal entries take them: int16 where every read is, else float64 (astype(np.float64)
    gives int16 samples the same values, which is what the reference computes on)"""
    raws = [np.asarray(r) for r in raws]
    if any(r.ndim != 1 for r in raws):
        raise ValueError('every read needs a one-dimensional signal')
    if not all(r.dtype == np.int16 for r in raws):
        raws = [r if r.dtype == np.float64 else r.astype(np.float64) for r in raws]
    return raws


def trim_rna_batch(raws, rsqgl_params, trim_rna_params=DEFAULT_TRIM_RNA_PARAMS, engine=None):
    """trim_rna of every read of `raws` in one engine call -> (int64 adapter ends, a list holding None or, for a read
    the reference's trim_rna raises on, that exception: th.TomboError('Fewer changepoints found than requested'),
    ValueError('negative dimensions are not allowed')); a failing read's end is 0 and the others are unaffected.
    Only the first max_raw_obs samples of a read are handed to the device."""
    raws = _raw_for_device(raws)
    if len(raws) == 0:
        return np.zeros(0, np.int64), []
    ends, status = _engine(engine).trim_rna(
        raws, (rsqgl_params.running_stat_width, rsqgl_params.min_obs_per_base, rsqgl_params.mean_obs_per_event),
        trim_rna_params)
    return ends, [_trim_error(st) for st in status]


def trim_rna(all_raw_signal, rsqgl_params, trim_rna_params=DEFAULT_TRIM_RNA_PARAMS, engine=None):
    """tombo_stats.py:235-267 -> the end of the DNA adapter at the head of a direct-RNA read's signal (acquisition
    order), 0 when no window qualifies; raises what the reference raises"""
    ends, errs = trim_rna_batch([all_raw_signal], rsqgl_params, trim_rna_params, engine)
    if errs[0] is not None:
        raise errs[0]
    return int(ends[0])


def estimate_global_scale(fast5s, num_reads=NUM_READS_FOR_SCALE, engine=None):
    """tombo_stats.py:452-480: np.mean of the MADs of up to num_reads reads.  fast5s: a list of open FAST5-like objects
    (th.get_raw_read_slot) or raw signal arrays, shuffled in place with numpy's global RNG as the reference shuffles
    its file names; items without a raw slot (or without a sample) are skipped, the first num_reads others are taken
    and go through one engine call (np.median and the MAD by exact selection, no normalised signal)."""
    np.random.shuffle(fast5s)
    sigs = []
    for item in fast5s:
        try:
            sig = np.asarray(item if isinstance(item, np.ndarray) else th.get_raw_read_slot(item)['Signal'][:])
            if sig.ndim != 1 or sig.shape[0] < 1:
                continue
        except Exception:
            continue
        sigs.append(sig)
        if len(sigs) >= num_reads:
            break
    if len(sigs) == 0:
        raise th.TomboError(_NO_SCALE_READS_MSG)
    if len(sigs) < num_reads:
        warnings.warn(_FEW_SCALE_READS_MSG)
    _, mads = _engine(engine).raw_med_mad(_raw_for_device(sigs))
    return np.mean(mads)


# ---------------------------------------------------------------------------------------------
# The documented per-read functions of tombo_stats.__all__ (tombo_stats.py:203-215, :370-450, :482-573,
# :2327-2338): the kernels are csrc/k_norm_api.h, the `*_batch` forms run one engine call for all reads and
# the reference's single-read functions are batches of one.
NORM_TYPES = ('none', 'pA', 'pA_raw', 'median', 'robust_median', 'median_const_scale')     # tombo_stats.py:107
_NORM_TYPE_CODES = {'none': _native.NORMTYPE_NONE, 'pA': _native.NORMTYPE_PA_RAW, 'pA_raw': _native.NORMTYPE_PA_RAW,
                    'median': _native.NORMTYPE_MEDIAN, 'median_const_scale': _native.NORMTYPE_MEDIAN_CONST_SCALE,
                    'robust_median': _native.NORMTYPE_ROBUST_MEDIAN}
_SLOPE_ZERO_MSG = 'Read failed sequence-based signal re-scaling parameter estimation.'


def compute_base_means(all_raw_signal, base_starts):
    """tombo_stats.py:203-215: base mean levels from raw signal and 0-based base start positions (with the end)"""
    from ._c_helper import c_new_means
    return c_new_means(all_raw_signal.astype(np.float64), base_starts)


def get_read_seg_scores_batch(reads, engine=None):
    """get_read_seg_score of every (r_means, r_ref_means, r_ref_sds) triple of `reads` in one engine call -> a list
    of float64 scores"""
    reads = [tuple(np.ascontiguousarray(a, dtype=np.float64) for a in rd) for rd in reads]
    if len(reads) == 0:
        return []
    if any(len(rd) != 3 or any(a.ndim != 1 or a.shape != rd[0].shape for a in rd) for rd in reads):
        raise ValueError('every read is a triple of one-dimensional arrays of one length')
    off = _csr_offsets([rd[0].shape[0] for rd in reads])
    scores = _engine(engine).seg_scores(*(np.concatenate([rd[j] for rd in reads]) for j in range(3)), off)
    return list(scores)


def get_read_seg_score(r_means, r_ref_means, r_ref_sds):
    """tombo_stats.py:2327-2338: np.mean(np.abs((r_means - r_ref_means) / r_ref_sds)), numpy's summation order"""
    return _only(get_read_seg_scores_batch([(r_means, r_ref_means, r_ref_sds)]))


def _mom_corr_factors(points, engine=None):
    """the 'mom' branch of calc_kmer_fitted_shift_scale (:427-440) for a list of (event means, model means, model
    inverse variances): the five sums of every read on the device in one call, the 2x2 solve on the host"""
    points = [tuple(np.ascontiguousarray(a, dtype=np.float64) for a in p) for p in points]
    off = _csr_offsets([p[0].shape[0] for p in points])
    sums = _engine(engine).mom_sums(*(np.concatenate([p[j] for p in points]) for j in range(3)), off)
    out = []
    for iv_sum, mv_sum, mvm_sum, ev_sum, evm_sum in sums:
        coef_mat = np.array(((iv_sum, mv_sum), (mv_sum, mvm_sum)))
        out.append(tuple(np.linalg.solve(coef_mat, np.array((ev_sum, evm_sum)))))
    return out


def calc_kmer_fitted_shift_scale(prev_shift, prev_scale, r_event_means, r_model_means, r_model_inv_vars=None,
                                 method='theil_sen'):
    """tombo_stats.py:370-450 -> (shift, scale, shift_corr_factor, scale_corr_factor).  'theil_sen': the slopes of
    c_compute_slopes and both medians on the device (above MAX_POINTS_FOR_THEIL_SEN points the np.random.choice draw is
    made here, in the reference's place in the random stream); 'mom': the five sums on the device, np.linalg.solve
    on the host; 'robust' (scipy's Nelder-Mead) is not built."""
    if method == 'robust':
        raise NotImplementedError("calc_kmer_fitted_shift_scale: method 'robust' (scipy Nelder-Mead) is not built")
    elif method == 'theil_sen':
        from ._c_helper import c_compute_slopes
        n_points = r_model_means.shape[0]
        if n_points > _native.MAX_POINTS_FOR_THEIL_SEN:
            samp_ind = np.random.choice(n_points, _native.MAX_POINTS_FOR_THEIL_SEN, replace=False)
            r_model_means = r_model_means[samp_ind]
            r_event_means = r_event_means[samp_ind]
        r_event_means = np.ascontiguousarray(r_event_means, dtype=np.float64)
        r_model_means = np.ascontiguousarray(r_model_means, dtype=np.float64)
        eng = _engine()
        slopes = c_compute_slopes(r_event_means, r_model_means)
        slope = eng.segment_medians(slopes, _csr_offsets([slopes.shape[0]]))[0]
        inters = r_model_means - (slope * r_event_means)
        inter = eng.segment_medians(inters, _csr_offsets([inters.shape[0]]))[0]
        if slope == 0:
            raise th.TomboError(_SLOPE_ZERO_MSG)
        scale_corr_factor = 1 / slope
        shift_corr_factor = -inter / slope
    elif method == 'mom':
        shift_corr_factor, scale_corr_factor = _only(_mom_corr_factors(
            [(r_event_means, r_model_means, r_model_inv_vars)]))
    else:
        raise th.TomboError('Invalid k-mer fitted normalization parameter method: ' + method +
                            '\n\t\tValid methods are "robust" and "mom".')
    shift = prev_shift + (shift_corr_factor * prev_scale)
    scale = prev_scale * scale_corr_factor
    return shift, scale, shift_corr_factor, scale_corr_factor


def _per_read(values, n, what):
    if values is None:
        return [None] * n
    values = list(values)
    if len(values) != n:
        raise ValueError('%s: one entry per read' % what)
    return values


def normalize_raw_signal_batch(raws, read_starts=None, read_obs_lens=None, norm_type='median', outlier_thresh=None,
                               channel_infos=None, scale_values=None, const_scale=None, event_means=None,
                               model_means=None, model_inv_vars=None, engine=None):
    """normalize_raw_signal of every read of `raws` in one engine call -> a list of (norm_signal, th.scaleValues); a
    read whose scale is exactly 0 (the reference's FloatingPointError) gets None and the others are unaffected.
    read_starts / read_obs_lens / channel_infos / scale_values / event_means / model_means / model_inv_vars: None, or
    one entry per read (which may be None).  int16 and float64 signals are taken as they are (a batch that mixes
    them is computed in float64, which gives int16 samples the same values), any other dtype is converted with
    astype(np.float64) first."""
    raws = [np.asarray(r) for r in raws]
    n = len(raws)
    if n == 0:
        return []
    starts = [0 if s is None else int(s) for s in _per_read(read_starts, n, 'read_starts')]
    lens = [r.shape[0] - s if ln is None else int(ln)
            for r, s, ln in zip(raws, starts, _per_read(read_obs_lens, n, 'read_obs_lens'))]
    svs = _per_read(scale_values, n, 'scale_values')
    chans = _per_read(channel_infos, n, 'channel_infos')
    if norm_type not in NORM_TYPES and any(sv is None for sv in svs):
        raise th.TomboError('Normalization type ' + norm_type + ' is not a valid ' +
                            'option and shift or scale parameters were not provided.')
    if norm_type == 'median_const_scale' and any(sv is None for sv in svs):
        assert const_scale is not None
    # the reference slices: a window that runs past the end is cut there
    lens = [max(0, min(ln, r.shape[0] - s)) for r, s, ln in zip(raws, starts, lens)]
    if any(r.ndim != 1 or s < 0 or ln < 1 for r, s, ln in zip(raws, starts, lens)):
        raise ValueError('every read needs a one-dimensional signal and a window of at least one sample inside it')
    if not all(r.dtype == np.int16 for r in raws):
        raws = [r if r.dtype == np.float64 else r.astype(np.float64) for r in raws]
    fitted = {}
    if norm_type == 'pA':
        todo = [i for i in range(n) if svs[i] is None]
        pts = list(zip(*(_per_read(a, n, 'event_means, model_means, model_inv_vars')
                         for a in (event_means, model_means, model_inv_vars))))
        for i, (shift_corr, scale_corr) in zip(todo, _mom_corr_factors([pts[i] for i in todo], engine) if todo else ()):
            shift, scale = -1 * chans[i].offset, chans[i].digitisation / chans[i].range
            fitted[i] = th.scaleValues(shift + (shift_corr * scale), scale * scale_corr, None, None, None)
    sv_in, sv_flags = _native.pack_scale_values([fitted.get(i, svs[i]) for i in range(n)])
    channel = None
    if norm_type == 'pA_raw' and any(sv is None for sv in svs):
        channel = np.zeros((n, 3), np.float64)
        for i in range(n):
            if svs[i] is None:
                channel[i] = chans[i].offset, chans[i].range, chans[i].digitisation
    sv, _, norms, status = _engine(engine).normalize_raw_batch(
        raws, starts, lens, _NORM_TYPE_CODES.get(norm_type, _native.NORMTYPE_NONE), sv_in, sv_flags, channel,
        outlier_thresh, const_scale)
    out = []
    for i in range(n):
        if status[i] != 0:
            out.append(None)
            continue
        shift, scale, lower_lim, upper_lim = sv[i]
        if svs[i] is not None:
            shift, scale = svs[i].shift, svs[i].scale
        elif norm_type == 'none':
            shift, scale = 0, 1
        elif norm_type == 'median_const_scale':
            scale = const_scale
        if outlier_thresh is None:
            lower_lim, upper_lim = (None, None) if svs[i] is None else (svs[i].lower_lim, svs[i].upper_lim)
        out.append((norms[i], th.scaleValues(shift, scale, lower_lim, upper_lim, outlier_thresh)))
    return out


def normalize_raw_signal(all_raw_signal, read_start_rel_to_raw=0, read_obs_len=None, norm_type='median',
                         outlier_thresh=None, channel_info=None, scale_values=None, event_means=None, model_means=None,
                         model_inv_vars=None, const_scale=None):
    """tombo_stats.py:482-573 -> (normalised signal, th.scaleValues(shift, scale, lower_lim, upper_lim,
    outlier_thresh)).  A scale of exactly 0 raises FloatingPointError, as the reference's division does under its
    np.seterr(all='raise')."""
    res = _only(normalize_raw_signal_batch(
        [all_raw_signal], [read_start_rel_to_raw], [read_obs_len], norm_type, outlier_thresh, [channel_info],
        [scale_values], const_scale, [event_means], [model_means], [model_inv_vars]))
    if res is None:
        raise FloatingPointError('divide by zero encountered in divide')
    return res


# ---------------------------------------------------------------------------------------------
# Row N4: per-read test statistics over resquiggled reads -- the three
# `compute_*_read_stats` functions of tombo_stats.py:3675-4083 after their file access.  The
# reference loads `norm_mean` / `base` of one read from its FAST5 file and computes with numpy /
# scipy / Cython, one read per call; here the read is a `th.resquiggledRead` (the same columns in
# memory, e.g. straight from `resquiggle_batch_events`), the `*_batch` forms take a list of reads
# and run ONE kernel launch for all tested positions of all reads (`Engine.read_pvals`,
# `Engine.llh_ratio_windows`); the single-read functions are batches of one and keep the
# reference's return shape ({name: stats}, {name: positions}, read_id).  Host code only does what
# the reference does with slices: clipping to the region, strand flips, motif search.
class AltModel(object):
    """Alternate-base k-mer model (tombo_stats.py:922-1125), from
    `kmer_ref=[(kmer, pos, mean, sd), ...]`: expected level of a k-mer when the base at `pos` is
    the alternate base.  `motif`: `th.TomboMotif` with a modified position (default: the bare
    alternate base)."""

    def __init__(self, kmer_ref, central_pos, alt_base, name=None, motif=None):
        self.means, self.sds = {}, {}
        for kmer, pos, m, s in kmer_ref:
            if isinstance(kmer, bytes):
                kmer = kmer.decode()
            self.means[(kmer, int(pos))] = float(m)
            self.sds[(kmer, int(pos))] = float(s)
        self.central_pos, self.alt_base, self.name = int(central_pos), alt_base, name
        self.motif = th.TomboMotif(alt_base, 1) if motif is None else motif
        assert self.motif.mod_pos is not None
        self.kmer_width = len(next(iter(self.means))[0])

    def get_exp_levels_from_kmers(self, seq_kmers, rev_strand=False):
        """levels across a central base: the alternate base is the last base of the first
        k-mer and the first base of the last one (tombo_stats.py:1096-1125)"""
        K = self.kmer_width
        pos_range = range(K) if rev_strand else range(K - 1, -1, -1)
        nan = float('nan')
        return (np.array([self.means.get((k, p), nan) for k, p in zip(seq_kmers, pos_range)]),
                np.array([self.sds.get((k, p), nan) for k, p in zip(seq_kmers, pos_range)]))

    def _make_constant_sd(self):
        """tombo_stats.py:955-958: every spread becomes the median spread"""
        med_sd = np.median(list(self.sds.values()))
        self.sds = dict((key, med_sd) for key in self.sds)

    def write_model(self, ref_fp):
        """tombo_stats.py:929-953 into `ref_fp`, any object with the h5py group interface (an open
        h5py.File, like `tombo_helper.write_new_fast5_group` takes one): the record array `model`
        (kmer, pos, mean, sd) and the attributes central_pos, model_name, alt_base, motif, mod_pos"""
        tab = np.array([(kmer, pos, self.means[(kmer, pos)], self.sds[(kmer, pos)]) for kmer, pos in self.means],
                       dtype=[(str('kmer'), 'S%d' % self.kmer_width), (str('pos'), 'u4'), (str('mean'), 'f8'),
                              (str('sd'), 'f8')])
        ref_fp.create_dataset('model', data=tab, compression='gzip')
        ref_fp.attrs['central_pos'] = self.central_pos
        ref_fp.attrs['model_name'] = self.name
        ref_fp.attrs['alt_base'] = self.alt_base
        ref_fp.attrs['motif'] = self.motif.raw_motif
        ref_fp.attrs['mod_pos'] = self.motif.mod_pos


def _csr_offsets(lengths):
    """int64 [0, l0, l0 + l1, ...]"""
    return np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int64)


def _concat_f64(arrays):
    return np.ascontiguousarray(np.concatenate(arrays) if arrays else np.empty(0), dtype=np.float64)


def _only(batch_of_one):
    """the result of a batch of one; an exception stored in its place is raised"""
    if isinstance(batch_of_one[0], Exception):
        raise batch_of_one[0]
    return batch_of_one[0]


def _fm_guard(n, fm_offset):
    if fm_offset > 0 and n < 2 * fm_offset + 1:   # calc_window_fishers_method, :2257-2259
        raise th.TomboError("P-values vector too short for Fisher's Method window compuation.")


def _clip_to_region(rd, reg_data, fm_offset, lags, *cols):
    """the region clip the z tests start with (:3815-3836, :3716-3737): the read-centric columns lose
    what lies further outside the region than fm_offset plus the k-mer lag of that end (`lags`:
    (before, after) on '+') -> (region start, read start, read end, the two lags, clipped columns)"""
    reg_start, reg_end = (rd.start, rd.end) if reg_data is None else (reg_data.start, reg_data.end)
    lag_b, lag_e = lags if rd.strand == '+' else lags[::-1]
    read_start, read_end = rd.start, rd.end
    if read_start + lag_b + fm_offset < reg_start:
        c = reg_start - (read_start + lag_b + fm_offset)
        read_start = reg_start - lag_b - fm_offset
        cols = [x[c:] if rd.strand == '+' else x[:-c] for x in cols]
    if read_end - lag_e - fm_offset > reg_end:
        c = (read_end - lag_e - fm_offset) - reg_end
        read_end = reg_end + lag_e + fm_offset
        cols = [x[:-c] if rd.strand == '+' else x[c:] for x in cols]
    return reg_start, read_start, read_end, lag_b, lag_e, cols


def _prep_de_novo_read(rd, std_ref, fm_offset, reg_data):
    """the per-read preparation of compute_de_novo_read_stats (:3796-3855): region clip, strand
    flip, k-mer levels, lags -> (means, ref_means, ref_sds, first position, end position)"""
    K, cp = std_ref.kmer_width, std_ref.central_pos
    dn = K - cp - 1
    if rd.means is None or rd.seq is None:
        raise th.TomboError('Read does not contain valid re-squiggled data.')
    _, read_start, read_end, lag_b, lag_e, (means, seq) = _clip_to_region(
        rd, reg_data, fm_offset, (cp, dn), np.asarray(rd.means, dtype=np.float64), rd.seq)
    if len(seq) < K:
        raise th.TomboError('Read does not contain information in this region.')
    ref_m, ref_s = std_ref.get_exp_levels_from_seq(seq, rd.strand == '-')
    if rd.strand == '-':
        means = means[::-1]
    means = means[lag_b:means.shape[0] - lag_e]
    _fm_guard(means.shape[0], fm_offset)
    return means, ref_m, ref_s, read_start + lag_b, read_end - lag_e


def _read_pvals(means, ref_means, ref_sds, off, fm_offset, floor_out, engine=None):
    return _engine(engine).read_pvals(means, ref_means, ref_sds, off, fm_offset, floor_out, SMALLEST_PVAL)


def _z_pvals_per_read(prep, fm_offset, floor_out, engine):
    """one `read_pvals` call for prepared reads (means, ref_means, ref_sds, ...) -> p-values per read"""
    off = _csr_offsets([p[0].shape[0] for p in prep])
    pv = _read_pvals(*(np.concatenate([p[k] for p in prep]) for k in range(3)), off, fm_offset, floor_out, engine)
    return [pv[a:b] for a, b in zip(off[:-1], off[1:])]


def compute_de_novo_read_stats_batch(reads, std_ref, fm_offset=FM_OFFSET_DEFAULT, reg_data=None,
                                     engine=None):
    """compute_de_novo_read_stats (tombo_stats.py:3771-3873) for a list of `th.resquiggledRead`;
    per read (pvals, positions) or the TomboError the reference raises."""
    prep, out = {}, [None] * len(reads)
    for i, rd in enumerate(reads):
        try:
            prep[i] = _prep_de_novo_read(rd, std_ref, fm_offset, reg_data)
        except th.TomboError as e:
            out[i] = e
    if prep:
        for (i, p), pv in zip(prep.items(), _z_pvals_per_read(list(prep.values()), fm_offset, True, engine)):
            out[i] = (pv.copy(), np.arange(p[3], p[4]))
    return out


def compute_de_novo_read_stats(r_data, std_ref, fm_offset=FM_OFFSET_DEFAULT, reg_data=None):
    res = _only(compute_de_novo_read_stats_batch([r_data], std_ref, fm_offset, reg_data))
    return {DE_NOVO_TXT: res[0]}, {DE_NOVO_TXT: res[1]}, r_data.read_id


def _prep_sample_compare_read(rd, cm, cs, fm_offset, reg_data):
    """the per-read preparation of compute_sample_compare_read_stats (:3700-3750): region clip,
    strand flip, the control levels under the read -> (means, ctrl_means, ctrl_sds, first position)"""
    if rd.means is None:
        raise th.TomboError('Read does not contain re-squiggled level means.')
    reg_start, read_start, read_end, _, _, (means,) = _clip_to_region(
        rd, reg_data, fm_offset, (0, 0), np.asarray(rd.means, dtype=np.float64))
    if rd.strand == '-':
        means = means[::-1]
    a, b = read_start - reg_start + fm_offset, read_end - reg_start + fm_offset
    if a < 0 or b > cm.shape[0] or b - a != means.shape[0]:
        raise ValueError('control levels do not cover the read inside the region')
    zvalid = ~(np.isnan(means) | np.isnan(cm[a:b]) | np.isnan(cs[a:b]))
    if not zvalid.any():
        raise th.TomboError('No valid z-scores in read.')
    _fm_guard(means.shape[0], fm_offset)
    return means, cm[a:b], cs[a:b], read_start


def compute_sample_compare_read_stats_batch(reads, ctrl_means, ctrl_sds,
                                            fm_offset=FM_OFFSET_DEFAULT, reg_data=None,
                                            engine=None):
    """compute_sample_compare_read_stats (tombo_stats.py:3675-3769) for a list of reads.
    `ctrl_means` / `ctrl_sds`: control-sample levels over the region extended by fm_offset on
    both sides (NaN where the control has no coverage); with reg_data=None every read is its own
    region, so they are per-read lists."""
    prep, out = {}, [None] * len(reads)
    for i, rd in enumerate(reads):
        try:
            if rd.means is None:
                raise th.TomboError('Read does not contain re-squiggled level means.')
            cm = np.asarray(ctrl_means[i] if reg_data is None else ctrl_means, dtype=np.float64)
            cs = np.asarray(ctrl_sds[i] if reg_data is None else ctrl_sds, dtype=np.float64)
            prep[i] = _prep_sample_compare_read(rd, cm, cs, fm_offset, reg_data)
        except th.TomboError as e:
            out[i] = e
    if prep:
        for (i, p), pv in zip(prep.items(), _z_pvals_per_read(list(prep.values()), fm_offset, False, engine)):
            poss = np.where(~np.isnan(pv))[0]
            out[i] = (pv[poss].copy(), poss + p[3])
    return out


def compute_sample_compare_read_stats(r_data, ctrl_means, ctrl_sds, fm_offset=FM_OFFSET_DEFAULT,
                                      reg_data=None):
    res = _only(compute_sample_compare_read_stats_batch(
        [r_data], [ctrl_means] if reg_data is None else ctrl_means,
        [ctrl_sds] if reg_data is None else ctrl_sds, fm_offset, reg_data))
    return {SAMP_COMP_TXT: res[0]}, {SAMP_COMP_TXT: res[1]}, r_data.read_id


def trim_seq_and_means(seq, means, r_start, reg_start, reg_end, strand, kmer_width, central_pos,
                       max_motif_bb, max_motif_ab):
    """tombo_stats.py:3889-3970: read-centric k-mers, model-able means, first alt-testable
    genomic position, motif search sequence"""
    r_end = r_start + means.shape[0]
    motif_search_seq = seq
    n_start_clip = n_end_clip = 0
    if r_start + kmer_width - 1 < reg_start:
        if strand == '+':
            n_start_clip = reg_start - (r_start + kmer_width - 1)
        else:
            n_end_clip = reg_start - (r_start + kmer_width - 1)
        r_start = reg_start - (kmer_width - 1)
    if r_end - kmer_width + 1 > reg_end:
        if strand == '+':
            n_end_clip = r_end - kmer_width + 1 - reg_end
        else:
            n_start_clip = r_end - kmer_width + 1 - reg_end
    seq = seq[n_start_clip:]
    if n_end_clip > 0:
        seq = seq[:-n_end_clip]
    means = means[n_start_clip + central_pos:]
    means = means[:-(n_end_clip + kmer_width - central_pos - 1)]
    if means.shape[0] < kmer_width:
        raise th.TomboError('Read sequence too short in this region.')
    kmers = th.get_seq_kmers(seq, kmer_width)
    if len(kmers) != means.shape[0]:
        raise th.TomboError('Mismatching k-mer and mean levels.')
    r_start += kmer_width - 1
    lead = n_start_clip + kmer_width - 1 - max_motif_bb
    motif_search_seq = motif_search_seq[lead:] if lead >= 0 else 'N' * -lead + motif_search_seq
    tail = n_end_clip + kmer_width - 1 - max_motif_ab
    # (tail == 0 slices with [:-0], i.e. to the empty string, as the reference's own line does)
    motif_search_seq = motif_search_seq[:-tail] if tail >= 0 else motif_search_seq + 'N' * -tail
    return kmers, means, r_start, motif_search_seq


def _alt_motif_bounds(alt_refs):
    return (max(ar.motif.mod_pos - 1 for _, ar in alt_refs),
            max(ar.motif.motif_len - ar.motif.mod_pos for _, ar in alt_refs))


def _prep_alt_model_read(rd, std_ref, alt_refs, use_standard_llhr, reg_data, max_bb, max_ab):
    """the per-read preparation of compute_alt_model_read_stats (:3995-4076): trim, motif search,
    levels -> per alternate model (name, positions, windows); a window is
    (means[K], ref_means[K], alt_means[K], ref_vars[K], alt_vars[K])"""
    K = std_ref.kmer_width
    if rd.means is None or rd.seq is None:
        raise th.TomboError('Read does not contain valid re-squiggled data.')
    reg_start, reg_end = (rd.start, rd.end) if reg_data is None else (reg_data.start, reg_data.end)
    kmers, means, r_start, msseq = trim_seq_and_means(
        rd.seq, np.asarray(rd.means, dtype=np.float64), rd.start, reg_start, reg_end,
        rd.strand, K, std_ref.central_pos, max_bb, max_ab)
    testable_len = means.shape[0] - K + 1
    idx = np.array([std_ref._kmer_code(k) for k in kmers], dtype=np.int64)
    ref_m, ref_v = std_ref.level_means[idx], np.square(std_ref.level_sds[idx])
    res = []
    for name, ar in alt_refs:
        s_seq = msseq[max_bb - (ar.motif.mod_pos - 1):]
        cut = max_ab - (ar.motif.motif_len - ar.motif.mod_pos)
        if cut > 0:
            s_seq = s_seq[:-cut]
        poss, wins = [], []
        for m in ar.motif.motif_pat.finditer(s_seq):
            ap = m.start()
            poss.append(r_start + ap if rd.strand == '+' else r_start + testable_len - ap - 1)
            am, asd = ar.get_exp_levels_from_kmers(kmers[ap:ap + ar.kmer_width])
            if not CONST_SD_MODEL and not use_standard_llhr:
                raise th.TomboError('Variable SD scaled likelihood ratio not implemented.')
            wins.append((means[ap:ap + K], ref_m[ap:ap + K], am, ref_v[ap:ap + K], np.square(asd)))
        res.append((name, np.array(poss), wins))
    return res


def _llh_kind(use_standard_llhr):
    return (1 if use_standard_llhr else 2) if CONST_SD_MODEL else 0


def compute_alt_model_read_stats_batch(reads, std_ref, alt_refs, use_standard_llhr=False,
                                       reg_data=None, engine=None):
    """compute_alt_model_read_stats (tombo_stats.py:3972-4083) for a list of reads: per read
    ({alt_name: llhrs}, {alt_name: positions}) or the TomboError.  Every motif hit of every read
    and model becomes one window of ONE `llh_ratio_windows` launch."""
    K = std_ref.kmer_width
    max_bb, max_ab = _alt_motif_bounds(alt_refs)
    out = [None] * len(reads)
    wins = []   # (read, alt name, means[K], ref_means[K], alt_means[K], vars)
    for i, rd in enumerate(reads):
        try:
            res = _prep_alt_model_read(rd, std_ref, alt_refs, use_standard_llhr, reg_data, max_bb, max_ab)
            out[i] = ({}, {})
            for name, poss, w in res:
                wins.extend((i, name) + x for x in w)
                out[i][1][name] = poss
                out[i][0][name] = np.empty(len(poss))
        except th.TomboError as e:
            out[i] = e
    if wins:
        kind = _llh_kind(use_standard_llhr)
        cols = [np.concatenate([w[k] for w in wins]) for k in range(2, 7)]
        vals = llh_ratio_windows(
            kind, *cols[:4], np.arange(len(wins), dtype=np.int64) * K, K,
            alt_vars=cols[4] if kind == 0 else None, scale_factor=OCLLHR_SCALE,
            density_height_factor=OCLLHR_HEIGHT, density_height_power=OCLLHR_POWER, engine=engine)
        fill = {}
        for (i, name, *_), v in zip(wins, vals):
            k = fill.get((i, name), 0)
            out[i][0][name][k] = v
            fill[(i, name)] = k + 1
    return out


def compute_alt_model_read_stats(r_data, std_ref, alt_refs, use_standard_llhr=False,
                                 reg_data=None):
    res = _only(compute_alt_model_read_stats_batch([r_data], std_ref, alt_refs, use_standard_llhr,
                                                   reg_data))
    return res[0], res[1], r_data.read_id


# ---------------------------------------------------------------------------------------------
# level_sample_compare and the control reference levels of model_sample_compare: a pileup of the
# levels of many reads at each genomic position (compute_group_reg_stats, tombo_stats.py:4236-4398;
# get_reads_ref, :3627-3673).  The reference loops over positions in numpy; here a list of regions
# is one engine call (`Engine.group_level_stats`, `Engine.reads_ref_levels`, kernels in
# csrc/k_group.h).  A region is a `th.regionData` (or anything with chrm / strand / start / end /
# reads [/ seq]).
KS_TEST_TXT = 'ks_test'
U_TEST_TXT = 'u_test'
T_TEST_TXT = 't_test'
KS_STAT_TEST_TXT = 'ks_stat_test'
U_STAT_TEST_TXT = 'u_stat_test'
T_STAT_TEST_TXT = 't_stat_test'
_GROUP_KINDS = {KS_TEST_TXT: (0, 1), U_TEST_TXT: (1, 1), T_TEST_TXT: (2, 1),
                KS_STAT_TEST_TXT: (0, 0), U_STAT_TEST_TXT: (1, 0), T_STAT_TEST_TXT: (2, 0)}
_STRAND_CODE = {'+': 0, '-': 1, None: 2}
_NO_READS_MSG = 'Must annotate region with reads (see `TomboInterval.add_reads`) to extract base levels.'

# CSR arrays of a list of regions and their reads; pos_off: the regions' extended positions
Pileup = namedtuple('Pileup', 'reg_start reg_end reg_strand reg_read_off read_start read_strand '
                              'read_ctrl read_off means pos_off')


def _check_regions(regions, ctrl_regions=None, paired=False):
    """region coordinates (paired: one control region with the same coordinates per region)"""
    if paired:
        if ctrl_regions is None or len(regions) != len(ctrl_regions):
            raise ValueError('one control region per sample region')
        for reg, ctrl in zip(regions, ctrl_regions):
            if (reg.start, reg.end) != (ctrl.start, ctrl.end):
                raise ValueError('sample and control regions must have the same coordinates')
    for reg in regions:
        if reg.end <= reg.start:
            raise ValueError('region end must be greater than its start')


def _pileup_inputs(regions, groups, fm_offset):
    """the Pileup of a list of regions: per region its reads (as many lists as `groups`, the group
    index of each list going to read_ctrl)"""
    reg_strand, reg_read_off = [], [0]
    read_start, read_strand, read_ctrl, means = [], [], [], []
    for reg_lists in zip(*groups):
        if reg_lists[0].strand not in _STRAND_CODE:
            raise ValueError('region strand must be "+", "-" or None')
        reg_strand.append(_STRAND_CODE[reg_lists[0].strand])
        for g, rg in enumerate(reg_lists):
            if rg.reads is None or len(rg.reads) == 0:
                raise th.TomboError(_NO_READS_MSG)
            for rd in rg.reads:
                if rd.means is None:
                    continue   # get_read_reg_events: a read without levels is left out
                m = np.asarray(rd.means, dtype=np.float64)
                if rd.strand not in ('+', '-'):
                    raise ValueError('read strand must be "+" or "-"')
                if rd.end is not None and rd.end - rd.start != m.shape[0]:
                    raise ValueError('read %r: end - start differs from its number of levels'
                                     % (rd.read_id,))
                read_start.append(int(rd.start))
                read_strand.append(_STRAND_CODE[rd.strand])
                read_ctrl.append(g)
                means.append(m)
        reg_read_off.append(len(read_start))
    i64, i8 = np.int64, np.int8
    reg_start = np.array([int(reg.start) for reg in regions], dtype=i64)
    reg_end = np.array([int(reg.end) for reg in regions], dtype=i64)
    return Pileup(reg_start, reg_end, np.array(reg_strand, dtype=i8), np.array(reg_read_off, dtype=i64),
                  np.array(read_start, dtype=i64), np.array(read_strand, dtype=i8),
                  np.array(read_ctrl, dtype=i8), _csr_offsets([m.shape[0] for m in means]),
                  _concat_f64(means), _csr_offsets(reg_end - reg_start + 2 * fm_offset))


def _check_group_args(fm_offset, min_test_reads):
    if int(fm_offset) != fm_offset or fm_offset < 0 or fm_offset > 64:
        raise ValueError('fm_offset must be an integer in [0, 64]')
    if int(min_test_reads) != min_test_reads or min_test_reads < 1:
        raise ValueError('min_test_reads must be a positive integer')


def compute_group_reg_stats_batch(regions, ctrl_regions, fm_offset, min_test_reads, stat_type,
                                  engine=None):
    """compute_group_reg_stats for a list of regions (sample) and their control regions (same
    coordinates), ONE engine call; per region what the reference returns: [] or
    [(stat_type, th.groupStats)].  U ranks equal sample and control levels sample first."""
    if stat_type not in _GROUP_KINDS:
        raise NotImplementedError('Unrecognized test type.')
    _check_group_args(fm_offset, min_test_reads)
    _check_regions(regions, ctrl_regions, paired=True)
    if len(regions) == 0:
        return []
    fm_offset, min_test_reads = int(fm_offset), int(min_test_reads)
    pileup = _pileup_inputs(regions, [regions, ctrl_regions], fm_offset)
    stats, poss, cov, ccov, counts = _engine(engine).group_level_stats(
        *_GROUP_KINDS[stat_type], fm_offset, min_test_reads, pileup, SMALLEST_PVAL)
    out = []
    for reg, a, n in zip(regions, pileup.pos_off.tolist(), counts.tolist()):
        b = a + n
        out.append([(stat_type, th.groupStats(
            stats[a:b].copy(), poss[a:b].copy(), reg.chrm, reg.strand, reg.start,
            cov[a:b].copy(), ccov[a:b].copy()))] if n else [])
    return out


def compute_group_reg_stats(reg_data, ctrl_reg_data, fm_offset, min_test_reads, stat_type):
    """tombo_stats.py:4336-4398 for one region (a batch of one)"""
    return compute_group_reg_stats_batch([reg_data], [ctrl_reg_data], fm_offset, min_test_reads,
                                         stat_type)[0]


def _prior_levels(regions, fm_offset, std_ref):
    """the model's levels over every region's extended positions (compute_posterior_samp_dists)"""
    K, cp = std_ref.kmer_width, std_ref.central_pos
    dn = K - cp - 1
    pm, ps = [], []
    for reg in regions:
        if reg.seq is None:
            raise ValueError('the prior blend needs the region sequence (regionData.seq)')
        want = reg.end - reg.start + 2 * fm_offset + 2 * (K - 1)
        if len(reg.seq) != want:
            raise ValueError('region sequence must span [start - fm_offset - K + 1, '
                             'end + fm_offset + K - 1) (%d bases, got %d)' % (want, len(reg.seq)))
        b_lag, e_lag = (cp, dn) if reg.strand == '+' else (dn, cp)
        seq = reg.seq[K - 1 - b_lag:len(reg.seq) - (K - 1 - e_lag)]
        if reg.strand == '-':
            seq = th.rev_comp(seq)
        m, s = std_ref.get_exp_levels_from_seq_with_gaps(seq, reg.strand == '-')
        pm.append(m)
        ps.append(s)
    return _concat_f64(pm), _concat_f64(ps)


def get_reads_ref_batch(regions, min_test_reads, fm_offset, std_ref=None, prior_weights=None,
                        est_mean=False, engine=None):
    """get_reads_ref for a list of regions in ONE engine call: per region
    (level_means, level_sds, cov_dict) over [start - fm_offset, end + fm_offset).  With std_ref
    the levels are blended with the model's (compute_posterior_samp_dists); each region then needs
    `seq`, the '+' strand genome over [start - fm_offset - K + 1, end + fm_offset + K - 1)."""
    _check_group_args(fm_offset, min_test_reads)
    _check_regions(regions)
    if len(regions) == 0:
        return []
    fm_offset, min_test_reads = int(fm_offset), int(min_test_reads)
    pileup = _pileup_inputs(regions, [regions], fm_offset)
    prior_m, prior_s, w_m, w_s = None, None, 0.0, 0.0
    if std_ref is not None:
        if prior_weights is None:
            prior_weights = (MEAN_PRIOR_CONST, SD_PRIOR_CONST)
        w_m, w_s = float(prior_weights[0]), float(prior_weights[1])
        prior_m, prior_s = _prior_levels(regions, fm_offset, std_ref)
    lm, ls, cov = _engine(engine).reads_ref_levels(est_mean, fm_offset, min_test_reads, pileup, prior_m,
                                                   prior_s, w_m, w_s)
    out = []
    for reg, a, b in zip(regions, pileup.pos_off[:-1].tolist(), pileup.pos_off[1:].tolist()):
        if not (cov[a:b] >= min_test_reads).any():   # no covered position: no blend, no dict
            out.append((np.full(b - a, np.nan), np.full(b - a, np.nan), {}))
            continue
        out.append((lm[a:b].copy(), ls[a:b].copy(),
                    dict(zip(range(reg.start - fm_offset, reg.end + fm_offset), cov[a:b].tolist()))))
    return out


def get_reads_ref(reg_data, min_test_reads, fm_offset, std_ref=None, prior_weights=None,
                  est_mean=False):
    """tombo_stats.py:3627-3673 for one region: (level_means, level_sds, cov_dict); the first two
    feed compute_sample_compare_read_stats(_batch) as ctrl_means / ctrl_sds"""
    return get_reads_ref_batch([reg_data], min_test_reads, fm_offset, std_ref, prior_weights,
                               est_mean)[0]


# ---------------------------------------------------------------------------------------------
# Per-site modified fractions of the model-based tests: compute_reg_stats (tombo_stats.py:4180-4229)
# with collate_reg_stats (:4124-4178), apply_per_read_thresh (:4084-4122) and calc_damp_fraction
# (:2537-2552).  The reference concatenates, argsorts, splits and thresholds the per-read
# statistics of one region in numpy; here a list of regions is one engine call
# (`Engine.site_fractions_z` / `Engine.site_fractions_windows`, kernels in csrc/k_site.h): the
# per-read statistics are computed on the device and only the per-site records come back.  A
# track is one (region, statistic name).
def _damp_pair(cov_damp_counts):
    if cov_damp_counts is None:
        return None
    cd = cov_damp_counts
    unmod, mod = (cd['unmod'], cd['mod']) if isinstance(cd, dict) else cd
    return float(unmod), float(mod)


def _check_reg_stats_args(regions, fm_offset, min_test_reads, ctrl_regions, std_ref, alt_refs,
                          stat_type):
    if stat_type not in (SAMP_COMP_TXT, DE_NOVO_TXT, ALT_MODEL_TXT):
        raise NotImplementedError('Unrecognized test type.')
    _check_group_args(fm_offset, min_test_reads)
    _check_regions(regions, ctrl_regions, paired=stat_type == SAMP_COMP_TXT)
    if stat_type != SAMP_COMP_TXT and std_ref is None:
        raise ValueError('%s needs the canonical model (std_ref)' % stat_type)
    if stat_type == ALT_MODEL_TXT and not alt_refs:
        raise ValueError('%s needs alternate models (alt_refs)' % stat_type)


def _read_id_str(rid):
    return rid.decode() if isinstance(rid, bytes) else rid


def _widen_tracks(trk_start, trk_end, trk, first, end):
    if trk.shape[0]:   # (widened to the statistics that reach further out than their region)
        np.minimum.at(trk_start, trk, first)
        np.maximum.at(trk_end, trk, end)


class _ZInputs(namedtuple('_ZInputs', 'means ref_means ref_sds off read_track read_pos read_ids n_ok '
                                      'fm_offset floor_out trk_start trk_end')):
    """flat inputs of the z form, one track per region: the arrays `read_pvals` takes plus per read its
    track, first position and id; n_ok: per region the number of reads that did not fail"""

    def site_fractions(self, eng, *thresholds):
        return eng.site_fractions_z(self.trk_start, self.trk_end, self.means, self.ref_means, self.ref_sds,
                                    self.off, self.read_track, self.read_pos, self.fm_offset, self.floor_out,
                                    SMALLEST_PVAL, *thresholds)

    def __getitem__(self, key):   # (fields by name too, as in the dict this bundle replaced)
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    def stat_index(self):
        """per statistic: its track, its position, the index of its read in the ids; the ids"""
        lens = np.diff(self.off)
        return (np.repeat(self.read_track, lens),
                np.repeat(self.read_pos - self.off[:-1], lens) + np.arange(self.off[-1]),
                np.repeat(np.arange(lens.shape[0]), lens), self.read_ids)


class _WinInputs(namedtuple('_WinInputs', 'kind means ref_means alt_means ref_vars alt_vars width starts '
                                          'win_track win_pos win_ids n_ok trk_start trk_end')):
    """flat inputs of the window form (alternate models): the arrays `llh_ratio_windows` takes plus
    per window its track (region * number of models + model), position and read id"""

    def site_fractions(self, eng, *thresholds):
        return eng.site_fractions_windows(
            self.trk_start, self.trk_end, self.kind, self.means, self.ref_means, self.alt_means, self.ref_vars,
            self.alt_vars, self.starts, self.width, self.win_track, self.win_pos,
            (OCLLHR_SCALE, OCLLHR_HEIGHT, OCLLHR_POWER), *thresholds)

    def stat_index(self):
        return self.win_track, self.win_pos, np.arange(self.win_pos.shape[0]), self.win_ids


def _reg_stats_z_inputs(regions, fm_offset, std_ref, stat_type, ctrl_levels=None):
    """the _ZInputs of a list of regions.  ctrl_levels[r]: (ctrl_means, ctrl_sds) or None (region
    already failed)."""
    cols, r_trk, r_pos, r_ids = ([], [], []), [], [], []
    n_ok = [0] * len(regions)
    for t, reg in enumerate(regions):
        if ctrl_levels is not None and ctrl_levels[t] is None:
            continue
        for rd in (reg.reads or ()):
            try:
                if stat_type == DE_NOVO_TXT:
                    prep = _prep_de_novo_read(rd, std_ref, fm_offset, reg)
                else:
                    prep = _prep_sample_compare_read(rd, *ctrl_levels[t], fm_offset, reg)
            except th.TomboError:
                continue   # compute_reg_stats :4210-4211
            for c, x in zip(cols, prep):
                c.append(x)
            r_trk.append(t); r_pos.append(prep[3]); r_ids.append(rd.read_id)
            n_ok[t] += 1
    off = _csr_offsets([m.shape[0] for m in cols[0]])
    r_trk, r_pos = np.array(r_trk, dtype=np.int64), np.array(r_pos, dtype=np.int64)
    # a track spans the region extended by fm_offset
    trk_start = np.array([reg.start - fm_offset for reg in regions], dtype=np.int64)
    trk_end = np.array([reg.end + fm_offset for reg in regions], dtype=np.int64)
    _widen_tracks(trk_start, trk_end, r_trk, r_pos, r_pos + np.diff(off))
    return _ZInputs(*(_concat_f64(c) for c in cols), off, r_trk, r_pos, r_ids, n_ok, int(fm_offset),
                    stat_type == DE_NOVO_TXT, trk_start, trk_end)


def _reg_stats_win_inputs(regions, std_ref, alt_refs, use_standard_llhr):
    """the _WinInputs of a list of regions"""
    K, n_alt = std_ref.kmer_width, len(alt_refs)
    max_bb, max_ab = _alt_motif_bounds(alt_refs)
    cols = [[] for _ in range(5)]
    w_trk, w_pos, w_ids = [], [], []
    n_ok = [0] * len(regions)
    for r, reg in enumerate(regions):
        for rd in (reg.reads or ()):
            try:
                res = _prep_alt_model_read(rd, std_ref, alt_refs, use_standard_llhr, reg, max_bb, max_ab)
            except th.TomboError:
                continue
            n_ok[r] += 1
            for k, (_, poss, wins) in enumerate(res):
                for p, w in zip(poss, wins):
                    for c, x in zip(cols, w):
                        c.append(x)
                    w_trk.append(r * n_alt + k); w_pos.append(int(p)); w_ids.append(rd.read_id)
    w_trk, w_pos = np.array(w_trk, dtype=np.int64), np.array(w_pos, dtype=np.int64)
    trk_start = np.repeat(np.array([reg.start for reg in regions], dtype=np.int64), n_alt)
    trk_end = np.repeat(np.array([reg.end for reg in regions], dtype=np.int64), n_alt)
    _widen_tracks(trk_start, trk_end, w_trk, w_pos, w_pos + 1)
    kind = _llh_kind(use_standard_llhr)
    return _WinInputs(kind, *(_concat_f64(c) for c in cols[:4]), _concat_f64(cols[4]) if kind == 0 else None,
                      K, np.arange(w_trk.shape[0], dtype=np.int64) * K, w_trk, w_pos, w_ids, n_ok,
                      trk_start, trk_end)


def _ctrl_levels(ctrl_regions, min_test_reads, fm_offset, std_ref, prior_weights, engine):
    """sample_compare: per region the control levels (means, sds) and coverage dict of one
    `get_reads_ref_batch` call, or the TomboError of a control region without reads"""
    levels, ctrl_cov = [None] * len(ctrl_regions), [None] * len(ctrl_regions)
    failed = [th.TomboError(_NO_READS_MSG) if ctrl.reads is None or len(ctrl.reads) == 0 else None
              for ctrl in ctrl_regions]   # get_base_levels of get_reads_ref
    have = [r for r, e in enumerate(failed) if e is None]
    if have:
        refs = get_reads_ref_batch([ctrl_regions[r] for r in have], min_test_reads, fm_offset,
                                   std_ref, prior_weights, engine=engine)
        for r, (lm, ls, cov) in zip(have, refs):
            levels[r], ctrl_cov[r] = (lm, ls), cov
    return levels, ctrl_cov, failed


def _reported_tracks(n_stats, r, n_names):
    """the tracks of region r up to and including its first one without statistics: there the
    reference's loop over the names ends, after that name's per-read block went out"""
    trks = list(range(r * n_names, (r + 1) * n_names))
    empty = [t for t in trks if n_stats[t] == 0]
    return trks[:trks.index(empty[0]) + 1] if empty else trks


def _per_read_blocks(inp, res, regions, names, failed):
    """per region the (name, (block, read_id_lookup, chrm, strand, start)) items of its reported
    tracks; a block is the per-read block of collate_reg_stats (:4136-4154): (pos, stat, read_id)
    records, the ids numbered in order of first appearance (the reference numbers them by iterating
    a set, so only the lookup back to the strings is defined)"""
    s_trk, s_pos, s_rd, ids = inp.stat_index()
    ok = ~np.isnan(res.per_read)
    out = [[] for _ in regions]
    for r, reg in enumerate(regions):
        for t in ([] if failed[r] is not None else _reported_tracks(res.n_stats, r, len(names))):
            sel = np.flatnonzero(ok & (s_trk == t))
            lookup = {}
            block = np.empty(sel.shape[0], dtype=[('pos', 'u4'), ('stat', 'f8'), ('read_id', 'u4')])
            block['pos'], block['stat'] = s_pos[sel], res.per_read[sel]
            block['read_id'] = [lookup.setdefault(_read_id_str(ids[q]), len(lookup)) for q in s_rd[sel]]
            out[r].append((names[t % len(names)], (block, lookup, reg.chrm, reg.strand, reg.start)))
    return out


def _region_stats(reg, r, names, res, ctrl_cov):
    """[(name, th.regionStats), ...] of region r from the flat outputs, or its TomboError.
    ctrl_cov: the control coverage dict (sample_compare) or None"""
    out = []
    for t in _reported_tracks(res.n_stats, r, len(names)):
        if res.n_stats[t] == 0:
            # (for model_compare the reference's list comprehension fails the whole region)
            return th.TomboError('No valid positions in this region.')
        a = int(res.pos_off[t])
        b = a + int(res.counts[t])
        poss, cov = res.poss[a:b].copy(), res.cov[a:b].copy()
        if ctrl_cov is None:
            cc_list = [0] * int(cov.sum())
        else:
            # one entry per statistic in sorted-position order (apply_per_read_thresh iterates
            # stat_locs, not the unique positions)
            cc_list = np.repeat(np.array([ctrl_cov.get(int(p), 0) for p in poss], dtype=np.int64), cov).tolist()
        rs = th.regionStats(res.frac[a:b].copy(), poss, reg.chrm, reg.strand, reg.start, cov, cc_list,
                            res.valid[a:b].copy())
        if res.damp is not None:
            rs.damp_frac = res.damp[a:b].copy()
        out.append((names[t % len(names)], rs))
    return out


def compute_reg_stats_batch(regions, fm_offset, min_test_reads, single_read_thresh, lower_thresh,
                            ctrl_regions, std_ref, alt_refs, use_standard_llhr, stat_type,
                            prior_weights, cov_damp_counts=None, return_per_read=False, engine=None):
    """compute_reg_stats for a list of regions in ONE `tba_site_fractions` call (sample_compare:
    after one `get_reads_ref_batch` call for the control levels).  Per region either the list
    [(stat_name, th.regionStats), ...] the reference returns or the th.TomboError it raises.
    With cov_damp_counts ((unmod, mod) or the reference's dict) the dampened fractions are computed on
    the device too: attribute `damp_frac` of each regionStats (same values as `calc_damp_fraction`).  return_per_read: returns
    (results, per_read) where per_read[r] lists (stat_name, (block, read_id_lookup, chrm, strand,
    start)) as the reference puts them on its per_read_q."""
    _check_reg_stats_args(regions, fm_offset, min_test_reads, ctrl_regions, std_ref, alt_refs,
                          stat_type)
    fm_offset, min_test_reads = int(fm_offset), int(min_test_reads)
    failed = ctrl_cov = [None] * len(regions)
    names = [stat_type]
    if stat_type == SAMP_COMP_TXT:
        levels, ctrl_cov, failed = _ctrl_levels(ctrl_regions, min_test_reads, fm_offset, std_ref,
                                                prior_weights, engine)
        inp = _reg_stats_z_inputs(regions, fm_offset, None, stat_type, levels)
    elif stat_type == DE_NOVO_TXT:
        inp = _reg_stats_z_inputs(regions, fm_offset, std_ref, stat_type)
    else:
        inp = _reg_stats_win_inputs(regions, std_ref, alt_refs, use_standard_llhr)
        names = [n for n, _ in alt_refs]
    failed = [e if e is not None or n else th.TomboError('Reads contains no statistics in this region.')
              for e, n in zip(failed, inp.n_ok)]
    out, per_read = failed, [[] for _ in regions]
    if any(inp.n_ok):   # (else nothing to compute: no engine call)
        res = inp.site_fractions(_engine(engine), single_read_thresh, lower_thresh, _damp_pair(cov_damp_counts),
                                 return_per_read)
        out = [e if e is not None else _region_stats(reg, r, names, res, ctrl_cov[r] if stat_type == SAMP_COMP_TXT else None)
               for r, (reg, e) in enumerate(zip(regions, failed))]
        if return_per_read:
            per_read = _per_read_blocks(inp, res, regions, names, failed)
    return (out, per_read) if return_per_read else out


def compute_reg_stats(reg_data, fm_offset, min_test_reads, single_read_thresh, lower_thresh,
                      ctrl_reg_data, std_ref, alt_refs, use_standard_llhr, per_read_q, stat_type,
                      prior_weights):
    """tombo_stats.py:4180-4229 for one region (a batch of one): raises the region's TomboError;
    a per_read_q that is not None receives the per-read blocks through `.put`"""
    res = compute_reg_stats_batch(
        [reg_data], fm_offset, min_test_reads, single_read_thresh, lower_thresh,
        None if ctrl_reg_data is None else [ctrl_reg_data], std_ref, alt_refs, use_standard_llhr,
        stat_type, prior_weights, return_per_read=per_read_q is not None)
    if per_read_q is not None:
        res, per_read = res
        for item in per_read[0]:
            per_read_q.put(item)
    return _only(res)


# The same results with the per-read preparation on the device (`Engine.site_fractions_reads`, kernels
# k_site_pair_plan / k_site_gather of csrc/k_site.h).  `_reg_stats_z_inputs` slices, flips and looks up every
# (region, read) pair in Python and uploads 24 bytes per statistic; here every read goes up once (8 bytes per
# level, 1 per base) with the (region, read) pairs, and clip, flip and expected levels are index arithmetic
# in the kernels.  The statistics then run through the kernels of the route above, so the results are its
# bits.
class _ReadsInputs(object):
    """the inputs of one `Engine.site_fractions_reads` call, one track per region: what `_ZInputs` offers to
    `_region_stats` and `_per_read_blocks`, built from the pair arrays the call returns"""

    def __init__(self, form, table, read_ids):
        self.form, self.table, self.read_ids = form, table, read_ids
        self.pair_reg = np.repeat(np.arange(table[0].shape[0], dtype=np.int64), np.diff(table[7]))
        self.pair_ok = self.pair_pos = self.pair_off = None

    def site_fractions(self, eng, *thresholds):
        res, self.pair_ok, self.pair_pos, self.pair_off = eng.site_fractions_reads(
            self.form, *self.table, SMALLEST_PVAL, *thresholds)
        return res

    @property
    def n_ok(self):
        """per region the number of pairs that did not fail"""
        return np.bincount(self.pair_reg, weights=self.pair_ok, minlength=self.table[0].shape[0]).astype(np.int64)

    def stat_index(self):
        lens = np.diff(self.pair_off)
        return (np.repeat(self.pair_reg, lens),
                np.repeat(self.pair_pos - self.pair_off[:-1], lens) + np.arange(self.pair_off[-1]),
                np.repeat(self.table[8], lens), self.read_ids)


def _reads_table(regions, need_seq, skip):
    """the unique reads (by identity) of the regions that have levels (need_seq: and a sequence), and the
    regions' pairs in `reg.reads` order; skip[r]: region r gets no pairs.  The loops collect references and
    lengths only -> (reads, reg_pair_off, pair_read)"""
    index, reads, pair_read, counts = {}, [], [], []
    for reg, no in zip(regions, skip):
        n0 = len(pair_read)
        for rd in (() if no else (reg.reads or ())):
            if rd.means is None or (need_seq and rd.seq is None):
                continue   # (the TomboError of the per-read functions: left out of the region)
            q = index.get(id(rd))
            if q is None:
                q = index[id(rd)] = len(reads)
                reads.append(rd)
            pair_read.append(q)
        counts.append(len(pair_read) - n0)
    return reads, _csr_offsets(counts), np.array(pair_read, dtype=np.int64)


def _reg_stats_reads_inputs(regions, fm_offset, stat_type, ctrl_levels=None):
    """the _ReadsInputs of a list of regions.  ctrl_levels[r]: (ctrl_means, ctrl_sds) over the extended
    region or None (region already failed)."""
    de_novo = stat_type == DE_NOVO_TXT
    skip = [ctrl_levels is not None and ctrl_levels[r] is None for r in range(len(regions))]
    reads, pair_off, pair_read = _reads_table(regions, de_novo, skip)
    means = [np.asarray(rd.means, dtype=np.float64) for rd in reads]
    lens = np.array([m.shape[0] for m in means], dtype=np.int64)
    start = np.array([rd.start for rd in reads], dtype=np.int64)
    if any(rd.strand not in ('+', '-') for rd in reads):
        raise ValueError('read strand must be "+" or "-"')
    bad = lens != np.array([rd.end for rd in reads], dtype=np.int64) - start
    seq = None
    if de_novo:
        bad |= lens != np.array([len(rd.seq) for rd in reads], dtype=np.int64)
        seq = encode_seq(b''.join(rd.seq.encode() if isinstance(rd.seq, str) else bytes(rd.seq) for rd in reads))
    if bad.any():
        raise ValueError('read %r: end - start, its number of levels and its sequence length disagree'
                         % (reads[int(np.flatnonzero(bad)[0])].read_id,))
    reg_start = np.array([reg.start for reg in regions], dtype=np.int64)
    reg_end = np.array([reg.end for reg in regions], dtype=np.int64)
    pos_means = pos_sds = None
    if not de_novo:   # the control levels once per region (NaN under a region that failed)
        ext = reg_end - reg_start + 2 * fm_offset
        cols = [[np.full(n, np.nan) if lv is None else np.asarray(lv[k], dtype=np.float64)
                 for lv, n in zip(ctrl_levels, ext.tolist())] for k in range(2)]
        if any(c.shape[0] != n for c, n in zip(cols[0] + cols[1], ext.tolist() * 2)):
            raise ValueError('control levels do not cover the extended region')
        pos_means, pos_sds = _concat_f64(cols[0]), _concat_f64(cols[1])
    table = (reg_start, reg_end, start, np.array([rd.strand == '-' for rd in reads], dtype=np.int8),
             _csr_offsets(lens), _concat_f64(means), seq, pair_off, pair_read, pos_means, pos_sds, int(fm_offset))
    return _ReadsInputs(0 if de_novo else 1, table, [rd.read_id for rd in reads])


def compute_reg_stats_reads_batch(regions, fm_offset, min_test_reads, single_read_thresh, lower_thresh,
                                  ctrl_regions, std_ref, alt_refs, use_standard_llhr, stat_type,
                                  prior_weights, cov_damp_counts=None, return_per_read=False, engine=None):
    """`compute_reg_stats_batch` (same arguments, same return value) with the per-read preparation of de_novo
    and sample_compare on the device: ONE `tba_site_fractions_reads` call on a reads table that holds every
    read of the regions once, however many regions it spans.  The reads of a region must overlap it (as
    `intervalData.add_reads` selects them); end - start, the levels and the sequence of a read must agree in
    length (ValueError).  model_compare goes through `compute_reg_stats_batch`."""
    if stat_type == ALT_MODEL_TXT:
        return compute_reg_stats_batch(regions, fm_offset, min_test_reads, single_read_thresh, lower_thresh,
                                       ctrl_regions, std_ref, alt_refs, use_standard_llhr, stat_type,
                                       prior_weights, cov_damp_counts, return_per_read, engine)
    _check_reg_stats_args(regions, fm_offset, min_test_reads, ctrl_regions, std_ref, alt_refs, stat_type)
    fm_offset, min_test_reads = int(fm_offset), int(min_test_reads)
    failed = ctrl_cov = [None] * len(regions)
    names, eng = [stat_type], _engine(engine)
    if stat_type == SAMP_COMP_TXT:
        levels, ctrl_cov, failed = _ctrl_levels(ctrl_regions, min_test_reads, fm_offset, std_ref,
                                                prior_weights, engine)
        inp = _reg_stats_reads_inputs(regions, fm_offset, stat_type, levels)
    else:
        eng.ensure_model(std_ref)
        inp = _reg_stats_reads_inputs(regions, fm_offset, stat_type)
    no_stats = th.TomboError('Reads contains no statistics in this region.')
    if inp.pair_reg.shape[0] == 0:   # (nothing to compute: no engine call)
        out = [e if e is not None else no_stats for e in failed]
        return (out, [[] for _ in regions]) if return_per_read else out
    res = inp.site_fractions(eng, single_read_thresh, lower_thresh, _damp_pair(cov_damp_counts), return_per_read)
    failed = [e if e is not None or n else no_stats for e, n in zip(failed, inp.n_ok.tolist())]
    out = [e if e is not None else _region_stats(reg, r, names, res, ctrl_cov[r] if stat_type == SAMP_COMP_TXT else None)
           for r, (reg, e) in enumerate(zip(regions, failed))]
    if return_per_read:
        return out, _per_read_blocks(inp, res, regions, names, failed)
    return out


def calc_damp_fraction(cov_damp_counts, fracs, valid_cov):
    """tombo_stats.py:2537-2552: (round(frac * valid) + unmod) / (valid + unmod + mod), np.round
    being round-half-even"""
    cd = cov_damp_counts
    unmod, total = (cd['unmod'], sum(list(cd.values()))) if isinstance(cd, dict) else (cd[0], cd[0] + cd[1])
    fracs, valid_cov = np.asarray(fracs), np.asarray(valid_cov)
    return (np.round(fracs * valid_cov) + unmod) / (valid_cov + total)


def region_stats_block(reg_stats, cov_damp_counts, damp_frac=None):
    """the record array ModelStats._write_stat_block builds from a regionStats (:2752-2764): rows
    with a NaN dampened fraction dropped; control_cov is reg_stats.ctrl_cov zipped against the
    per-site arrays, i.e. truncated to their length.  damp_frac: the dampened fractions where the
    device has computed them already, else calc_damp_fraction"""
    with np.errstate(invalid='ignore'):
        damp = calc_damp_fraction(cov_damp_counts, reg_stats.reg_frac_standard_base, reg_stats.valid_cov) \
            if damp_frac is None else np.asarray(damp_frac)
    n = min(damp.shape[0], len(reg_stats.ctrl_cov))
    keep = np.flatnonzero(~np.isnan(damp[:n]))
    block = np.empty(keep.shape[0], dtype=[('damp_frac', 'f8'), ('frac', 'f8'), ('pos', 'u4'),
                                           ('cov', 'u4'), ('control_cov', 'u4'), ('valid_cov', 'u4')])
    block['damp_frac'] = damp[keep]
    block['frac'] = np.asarray(reg_stats.reg_frac_standard_base)[keep]
    block['pos'] = np.asarray(reg_stats.reg_poss)[keep]
    block['cov'] = np.asarray(reg_stats.reg_cov)[keep]
    block['control_cov'] = np.asarray(reg_stats.ctrl_cov[:n], dtype=np.int64)[keep]
    block['valid_cov'] = np.asarray(reg_stats.valid_cov)[keep]
    return block


# ---------------------------------------------------------------------------------------------
# Statistics files: ModelStats (:2554-3061), LevelStats (:3063-3224), TomboStats (:3226-3237),
# PerReadStats (:3239-3565) and aggregate_per_read_stats (:4664-4777).  The constructor
# signatures, attribute names, HDF5 layout and error strings are the reference's.  The first
# argument is a file name (opened with h5py, which must then be installed) or any object with the
# h5py group interface (`attrs`, `create_group`, `create_dataset`, `items`, `__getitem__`,
# `close`, `flush`), as `tombo_helper.write_new_fast5_group` takes one.  Differences, all stated
# in DESIGN.md section 3g: the most significant sites are sorted once at `close` (same array,
# see `_close_write`); `get_reg_stats` concatenates overlapping blocks; where the reference
# prints a message and exits the process a th.TomboError with that message is raised, where it
# prints a warning `warnings.warn` is called.
STAT_BLOCKS_H5_NAME = 'Statistic_Blocks'
MOST_SIGNIF_H5_NAME = 'Most_Significant_Stats'
COV_DAMP_COUNTS_H5_NAME = 'Cov_Damp_Counts'
COV_THRESH_H5_NAME = 'Cov_Threshold'
MOST_SIGNIF_NUM_BATCHES_DEFAULT = 10
PER_READ_STATS = (SAMP_COMP_TXT, DE_NOVO_TXT, ALT_MODEL_TXT)
LEVEL_STATS_TXTS = (KS_TEST_TXT, U_TEST_TXT, T_TEST_TXT, KS_STAT_TEST_TXT, U_STAT_TEST_TXT, T_STAT_TEST_TXT)
_MODEL_BLOCK_DTYPE = [('damp_frac', 'f8'), ('frac', 'f8'), ('pos', 'u4'), ('cov', 'u4'), ('control_cov', 'u4'),
                      ('valid_cov', 'u4')]
_LEVEL_BLOCK_DTYPE = [('stat', 'f8'), ('pos', 'u4'), ('cov', 'u4'), ('control_cov', 'u4')]
_SITE_ID_DTYPE = [('chrm', 'u4'), ('strand', 'S1')]
_INVALID_STATS_MSG = ('Invalid statistics file provided. Try running tombo/scripts/convert_stats.py if this '
                      'stats file was created before Tombo v1.3.1')
_NO_SITES_MSG = 'No genomic positions contain --minimum-test-reads.'


def _open_store(store, mode):
    """a file name -> h5py.File (ImportError without h5py); anything else is used as the group it is"""
    if isinstance(store, (str, bytes, os.PathLike)):
        import h5py
        return h5py.File(store, mode)
    return store


def _text(v):
    return v.decode() if isinstance(v, bytes) else v


def _blocks_index(blocks):
    """{(chrm, strand): {start: block name}} in stored order, number of blocks"""
    index, n = {}, 0
    for name, block in blocks.items():
        cs = (_text(block.attrs.get('chrm')), _text(block.attrs.get('strand')))
        index.setdefault(cs, {})[block.attrs.get('start')] = name
        n += 1
    return index, n


def _neg_log10(self, pos_stat):
    with np.errstate(divide='ignore'):
        return -np.log10(pos_stat[self._stat_slot])


class _BlockStore(object):
    """what the three containers share: the block iterator and get_reg_stats"""
    _sort_keys = False

    def _new_block(self, chrm, strand, start):
        block = self._blocks.create_group('Block_' + str(self.curr_block_num))
        self.curr_block_num += 1
        block.attrs['chrm'], block.attrs['strand'], block.attrs['start'] = chrm, strand, start
        return block

    def __iter__(self):
        """(chrm, strand, start, end, block_stats) of every block: the blocks of the first (chrm, strand) in
        stored order, those of the later ones sorted by start (:2984-3014, :3505-3530)"""
        self.iter_all_cs = iter(sorted(self.blocks_index) if self._sort_keys else list(self.blocks_index))
        try:
            self.iter_curr_cs = next(self.iter_all_cs)
        except StopIteration:   # (a file without blocks: nothing to iterate, for PerReadStats too)
            self.iter_curr_cs, self.iter_curr_cs_blocks = None, iter([])
        else:
            self.iter_curr_cs_blocks = iter(self.blocks_index[self.iter_curr_cs].items())
        return self

    def __next__(self):
        try:
            next_start, next_block_name = next(self.iter_curr_cs_blocks)
        except StopIteration:
            self.iter_curr_cs = next(self.iter_all_cs)   # (the second StopIteration ends the iteration)
            self.iter_curr_cs_blocks = iter(sorted(self.blocks_index[self.iter_curr_cs].items()))
            next_start, next_block_name = next(self.iter_curr_cs_blocks)
        chrm, strand = self.iter_curr_cs
        return (chrm, strand, next_start, next_start + self.region_size,
                self._blocks[next_block_name]['block_stats'][:])

    next = __next__

    def get_reg_stats(self, chrm, strand, start, end):
        """the records with start <= pos < end, blocks in order of their start; None without an overlapping
        block.  Several overlapping blocks are concatenated (the reference's np.vstack needs them to be of one
        length)."""
        if (chrm, strand) not in self.blocks_index:
            return
        reg_stats = []
        for reg_start, block_name in sorted(self.blocks_index[(chrm, strand)].items()):
            if reg_start < end and reg_start + self.region_size > start:
                block = self._blocks[block_name]['block_stats'][:]
                reg_stats.append(block[(block['pos'] >= start) & (block['pos'] < end)])
        if len(reg_stats) == 0:
            return
        return reg_stats[0] if len(reg_stats) == 1 else np.concatenate(reg_stats)

    # the (statistic, has_mod) pairs behind `tombo plot roc` (:2406-2535): see the module functions of these names
    def compute_motif_stats(self, motif_descs, genome_index, stats_per_block=None, total_stats_limit=None,
                            engine=None):
        return compute_motif_stats(self, motif_descs, genome_index, stats_per_block, total_stats_limit, engine)

    def compute_ground_truth_stats(self, ground_truth_locs, engine=None):
        return compute_ground_truth_stats(self, ground_truth_locs, engine)

    def compute_ctrl_motif_stats(self, ctrl_stats, motif_descs, genome_index, stats_per_block=None,
                                 total_stats_limit=None, engine=None):
        return compute_ctrl_motif_stats(self, ctrl_stats, motif_descs, genome_index, stats_per_block,
                                        total_stats_limit, engine)


class ModelStats(_BlockStore):
    """A standard (per genomic base) statistics file of the model-based tests: all of stat_type, region_size,
    cov_damp_counts, cov_thresh and num_most_signif given opens a fresh file for writing, else `stats_fn` is
    parsed."""
    _sort_keys = True
    _block_dtype = _MODEL_BLOCK_DTYPE
    _blocks = property(lambda self: self.stat_blocks)

    def _parse_stats(self):
        self.stat_type = _text(self._fp.attrs.get('stat_type'))
        self.region_size = self._fp.attrs.get('block_size')
        self.stat_blocks = self._fp[STAT_BLOCKS_H5_NAME]
        self.blocks_index, self.num_blocks = _blocks_index(self.stat_blocks)
        self.cov_thresh = self._fp.attrs.get(COV_THRESH_H5_NAME)
        most_signif_grp = self._fp[MOST_SIGNIF_H5_NAME]
        self.most_signif_stats = most_signif_grp[MOST_SIGNIF_H5_NAME][:]
        self.most_signif_chrm_map = dict((v, k) for k, v in most_signif_grp['chrm_ids'].attrs.items())
        try:   # (LevelStats has no damp counts)
            self.cov_damp_counts = dict(self._fp[COV_DAMP_COUNTS_H5_NAME].attrs.items())
        except Exception:
            self.cov_damp_counts = None

    def _create_new_stats_file(self):
        self._fp = _open_store(self.stats_fn, 'w')
        self._fp.attrs['stat_type'] = self.stat_type
        self._fp.attrs['block_size'] = self.region_size
        self.stat_blocks = self._fp.create_group(STAT_BLOCKS_H5_NAME)
        self._fp.attrs[COV_THRESH_H5_NAME] = self.cov_thresh
        if self.cov_damp_counts is not None:
            self.cov_damp_counts_grp = self._fp.create_group(COV_DAMP_COUNTS_H5_NAME)
            self.cov_damp_counts_grp.attrs['unmod'] = self.cov_damp_counts['unmod']
            self.cov_damp_counts_grp.attrs['mod'] = self.cov_damp_counts['mod']
        self.most_signif_sites = self._fp.create_group(MOST_SIGNIF_H5_NAME)
        self.queued_stat_batches = []
        self.curr_chrm_id = 0
        self.chrm_names = {}
        self.chrm_id_grp = self.most_signif_sites.create_group('chrm_ids')
        self.is_empty = True

    def _open(self, stats_fn, write_args, stat_type, region_size, cov_thresh, num_most_signif,
              most_signif_num_batches):
        self.stats_fn = stats_fn
        self.open_for_writing = not any(arg is None for arg in write_args)
        if self.open_for_writing:
            self.stat_type, self.region_size, self.curr_block_num = stat_type, region_size, 0
            self.cov_thresh, self.num_most_signif = cov_thresh, num_most_signif
            self.most_signif_num_batches = most_signif_num_batches
            self._create_new_stats_file()
        else:
            if isinstance(stats_fn, (str, bytes, os.PathLike)) and not os.path.isfile(stats_fn):
                raise th.TomboError('Statistics file not provided or provided file does not exist.')
            self._fp = _open_store(stats_fn, 'r')
            try:
                self._parse_stats()
            except Exception:
                raise th.TomboError(_INVALID_STATS_MSG)

    def __init__(self, stats_fn, stat_type=None, region_size=None, cov_damp_counts=None, cov_thresh=None,
                 num_most_signif=None, most_signif_num_batches=MOST_SIGNIF_NUM_BATCHES_DEFAULT):
        if cov_damp_counts is not None:
            self.cov_damp_counts = dict(zip(('unmod', 'mod'), cov_damp_counts))
        self._open(stats_fn, (stat_type, region_size, cov_damp_counts, cov_thresh, num_most_signif), stat_type,
                   region_size, cov_thresh, num_most_signif, most_signif_num_batches)
        if self.stat_type not in PER_READ_STATS:
            if self.stat_type in LEVEL_STATS_TXTS:
                raise th.TomboError('This appears to be a group-comparison stats file. Open with '
                                    'tombo_stats.LevelStats.')
            raise th.TomboError('This file is not a valid ModelStats file. `stat_type` listed as "' +
                                str(self.stat_type) + '".')
        self.is_model_stats = True
        self._stat_slot = 'damp_frac'
        self._stat_text = 'Est. Frac. Alternate: {0:.2g}'
        self._stat_transform = lambda pos_stat: 1 - pos_stat[self._stat_slot]

    def _add_block(self, chrm, strand, start, block):
        try:
            block_data = self._new_block(chrm, strand, start)
        except Exception:
            warnings.warn('Statistics file not opened for writing.')
            return
        block_data.create_dataset('block_stats', data=block, compression='gzip')
        if chrm not in self.chrm_names:
            self.chrm_names[chrm] = self.curr_chrm_id
            self.curr_chrm_id += 1
        sites = np.empty(block.shape[0], dtype=self._block_dtype + _SITE_ID_DTYPE)
        for name in block.dtype.names:
            sites[name] = block[name]
        sites['chrm'], sites['strand'] = self.chrm_names[chrm], strand
        self.queued_stat_batches.append(sites)
        self.is_empty = False

    def _write_stat_block(self, reg_stats, damp_frac=None):
        """one th.regionStats as a block (:2737-2773).  damp_frac: the dampened fractions under THIS file's
        pseudo-counts where the device has computed them already (aggregate_per_read_stats), else
        calc_damp_fraction"""
        self._add_block(reg_stats.chrm, reg_stats.strand, reg_stats.start,
                        region_stats_block(reg_stats, self.cov_damp_counts, damp_frac))

    def _close_write(self):
        # The reference keeps a running array of num_most_signif rows (NaN at first), merges the queued blocks
        # into it every most_signif_num_batches blocks with `sort(order=<statistic>)` and cuts it again, then trims
        # it at its first NaN.  numpy breaks ties of the named field by the remaining fields in dtype order, so that
        # sort is a total order on the records (equal records are equal bytes) and a row that is cut has
        # num_most_signif rows in front of it for good: the result is the sort of all sites, cut and trimmed --
        # computed here once, whatever most_signif_num_batches is.
        sites = np.concatenate([np.empty(0, dtype=self._block_dtype + _SITE_ID_DTYPE)] + self.queued_stat_batches)
        sites.sort(kind='mergesort', order=self._stat_slot)
        sites = sites[:self.num_most_signif]
        nans = np.flatnonzero(np.isnan(sites[self._stat_slot]))
        self.running_most_signif_sites = sites[:nans[0]] if nans.shape[0] else sites
        self.queued_stat_batches = []
        self.most_signif_sites.create_dataset(MOST_SIGNIF_H5_NAME, data=self.running_most_signif_sites,
                                              compression='gzip')
        for chrm_name, chrm_id in self.chrm_names.items():
            self.chrm_id_grp.attrs[chrm_name] = chrm_id

    def close(self):
        """writes the most significant sites if open for writing, then closes the file"""
        if self.open_for_writing:
            self._close_write()
        self._fp.close()

    def _get_chrm_name(self, pos_stat):
        return self.most_signif_chrm_map[pos_stat['chrm']]

    def iter_stat_seqs(self, genome_index, before_bases, after_bases, include_pos=True):
        """the genome sequence around every stored most significant site, in strand orientation (:2811-2848):
        (seq, chrm, strand, start, end), or seq alone without include_pos.  A site whose window the genome index
        refuses (th.TomboError: it leaves the chromosome) is skipped."""
        for pos_stat in self.most_signif_stats:
            chrm, strand, pos = self._get_chrm_name(pos_stat), pos_stat['strand'].decode(), int(pos_stat['pos'])
            if strand == '+':
                start, end = pos - before_bases, pos + after_bases + 1
            else:
                start, end = pos - after_bases, pos + before_bases + 1
            try:
                stat_seq = genome_index.get_seq(chrm, start, end)
            except th.TomboError:
                continue
            if strand != '+':
                stat_seq = th.rev_comp(stat_seq)
            yield (stat_seq, chrm, strand, start, end) if include_pos else stat_seq

    def iter_most_signif_sites(self):
        """(chrm, strand, pos, transformed statistic) of the stored most significant sites.  (:2850-2859 applies
        the transform to the statistic's value instead of the record, which raises there; the record is passed)"""
        for pos_stat in self.most_signif_stats:
            yield (self._get_chrm_name(pos_stat), pos_stat['strand'].decode(), pos_stat['pos'],
                   self._stat_transform(pos_stat))

    def get_most_signif_regions(self, num_bases, num_regions, unique_pos=True, prepend_loc_to_text=False):
        """:2861-2913 -> [(chrm, start, end, strand, reg_id, reg_text), ...] (the fields the reference gives its
        intervalData)"""
        selected_regs, used_intervals = [], {}
        for i, pos_stat in enumerate(self.most_signif_stats):
            pos = int(pos_stat['pos'])
            int_start = max(0, pos - int(num_bases / 2.0))
            chrm, strand = self._get_chrm_name(pos_stat), pos_stat['strand'].decode()
            used = used_intervals.setdefault((chrm, strand), set())
            if not unique_pos or pos not in used:
                used.update(range(int_start, int_start + num_bases))
                int_text = self._stat_text.format(self._stat_transform(pos_stat))
                if prepend_loc_to_text:
                    int_text = '{0}:{1:d}:{2}'.format(chrm, pos + 1, strand) + ' ' + int_text
                selected_regs.append((chrm, int_start, int_start + num_bases, strand, '{:03d}'.format(i), int_text))
                if len(selected_regs) >= num_regions:
                    break
        if len(selected_regs) == 0:
            raise th.TomboError('No locations identified. Most likely an empty statistics file.')
        if len(selected_regs) < num_regions:
            warnings.warn('Fewer unique significant locations more than [--num-bases]/2 apart were identified. '
                          'Continuing with ' + str(len(selected_regs)) + ' unique locations. Must raise '
                          '--num-most-significant-stored in order to see more most significant stats.')
        return selected_regs

    def get_pos_stat(self, chrm, strand, pos, missing_value=None):
        try:
            pos_block_start = np.floor_divide(pos, self.region_size) * self.region_size
            block_data = self.stat_blocks[self.blocks_index[(chrm, strand)][pos_block_start]]['block_stats'][:]
            pos_index = np.where(block_data['pos'] == pos)[0]
            if len(pos_index) != 1:
                raise KeyError
            return self._stat_transform(block_data[pos_index[0]])
        except KeyError:
            return missing_value


class LevelStats(ModelStats):
    """A statistics file of the level sample comparison (ks / u / t tests)"""
    _block_dtype = _LEVEL_BLOCK_DTYPE
    cov_damp_counts = None

    def __init__(self, stats_fn, stat_type=None, region_size=None, cov_thresh=None, num_most_signif=None,
                 most_signif_num_batches=MOST_SIGNIF_NUM_BATCHES_DEFAULT):
        self._open(stats_fn, (stat_type, region_size, cov_thresh, num_most_signif), stat_type, region_size,
                   cov_thresh, num_most_signif, most_signif_num_batches)
        if self.stat_type not in LEVEL_STATS_TXTS:
            if self.stat_type in PER_READ_STATS:
                raise th.TomboError('This appears to be a model-based comparison stats file. Open with '
                                    'tombo_stats.ModelStats.')
            raise th.TomboError('This file is not a valid LevelStats file. `stat_type` listed as "' +
                                str(self.stat_type) + '".')
        self.is_model_stats = False
        self._stat_slot = 'stat'
        if self.stat_type in (KS_TEST_TXT, U_TEST_TXT, T_TEST_TXT):
            self._stat_text = '-log10(p-value): {0:.2g}'
            self._stat_transform = lambda pos_stat: _neg_log10(self, pos_stat)
        elif self.stat_type == KS_STAT_TEST_TXT:
            self._stat_text = 'D Statistic: {0:.2g}'
            self._stat_transform = lambda pos_stat: 1 - pos_stat[self._stat_slot]
        else:
            self._stat_text = ('Common Language Marginal Effect: {0:.2g}' if self.stat_type == U_STAT_TEST_TXT
                               else "Cohen's D: {0:.2g}")
            self._stat_transform = lambda pos_stat: -pos_stat[self._stat_slot]

    def _write_stat_block(self, grp_stats):
        """one th.groupStats as a block (:3194-3224): rows with a NaN statistic dropped"""
        rows = [r for r in zip(grp_stats.reg_stats, grp_stats.reg_poss, grp_stats.reg_cov, grp_stats.ctrl_cov)
                if not np.isnan(r[0])]
        self._add_block(grp_stats.chrm, grp_stats.strand, grp_stats.start, np.array(rows, dtype=_LEVEL_BLOCK_DTYPE))


def TomboStats(stat_fn):
    """ModelStats or LevelStats, whichever the file is (read only)"""
    try:
        return ModelStats(stat_fn)
    except th.TomboError:
        return LevelStats(stat_fn)


class PerReadStats(_BlockStore):
    """A per-read statistics file: stat_type and region_size given opens a fresh file for writing, else
    `per_read_stats_fn` is parsed.  A block holds (pos, stat, read_id) records (`_native.PER_READ_DTYPE`)."""
    _blocks = property(lambda self: self.per_read_blocks)

    def __init__(self, per_read_stats_fn, stat_type=None, region_size=None):
        self.per_read_stats_fn = per_read_stats_fn
        if stat_type is None or region_size is None:
            self._fp = _open_store(per_read_stats_fn, 'r')
            try:
                self.stat_type = _text(self._fp.attrs.get('stat_type'))
                self.region_size = self._fp.attrs.get('block_size')
                self.per_read_blocks = self._fp[STAT_BLOCKS_H5_NAME]
                self.blocks_index, self.num_blocks = _blocks_index(self.per_read_blocks)
            except Exception:
                raise th.TomboError('Non-existent or invalid per-read statistics file provided.')
        else:
            self.stat_type, self.region_size = stat_type, region_size
            self._fp = _open_store(per_read_stats_fn, 'w')
            self.curr_block_num = 0
            self._fp.attrs['stat_type'] = self.stat_type
            self._fp.attrs['block_size'] = self.region_size
            self.per_read_blocks = self._fp.create_group(STAT_BLOCKS_H5_NAME)
        self.are_pvals = self.stat_type != ALT_MODEL_TXT
        self._stat_slot = 'stat'
        self._stat_text = '-log10(p-value): {0:.2g}'
        self._stat_transform = lambda pos_stat: _neg_log10(self, pos_stat)

    def _write_per_read_block(self, per_read_block, read_id_lookup, chrm, strand, start):
        """:3335-3366: the records, and the lookup from their read_id numbers back to the ids as the two datasets
        read_ids (variable-length strings) and read_id_vals"""
        try:
            block_data = self._new_block(chrm, strand, start)
        except Exception:
            warnings.warn('Per-read statistics file not opened for writing.')
            return
        block_data.create_dataset('block_stats', data=per_read_block, compression='gzip')
        try:
            import h5py
            dt = h5py.special_dtype(vlen=str)
        except ImportError:   # (a stand-in group: objects)
            dt = object
        read_ids = np.array(list(read_id_lookup.keys()), dtype=dt)
        read_ids_ds = block_data.create_dataset('read_ids', read_ids.shape, dtype=dt, compression='gzip')
        read_ids_ds[...] = read_ids
        block_data.create_dataset('read_id_vals', data=np.array(list(read_id_lookup.values())), compression='gzip')
        self._fp.flush()

    def get_region_per_read_stats(self, interval_data):
        """:3368-3434 without the num_reads sampling: (pos, stat, read id string) records of the interval
        (`chrm`, `strand`, `start`, `end` attributes), None for an unknown (chrm, strand) or no block"""
        try:
            cs_blocks = self.blocks_index[(interval_data.chrm, interval_data.strand)]
        except KeyError:
            return
        int_block_stats = []
        for block_start, block_name in cs_blocks.items():
            if interval_data.end < block_start or interval_data.start > block_start + self.region_size:
                continue
            block = self.per_read_blocks[block_name]
            block_stats = block['block_stats'][:]
            lookup = dict((val, _text(rid)) for rid, val in zip(block['read_ids'][()], block['read_id_vals'][()]))
            rows = np.empty(block_stats.shape[0], dtype=[('pos', 'u4'), ('stat', 'f8'), ('read_id', object)])
            rows['pos'], rows['stat'] = block_stats['pos'], block_stats[self._stat_slot]
            rows['read_id'] = [lookup[r_id] for r_id in block_stats['read_id']]
            int_block_stats.append(rows)
        if len(int_block_stats) == 0:
            return
        stats = np.concatenate(int_block_stats)
        return stats[(stats['pos'] >= interval_data.start) & (stats['pos'] < interval_data.end)]

    def close(self):
        self._fp.close()


# aggregate_per_read_stats (:4699-4777): the reference sorts every stored block by position, splits it per
# site and thresholds the pieces in worker processes.  Here consecutive blocks go to the device as they are
# stored, one `Engine.site_aggregate` call (kernel k_site_rec, csrc/k_site.h) per group of blocks.
_AGG_BYTES_PER_RECORD = 16      # a stored record, uploaded as it is
_AGG_BYTES_PER_POSITION = 60    # three i32 counters, frac / pos / cov / valid_cov / damp_frac, per block position
_AGG_MEM_FRACTION = 0.5         # of the device's free memory, for one call


def _default_max_records(engine):
    """records per site_aggregate call that fit into half of the engine's free memory (`_agg_groups` counts a
    block as at least one record per position); a stand-in engine without `device_mem`: 2^24"""
    if not hasattr(engine, 'device_mem'):
        return 1 << 24
    free = engine.device_mem()[0]
    return max(1, int(free * _AGG_MEM_FRACTION) // (_AGG_BYTES_PER_RECORD + _AGG_BYTES_PER_POSITION))


def _agg_groups(pr_stats, max_records, max_positions=2 ** 31 - 1):
    """consecutive blocks of the per-read file, in its own order, grouped into calls of at most max_records
    records (a larger block stands alone) and fewer than 2^31 positions.  The device holds per-position arrays
    too, so a block counts as at least region_size records."""
    group, n_rec = [], 0
    for block in pr_stats:
        n = max(block[4].shape[0], int(pr_stats.region_size))
        if group and (n_rec + n > max_records or (len(group) + 1) * pr_stats.region_size > max_positions):
            yield group
            group, n_rec = [], 0
        group.append(block)
        n_rec += n
    if group:
        yield group


def aggregate_per_read_stats(pr_stats, single_read_thresh, lower_thresh, stats, cov_damp_counts, min_test_reads,
                             num_most_signif, engine=None, max_records=None):
    """:4736-4777: the per-site statistics of a per-read statistics file under new thresholds, written to
    `stats` (pr_stats / stats: file names or group objects).  Every stored block becomes one block of the new
    file, control coverage 0 (_agg_stats_worker)."""
    pr_stats = PerReadStats(pr_stats)
    eng = _engine(engine)
    if max_records is None:
        max_records = _default_max_records(eng)
    cd = cov_damp_counts
    all_stats = ModelStats(stats, stat_type=pr_stats.stat_type, region_size=pr_stats.region_size,
                           cov_damp_counts=(cd['unmod'], cd['mod']) if isinstance(cd, dict) else cd,
                           cov_thresh=min_test_reads, num_most_signif=num_most_signif)
    damp = _damp_pair(cov_damp_counts)
    for group in _agg_groups(pr_stats, int(max_records)):
        starts = np.array([b[2] for b in group], dtype=np.int64)
        ends = np.array([b[3] for b in group], dtype=np.int64)
        rec_off = _csr_offsets([b[4].shape[0] for b in group])
        records = np.concatenate([np.asarray(b[4], dtype=_native.PER_READ_DTYPE) for b in group])
        res = eng.site_aggregate(starts, ends, rec_off, records, single_read_thresh, lower_thresh,
                                 pr_stats.stat_type == ALT_MODEL_TXT, damp)
        for t, (chrm, strand, start, _, _) in enumerate(group):
            a = int(res.pos_off[t])
            b = a + int(res.counts[t])
            rs = th.regionStats(res.frac[a:b], res.poss[a:b], chrm, strand, start, res.cov[a:b], [0] * (b - a),
                                res.valid[a:b])
            all_stats._write_stat_block(rs, res.damp[a:b])
    pr_stats.close()
    all_stats.close()
    if all_stats.is_empty:
        raise th.TomboError(_NO_SITES_MSG)


def write_stats_from_regions(results, per_read, stats, pr_stats=None):
    """Stores what `compute_reg_stats_batch(..., return_per_read=True)` returned: every regionStats of
    `results` (regions that failed are skipped) through `stats._write_stat_block`, every per-read block of
    `per_read` through `pr_stats._write_per_read_block` (stats: an open ModelStats; pr_stats: an open
    PerReadStats or None).  The containers stay open."""
    for reg_res, reg_blocks in zip(results, per_read):
        if pr_stats is not None:
            for _, block in reg_blocks:
                pr_stats._write_per_read_block(*block)
        if not isinstance(reg_res, Exception):
            for _, reg_stats in reg_res:
                stats._write_stat_block(reg_stats)


# ---------------------------------------------------------------------------------------------
# test_significance (tombo_stats.py:4574-4657, worker :4400-4438): the reference cuts the covered genome into
# regions, hands them to worker processes and collects their results in writer processes.  Here the regions
# are taken in the order `th.iter_cov_regs` gives them and go to the engine in batches; one process, no queues.
TEST_SIGNIF_MAX_STATS = 1 << 24     # upper bound on the statistics of one engine call (24 bytes each on the device)


def _region_stat_bound(reg, fm_offset, n_names=1):
    """an upper bound on the statistics region `reg` yields: its reads' overlaps with the extended region"""
    s = np.array([rd.start for rd in reg.reads], dtype=np.int64)
    e = np.array([rd.end for rd in reg.reads], dtype=np.int64)
    ov = np.minimum(e, reg.end + fm_offset) - np.maximum(s, reg.start - fm_offset)
    return int(np.maximum(ov, 0).sum()) * n_names


def _ctrl_region_seq(ctrl, fm_offset, std_ref):
    """the sequence of a control region as the prior blend reads it (compute_posterior_samp_dists,
    :3575-3584): from the control reads over [start - lag_b - fm, end + lag_e + fm), padded with '-' to the
    span `_prior_levels` takes"""
    K, cp = std_ref.kmer_width, std_ref.central_pos
    dn = K - cp - 1
    lag_b, lag_e = (cp, dn) if ctrl.strand == '+' else (dn, cp)
    seq = th.get_region_seq(ctrl.reads, ctrl.start - lag_b - fm_offset, ctrl.end + lag_e + fm_offset)
    return '-' * (K - 1 - lag_b) + seq + '-' * (K - 1 - lag_e)


def iter_signif_region_batches(reads_index, stat_type, region_size, fm_offset, ctrl_reads_index=None, std_ref=None,
                               alt_refs=None, max_stats_per_call=TEST_SIGNIF_MAX_STATS, engine=None):
    """The region batches of `test_significance` -> (regions, ctrl_regions or None) per engine call: the
    regions of `th.iter_cov_regs(reads_index, 1, region_size, ctrl_reads_index)` in that order, each with its
    reads (`intervalData.add_reads`; the control copy likewise), those without sample reads left out; a batch
    ends before the upper bound on its statistics passes max_stats_per_call (a region above it goes alone)."""
    n_names = len(alt_refs) if stat_type == ALT_MODEL_TXT else 1
    regs, ctrls, n = [], [], 0
    for chrm, strand, start in th.iter_cov_regs(reads_index, 1, region_size, ctrl_reads_index, engine=engine):
        reg = th.intervalData(chrm, start, start + region_size, strand).add_reads(reads_index)
        if len(reg.reads) == 0:
            continue
        ctrl = None
        if ctrl_reads_index is not None:
            ctrl = reg.copy(include_reads=False).add_reads(ctrl_reads_index)
            if stat_type in LEVEL_STATS_TXTS and len(ctrl.reads) == 0:
                continue   # (get_base_levels of the control raises: the worker skips the region)
            if stat_type == SAMP_COMP_TXT and std_ref is not None:
                ctrl.update(seq=_ctrl_region_seq(ctrl, fm_offset, std_ref))
        bound = _region_stat_bound(reg, fm_offset, n_names)
        if regs and n + bound > max_stats_per_call:
            yield regs, (ctrls if ctrl_reads_index is not None else None)
            regs, ctrls, n = [], [], 0
        regs.append(reg)
        ctrls.append(ctrl)
        n += bound
    if regs:
        yield regs, (ctrls if ctrl_reads_index is not None else None)


def signif_store_names(stat_type, stats_file_bn, per_read_bn=None, alt_refs=None):
    """the file names of `test_significance` (_get_stats_queue :4452-4470, _get_per_read_queue :4507-4516)
    -> ({statistic name: statistics file}, {statistic name: per-read file})"""
    names = [n for n, _ in alt_refs] if stat_type == ALT_MODEL_TXT else [stat_type]
    infix = dict((n, '.' + n if stat_type == ALT_MODEL_TXT else '') for n in names)
    return (dict((n, stats_file_bn + infix[n] + '.tombo.stats') for n in names),
            {} if per_read_bn is None else dict((n, per_read_bn + infix[n] + '.tombo.per_read_stats') for n in names))


def test_significance(reads_index, stat_type, stats_file_bn, region_size, num_processes, min_test_reads,
                      num_most_signif, per_read_bn=None, single_read_thresh=None, lower_thresh=None,
                      cov_damp_counts=None, fm_offset=None, ctrl_reads_index=None, std_ref=None, alt_refs=None,
                      use_standard_llhr=False, prior_weights=None, engine=None, stores=None,
                      max_stats_per_call=TEST_SIGNIF_MAX_STATS):
    """tombo_stats.py:4574-4657 on an in-memory reads index ({(chrm, strand): [reads]}): modified base
    detection over every covered region, written to the statistics file(s) `<stats_file_bn>[.<alt name>]
    .tombo.stats` and, with per_read_bn, `<per_read_bn>[.<alt name>].tombo.per_read_stats`.  de_novo and
    sample_compare run through `compute_reg_stats_reads_batch`, model_compare through
    `compute_reg_stats_batch`, the six level tests through `compute_group_reg_stats_batch` (a LevelStats
    file).  Regions without sample reads, and regions whose computation raises th.TomboError, are skipped.
    stores: {file name: open group-interface object} to write into instead of opening the files (h5py).
    num_processes is accepted and ignored: the regions go to the engine in batches of at most
    max_stats_per_call statistics (an upper bound)."""
    is_level = stat_type in LEVEL_STATS_TXTS
    if not is_level and stat_type not in PER_READ_STATS:
        raise NotImplementedError('Unrecognized test type.')
    fm_offset = FM_OFFSET_DEFAULT if fm_offset is None else int(fm_offset)
    if is_level and ctrl_reads_index is None:
        raise ValueError('%s needs control reads (ctrl_reads_index)' % stat_type)
    if not is_level and (single_read_thresh is None or cov_damp_counts is None):
        raise ValueError('%s needs single_read_thresh and cov_damp_counts' % stat_type)
    stores = stores or {}
    stat_fns, pr_fns = signif_store_names(stat_type, stats_file_bn, None if is_level else per_read_bn, alt_refs)
    if is_level:
        all_stats = dict((n, LevelStats(stores.get(fn, fn), stat_type, region_size, min_test_reads, num_most_signif))
                         for n, fn in stat_fns.items())
    else:
        cd = cov_damp_counts   # (stored as given: a pair, or the reference's dict)
        damp = (cd['unmod'], cd['mod']) if isinstance(cd, dict) else tuple(cd)
        all_stats = dict((n, ModelStats(stores.get(fn, fn), stat_type, region_size, damp, min_test_reads,
                                        num_most_signif)) for n, fn in stat_fns.items())
    all_pr = dict((n, PerReadStats(stores.get(fn, fn), stat_type, region_size)) for n, fn in pr_fns.items())
    try:
        for regs, ctrls in iter_signif_region_batches(reads_index, stat_type, region_size, fm_offset, ctrl_reads_index,
                                                      std_ref, alt_refs, max_stats_per_call, engine):
            if is_level:
                results = compute_group_reg_stats_batch(regs, ctrls, fm_offset, min_test_reads, stat_type, engine)
                per_read = [[] for _ in regs]
            else:
                compute = compute_reg_stats_batch if stat_type == ALT_MODEL_TXT else compute_reg_stats_reads_batch
                results = compute(regs, fm_offset, min_test_reads, single_read_thresh, lower_thresh, ctrls, std_ref,
                                  alt_refs, use_standard_llhr, stat_type, prior_weights,
                                  return_per_read=bool(all_pr), engine=engine)
                results, per_read = results if all_pr else (results, [[] for _ in regs])
            for reg_res, reg_blocks in zip(results, per_read):
                for name, block in reg_blocks:
                    all_pr[name]._write_per_read_block(*block)
                if not isinstance(reg_res, Exception):
                    for name, reg_stats in reg_res:
                        all_stats[name]._write_stat_block(reg_stats)
    finally:
        for container in list(all_stats.values()) + list(all_pr.values()):
            container.close()


test_significance.__test__ = False   # (the reference's name; not a test)


# ---------------------------------------------------------------------------------------------
# ROC and precision-recall from statistics files: the numbers behind `tombo plot roc`, `per_read_roc`,
# `sample_compare_roc` and `sample_compare_per_read_roc` (tombo_stats.py:2377-2535, _plot_commands.py:60-82).
# The reference labels every record in a Python loop and sorts a list of tuples; here the records of many blocks
# are labelled and compacted in one call (`Engine.roc_motif_labels` / `roc_loc_labels`) and the sorted
# cumulative counts come from `Engine.roc_rank_counts` (kernels in csrc/k_roc.h).  Every output is an integer
# count or one float64 division of two integers.
#
# Deviations from the reference, all at places where it fails or reads the wrong bases:
#   * a motif whose window around a record leaves the fetched sequence does not match; the test of the
#     record's own base still applies.  At a chromosome start the reference slices with a negative offset
#     (an empty or shifted window: IndexError or wrong bases), and for a minus-strand record within
#     before_bases of a chromosome end its reverse-complemented window is shifted.  Everywhere else, the end of
#     a plus-strand chromosome included, the two agree.
#   * a genome letter that is not A, C, G or T never equals mod_base (the reference compares letters, so an `N`
#     in the genome under a motif whose modified position is `N` is emitted there, always with label False).
#   * prep_accuracy_rates raises ValueError for a name without entries (the reference fails inside zip(); its
#     callers drop empty names first) and for a NaN statistic (sorted() is order-dependent there).
# (record, motif) pairs per labelling call: the engine holds an output slot of up to 17 bytes for each, on the host
# and on the device, before compaction
_ROC_MAX_PAIRS = 1 << 26
# with a total_stats_limit the control form sends at most as many records per call as entries are still missing
# (what a call emits is known only when it returns), but not fewer than this
_ROC_LIMIT_MIN_RECORDS = 1 << 16
_SEQ_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _b in enumerate(b'ACGT'):
    _SEQ_CODE[_b] = _i
_EMPTY_I64 = np.zeros(0, dtype=np.int64)


class MotifStats(object):
    """The (statistic, has_mod) pairs of one modification name: `stats` float64 and `has_mod` bool, in the
    reference's order.  len() and iteration (tuples) stand in for the reference's list of tuples."""

    def __init__(self, stats=(), has_mod=()):
        self.stats = np.ascontiguousarray(stats, dtype=np.float64)
        self.has_mod = np.ascontiguousarray(has_mod, dtype=np.bool_)
        if self.stats.ndim != 1 or self.stats.shape != self.has_mod.shape:
            raise ValueError('stats and has_mod must be one-dimensional and of one length')

    def __len__(self):
        return self.stats.shape[0]

    def __iter__(self):
        return iter(zip(self.stats.tolist(), self.has_mod.tolist()))

    @classmethod
    def concat(cls, parts):
        parts = list(parts)
        if not parts:
            return cls()
        return cls(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


def _as_motif_stats(mod_stats):
    if isinstance(mod_stats, MotifStats):
        return mod_stats
    pairs = list(mod_stats)
    return MotifStats([p[0] for p in pairs], [bool(p[1]) for p in pairs])


def motif_base_sets(motif):
    """(length, mod_pos, code of mod_base or 255, uint8 base sets: bit c set when code c is allowed)"""
    sets = np.array([sum(1 << 'ACGT'.index(b) for b in th.SINGLE_LETTER_CODE[c].strip('[]')) for c in motif.raw_motif],
                    dtype=np.uint8)
    code = 'ACGT'.find(motif.mod_base)
    return motif.motif_len, motif.mod_pos, code if code >= 0 else 255, sets


def motif_can_overlap_itself(motif):
    """can two matches of the motif overlap?  (Only then does re.finditer, leftmost and non-overlapping, differ
    from `matches at this position`.)"""
    sets = motif_base_sets(motif)[3]
    return any(np.all(sets[shift:] & sets[:len(sets) - shift]) for shift in range(1, len(sets)))


def _check_motif_descs(motif_descs):
    motif_descs = list(motif_descs)
    if not motif_descs:
        raise ValueError('motif_descs needs at least one motif')
    motifs = [motif for motif, _ in motif_descs]
    before_bases = max(m.mod_pos for m in motifs) - 1
    after_bases = max(m.motif_len - m.mod_pos for m in motifs)
    return motifs, [name for _, name in motif_descs], before_bases, after_bases


def _by_name(names, parts):
    """{name: MotifStats} from the pieces of every motif.  parts[k]: one (stats, has_mod, order key) per call, in call
    order.  Motifs that share a name share a list, as in the reference: within a call the entries are ordered by the
    key (the record in the motif form, the block in the control form), then by the motif's place in motif_descs."""
    out = {}
    for name in names:
        if name in out:
            continue
        ks = [k for k, n in enumerate(names) if n == name]
        pieces = []
        for call in range(len(parts[ks[0]])):
            st, hm = (np.concatenate([parts[k][call][j] for k in ks]) for j in (0, 1))
            if len(ks) > 1:
                order = np.argsort(np.concatenate([parts[k][call][2] for k in ks]), kind='stable')
                st, hm = st[order], hm[order]
            pieces.append((st, hm))
        out[name] = MotifStats.concat(pieces)
    return out


class _RocBlocks(object):
    """the blocks of one labelling call: sequences and records, concatenated"""

    def __init__(self):
        self.minus, self.seq_start, self.seqs, self.recs = [], [], [], []
        self.n_rec = 0

    def add(self, strand, seq_start, reg_seq, rec_pos, rec_stat):
        self.minus.append(strand == '-')
        self.seq_start.append(seq_start)
        self.seqs.append(reg_seq)
        self.recs.append((np.asarray(rec_pos, dtype=np.int64), np.asarray(rec_stat, dtype=np.float64)))
        self.n_rec += self.recs[-1][0].shape[0]

    def __len__(self):
        return len(self.minus)

    def rec_arrays(self):
        off = _csr_offsets([p.shape[0] for p, _ in self.recs])
        pos = np.concatenate([p for p, _ in self.recs]) if self.recs else _EMPTY_I64
        return off, pos, _concat_f64([s for _, s in self.recs])

    def seq_arrays(self):
        codes = _SEQ_CODE[np.frombuffer(''.join(self.seqs).encode('latin-1', 'replace'), dtype=np.uint8)]
        return (np.array(self.minus, dtype=np.uint8), np.array(self.seq_start, dtype=np.int64),
                _csr_offsets([len(s) for s in self.seqs]), codes)


def _block_seq(genome_index, chrm, strand, start, end, before_bases, after_bases):
    """(seq_start, reg_seq) of a block as the reference fetches it (:2417-2425)"""
    if strand == '+':
        seq_start, seq_end = max(start - before_bases, 0), end + after_bases
    else:
        seq_start, seq_end = max(start - after_bases, 0), end + before_bases
    return seq_start, genome_index.get_seq(chrm, seq_start, seq_end, error_end=False)


def compute_motif_stats(stats, motif_descs, genome_index, stats_per_block=None, total_stats_limit=None,
                        engine=None):
    """:2406-2456: for every record of `stats` (a ModelStats, LevelStats or PerReadStats; blocks in the order of
    its iterator) and every motif whose mod_base is the base under the record, the pair (statistic, does the
    motif match with its modified position on the record) -> {mod_name: MotifStats}.  stats_per_block: blocks
    with more records are sub-sampled with np.random.choice (global state, one draw per such block, in block
    order); total_stats_limit: no further block is read once that many rows were seen.  Blocks go to the engine
    in groups of at most _ROC_MAX_PAIRS (record, motif) pairs."""
    motifs, names, before_bases, after_bases = _check_motif_descs(motif_descs)
    eng = _engine(engine)
    descs = [motif_base_sets(m) for m in motifs]
    max_records = max(1, _ROC_MAX_PAIRS // len(motifs))
    shared_names = len(set(names)) < len(names)
    parts = [[] for _ in motifs]

    def flush(group):
        if group.n_rec:
            res = eng.roc_motif_labels(*(group.seq_arrays() + group.rec_arrays() + (descs,)), return_index=shared_names)
            for k, r in enumerate(res):
                parts[k].append(r)

    group, total_num_stats = _RocBlocks(), 0
    for chrm, strand, start, end, block_stats in stats:
        seq_start, reg_seq = _block_seq(genome_index, chrm, strand, start, end, before_bases, after_bases)
        if stats_per_block is not None and block_stats.shape[0] > stats_per_block:
            block_stats = block_stats[np.random.choice(block_stats.shape[0], stats_per_block, replace=False)]
        total_num_stats += block_stats.shape[0]
        if group.n_rec and group.n_rec + block_stats.shape[0] > max_records:
            flush(group)
            group = _RocBlocks()
        group.add(strand, seq_start, reg_seq, block_stats['pos'], block_stats[stats._stat_slot])
        if total_stats_limit is not None and total_num_stats >= total_stats_limit:
            break
    flush(group)
    return _by_name(names, parts)


def _truth_group(eng, mod_locs, unmod_locs, slot, blocks):
    """the kept (stats, has_mod) of a group of blocks against the position lists of their (chrm, strand) keys"""
    lists, where, sizes = ([], []), ({}, {}), [0, 0]   # per list: pieces, key -> (sorted positions, first index)

    def cs_slice(which, locs, cs, start, end):
        if cs not in where[which]:
            v = np.unique(np.asarray(locs.get(cs, ()), dtype=np.int64))
            where[which][cs] = (v, sizes[which])
            lists[which].append(v)
            sizes[which] += v.shape[0]
        v, base = where[which][cs]
        return base + int(np.searchsorted(v, start)), base + int(np.searchsorted(v, end))

    blk_loc, recs = [], _RocBlocks()
    for chrm, strand, start, end, block_stats in blocks:
        blk_loc.append(cs_slice(0, mod_locs, (chrm, strand), start, end) +
                       cs_slice(1, unmod_locs, (chrm, strand), start, end))
        recs.add(strand, 0, '', block_stats['pos'], block_stats[slot])
    return eng.roc_loc_labels(np.array(blk_loc, dtype=np.int64).reshape(-1, 4), np.concatenate(lists[0]),
                              np.concatenate(lists[1]), *recs.rec_arrays())


def compute_ground_truth_stats(stats, ground_truth_locs, engine=None):
    """:2458-2483: ground_truth_locs = (mod_locs, unmod_locs, mod_name), the first two {(chrm, strand):
    positions} as parse_locs_file returns them.  A record whose position is in either list of its block's
    (chrm, strand) is kept; it counts as modified when the position is in mod_locs -> {mod_name: MotifStats}.
    Blocks go to the engine in groups of at most _ROC_MAX_PAIRS records."""
    mod_locs, unmod_locs, mod_name = ground_truth_locs
    eng = _engine(engine)
    pieces, group, n_rec = [], [], 0
    for block in stats:
        n = block[4].shape[0]
        if n == 0:
            continue
        if group and n_rec + n > _ROC_MAX_PAIRS:
            pieces.append(_truth_group(eng, mod_locs, unmod_locs, stats._stat_slot, group))
            group, n_rec = [], 0
        group.append(block)
        n_rec += n
    if group:
        pieces.append(_truth_group(eng, mod_locs, unmod_locs, stats._stat_slot, group))
    return {mod_name: MotifStats.concat(pieces)}


def _interleave_by_block(samp, ctrl, samp_off, ctrl_off):
    """per block the kept sample entries, then the kept control entries.  samp / ctrl: (stats, has_mod, record
    index) in record order; *_off: the blocks' record offsets -> (stats, has_mod, block of every entry)"""
    n_blk = samp_off.shape[0] - 1
    s_blk = np.searchsorted(samp_off, samp[2], side='right') - 1
    c_blk = np.searchsorted(ctrl_off, ctrl[2], side='right') - 1
    s_cnt, c_cnt = np.bincount(s_blk, minlength=n_blk), np.bincount(c_blk, minlength=n_blk)
    s_first, c_first = np.concatenate([[0], np.cumsum(s_cnt)]), np.concatenate([[0], np.cumsum(c_cnt)])
    n = samp[0].shape[0] + ctrl[0].shape[0]
    st, hm, blk = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.bool_), np.empty(n, dtype=np.int64)
    s_dest = np.arange(samp[0].shape[0]) + c_first[s_blk]          # the control entries of earlier blocks go before
    c_dest = np.arange(ctrl[0].shape[0]) + s_first[c_blk + 1]      # the sample entries up to this block go before
    st[s_dest], hm[s_dest], blk[s_dest] = samp[0], samp[1], s_blk
    st[c_dest], hm[c_dest], blk[c_dest] = ctrl[0], ctrl[1], c_blk
    return st, hm, blk


_NO_PAIRS = (np.zeros(0), np.zeros(0, dtype=np.bool_), _EMPTY_I64)


def _ctrl_group(eng, motifs, on_device, samp, ctrl):
    """the control form for a group of blocks (samp / ctrl: _RocBlocks with the same blocks and sequences) -> per
    motif (stats, has_mod, block of every entry): per block the sample's kept records, then the control's"""
    n_blk = len(samp)
    seq_args, samp_recs, ctrl_recs = samp.seq_arrays(), samp.rec_arrays(), ctrl.rec_arrays()
    kept = {}                 # motif -> [(stats, has_mod, index) of the sample, of the control]
    if on_device:
        descs = [motif_base_sets(motifs[k]) for k in on_device]
        for which, recs in enumerate((samp_recs, ctrl_recs)):
            res = eng.roc_motif_labels(*(seq_args + recs + (descs,)), ctrl_label=which == 0, return_index=True) \
                if recs[1].shape[0] else [_NO_PAIRS] * len(descs)
            for k, r in zip(on_device, res):
                kept.setdefault(k, []).append(r)
    for k, motif in enumerate(motifs):
        if k in kept:
            continue
        # a motif that can overlap itself: the reference's own scan, block by block (:2507-2515)
        sites, blk_loc, n_sites = [], np.zeros((n_blk, 4), dtype=np.int64), 0
        for t in range(n_blk):
            if samp.minus[t]:
                poss = [m.start() + motif.motif_len - motif.mod_pos for m in motif.rev_comp_pat.finditer(samp.seqs[t])]
            else:
                poss = [m.start() + motif.mod_pos - 1 for m in motif.motif_pat.finditer(samp.seqs[t])]
            sites.append(np.array(poss, dtype=np.int64) + samp.seq_start[t])
            blk_loc[t] = n_sites, n_sites + len(poss), 0, 0
            n_sites += len(poss)
        sites = np.concatenate(sites)
        kept[k] = [
            eng.roc_loc_labels(blk_loc, sites, _EMPTY_I64, *samp_recs, return_index=True)
            if samp_recs[1].shape[0] else _NO_PAIRS,
            eng.roc_loc_labels(blk_loc[:, [2, 3, 0, 1]], _EMPTY_I64, sites, *ctrl_recs, return_index=True)
            if ctrl_recs[1].shape[0] else _NO_PAIRS]
    return [_interleave_by_block(kept[k][0], kept[k][1], samp_recs[0], ctrl_recs[0]) for k in range(len(motifs))]


def compute_ctrl_motif_stats(stats, ctrl_stats, motif_descs, genome_index, stats_per_block=None,
                             total_stats_limit=None, engine=None):
    """:2485-2535: the records of `stats` at motif sites count as modified, those of `ctrl_stats` at the same sites
    of the same block as unmodified -> {mod_name: MotifStats}, per block and motif the sample entries, then the
    control entries.  The sites of a block are those of re.finditer over the block's fetched sequence: for a
    motif that cannot overlap itself that is every position where it matches (found on the device); for one that
    can, the positions come from the regular expression here and the device tests membership.  stats_per_block
    is accepted and unused, as in the reference.  total_stats_limit counts emitted entries and ends the output
    after the block that reaches it.  Blocks are sent in groups of at most _ROC_MAX_PAIRS (record,
    motif) pairs; with a limit a group holds at most as many records as entries are still missing (at least
    _ROC_LIMIT_MIN_RECORDS, a larger block stands alone), and nothing is read or sent after the group that reaches
    it."""
    motifs, names, before_bases, after_bases = _check_motif_descs(motif_descs)
    eng = _engine(engine)
    on_device = [k for k, m in enumerate(motifs) if not motif_can_overlap_itself(m)]
    max_records = max(1, _ROC_MAX_PAIRS // len(motifs))
    parts = [[] for _ in motifs]
    total_num_stats = 0

    def flush(samp, ctrl):
        """-> the limit was reached"""
        nonlocal total_num_stats
        if len(samp) == 0:
            return False
        merged = _ctrl_group(eng, motifs, on_device, samp, ctrl)
        emitted = total_num_stats + np.cumsum(sum(np.bincount(blk, minlength=len(samp)) for _, _, blk in merged))
        total_num_stats = int(emitted[-1])
        reached = np.flatnonzero(emitted >= total_stats_limit) if total_stats_limit is not None else _EMPTY_I64
        for k, (st, hm, blk) in enumerate(merged):
            if reached.shape[0]:
                keep = blk <= reached[0]
                st, hm, blk = st[keep], hm[keep], blk[keep]
            parts[k].append((st, hm, blk))
        return reached.shape[0] > 0

    samp, ctrl, done = _RocBlocks(), _RocBlocks(), False
    for chrm, strand, start, end, block_stats in stats:
        ctrl_block = ctrl_stats.get_reg_stats(chrm, strand, start, end)
        n = max(block_stats.shape[0], 0 if ctrl_block is None else ctrl_block.shape[0])
        budget = max_records if total_stats_limit is None else \
            min(max_records, max(total_stats_limit - total_num_stats, _ROC_LIMIT_MIN_RECORDS))
        if len(samp) and max(samp.n_rec, ctrl.n_rec) + n > budget:
            done = flush(samp, ctrl)
            if done:
                break
            samp, ctrl = _RocBlocks(), _RocBlocks()
        seq_start, reg_seq = _block_seq(genome_index, chrm, strand, start, end, before_bases, after_bases)
        samp.add(strand, seq_start, reg_seq, block_stats['pos'], block_stats[stats._stat_slot])
        if ctrl_block is None:
            ctrl.add(strand, seq_start, reg_seq, _EMPTY_I64, np.zeros(0))
        else:
            ctrl.add(strand, seq_start, reg_seq, ctrl_block['pos'], ctrl_block[stats._stat_slot])
    if not done:
        flush(samp, ctrl)
    return _by_name(names, parts)


def compute_auc(tp_rate, fp_rate):
    return np.sum(tp_rate[:-1] * (fp_rate[1:] - fp_rate[:-1]))


def compute_mean_avg_precison(tp_rate, precision):
    return np.sum(np.diff(np.concatenate([[0, ], tp_rate, [1, ]]), ) *
                  np.concatenate([[0, ], precision, [1, ]])[:-1])


def compute_accuracy_rates(stat_has_mod, num_plot_points=ROC_PLOT_POINTS):
    """:2384-2404, on the host: num_plot_points evenly spaced values of the true positive rate, the false
    positive rate and the precision along an ordered sequence of True / False"""
    with np.errstate(invalid='ignore', divide='ignore'):
        tp_cumsum = np.cumsum(stat_has_mod)
        tp_rate = tp_cumsum / tp_cumsum[-1]
        fp_cumsum = np.cumsum(np.logical_not(stat_has_mod))
        fp_rate = fp_cumsum / fp_cumsum[-1]
        precision = tp_cumsum / np.arange(1, len(stat_has_mod) + 1, dtype=float)
    tp_rate = tp_rate[np.linspace(0, tp_rate.shape[0] - 1, num_plot_points).astype(np.int64)]
    fp_rate = fp_rate[np.linspace(0, fp_rate.shape[0] - 1, num_plot_points).astype(np.int64)]
    precision = precision[np.linspace(0, precision.shape[0] - 1, num_plot_points + 1).astype(np.int64)][1:]
    return tp_rate, fp_rate, precision


def sampled_accuracy_rates(mod_stats, num_plot_points=ROC_PLOT_POINTS, engine=None, mod_name=None):
    """compute_accuracy_rates of the entries ordered by (statistic, has_mod), the ordering and the cumulative counts
    on the device: only the counts at the sampled ranks come back, the divisions are the reference's"""
    mod_stats = _as_motif_stats(mod_stats)
    n = len(mod_stats)
    if n == 0:
        raise ValueError('No statistics for modification %s' % (mod_name,))
    rate_idx = np.linspace(0, n - 1, num_plot_points).astype(np.int64)
    prec_idx = np.linspace(0, n - 1, num_plot_points + 1).astype(np.int64)[1:]
    ranks = np.union1d(rate_idx, prec_idx)
    tp_at, tp_total, n_nan = _engine(engine).roc_rank_counts(mod_stats.stats, mod_stats.has_mod, ranks)
    if n_nan:
        raise ValueError('NaN statistic')
    tp_rate_at, tp_prec_at = tp_at[np.searchsorted(ranks, rate_idx)], tp_at[np.searchsorted(ranks, prec_idx)]
    with np.errstate(invalid='ignore', divide='ignore'):
        tp_rate = tp_rate_at / np.int64(tp_total)
        fp_rate = (rate_idx + 1 - tp_rate_at) / np.int64(n - tp_total)
        precision = tp_prec_at / (prec_idx + 1).astype(float)
    return tp_rate, fp_rate, precision


def prep_accuracy_rates(all_motif_stats, engine=None, summary=None):
    """_plot_commands.py:60-82: the flat lists (tp rates, fp rates, precisions, names) that go into the ROC and
    precision-recall plots, ROC_PLOT_POINTS per name.  summary (a dict): receives name -> (AUC, mean average
    precision).  ValueError for a name without entries and for a NaN statistic."""
    tp_rates, fp_rates, precisions, mod_names_for_r = [], [], [], []
    for mod_name, mod_stats in all_motif_stats.items():
        mod_tp_rate, mod_fp_rate, mod_precision = sampled_accuracy_rates(mod_stats, engine=engine, mod_name=mod_name)
        if summary is not None:
            summary[mod_name] = (compute_auc(mod_tp_rate, mod_fp_rate),
                                 compute_mean_avg_precison(mod_tp_rate, mod_precision))
        tp_rates.extend(mod_tp_rate)
        fp_rates.extend(mod_fp_rate)
        precisions.extend(mod_precision)
        mod_names_for_r.extend([mod_name] * len(mod_tp_rate))
    return tp_rates, fp_rates, precisions, mod_names_for_r


# ---------------------------------------------------------------------------------------------
# Alternate-base model estimation: `tombo build_model estimate_alt_reference`, estimate_alt_model
# (tombo_stats.py:1747-2098).  The reference bins the levels of every read by k-mer in worker
# processes and fits one scipy gaussian_kde per k-mer; here a batch of reads is one
# `Engine.kmer_levels` call and the densities of all k-mers one `Engine.kde_eval` call (kernels in
# csrc/k_kde.h).  The density isolation that follows is 4**K x num_dens_points values and stays in
# numpy.  Reads are lists of `th.resquiggledRead`; k-mers are in lexicographic order throughout.
def _all_kmers(kmer_width):
    from itertools import product
    return [''.join(p) for p in product('ACGT', repeat=kmer_width)]


def _kmer_levels_batch(reads, kmer_width, central_pos, completed, engine):
    """one `kmer_levels` call for a list of reads -> (counts, levels, lv_off); a read without levels is left out"""
    reads = [rd for rd in reads if rd.means is not None]
    n_kmers = 4 ** kmer_width
    if not reads:
        return np.zeros(n_kmers, dtype=np.int64), np.empty(0), np.zeros(n_kmers + 1, dtype=np.int64)
    means = [np.asarray(rd.means, dtype=np.float64) for rd in reads]
    codes = [encode_seq(rd.seq) for rd in reads]
    for rd, m, c in zip(reads, means, codes):
        if m.shape[0] != c.shape[0]:
            raise ValueError('read %r: levels and bases differ in number' % (rd.read_id,))
    return _engine(engine).kmer_levels(
        _concat_f64(means), np.ascontiguousarray(np.concatenate(codes), dtype=np.uint8),
        _csr_offsets([m.shape[0] for m in means]), kmer_width, central_pos, completed)


def parse_base_levels(reads, std_ref, parse_levels_batch_size, kmer_obs_thresh, max_kmer_obs,
                      min_kmer_obs_to_est, engine=None):
    """tombo_stats.py:1811-1884: the levels of `reads` grouped by k-mer -> (levels, lv_off), the
    levels of k-mer k (lexicographic index) being levels[lv_off[k]:lv_off[k + 1]] in the order the
    reads were given and, inside a read, position order.  Reads are taken in batches of
    parse_levels_batch_size; a k-mer whose total exceeds max_kmer_obs after a batch is complete
    and skipped from then on; the loop ends once the rarest k-mer still open after a batch exceeds
    kmer_obs_thresh, or with the reads.  Raises th.TomboError where the reference exits (fewer than
    min_kmer_obs_to_est observations of some k-mer), warns where it warns.  Deterministic: the
    caller shuffles."""
    K = std_ref.kmer_width
    n_kmers = 4 ** K
    bs = int(parse_levels_batch_size)
    if bs < 1:
        raise ValueError('parse_levels_batch_size must be positive')
    completed = np.zeros(n_kmers, dtype=np.uint8)
    totals = np.zeros(n_kmers, dtype=np.int64)
    batches = []   # (counts, levels, lv_off) per batch, on the host
    reads = list(reads)
    pos = 0
    while True:
        batch, pos = reads[pos:pos + bs], pos + bs
        no_more_reads = len(batch) < bs
        is_open = completed == 0
        if not is_open.any():
            break   # (every k-mer complete: the reference's min() of nothing)
        counts, levels, lv_off = _kmer_levels_batch(batch, K, std_ref.central_pos, completed, engine)
        batches.append((counts, levels, lv_off))
        totals += counts
        completed[is_open & (totals > max_kmer_obs)] = 1
        if totals[is_open].min() > kmer_obs_thresh or no_more_reads:
            break
    fewest = int(totals.min())
    if fewest < kmer_obs_thresh:
        if fewest < min_kmer_obs_to_est:
            raise th.TomboError(
                'Too few minimal k-mer observations to continue to alternative estimation. Minimal k-mer has ' +
                str(fewest) + ' total observations and ' + str(min_kmer_obs_to_est) +
                ' observations per k-mer are required.')
        warnings.warn('Requested minimal k-mer observations not found in all reads. Continuing to estimation '
                      'using a k-mer with ' + str(fewest) + ' total observations')
    # the one concatenation per k-mer: batch b's levels of k-mer k follow those of the earlier batches
    out_off = _csr_offsets(totals)
    out = np.empty(int(out_off[-1]), dtype=np.float64)
    before = np.zeros(n_kmers, dtype=np.int64)
    for counts, levels, lv_off in batches:
        out[np.repeat(out_off[:-1] + before - lv_off[:-1], counts) + np.arange(levels.shape[0])] = levels
        before += counts
    return out, out_off


def write_kmer_densities_file(dens_fn, kmer_dens, save_x):
    """tombo_stats.py:1886-1893: one `Kmer<TAB>Signal<TAB>Density` line per k-mer and grid point"""
    with io.open(dens_fn, 'wt') as fp:
        fp.write('Kmer\tSignal\tDensity\n')
        for kmer, dens_i in kmer_dens.items():
            for x, y in zip(save_x, dens_i):
                fp.write('%s\t%s\t%s\n' % (kmer, str(x), str(y)))


def parse_kmer_densities_file(dens_fn):
    """tombo_stats.py:1895-1912 -> {kmer: densities} in file order"""
    raw = {}
    with io.open(dens_fn) as fp:
        fp.readline()   # header
        for line in fp:
            kmer, _, dens_i = line.split()
            raw.setdefault(kmer, []).append(float(dens_i))
    first_len = None
    kmer_dens = {}
    for kmer, dens_i in raw.items():
        if first_len is None:
            first_len = len(dens_i)
        if len(dens_i) != first_len:
            raise th.TomboError('Density file is valid.')   # (the reference's own wording)
        kmer_dens[kmer] = np.array(dens_i)
    return kmer_dens


def est_kernel_density(reads, std_ref, kmer_obs_thresh, density_basename, save_x, kernel_dens_bw,
                       alt_or_stnd_name='alt', parse_levels_batch_size=ALT_EST_BATCH,
                       max_kmer_obs=MAX_KMER_OBS, min_kmer_obs_to_est=MIN_KMER_OBS_TO_EST, engine=None,
                       shuffle=True):
    """tombo_stats.py:1914-1939 -> {kmer: density on save_x}: the Gaussian kernel density (bandwidth
    kernel_dens_bw in level units) of every k-mer's levels, ONE `kde_eval` call for all k-mers.
    shuffle: np.random.shuffle of the reads first, as the reference does."""
    reads = list(reads)
    if shuffle:
        np.random.shuffle(reads)
    levels, lv_off = parse_base_levels(reads, std_ref, parse_levels_batch_size, kmer_obs_thresh,
                                       max_kmer_obs, min_kmer_obs_to_est, engine)
    if (np.diff(lv_off) < 2).any():   # (scipy's gaussian_kde raises for a single observation)
        raise th.TomboError('Kernel density estimation requires at least two observations per k-mer.')
    dens = _engine(engine).kde_eval(levels, lv_off, np.ascontiguousarray(save_x, dtype=np.float64),
                                    float(kernel_dens_bw))
    kmer_dens = dict(zip(_all_kmers(std_ref.kmer_width), dens))
    if density_basename is not None:
        write_kmer_densities_file(density_basename + '.' + alt_or_stnd_name + '_density.txt', kmer_dens, save_x)
    return kmer_dens


def estimate_kmer_densities(reads, ctrl_reads, std_ref, kmer_obs_thresh, density_basename, kernel_dens_bw,
                            save_x, engine=None, **kwargs):
    """tombo_stats.py:1941-1961 -> (alt_dens, std_dens, std_ref); kwargs go to est_kernel_density"""
    alt_dens = est_kernel_density(reads, std_ref, kmer_obs_thresh, density_basename, save_x, kernel_dens_bw,
                                  'alternate', engine=engine, **kwargs)
    std_dens = est_kernel_density(ctrl_reads, std_ref, kmer_obs_thresh, density_basename, save_x,
                                  kernel_dens_bw, 'control', engine=engine, **kwargs)
    return alt_dens, std_dens, std_ref


def load_kmer_densities(alt_dens_fn, std_dens_fn, std_ref):
    """tombo_stats.py:1963-1989 -> (alt_dens, std_dens, std_ref, save_x)"""
    alt_dens = parse_kmer_densities_file(alt_dens_fn)
    std_dens = parse_kmer_densities_file(std_dens_fn)
    num_dens_points = next(v for v in alt_dens.values()).shape[0]
    if num_dens_points != next(v for v in std_dens.values()).shape[0]:
        raise th.TomboError('Alternative and standard density estimates do not correspond.')
    save_x = np.linspace(KERNEL_DENSITY_RANGE[0], KERNEL_DENSITY_RANGE[1], num_dens_points)
    return alt_dens, std_dens, std_ref, save_x


def isolate_alt_density(alt_dens, std_dens, alt_base, alt_frac_pctl, std_ref, save_x):
    """tombo_stats.py:1991-2071 (host only, no engine): the alternate sample's densities shifted onto
    the standard sample's (a quadratic fit of the mean shift of the k-mers without the alternate
    base), the standard-base fraction of the sample from the matched peaks of the k-mers with one
    alternate base (its alt_frac_pctl-th percentile), and per k-mer with the alternate base the mean
    of what is left of its shifted density after that fraction of the standard density is taken
    away -> AltModel.  Same operations in the same order as the reference."""
    def calc_mean(dens):
        keep = dens > 1e-10
        return np.average(save_x[keep], weights=dens[keep])

    no_alt_std_means, no_alt_mean_diffs = [], []
    for kmer in std_dens:
        if alt_base in kmer:
            continue
        no_alt_std_means.append(calc_mean(std_dens[kmer]))
        no_alt_mean_diffs.append(calc_mean(alt_dens[kmer]) - no_alt_std_means[-1])
    calc_offset = np.poly1d(np.polyfit(no_alt_std_means, no_alt_mean_diffs, 2))
    save_x_unit = save_x[1] - save_x[0]

    shifted_alt_dens = {}
    for kmer, kmer_alt_dens in alt_dens.items():
        est_offset = int(calc_offset(calc_mean(std_dens[kmer])) / save_x_unit)
        if est_offset < 0:   # standard mean above: the alternate density moves right
            shifted_alt_dens[kmer] = np.concatenate([np.zeros(-est_offset), kmer_alt_dens[:est_offset]])
        else:
            shifted_alt_dens[kmer] = np.concatenate([kmer_alt_dens[est_offset:], np.zeros(est_offset)])

    def get_peak_frac(kmer_std_dens, kmer_alt_dens):
        std_peak = np.argmax(kmer_std_dens)
        inner = kmer_alt_dens[1:-1]
        alt_local_peaks = np.flatnonzero((inner > kmer_alt_dens[:-2]) & (inner > kmer_alt_dens[2:])) + 1
        matched = alt_local_peaks[np.argmin(abs(alt_local_peaks - std_peak))]
        return kmer_alt_dens[matched] / kmer_std_dens[std_peak]

    std_frac = np.percentile([get_peak_frac(std_dens[kmer], shifted_alt_dens[kmer])
                              for kmer in std_dens if kmer.count(alt_base) == 1], alt_frac_pctl)
    if std_frac >= 1:
        warnings.warn('Alternative base incorporation rate estimate is approximately 0. Consider lowering '
                      '--alt-fraction-percentile.')
    model_sd = np.mean(list(std_ref.sds.values()))
    alt_ref = []
    for kmer in std_ref.means:
        n_alt = kmer.count(alt_base)
        if n_alt == 0:
            continue
        with np.errstate(under='ignore'):
            diff_dens = shifted_alt_dens[kmer] - (std_dens[kmer] * std_frac ** n_alt)
            diff_dens[diff_dens < 0] = 0
            alt_level = np.average(save_x, weights=diff_dens)
        for m in re.finditer(alt_base, kmer):
            alt_ref.append((kmer, m.start(), alt_level, model_sd))
    return AltModel(kmer_ref=alt_ref, central_pos=std_ref.central_pos, alt_base=alt_base)


def estimate_alt_model(reads, ctrl_reads, std_ref, alt_base, alt_frac_pctl, kmer_obs_thresh,
                       density_basename, kernel_dens_bw, alt_dens_fn, std_dens_fn,
                       num_dens_points=NUM_DENS_POINTS, engine=None, **kwargs):
    """tombo_stats.py:2073-2098: an alternate-base model from a sample with one known, randomly
    incorporated alternate base (`reads`) and a standard sample (`ctrl_reads`), or from two density
    files written by an earlier run (then the reads are not used).  kwargs go to est_kernel_density."""
    if alt_dens_fn is None or std_dens_fn is None:
        save_x = np.linspace(KERNEL_DENSITY_RANGE[0], KERNEL_DENSITY_RANGE[1], num_dens_points)
        alt_dens, std_dens, std_ref = estimate_kmer_densities(
            reads, ctrl_reads, std_ref, kmer_obs_thresh, density_basename, kernel_dens_bw, save_x,
            engine=engine, **kwargs)
    else:
        alt_dens, std_dens, std_ref, save_x = load_kmer_densities(alt_dens_fn, std_dens_fn, std_ref)
    return isolate_alt_density(alt_dens, std_dens, alt_base, alt_frac_pctl, std_ref, save_x)


# ---------------------------------------------------------------------------------------------
# Canonical and motif k-mer model estimation: `tombo build_model estimate_reference` /
# `estimate_motif_alt_reference` (tombo_stats.py:1242-1501, :1716-1740, :2108-2189).  The reference
# loops over the covered positions of every region in worker processes; here the host does what
# the reference does with strings (region sequence, motif search, k-mer codes, the key of each
# entry) and the coverage intervals, and a batch of regions is ONE `Engine.region_key_levels` call
# that does all arithmetic over levels (kernels in csrc/k_kmer_est.h).  The tabulation is one
# `Engine.segment_medians` call per column.
NUM_READS_TO_ADJUST_MODEL = 5000     # _default_parameters.py:174
STANDARD_MODEL_NAME = 'standard'     # tombo_stats.py:87
KMER_EST_MAX_LEVELS = 1 << 24        # levels piled up per engine call (128 MB of float64)

# keys: k-mers in lexicographic order, or (k-mer, offset) in the order of tabulate_mod_kmer_levels;
# levels[off[k]:off[k + 1]] / sds[...]: the (level, spread) pairs of key k in region order, then
# position order; n_regions: the regions that got as far as a coverage interval
KmerLevelTable = namedtuple('KmerLevelTable', 'keys off levels sds n_regions')


def motif_kmer_keys(kmer_width, motif):
    """[(kmer, offset)] in the order tabulate_mod_kmer_levels walks them (tombo_stats.py:2116-2118)"""
    return [(kmer, p - 1) for kmer in _all_kmers(kmer_width) for p in motif.find_mod_poss(kmer)]


def _window_codes(int_seq, kmer_width, minus):
    """the k-mer index of every window of int_seq (the reverse complement's on the minus strand); -1 for a
    window with anything but ACGT"""
    codes = encode_seq(int_seq).astype(np.int64)
    n = codes.shape[0] - kmer_width + 1
    if n <= 0:
        return np.empty(0, dtype=np.int64)
    idx, bad = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for j in range(kmer_width):
        c = codes[kmer_width - 1 - j:kmer_width - 1 - j + n] if minus else codes[j:j + n]
        bad |= c > 3
        idx = idx * 4 + ((3 - c) if minus else c)
    idx[bad] = -1
    return idx


def _subsample_region_reads(reads, reg_start, reg_end, region_size, cs_cov_thresh):
    """tombo_stats.py:1247-1260: shuffle, then keep the reads before the first one at which the running sum of
    max(r.end, reg.end) - min(r.start, reg.start) reaches region_size * cs_cov_thresh (all, if it never does)"""
    np.random.shuffle(reads)
    csum = np.cumsum([max(rd.end, reg_end) - min(rd.start, reg_start) for rd in reads])
    hit = np.flatnonzero(csum >= region_size * cs_cov_thresh)
    return reads[:int(hit[0])] if hit.shape[0] else reads


def _region_entries(chrm, strand, reg_start, region_size, reads, lv_reads, cov_thresh, upstrm_bases, dnstrm_bases,
                    motif, valid_poss, key_of):
    """get_region_kmer_levels after the subsampling, up to the arithmetic: (genomic position, key) of every
    entry of the region in the reference's order, or None when the region has no coverage interval.
    reads: the region's reads (they give the sequence); lv_reads: those whose levels count."""
    K = upstrm_bases + dnstrm_bases + 1
    diff = np.zeros(region_size + 1, dtype=np.int64)
    for rd in lv_reads:
        a, b = max(rd.start, reg_start) - reg_start, min(rd.end, reg_start + region_size) - reg_start
        if b > a:
            diff[a] += 1
            diff[b] -= 1
    reg_cov = np.cumsum(diff[:-1])
    edges = np.flatnonzero(np.diff(np.concatenate([[False], reg_cov > cov_thresh])))
    if reg_cov[-1] > cov_thresh:
        edges = np.concatenate([edges, [region_size]])
    if edges.shape[0] <= 1:
        return None
    minus = strand == '-'
    bb, ab = (dnstrm_bases, upstrm_bases) if minus else (upstrm_bases, dnstrm_bases)
    ent_g, ent_key = [], []
    for cov_start, cov_end in edges.reshape(-1, 2).tolist():
        int_len = cov_end - cov_start
        int_seq = th.get_region_seq(reads, reg_start + cov_start - bb, reg_start + cov_end + ab)
        win = _window_codes(int_seq, K, minus)
        if valid_poss is None and motif is None:
            poss, keys = np.arange(min(int_len, win.shape[0]), dtype=np.int64), win[:int_len]
        else:
            if valid_poss is not None:
                if (chrm, strand) not in valid_poss:
                    continue
                mod_poss = np.asarray(valid_poss[(chrm, strand)], dtype=np.int64) - reg_start - cov_start
                mod_poss = mod_poss[(mod_poss >= 0) & (mod_poss < int_len)].tolist()
            elif not minus:
                mod_poss = [m.start() + motif.mod_pos - 1 - bb for m in motif.motif_pat.finditer(int_seq)]
            else:
                mod_poss = [m.start() + motif.motif_len - motif.mod_pos - bb
                            for m in motif.rev_comp_pat.finditer(int_seq)]
            pairs = [(mp - i + bb, K - i - 1 if minus else i) for mp in mod_poss if 0 <= mp < int_len
                     for i in range(K) if 0 <= mp - i + bb < min(int_len, win.shape[0])]
            poss = np.array([p for p, _ in pairs], dtype=np.int64)
            offs = np.array([o for _, o in pairs], dtype=np.int64)
            keys = np.where(win[poss] >= 0, key_of[np.maximum(win[poss], 0) * K + offs], -1) if pairs else poss
        # (a position no read of the region has a level at: the reference's KeyError, skipped)
        keep = (keys >= 0) & (reg_cov[poss + cov_start] > 0)
        ent_g.append(poss[keep] + reg_start + cov_start)
        ent_key.append(keys[keep])
    cat = (lambda xs: np.concatenate(xs) if xs else np.empty(0, dtype=np.int64))
    return cat(ent_g), cat(ent_key), reg_cov


class _KmerEstBatch(object):
    """the regions of one `region_key_levels` call: reads once, regions by read index, positions once"""

    def __init__(self):
        self.read_idx, self.reads, self.reg_reads, self.reg_read_off = {}, [], [], [0]
        self.pos_reg, self.pos_g, self.ent_pos, self.ent_key, self.n_pos, self.n_levels = [], [], [], [], 0, 0

    def add(self, lv_reads, ent_g, ent_key, reg_start, reg_cov):
        for rd in lv_reads:
            if id(rd) not in self.read_idx:
                self.read_idx[id(rd)] = len(self.reads)
                self.reads.append(rd)
            self.reg_reads.append(self.read_idx[id(rd)])
        self.reg_read_off.append(len(self.reg_reads))
        uniq, inv = np.unique(ent_g, return_inverse=True)
        self.pos_reg.append(np.full(uniq.shape[0], len(self.reg_read_off) - 2, dtype=np.int64))
        self.pos_g.append(uniq)
        self.ent_pos.append(inv.astype(np.int64).reshape(-1) + self.n_pos)
        self.ent_key.append(ent_key)
        self.n_pos += uniq.shape[0]
        self.n_levels += int(reg_cov[uniq - reg_start].sum())

    def run(self, engine, est_mean, n_keys):
        cat = (lambda xs: np.ascontiguousarray(np.concatenate(xs), dtype=np.int64))
        means = [np.asarray(rd.means, dtype=np.float64) for rd in self.reads]
        return engine.region_key_levels(
            est_mean, np.array([rd.start for rd in self.reads], dtype=np.int64),
            np.array([rd.strand == '-' for rd in self.reads], dtype=np.uint8),
            _csr_offsets([m.shape[0] for m in means]), _concat_f64(means),
            np.array(self.reg_read_off, dtype=np.int64), np.array(self.reg_reads, dtype=np.int64),
            cat(self.pos_reg), cat(self.pos_g), cat(self.ent_pos), cat(self.ent_key), n_keys)


def extract_kmer_levels(reads_index, region_size, cov_thresh, upstrm_bases, dnstrm_bases, cs_cov_thresh,
                        est_mean=False, motif=None, valid_poss=None, engine=None,
                        max_levels=KMER_EST_MAX_LEVELS):
    """tombo_stats.py:1398-1452 with get_region_kmer_levels (:1242-1359) -> one KmerLevelTable for the run.
    reads_index: {(chrm, strand): [th.resquiggledRead]}.  Regions come from th.iter_cov_regs; a region's reads
    are those that overlap it (intervalData.add_reads).  With cs_cov_thresh the region's reads are shuffled
    with np.random.shuffle and cut as the reference cuts them.  A read without levels, or whose number of
    levels differs from end - start, gives no levels but still counts in the subsampling and in the sequence.
    A position is used when more than cov_thresh reads have a level there (NaN levels count, and make that
    position's pair NaN).  valid_poss: {(chrm, strand): int array} of modified positions, replacing the motif
    search.  Regions are cut into engine calls of at most max_levels piled-up levels (a single region may
    exceed it); the result does not depend on the cut.  Raises th.TomboError where the reference exits."""
    region_size = int(region_size)
    if region_size < 1 or int(max_levels) < 1:
        raise ValueError('region_size and max_levels must be positive')
    if upstrm_bases < 0 or dnstrm_bases < 0:
        raise ValueError('upstrm_bases and dnstrm_bases must not be negative')
    if valid_poss is not None and motif is None:
        raise ValueError('valid_poss needs the motif')
    eng = _engine(engine)
    K = upstrm_bases + dnstrm_bases + 1
    key_of = None
    if motif is None:
        keys = _all_kmers(K)
    else:
        keys = motif_kmer_keys(K, motif)
        key_of = np.full(4 ** K * K, -1, dtype=np.int64)
        for i, (kmer, offset) in enumerate(keys):
            key_of[TomboModel._kmer_code(kmer) * K + offset] = i
    n_keys, results, n_regions = len(keys), [], 0
    batch, spans = _KmerEstBatch(), {}
    for chrm, strand, reg_start in th.iter_cov_regs(reads_index, cov_thresh, region_size, engine=eng):
        reg_start, reg_end = int(reg_start), int(reg_start) + region_size
        if (chrm, strand) not in spans:     # (start, end of the strand's reads once: the overlap test is one numpy line)
            cs_reads = reads_index.get((chrm, strand), ())
            spans[(chrm, strand)] = (cs_reads, np.array([rd.start for rd in cs_reads], dtype=np.int64),
                                     np.array([rd.end for rd in cs_reads], dtype=np.int64))
        cs_reads, cs_start, cs_end = spans[(chrm, strand)]
        reads = [cs_reads[i] for i in np.flatnonzero((cs_start < reg_end) & (cs_end > reg_start)).tolist()]
        if len(reads) == 0:
            continue
        if cs_cov_thresh is not None:
            reads = _subsample_region_reads(reads, reg_start, reg_end, region_size, cs_cov_thresh)
        lv_reads = [rd for rd in reads if rd.means is not None and len(rd.means) == rd.end - rd.start]
        if len(lv_reads) == 0:
            continue
        ent = _region_entries(chrm, strand, reg_start, region_size, reads, lv_reads, cov_thresh, upstrm_bases,
                              dnstrm_bases, motif, valid_poss, key_of)
        if ent is None:
            continue
        n_regions += 1
        if ent[0].shape[0] == 0:
            continue
        batch.add(lv_reads, ent[0], ent[1], reg_start, ent[2])
        if batch.n_levels >= max_levels:
            results.append(batch.run(eng, est_mean, n_keys))
            batch = _KmerEstBatch()
    if batch.n_pos:
        results.append(batch.run(eng, est_mean, n_keys))
    if n_regions == 0:
        raise th.TomboError('No genomic positions contain --minimum-test-reads. Consider ' +
                            'setting this option to a lower value.')
    # the one concatenation per key: batch b's pairs of key k follow those of the earlier batches
    totals = np.zeros(n_keys, dtype=np.int64)
    for counts, _, _, _ in results:
        totals += counts
    out_off = _csr_offsets(totals)
    levels, sds = np.empty(int(out_off[-1]), dtype=np.float64), np.empty(int(out_off[-1]), dtype=np.float64)
    before = np.zeros(n_keys, dtype=np.int64)
    for counts, koff, lv, sd in results:
        at = np.repeat(out_off[:-1] + before - koff[:-1], counts) + np.arange(lv.shape[0])
        levels[at], sds[at] = lv, sd
        before += counts
    return KmerLevelTable(keys, out_off, levels, sds, n_regions)


_NO_OBS_MSG = ('At least one %sk-mer is not covered at any poitions by --minimum-test-reads.\n\t\tConsider fitting '
               'to a smaller k-mer via the --upstream-bases and --downstream-bases, or lowering '
               '--minimum-test-reads.\n\t\tNote that this may result in a lower quality model.')
_FEW_OBS_MSG = ('K-mers represeneted in fewer observations than requested in the provided reads. Consider a '
                'shorter k-mer or providing more reads.\n\t%d observations found in least common kmer.')


def _tabulate(table, min_kmer_obs, engine, what):
    counts = np.diff(table.off)
    short = np.flatnonzero((counts == 0) | (counts < min_kmer_obs))
    if short.shape[0]:     # the reference meets the keys in order: the first one that falls short decides
        if counts[short[0]] == 0:
            raise th.TomboError(_NO_OBS_MSG % what)
        raise th.TomboError(_FEW_OBS_MSG % int(counts.min()))
    eng = _engine(engine)
    return eng.segment_medians(table.levels, table.off), eng.segment_medians(table.sds, table.off)


def tabulate_kmer_levels(table, min_kmer_obs, engine=None):
    """tombo_stats.py:1454-1501: [(kmer, median level, median sd)] in lexicographic k-mer order.  Where the
    reference names an undefined `motif` in its too-few-observations branch (and dies with NameError), the
    message it meant is raised."""
    lv, sd = _tabulate(table, min_kmer_obs, engine, '')
    return [(kmer, lv[i], sd[i]) for i, kmer in enumerate(table.keys)]


def tabulate_mod_kmer_levels(table, min_kmer_obs, motif, engine=None):
    """tombo_stats.py:2108-2158: [(kmer, offset, median level, median sd)] in the order of motif_kmer_keys"""
    if list(table.keys) != motif_kmer_keys(len(table.keys[0][0]) if table.keys else 1, motif):
        raise ValueError('the table was not extracted with this motif')
    lv, sd = _tabulate(table, min_kmer_obs, engine, 'modified ')
    return [(kmer, offset, lv[i], sd[i]) for i, (kmer, offset) in enumerate(table.keys)]


# what center_model_to_median_norm takes per read, in memory: the raw signal, the `start` column of the read's
# Events table, its bases (read-centric, one per event) and read_start_rel_to_raw
# (center_model_to_median_norm_batch also takes RNA reads: raw_signal in acquisition order, as the FAST5 file has
# it, and map_len: the read's mapped length end - start, which the reference hands to compute_num_events; None:
# the number of bases)
CenterRead = namedtuple('CenterRead', 'raw_signal event_starts seq read_start_rel_to_raw rna map_len')
CenterRead.__new__.__defaults__ = (False, None)
_NO_CENTER_READS_MSG = 'No reads succcessfully processed for sequence-based normalization parameter re-fitting.'
_FEW_CENTER_READS_MSG = ('Fewer reads succcessfully processed for sequence-based normalization parameter '
                         're-fitting than requested.')


def _read_corr_factors(eng, rd, init_ref, params, opts, min_raw):
    """get_read_corr_factors (tombo_stats.py:1624-1667) of one DNA read -> (shift_corr_factor, scale_corr_factor).
    Two slices of the resident pipeline: the median normalisation of the whole raw signal, then the read's own
    boundaries over that signal against init_ref's levels of its sequence through the Theil-Sen stage.  Raises
    th.TomboError where the reference's read raises (and is skipped)."""
    from . import errors
    K, up = init_ref.kmer_width, init_ref.central_pos
    dn = K - up - 1
    if dn < 1:
        raise th.TomboError('Must have at least one upstream and downstream base for a Tombo model.')
    raw = np.ascontiguousarray(rd.raw_signal, dtype=np.float64)
    starts = np.asarray(rd.event_starts).astype(np.int64)
    codes = encode_seq(rd.seq)
    if (codes > 3).any():
        raise th.TomboError(errors.MESSAGES[22])
    if starts.shape[0] != codes.shape[0] or codes.shape[0] < K + 1:
        raise th.TomboError('Read events and sequence differ in number, or the read is shorter than two k-mers.')
    rsrtr = int(rd.read_start_rel_to_raw) + int(starts[up])
    starts = starts[up:-(dn - 1)] if dn > 1 else starts[up:]
    starts = starts - starts[0]
    norm_len = int(starts[-1])
    if rsrtr < 0 or rsrtr + norm_len > raw.shape[0] or (np.diff(starts) <= 0).any() or raw.shape[0] < min_raw:
        raise th.TomboError('Read events do not fit the raw signal.')
    # (the draw comes after everything that can fail on the host, as in the reference: tombo_stats.py:411-414)
    n_points = starts.shape[0] - 1
    samp = None
    if n_points > _native.MAX_POINTS_FOR_THEIL_SEN:
        samp = _native.pack_samp_inds([np.random.choice(n_points, _native.MAX_POINTS_FOR_THEIL_SEN, replace=False)])
    # slice 1: normalize_raw_signal(all_raw_signal) -- the segmentation that shares the stage is not used
    eng.set_num_events([2])
    eng.upload(params, opts, [raw], [codes])
    eng.run_stages(_native.STAGE_SEGMENT, _native.STAGE_SEGMENT)
    st = int(eng.get(_native.GET_STATUS)[0])
    if st not in (0, 2):     # (2: the two change points asked for were not found; the signal is normalised before)
        errors.raise_for_status(st)
    norm = eng.get(_native.GET_SEG_NORM)[:raw.shape[0]].copy()
    # slice 2: expected levels of the sequence, base means over the given boundaries, Theil-Sen
    eng.set_num_events([2])
    eng.upload(params, opts, [norm], [codes], samp_ind=samp)
    eng.put(_native.PUT_NORM, norm)
    eng.put(_native.PUT_DP_SEGS, starts, per_read=[rsrtr, norm_len])
    eng.run_stages(_native.STAGE_REF_LEVELS, _native.STAGE_REF_LEVELS)
    eng.run_stages(_native.STAGE_SKIP, _native.STAGE_RESCALE)
    errors.raise_for_status(int(eng.get(_native.GET_STATUS)[0]))
    fit = eng.get(_native.GET_THEIL_SEN)[0]
    return fit[2], fit[3]     # -inter / slope, 1 / slope


def center_model_to_median_norm(reads, init_ref, max_reads=NUM_READS_TO_ADJUST_MODEL, engine=None):
    """tombo_stats.py:1599-1705: shift and scale init_ref (in place; it is returned) so that median-normalised
    reads fit it.  reads: CenterRead-like objects (raw_signal, event_starts, seq, read_start_rel_to_raw, rna).
    They are shuffled with np.random.shuffle; then read by read the raw signal is median-normalised, the event
    starts clipped to the model's k-mer flanks, and the Theil-Sen line of init_ref's levels over the base means
    gives shift_corr_factor = -inter / slope and scale_corr_factor = 1 / slope (a read of more than
    MAX_POINTS_FOR_THEIL_SEN points is drawn with np.random.choice, in read order).  A read that fails is skipped;
    the first max_reads successes count; the medians of their factors go to init_ref._center_model.  Raises
    th.TomboError without a success, warns with fewer than max_reads.  RNA reads are refused.  A read with fewer
    raw samples than the engine's segmentation needs (4 * running_stat_width + 2) counts as failed."""
    reads = list(reads)
    if any(getattr(rd, 'rna', False) for rd in reads):
        raise NotImplementedError('center_model_to_median_norm: RNA reads (signal reversal, event-based scale '
                                  'values) are not built')
    eng = _engine(engine)
    rsqgl_params = load_resquiggle_parameters(th.seqSampleType(DNA_SAMP_TYPE, False))
    params, opts = _native.make_params(rsqgl_params), _native.make_opts()
    min_raw = 4 * int(rsqgl_params.running_stat_width) + 2
    eng.ensure_model(init_ref)      # (Engine.set_model, and the engine knows which table it holds)
    np.random.shuffle(reads)
    shifts, scales = [], []
    for rd in reads:
        try:
            shift_corr, scale_corr = _read_corr_factors(eng, rd, init_ref, params, opts, min_raw)
        except th.TomboError:
            continue
        shifts.append(shift_corr)
        scales.append(scale_corr)
        if len(shifts) >= max_reads:
            break
    if len(shifts) < max_reads:
        if len(shifts) == 0:
            raise th.TomboError(_NO_CENTER_READS_MSG)
        warnings.warn(_FEW_CENTER_READS_MSG)
    init_ref._center_model(np.median(shifts), np.median(scales))
    return init_ref

_CENTER_MEM_FRACTION = 0.5      # of the device's free memory, for one centring call


def _default_center_chunk(engine, reads, params, opts, kmer_width):
    """reads per centring call that fit into half of the engine's free memory, counting every read as the longest
    one (the footprint of a resquiggle batch of such reads: the centring entries use its buffers); a stand-in
    engine without `device_mem`: 4096"""
    from . import planner
    if not hasattr(engine, 'device_mem'):
        return 4096
    n_raw = max(max(len(rd.raw_signal) for rd in reads), 1)
    n_seq = max(max(len(rd.seq) for rd in reads), 1)
    some, more = (planner.exact_bytes([n_raw] * k, [n_seq] * k, params, opts, kmer_width) for k in (8, 16))
    per_read = max((more - some) / 8.0, 1.0)
    room = engine.device_mem()[0] * _CENTER_MEM_FRACTION - some
    return int(min(max(room // per_read + 8, 1), planner.MAX_READS))


def center_model_to_median_norm_batch(reads, init_ref, max_reads=NUM_READS_TO_ADJUST_MODEL, engine=None,
                                      chunk_reads=None):
    """center_model_to_median_norm for all reads at once, RNA too: the reads go to the device in chunks of
    chunk_reads (default: what fits into half of the engine's free memory, and no more than the successes still
    wanted, but at least 256), each chunk two calls -- Engine.center_prepare (normalisation of the whole raw
    signal, which stays on the device; the model's levels; the reads' own boundaries) and Engine.center_fit
    (Theil-Sen fit, the pick of the first max_reads successes, the medians of their factors).  Between the two the
    subsamples of the reads of more than MAX_POINTS_FOR_THEIL_SEN points are drawn with np.random.choice, in read
    order, for the reads that came through the first call: the reference's order of draws.  The work ends with the
    chunk that holds the max_reads-th success.

    reads: CenterRead-like objects, all DNA or all RNA (rna; a mixed list is a ValueError: th.is_sample_rna decides
    the type for a whole sample).  RNA (get_event_scale_values, tombo_stats.py:1603-1622): raw_signal in acquisition
    order; it is reversed, stalls are detected and their change points removed, and the scale values come from
    the events of compute_num_events(len(raw_signal), map_len, ...) t-test change points.  The raw signal may be
    int16 DAC values or float64 with the same bits in the result (the reference itself fails on int16 RNA input:
    identify_stalls assigns NaN into an array of the signal's dtype, and every read is skipped).

    The factors handed to init_ref._center_model equal, bit for bit, those of the per-read loop under the same
    seed.  The state of the global random generator AFTER the call may differ from the per-read form's: a chunk
    draws for all its reads, those behind the read that ended the per-read loop included.  Raises and warns with
    the per-read form's messages."""
    reads = list(reads)
    rna = set(bool(getattr(rd, 'rna', False)) for rd in reads)
    if len(rna) > 1:
        raise ValueError('center_model_to_median_norm_batch: RNA and DNA reads in one list')
    rna = bool(rna.pop()) if rna else False
    max_reads = int(max_reads)
    if max_reads < 1:
        raise ValueError('max_reads must be positive')
    if chunk_reads is not None and int(chunk_reads) < 1:
        raise ValueError('chunk_reads must be positive')
    eng = _engine(engine)
    K, up = init_ref.kmer_width, init_ref.central_pos
    if rna:
        rsqgl_params = load_resquiggle_parameters(th.seqSampleType(RNA_SAMP_TYPE, True))
        opts = _native.make_opts(outlier_thresh=OUTLIER_THRESH, reverse_raw=True,
                                 stall_params=th.stallParams(**STALL_PARAMS) if COLLAPSE_RNA_STALLS else None)
    else:
        rsqgl_params = load_resquiggle_parameters(th.seqSampleType(DNA_SAMP_TYPE, False))
        opts = _native.make_opts()
    params = _native.make_params(rsqgl_params)
    eng.ensure_model(init_ref)
    np.random.shuffle(reads)
    factors = np.zeros((0, 2), dtype=np.float64)    # of the successes so far, in read order
    medians, at = None, 0
    if K - up - 1 < 1:      # ('Must have at least one upstream and downstream base for a Tombo model.': every read fails)
        reads = []
    mem_chunk = None
    while at < len(reads) and factors.shape[0] < max_reads:
        if chunk_reads is not None:
            n_chunk = int(chunk_reads)
        else:
            if mem_chunk is None:
                mem_chunk = _default_center_chunk(eng, reads, params, opts, K)
            n_chunk = min(mem_chunk, max(max_reads - factors.shape[0], 256))
        chunk = reads[at:at + n_chunk]
        at += len(chunk)
        codes = [encode_seq(rd.seq) for rd in chunk]
        num_events = None
        if rna:
            num_events = [max(compute_num_events(len(rd.raw_signal), len(rd.seq) if getattr(rd, 'map_len', None) is None
                                                 else int(rd.map_len), rsqgl_params.mean_obs_per_event), 1)
                          for rd in chunk]
        status = eng.center_prepare(params, opts, [rd.raw_signal for rd in chunk], codes,
                                    [rd.event_starts for rd in chunk],
                                    [int(rd.read_start_rel_to_raw) for rd in chunk], num_events)
        # the draws, in read order, of the reads that got as far as the fit (tombo_stats.py:411-414)
        n_points = [c.shape[0] - K + 1 for c in codes]
        samp = None
        if max(n_points) > _native.MAX_POINTS_FOR_THEIL_SEN:
            samp = _native.pack_samp_inds([
                np.random.choice(n, _native.MAX_POINTS_FOR_THEIL_SEN, replace=False)
                if st == 0 and n > _native.MAX_POINTS_FOR_THEIL_SEN else None
                for n, st in zip(n_points, status.tolist())])
        status, chunk_factors, medians, n_used = eng.center_fit(samp, factors, max_reads)
        factors = np.concatenate([factors, chunk_factors[status == 0]])[:max_reads]
        assert n_used == factors.shape[0]
    if factors.shape[0] < max_reads:
        if factors.shape[0] == 0:
            raise th.TomboError(_NO_CENTER_READS_MSG)
        warnings.warn(_FEW_CENTER_READS_MSG)
    init_ref._center_model(np.float64(medians[0]), np.float64(medians[1]))
    return init_ref


def estimate_kmer_model(reads_index, cov_thresh, upstrm_bases, dnstrm_bases, min_kmer_obs, kmer_specific_sd,
                        cs_cov_thresh, est_mean, region_size, center_reads=None, engine=None, center_batch=False):
    """The canonical k-mer model of the reads; WITHOUT center_reads it is left uncentred, which the reference never
    returns (a warning says so).  tombo_stats.py:1716-1740 after the file access.  center_reads: the reads
    center_model_to_median_norm takes; the reference centres on reads of the same index.  center_batch, or an RNA
    read among center_reads: centred by center_model_to_median_norm_batch (the same factors, all reads in a few
    device calls; the only form that takes RNA reads)."""
    table = extract_kmer_levels(reads_index, region_size, cov_thresh, upstrm_bases, dnstrm_bases, cs_cov_thresh,
                                est_mean, engine=engine)
    ref = TomboModel(kmer_ref=tabulate_kmer_levels(table, min_kmer_obs, engine=engine), central_pos=upstrm_bases)
    if center_reads is not None:
        center_reads = list(center_reads)
        if center_batch or any(getattr(rd, 'rna', False) for rd in center_reads):
            ref = center_model_to_median_norm_batch(center_reads, ref, engine=engine)
        else:
            ref = center_model_to_median_norm(center_reads, ref, engine=engine)
    else:
        warnings.warn('estimate_kmer_model: no center_reads given, the model is not centred to median normalisation')
    if not kmer_specific_sd:
        ref._make_constant_sd()
    return ref


def estimate_motif_alt_model(reads_index, motif_desc, upstrm_bases, dnstrm_bases, valid_poss, min_kmer_obs,
                             cov_thresh, cs_cov_thresh, region_size, engine=None):
    """tombo_stats.py:2160-2189 after the file access: a motif-centred alternate-base model, constant sd.
    motif_desc: 'MOTIF:mod_pos' (1-based); valid_poss: None or {(chrm, strand): int array}."""
    try:
        raw_motif, mod_pos = motif_desc.split(':')
    except Exception:
        raise th.TomboError('Invalid motif decription format.')
    motif = th.TomboMotif(raw_motif, int(mod_pos))
    table = extract_kmer_levels(reads_index, region_size, cov_thresh, upstrm_bases, dnstrm_bases, cs_cov_thresh,
                                False, motif, valid_poss, engine=engine)
    alt_ref = AltModel(kmer_ref=tabulate_mod_kmer_levels(table, min_kmer_obs, motif, engine=engine),
                       central_pos=upstrm_bases, alt_base=motif.mod_base, motif=motif)
    alt_ref._make_constant_sd()
    return alt_ref

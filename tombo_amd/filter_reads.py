"""Read filters: `tombo filter` on an existing reads index (tombo/_filter_reads.py:29-280).

Every filter comes in two forms:

  * an index form, `<name>_index(reads_index, ...)`: a pure function from {(chrm, strand): [readData]} to
    (new_index, (num_filt, prev_unfilt, total)) -- nothing is read from or written to disk;
  * the reference's signature, `<name>(fast5s_dir, corr_grp, ...)`: finds the index file of the directory
    (`.<dir>.<corr_grp>.tombo.index` beside it), reads it, filters, emits the reference's message on stderr and
    writes the index back.

Only the "stuck read" filter touches per-base data: np.percentile of every read's base lengths for a few
(percentile, threshold) pairs.  That runs on the device (Engine.dwell_pctl_flags, csrc/k_filter.h) for all
unfiltered reads in calls of bounded size; the coverage filter takes its coverage from th.compute_coverage, which
is on the device as well.  The other filters compare a few numbers per index record on the host.

Where the reference exits ("No unfiltered reads present in current Tombo index.") a TomboError is raised; an index
left without reads raises TomboError('Cannot replace with an empty index.') as TomboReads.replace_index does.
"""
import os
import sys
from time import strftime

import numpy as np

from . import tombo_helper as th

NO_UNFILTERED_MSG = 'No unfiltered reads present in current Tombo index.'
EMPTY_INDEX_MSG = 'Cannot replace with an empty index.'
STUCK_CALL_BYTES = 1 << 28    # boundaries sent to the engine per dwell_pctl_flags call


def status_message(message):
    sys.stderr.write(strftime('[%H:%M:%S] ') + message + '\n')
    sys.stderr.flush()


def filter_message(num_filt, prev_unfilt, total, fast5s_dir, filter_text):
    """the text of print_filter_mess (_filter_reads.py:44-56); no unfiltered reads is the reference's exit"""
    if prev_unfilt == 0:
        raise th.TomboError(NO_UNFILTERED_MSG)
    return ('Filtered {:d} reads ({:.1%} of previously filtered and '.format(
                num_filt, float(num_filt) / prev_unfilt) +
            '{:.1%} of all valid reads)'.format(float(num_filt) / total) +
            ' reads due to ' + filter_text + ' filter from ' + fast5s_dir + '.')


def get_index_fn(fast5s_dir, corr_grp):
    """TomboReads._get_index_fn (tombo_helper.py:1095-1106)"""
    if fast5s_dir.endswith('/'):
        fast5s_dir = fast5s_dir[:-1]
    head, tail = os.path.split(fast5s_dir)
    return os.path.join(head, '.' + tail + '.' + corr_grp + '.tombo.index')


def _basedir(fast5s_dir):
    return fast5s_dir if fast5s_dir.endswith('/') else fast5s_dir + '/'


def load_index(fast5s_dir, corr_grp):
    """the whole index of a directory, filtered reads included (TomboReads(..., remove_filtered=False))"""
    index = th.read_index(get_index_fn(fast5s_dir, corr_grp), _basedir(fast5s_dir))
    return dict((cs, rds) for cs, rds in index.items() if len(rds) > 0)


def replace_index(fast5s_dir, corr_grp, new_index):
    """replace_index + write_index_file (tombo_helper.py:1137-1185)"""
    if sum(len(rds) for rds in new_index.values()) == 0:
        raise th.TomboError(EMPTY_INDEX_MSG)
    th.write_index(new_index, get_index_fn(fast5s_dir, corr_grp), _basedir(fast5s_dir))


def _open_fast5(fn):
    import h5py
    return h5py.File(fn, 'r')


def events_length_accessor(open_fast5=None):
    """rd -> the `length` column of the read's Events table, or None when it cannot be had
    (th.get_single_slot_read_centric(fast5_data, 'length', corr_group), tombo_helper.py:1622-1647)"""
    open_fast5 = open_fast5 or _open_fast5

    def base_lens(rd):
        try:
            f5 = open_fast5(rd.fn)
            try:
                return f5['/'.join(('/Analyses', rd.corr_group, 'Events'))]['length']
            finally:
                if hasattr(f5, 'close'):
                    f5.close()
        except Exception:
            return None
    return base_lens


# ---- index forms ----------------------------------------------------------------------------------
def clear_filters_index(reads_index):
    """every read unfiltered, order kept"""
    new = dict((cs, [rd._replace(filtered=False) for rd in rds]) for cs, rds in reads_index.items())
    total = sum(len(rds) for rds in new.values())
    prev_unfilt = sum(not rd.filtered for rds in reads_index.values() for rd in rds)
    return new, (0, prev_unfilt, total)


def _per_read_filter(reads_index, is_filtered):
    """the loop the q-score, signal-matching and genome-position filters share: filtered reads stay, the others
    are asked; order kept"""
    new, num_filt, prev_unfilt, total = {}, 0, 0, 0
    for cs, rds in reads_index.items():
        out = []
        for rd in rds:
            total += 1
            if not rd.filtered:
                prev_unfilt += 1
                if is_filtered(cs, rd):
                    num_filt += 1
                    rd = rd._replace(filtered=True)
            out.append(rd)
        new[cs] = out
    return new, (num_filt, prev_unfilt, total)


def stuck_flags(lens_list, obs_filter, engine=None, call_bytes=STUCK_CALL_BYTES):
    """bool per read: any(np.percentile(lens, pctl) > thresh for pctl, thresh in obs_filter), on the device.
    lens_list: one integer array of base lengths per read (an empty one answers True, as np.percentile raising
    does in the reference).  The reads go to the engine as boundaries (a running sum from 0), in calls of at most
    `call_bytes` bytes of them (one read at least)."""
    eng = th._tracks_engine(engine)
    flags, i, n = np.zeros(len(lens_list), dtype=bool), 0, len(lens_list)
    while i < n:
        j, entries = i, 0
        while j < n and (j == i or (entries + len(lens_list[j]) + 1) * 8 <= call_bytes):
            entries += len(lens_list[j]) + 1
            j += 1
        off = np.zeros(j - i + 1, dtype=np.int64)
        np.cumsum([len(v) + 1 for v in lens_list[i:j]], out=off[1:])
        segs = np.zeros(int(off[-1]), dtype=np.int64)
        for k, v in enumerate(lens_list[i:j]):
            np.cumsum(np.asarray(v, dtype=np.int64), out=segs[off[k] + 1:off[k + 1]])
        flags[i:j] = eng.dwell_pctl_flags(segs, off, obs_filter)[1]
        i = j
    return flags


def filter_reads_for_stuck_index(reads_index, obs_filter, base_lens, engine=None, call_bytes=STUCK_CALL_BYTES):
    """base_lens: rd -> integer array of the read's base lengths, or None (then the read is filtered).  Already
    filtered reads are not asked.  Order kept."""
    todo = [(cs, i) for cs, rds in reads_index.items() for i, rd in enumerate(rds) if not rd.filtered]
    lens = [base_lens(reads_index[cs][i]) for cs, i in todo]
    have = [k for k, v in enumerate(lens) if v is not None]
    stuck = np.ones(len(todo), dtype=bool)
    if have:
        stuck[have] = stuck_flags([lens[k] for k in have], obs_filter, engine, call_bytes)
    verdict = dict(zip(todo, stuck))
    new = dict((cs, [rd._replace(filtered=True) if verdict.get((cs, i), False) else rd for i, rd in enumerate(rds)])
               for cs, rds in reads_index.items())
    total = sum(len(rds) for rds in reads_index.values())
    return new, (int(stuck.sum()), len(todo), total)


def filter_reads_for_coverage_index(reads_index, frac_to_filter, engine=None, before_draw=None):
    """Per key the previously filtered reads first, then the others in iteration order.  The draw is
    np.random.choice(prev_unfilt, size=num_filt, replace=False, p=p) on numpy's global state: seed it to get the
    reference's reads.  before_draw(counts): called with (num_filt, prev_unfilt, total) before the draw (the
    reference prints its message there)."""
    new = dict((cs, [rd for rd in rds if rd.filtered]) for cs, rds in reads_index.items())
    cov = th.compute_coverage(reads_index, engine=engine)     # every read counts, filtered ones included
    unfilt, unfilt_cov, total = [], [], 0
    for cs, rds in reads_index.items():
        total += len(rds)
        for rd in rds:
            if not rd.filtered:
                unfilt_cov.append(cov[cs][rd.start + ((rd.end - rd.start) // 2)])
                unfilt.append((cs, rd))
    prev_unfilt = len(unfilt)
    if prev_unfilt == 0:
        raise th.TomboError(NO_UNFILTERED_MSG)
    num_filt = int(frac_to_filter * prev_unfilt)
    counts = (num_filt, prev_unfilt, total)
    if before_draw is not None:
        before_draw(counts)
    unfilt_cov = np.array(unfilt_cov, dtype=np.float64)
    p = unfilt_cov / unfilt_cov.sum()
    filt_indices = set(np.random.choice(prev_unfilt, size=num_filt, replace=False, p=p))
    for i, (cs, rd) in enumerate(unfilt):
        new[cs].append(rd._replace(filtered=True) if i in filt_indices else rd)
    return new, counts


def fastq_q_score_accessor(bc_grp, open_fast5=None):
    """rd -> th.get_mean_q_score of the fourth line of the read's FASTQ (_filter_reads.py:156-163)"""
    open_fast5 = open_fast5 or _open_fast5

    def mean_q_score(rd):
        f5 = open_fast5(rd.fn)
        try:
            fastq = f5['/Analyses/' + bc_grp + '/' + rd.corr_group.split('/')[-1] + '/Fastq'][()]
            fastq = fastq.decode() if isinstance(fastq, bytes) else fastq
            return th.get_mean_q_score(fastq.split('\n')[3])
        finally:
            if hasattr(f5, 'close'):
                f5.close()
    return mean_q_score


def sig_match_score_accessor(open_fast5=None):
    """rd -> the signal_match_score attribute of the read's corrected group (_filter_reads.py:199-205)"""
    open_fast5 = open_fast5 or _open_fast5

    def sig_match_score(rd):
        f5 = open_fast5(rd.fn)
        try:
            return f5['/Analyses/' + rd.corr_group].attrs.get('signal_match_score')
        finally:
            if hasattr(f5, 'close'):
                f5.close()
    return sig_match_score


def _failing(accessor, test):
    """test(accessor(rd)); a failing accessor (or comparison) filters the read"""
    def is_filtered(rd):
        try:
            return bool(test(accessor(rd)))
        except Exception:
            return True
    return is_filtered


def filter_reads_for_qscore_index(reads_index, q_score_thresh, mean_q_score=None):
    """rd.mean_q_score < thresh; a read whose index holds None is asked through `mean_q_score` (rd -> float)"""
    fallback = _failing(mean_q_score, lambda q: q < q_score_thresh)
    return _per_read_filter(reads_index, lambda cs, rd: (
        fallback(rd) if rd.mean_q_score is None else rd.mean_q_score < q_score_thresh))


def filter_reads_for_signal_matching_index(reads_index, sig_match_thresh, sig_match_score=None):
    """rd.sig_match_score > thresh; a read whose index holds None is asked through `sig_match_score`"""
    fallback = _failing(sig_match_score, lambda s: s > sig_match_thresh)
    return _per_read_filter(reads_index, lambda cs, rd: (
        fallback(rd) if rd.sig_match_score is None else rd.sig_match_score > sig_match_thresh))


def read_included(start, end, chrm_include_regs, include_partial=False):
    """_filter_reads.py:241-251, comparisons inclusive as there"""
    if chrm_include_regs is None:
        return True
    if include_partial:
        return any(not (start > i_end or end < i_start) for i_start, i_end in chrm_include_regs)
    return any((start >= i_start and end <= i_end) for i_start, i_end in chrm_include_regs)


def filter_reads_for_genome_pos_index(reads_index, include_regs, include_partial=False):
    """include_regs: {chrm: [(start, end), ...] or None} (th.parse_genome_regions).  A chromosome that is not in it
    filters all its reads; None keeps all of them."""
    return _per_read_filter(reads_index, lambda cs, rd: (
        cs[0] not in include_regs or not read_included(rd.start, rd.end, include_regs[cs[0]], include_partial)))


# ---- the reference's signatures -----------------------------------------------------------------------
def clear_filters(fast5s_dir, corr_grp):
    index = load_index(fast5s_dir, corr_grp)
    status_message('Clearing all filters.')
    new, _ = clear_filters_index(index)
    replace_index(fast5s_dir, corr_grp, new)
    status_message('All filters successfully cleared!')


def _run(fast5s_dir, corr_grp, start_text, filter_text, index_form):
    index = load_index(fast5s_dir, corr_grp)
    status_message(start_text)
    new, counts = index_form(index)
    status_message(filter_message(*counts, fast5s_dir=fast5s_dir, filter_text=filter_text))
    replace_index(fast5s_dir, corr_grp, new)


def filter_reads_for_stuck(fast5s_dir, corr_grp, obs_filter, base_lens=None, engine=None, open_fast5=None):
    """base_lens: rd -> base lengths or None; default: the `length` column of the read's Events table, read from
    the FAST5 object open_fast5(rd.fn) gives (default: h5py.File(fn, 'r'))"""
    base_lens = base_lens or events_length_accessor(open_fast5)
    _run(fast5s_dir, corr_grp, 'Filtering stuck reads.', 'observations per base',
         lambda index: filter_reads_for_stuck_index(index, obs_filter, base_lens, engine))


def filter_reads_for_coverage(fast5s_dir, corr_grp, frac_to_filter, engine=None):
    index = load_index(fast5s_dir, corr_grp)
    status_message('Filtering reads to obtain more uniform coverage.')
    new, _ = filter_reads_for_coverage_index(
        index, frac_to_filter, engine,
        before_draw=lambda counts: status_message(filter_message(
            *counts, fast5s_dir=fast5s_dir, filter_text='even coverage')))
    replace_index(fast5s_dir, corr_grp, new)


def filter_reads_for_qscore(fast5s_dir, bc_grp, corr_grp, q_score_thresh, open_fast5=None):
    _run(fast5s_dir, corr_grp, 'Filtering reads below a mean q-score cutoff.', 'q-score',
         lambda index: filter_reads_for_qscore_index(index, q_score_thresh,
                                                     fastq_q_score_accessor(bc_grp, open_fast5)))


def filter_reads_for_signal_matching(fast5s_dir, corr_grp, sig_match_thresh, open_fast5=None):
    _run(fast5s_dir, corr_grp, 'Filtering reads above a signal matching score threshold.', 'signal matching',
         lambda index: filter_reads_for_signal_matching_index(index, sig_match_thresh,
                                                              sig_match_score_accessor(open_fast5)))


def filter_reads_for_genome_pos(fast5s_dir, corr_grp, include_regs, include_partial=False):
    _run(fast5s_dir, corr_grp, 'Filtering reads outside of the specified genomic location.', 'genomic position',
         lambda index: filter_reads_for_genome_pos_index(index, include_regs, include_partial))

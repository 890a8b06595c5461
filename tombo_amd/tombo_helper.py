"""Interface types of the resquiggle hot path.

Own declarations of the namedtuples that make up the data contract of
`tombo.resquiggle.resquiggle_read()` -- field names and order follow the reference so a caller
can switch packages without touching its code:

  TomboError        /root/reference/tombo/tombo_helper.py:67
  alignInfo         tombo_helper.py:109      scaleValues       tombo_helper.py:160
  resquiggleParams  tombo_helper.py:173      stallParams       tombo_helper.py:207
  startClipParams   tombo_helper.py:217      resquiggleResults tombo_helper.py:229
  dpResults         tombo_helper.py:255      genomeLocation    tombo_helper.py:268
  channelInfo       tombo_helper.py:286      seqSampleType     tombo_helper.py:330
  get_seq_kmers     tombo_helper.py:526
  sequenceData      tombo_helper.py:277      comp_seq / rev_comp / invalid_seq /
  rev_transcribe / get_mean_q_score          tombo_helper.py:370-394
  get_raw_read_slot tombo_helper.py:1071     get_channel_info  tombo_helper.py:2071
"""
import io
import os
import re
import warnings
from collections import namedtuple
from itertools import islice

import numpy as np


class TomboError(Exception):
    """Expected (per-read) failure; the message string is the failure taxonomy."""


alignInfo = namedtuple('alignInfo', (
    'ID', 'Subgroup', 'ClipStart', 'ClipEnd', 'Insertions', 'Deletions', 'Matches',
    'Mismatches'))

scaleValues = namedtuple('scaleValues', (
    'shift', 'scale', 'lower_lim', 'upper_lim', 'outlier_thresh'))

resquiggleParams = namedtuple('resquiggleParams', (
    'match_evalue', 'skip_pen', 'bandwidth', 'max_half_z_score', 'running_stat_width',
    'min_obs_per_base', 'raw_min_obs_per_base', 'mean_obs_per_event', 'z_shift', 'stay_pen',
    'use_t_test_seg', 'band_bound_thresh', 'start_bw', 'start_save_bw', 'start_n_bases'))
resquiggleParams.__new__.__defaults__ = (None, None, None)

stallParams = namedtuple('stallParams', (
    'window_size', 'threshold', 'min_consecutive_obs', 'edge_buffer', 'lower_pctl',
    'upper_pctl', 'mini_window_size', 'n_windows'))
stallParams.__new__.__defaults__ = (None,) * 4

trimRnaParams = namedtuple('trimRnaParams', (
    'moving_window_size', 'min_running_values', 'thresh_scale', 'max_raw_obs'))

startClipParams = namedtuple('startClipParams', ('bandwidth', 'num_genome_bases'))

resquiggleResults = namedtuple('resquiggleResults', (
    'align_info', 'genome_loc', 'genome_seq', 'mean_q_score', 'raw_signal', 'channel_info',
    'read_start_rel_to_raw', 'segs', 'scale_values', 'sig_match_score', 'norm_params_changed',
    'start_clip_bases', 'stall_ints'))
resquiggleResults.__new__.__defaults__ = (None,) * 9

dpResults = namedtuple('dpResults', (
    'read_start_rel_to_raw', 'segs', 'ref_means', 'ref_sds', 'genome_seq'))

genomeLocation = namedtuple('genomeLocation', ('Start', 'Strand', 'Chrom'))

channelInfo = namedtuple('channelInfo', (
    'offset', 'range', 'digitisation', 'number', 'sampling_rate'))

seqSampleType = namedtuple('seqSampleType', ('name', 'rev_sig'))

sequenceData = namedtuple('sequenceData', ('seq', 'id', 'mean_q_score'))

PHRED_BASE = 33                      # _default_parameters.py:184
_COMPLEMENT = str.maketrans('ACGT', 'TGCA')
_NOT_ACGT = re.compile('[^ACGT]')


def comp_seq(seq):
    """complement of a DNA string (other characters pass through)"""
    return seq.translate(_COMPLEMENT)


def rev_comp(seq):
    return seq.translate(_COMPLEMENT)[::-1]


def invalid_seq(seq):
    """True when the sequence holds anything but A, C, G, T"""
    return _NOT_ACGT.search(seq) is not None


def rev_transcribe(seq):
    """RNA basecalls to the DNA alphabet (U -> T)"""
    return seq.replace('U', 'T')


def get_mean_q_score(read_q):
    """mean Phred score of a FASTQ quality string (np.mean of the per-base integers)"""
    return np.mean([q - PHRED_BASE for q in read_q.encode('ASCII')])


def get_raw_read_slot(fast5_data):
    """the (single) read group under /Raw/Reads of an open single-read FAST5"""
    try:
        return next(iter(fast5_data['/Raw/Reads'].values()))
    except KeyError:
        raise TomboError(
            'Raw data is not found in /Raw/Reads/Read_[read#]. Note that ' +
            'Tombo does not support multi-fast5 format.')


def get_channel_info(fast5_data):
    try:
        attrs = fast5_data['UniqueGlobalKey/channel_id'].attrs
    except KeyError:
        raise TomboError("No channel_id group in HDF5 file. " +
                         "Probably mux scan HDF5 file.")
    try:
        return channelInfo(attrs.get('offset'), attrs.get('range'), attrs.get('digitisation'),
                           attrs.get('channel_number'),
                           attrs.get('sampling_rate').astype(np.int64))
    except KeyError:
        raise TomboError("Channel info parameters not available.")


def get_seq_kmers(seq, kmer_width, rev_strand=False):
    """All overlapping k-mers of `seq` (reversed order for the reverse strand)."""
    kmers = [seq[i:i + kmer_width] for i in range(len(seq) - kmer_width + 1)]
    return kmers[::-1] if rev_strand else kmers


# ---- the Events table of a resquiggled read (compute part) -----------------
EVENTS_DTYPE = [(str('norm_mean'), 'f8'), (str('norm_stdev'), 'f8'), (str('start'), 'u4'),
                (str('length'), 'u4'), (str('base'), 'S1')]


def events_table(rsqgl_res, norm_means, norm_stds=None):
    """The structured array `write_new_fast5_group` stores as `Events`
    (tombo_helper.py:2341-2362): per base its normalised mean, standard deviation (NaN when
    `compute_sd` is off), start and length in raw samples and the base letter."""
    import numpy as np
    segs = np.asarray(rsqgl_res.segs, dtype=np.int64)
    n = segs.shape[0] - 1
    tab = np.empty(n, dtype=EVENTS_DTYPE)
    tab['norm_mean'] = norm_means
    tab['norm_stdev'] = np.nan if norm_stds is None else norm_stds
    tab['start'] = segs[:-1]
    tab['length'] = np.diff(segs)
    tab['base'] = np.frombuffer(rsqgl_res.genome_seq.encode(), dtype='S1')
    return tab


def get_event_data(rsqgl_res, compute_sd=True):
    """Events table of one finished read; the statistics come from the HIP kernels behind
    c_new_mean_stds / c_new_means."""
    from ._c_helper import c_new_mean_stds, c_new_means
    import numpy as np
    sig = np.ascontiguousarray(rsqgl_res.raw_signal, dtype=np.float64)
    segs = np.ascontiguousarray(rsqgl_res.segs, dtype=np.int64)
    if compute_sd:
        m, s = c_new_mean_stds(sig, segs)
        return events_table(rsqgl_res, m, s)
    return events_table(rsqgl_res, c_new_means(sig, segs))


# ---- what downstream Tombo commands read back: readData + index ------------
readData = namedtuple('readData', (
    'start', 'end', 'filtered', 'read_start_rel_to_raw', 'strand', 'fn', 'corr_group', 'rna',
    'sig_match_score', 'mean_q_score', 'read_id'))   # tombo_helper.py:127-158
readData.__new__.__defaults__ = (None, None, None)

# A resquiggled read as the statistics functions need it: the index record plus the two Events
# columns they load from the FAST5 file (`norm_mean`, `base`; tombo_helper.py:1593-1647), held in
# memory -- `means` / `seq` are read-centric (5'->3' of the read), like the table.
resquiggledRead = namedtuple('resquiggledRead', readData._fields + ('means', 'seq'))
resquiggledRead.__new__.__defaults__ = (None,) * 5

SINGLE_LETTER_CODE = {
    'A': 'A', 'C': 'C', 'G': 'G', 'T': 'T', 'B': '[CGT]', 'D': '[AGT]', 'H': '[ACT]',
    'K': '[GT]', 'M': '[AC]', 'N': '[ACGT]', 'R': '[AG]', 'S': '[CG]', 'V': '[ACG]',
    'W': '[AT]', 'Y': '[CT]'}   # tombo_helper.py:54-58


class TomboMotif(object):
    """Sequence motif with the (1-based) modified position (tombo_helper.py:542-707): `motif_pat`,
    `rev_comp_pat`, `is_palindrome`, `motif_len`, `mod_pos`, `mod_base`; with a modified position
    also `find_mod_poss` and `matches_seq`, which count partial matches at either end of a
    sequence as long as they hold the modified position."""

    @staticmethod
    def _parse_motif(raw_motif, rev_comp_motif=False):
        conv = ''.join(SINGLE_LETTER_CODE[c] for c in raw_motif)
        if rev_comp_motif:   # reverse complement, then the group brackets the right way round again
            conv = rev_comp(conv).translate({ord('['): ']', ord(']'): '['})
        return re.compile(conv)

    def __init__(self, raw_motif, mod_pos=None):
        bad = [c for c in raw_motif if c not in SINGLE_LETTER_CODE]
        if bad:
            raise ValueError('Invalid characters in motif: ' + ', '.join(bad))
        self.raw_motif = raw_motif
        self.motif_len = len(raw_motif)
        self.motif_pat = self._parse_motif(raw_motif)
        self.rev_comp_pat = self._parse_motif(raw_motif, True)
        self.is_palindrome = self.motif_pat == self.rev_comp_pat
        self.mod_pos = mod_pos
        self.mod_base = None if mod_pos is None else raw_motif[mod_pos - 1]
        if mod_pos is not None:
            assert 0 < mod_pos <= self.motif_len
            # partial patterns that still hold mod_pos: by length, (pattern, mod_pos inside it) for a
            # sequence start, a sequence end, and (a list) for a sequence shorter than the motif
            L, mp = self.motif_len, mod_pos
            self._partial_pats = {
                'start': dict((L - o - 1, (self._parse_motif(raw_motif[o + 1:]), mp - o - 1)) for o in range(mp - 1)),
                'end': dict((L - o - 1, (self._parse_motif(raw_motif[:-(o + 1)]), mp)) for o in range(L - mp)),
                'short': dict((n, [(self._parse_motif(raw_motif[o:o + n]), mp - o)
                                   for o in range(max(0, mp - n), min(L - n + 1, mp))]) for n in range(1, L))}

    def _iter_partial(self, seq):
        """(where, matched length, mod_pos in the pattern, match start) of every full or partial match"""
        for n in range(1, min(len(seq) + 1, self.motif_len)):
            if n in self._partial_pats['start'] and self._partial_pats['start'][n][0].match(seq[:n]):
                yield self._partial_pats['start'][n][1]
        if len(seq) < self.motif_len:
            for pat, mp in self._partial_pats['short'].get(len(seq), ()):
                if pat.match(seq):
                    yield mp
        else:
            for m in self.motif_pat.finditer(seq):
                yield m.start() + self.mod_pos
        for n in range(1, min(len(seq) + 1, self.motif_len)):
            if n in self._partial_pats['end'] and self._partial_pats['end'][n][0].match(seq[-n:]):
                yield len(seq) - n + self._partial_pats['end'][n][1]

    def find_mod_poss(self, seq):
        """sorted 1-based positions of the modified base in `seq` (tombo_helper.py:672-707)"""
        return sorted(set(self._iter_partial(seq)))

    def matches_seq(self, seq):
        """does the motif match `seq` with the modified position inside it? (tombo_helper.py:637-670)"""
        return next(self._iter_partial(seq), None) is not None


_MOTIF_DESCS_MSG = ('Invalid motif decriptions format. Format descriptions as: '
                    '"motif:mod_pos:name[::motif2:mod_pos2:name2...]".')


def parse_motif_descs(stat_motif_descs):
    """`--motif-descriptions` text -> [(TomboMotif, name), ...] (tombo_helper.py:710-730); the reference's
    message, which it prints before exiting, is raised as a TomboError"""
    parsed_motif_descs = []
    try:
        for motif_desc in stat_motif_descs.split('::'):
            raw_motif, mod_pos, mod_name = motif_desc.split(':')
            parsed_motif_descs.append((TomboMotif(raw_motif, int(mod_pos)), mod_name))
    except Exception:
        raise TomboError(_MOTIF_DESCS_MSG)
    return parsed_motif_descs


def parse_locs_file(locs_fn):
    """BED file of single-base locations -> {(chrm, strand): sorted positions} (tombo_helper.py:475-506: the
    0-based start column is the position, the end column is ignored, repeated lines count once)"""
    n_added, n_failed = 0, 0
    raw_locs = {}
    with open(locs_fn) as locs_fp:
        for line in locs_fp:
            try:
                chrm, pos, _, _, _, strand = line.split()[:6]
                pos = int(pos)
            except ValueError:
                n_failed += 1
                continue
            raw_locs.setdefault((chrm, strand), set()).add(pos)
            n_added += 1
    if n_failed > 0:
        if n_added > 0:
            warnings.warn(('Some provided locations ({}) were incorrectly formatted. ' +
                           'Ensure that provided file ({}) is in BED format.').format(n_failed, locs_fn))
        else:
            warnings.warn(('All provided locations from {} were incorrectly formatted. ' +
                           'Ensure that provided file is in BED format.').format(locs_fn))
    return dict((cs, np.array(sorted(cs_poss))) for cs, cs_poss in raw_locs.items())


def parse_genome_regions(all_regs_text):
    """`--include-regions` texts ('chrm' or 'chrm:start-end', commas allowed in the numbers) -> {chrm: [[start,
    end], ...], or None for a chromosome named whole anywhere} (tombo_helper.py:447-473); the message the
    reference prints before exiting is raised as a TomboError"""
    parsed_regs, include_whole_chrms = {}, set()
    for reg_text in all_regs_text:
        try:
            chrm_reg = reg_text.replace('"', '').replace("'", "").split(':')
            if len(chrm_reg) == 1:
                chrm, reg_pos = chrm_reg[0], None
                include_whole_chrms.add(chrm)
            elif len(chrm_reg) == 2:
                chrm, reg_pos = chrm_reg
                reg_pos = [int(x.replace(',', '')) for x in reg_pos.split('-')]
            else:
                raise TomboError('Invalid region text provided.')
        except Exception:
            raise TomboError('Invalid [--include-region] format.')
        parsed_regs.setdefault(chrm, []).append(reg_pos)
    for chrm in include_whole_chrms:
        parsed_regs[chrm] = None
    return parsed_regs


def parse_obs_filter(obs_filter):
    """`--obs-per-base-filter` texts ('pctl:thresh', integers) -> [[pctl, thresh], ...], None for no text
    (tombo_helper.py:508-524); a percentile outside [0, 100] is the reference's exit, raised here"""
    if len(obs_filter) < 1:
        return None
    try:
        obs_filter = [[int(v) for v in pctl_nobs.split(':')] for pctl_nobs in obs_filter]
    except Exception:
        raise TomboError('Invalid format for observation filter')
    if any(pf[0] < 0 or pf[0] > 100 for pf in obs_filter):
        raise TomboError('Invalid percentile value.')
    return obs_filter


class Fasta(object):
    """A FASTA file held in memory (tombo_helper.py:744-865, the branch without pyfaidx; `force_in_mem` is
    accepted for the reference's call sites and changes nothing).  Sequence is upper-cased and, when the first
    records hold uridines, converted to the DNA alphabet."""

    def _load_in_mem(self):
        genome_index, curr_id, curr_seq = {}, None, []
        with io.open(self.fasta_fn) as fasta_fp:
            for line in fasta_fp:
                if line.startswith('>'):
                    if curr_id is not None:
                        genome_index[curr_id] = ''.join(curr_seq)
                    curr_seq = []
                    curr_id = line.replace('>', '').split()[0]
                else:
                    curr_seq.append(line.strip())
            if curr_id is not None:
                genome_index[curr_id] = ''.join(curr_seq)
        return genome_index

    def _index_contains_uridines(self, n_chrms=10, n_bases=1000):
        return any(re.search('U', self.get_seq(chrm, 1, n_bases, error_end=False))
                   for chrm in islice(self.index.keys(), n_chrms))

    def __init__(self, fasta_fn, dry_run=False, force_in_mem=True, assume_dna_base=False):
        self.fasta_fn = os.path.realpath(os.path.expanduser(fasta_fn))
        self.has_rna_bases = False
        self.has_pyfaidx = False
        if not dry_run:
            self.index = self._load_in_mem()
            # (the reference's expression, :810-811)
            self.has_rna_bases = assume_dna_base or self._index_contains_uridines()

    def get_seq(self, chrm, start=None, end=None, error_end=True):
        """bases [start, end) of `chrm`, 0-based; a start outside the chromosome, or with error_end an end outside
        it, raises TomboError"""
        if (start is not None and (start < 0 or start > len(self.index[chrm]))) or (
                error_end and end is not None and (end < 0 or end > len(self.index[chrm]))):
            raise TomboError('Encountered invalid genome sequence request.')
        r_seq = self.index[chrm][start:end].upper()
        if self.has_rna_bases:
            r_seq = rev_transcribe(r_seq)
        return r_seq

    def iter_chrms(self):
        for chrm in self.index:
            yield chrm

    def __contains__(self, chrm):
        return chrm in self.index


def read_from_results(rsqgl_res, norm_means, fn=None, corr_group='RawGenomeCorrected_000',
                      rna=False, read_id=None, filtered=False):
    """`resquiggledRead` of a finished read: the index fields `_resquiggle_worker` records
    (resquiggle.py:1591-1600 -> tombo_helper.py:1169-1176) plus the Events columns the statistics
    read back.  `norm_means`: per-base means (tba_batch_base_stats / get_event_data)."""
    start = rsqgl_res.genome_loc.Start
    return resquiggledRead(
        start=start, end=start + len(rsqgl_res.segs) - 1, filtered=filtered,
        read_start_rel_to_raw=rsqgl_res.read_start_rel_to_raw,
        strand=rsqgl_res.genome_loc.Strand, fn=fn,
        corr_group=corr_group + '/' + rsqgl_res.align_info.Subgroup, rna=rna,
        sig_match_score=rsqgl_res.sig_match_score, mean_q_score=rsqgl_res.mean_q_score,
        read_id=read_id if read_id is not None else rsqgl_res.align_info.ID,
        means=norm_means, seq=rsqgl_res.genome_seq)


def index_entry(rd, basedir=''):
    """The tuple `TomboReads._write_index` pickles per read (tombo_helper.py:1169-1183):
    (fn relative to the base directory, start, end, read_start_rel_to_raw, corrected group,
    basecall subgroup, filtered, rna, sig_match_score, mean_q_score, read_id)."""
    fn = rd.fn or ''
    if basedir and fn.startswith(basedir):
        fn = fn[len(basedir):]
    grp = rd.corr_group.split('/')
    return (fn, rd.start, rd.end, rd.read_start_rel_to_raw, grp[0], grp[-1], rd.filtered, rd.rna,
            rd.sig_match_score, rd.mean_q_score, rd.read_id)


def write_index(reads_by_chrm_strand, index_fn, basedir=''):
    """Tombo index file: pickle (protocol 2) of {(chrm, strand): [index_entry, ...]}
    (tombo_helper.py:1160-1187)."""
    import pickle
    data = dict((cs, [index_entry(rd, basedir) for rd in rds])
                for cs, rds in reads_by_chrm_strand.items())
    with open(index_fn, 'wb') as fp:
        pickle.dump(data, fp, protocol=2)
    return data


def read_index(index_fn, basedir=''):
    """{(chrm, strand): [readData, ...]} from a Tombo index file (inverse of `write_index`;
    the reference's parser: tombo_helper.py:1226-1260)."""
    import pickle
    with open(index_fn, 'rb') as fp:
        data = pickle.load(fp)
    out = {}
    for (chrm, strand), recs in data.items():
        out[(chrm, strand)] = [
            readData(start=s, end=e, filtered=flt, read_start_rel_to_raw=rsr, strand=strand,
                     fn=basedir + fn, corr_group=cg + '/' + sub, rna=rna, sig_match_score=sms,
                     mean_q_score=mq, read_id=rid)
            for fn, s, e, rsr, cg, sub, flt, rna, sms, mq, rid in recs]
    return out


# The on-disk layout of a resquiggled read (tombo_helper.py:2341-2460; docs/resquiggle.rst:172-194)
# as DATA: (attribute name, getter, written only when not None).  Names and order are the format.
_SUBGROUP_ATTRS = (
    ('status', lambda r, x: 'success', False),
    ('rna', lambda r, x: x['rna'], False),
    ('signal_match_score', lambda r, x: r.sig_match_score, True),
    ('shift', lambda r, x: r.scale_values.shift, False),
    ('scale', lambda r, x: r.scale_values.scale, False),
    ('norm_type', lambda r, x: x['norm_type'], False),
    ('lower_lim', lambda r, x: r.scale_values.lower_lim, True),
    ('upper_lim', lambda r, x: r.scale_values.upper_lim, True),
    ('outlier_threshold', lambda r, x: r.scale_values.outlier_thresh, True),
)
_ALIGNMENT_ATTRS = (
    ('mapped_start', lambda r: r.genome_loc.Start),
    ('mapped_end', lambda r: r.genome_loc.Start + len(r.segs) - 1),
    ('mapped_strand', lambda r: r.genome_loc.Strand),
    ('mapped_chrom', lambda r: r.genome_loc.Chrom),
)
_ALIGN_INFO_ATTRS = (   # only when the read carries an alignInfo
    ('clipped_bases_start', 'ClipStart'), ('clipped_bases_end', 'ClipEnd'),
    ('num_insertions', 'Insertions'), ('num_deletions', 'Deletions'),
    ('num_matches', 'Matches'), ('num_mismatches', 'Mismatches'),
)


# the Tombo release whose FAST5 layout this writer follows (the reference stamps its own version
# into the corrected group, tombo_helper.py:2311)
TOMBO_VERSION = '1.5.1'


def prep_fast5_data(fast5_data, corr_grp, overwrite, bc_grp=None):
    """`prep_fast5` (tombo_helper.py:2259-2324) on an OPEN, writable FAST5 object: the checks the
    reference makes before it spends any compute on a read.  The basecalls must be there; an
    existing corrected group is an error unless `overwrite` (then it is deleted); the corrected
    group is created with its `tombo_version` / `basecall_group` attributes.  Returns None, or
    the reference's message for the failed-reads list (always a "Tombo error")."""
    try:
        try:
            analyses = fast5_data['/Analyses']
            if bc_grp is not None:
                analyses[bc_grp]
        except Exception:
            return 'Base calls not found in FAST5 (see `tombo preprocess`)'
        try:
            analyses[corr_grp]
            exists = True
        except Exception:
            exists = False
        if exists:
            if not overwrite:
                return 'Tombo data exists in [--corrected-group] and [--overwrite] is not set'
            del analyses[corr_grp]
        grp = analyses.create_group(corr_grp)
        grp.attrs['tombo_version'] = TOMBO_VERSION
        grp.attrs['basecall_group'] = bc_grp
    except Exception:
        return 'Error opening or writing to fast5 file'
    return None


def write_error_status_data(fast5_data, corr_grp, bc_subgrp, error_text):
    """`write_error_status` (tombo_helper.py:2326-2339) on an open FAST5 object: the message of a
    failed read as the `status` attribute of its corrected (sub)group."""
    grp = fast5_data['/Analyses'][corr_grp]
    if bc_subgrp is not None:
        grp = grp.create_group(bc_subgrp)
    grp.attrs['status'] = error_text


def write_new_fast5_group(fast5_data, corr_grp_slot, rsqgl_res, norm_type, compute_sd,
                          alignVals=None, old_segs=None, rna=False, event_data=None):
    """Write a resquiggled read into an open FAST5 file: the groups, attributes and `Events`
    dataset of the tables above (the reference's writer: tombo_helper.py:2341-2460).
    `fast5_data` is anything with the h5py group interface (`__getitem__`, `create_group`,
    `create_dataset`, `.attrs`): an `h5py.File` where h5py is installed, or an in-memory stand-in
    (the image this engine is built in has no HDF5 library; tests use a dict-backed group and
    compare the tree with the one the reference's own writer leaves on it).
    `event_data`: the Events table if already computed on the device
    (`resquiggle_batch_events`), else it is computed here through the HIP kernels."""
    import numpy as np
    try:
        if event_data is None:
            event_data = get_event_data(rsqgl_res, compute_sd)
        datasets = []
        if alignVals is not None:
            for name, col in zip(('read_alignment', 'genome_alignment'), zip(*alignVals)):
                datasets.append((name, np.array(col, dtype='S1')))
        if old_segs is not None:
            datasets.append(('read_segments', old_segs))
    except Exception:
        raise TomboError('Error computing new events')
    try:
        sub = fast5_data['/Analyses'][corr_grp_slot].create_group(rsqgl_res.align_info.Subgroup)
        ctx = dict(rna=rna, norm_type=norm_type)
        for name, get, optional in _SUBGROUP_ATTRS:
            value = get(rsqgl_res, ctx)
            if not (optional and value is None):
                sub.attrs[name] = value
        aln = sub.create_group('Alignment')
        for name, get in _ALIGNMENT_ATTRS:
            aln.attrs[name] = get(rsqgl_res)
        if rsqgl_res.align_info is not None:
            for name, field in _ALIGN_INFO_ATTRS:
                aln.attrs[name] = getattr(rsqgl_res.align_info, field)
        for name, data in datasets:
            aln.create_dataset(name, data=data, compression='gzip')
        ev = sub.create_dataset('Events', data=event_data, compression='gzip')
        ev.attrs['read_start_rel_to_raw'] = rsqgl_res.read_start_rel_to_raw
    except Exception:
        raise TomboError('Error writing resquiggle information back into fast5 file.')
    return event_data


# ---- group statistics over a pileup of reads (level_sample_compare) ---------------------------
groupStats = namedtuple('groupStats', (
    'reg_stats', 'reg_poss', 'chrm', 'strand', 'start', 'reg_cov', 'ctrl_cov'))   # tombo_helper.py:315-317

class regionStats(namedtuple('regionStats', (
        'reg_frac_standard_base', 'reg_poss', 'chrm', 'strand', 'start', 'reg_cov', 'ctrl_cov',
        'valid_cov'))):
    """Per-site statistics of one region and statistic name (tombo_helper.py:299-301).
    `compute_reg_stats_batch(..., cov_damp_counts=...)` also sets the attribute `damp_frac` (the
    dampened fractions, computed on the device)."""


INVALID_BASE_RUNS = re.compile('[^ACGT]+')


class regionData(object):
    """A genomic region with its reads (the part of the reference's intervalData the statistics
    read): `reads` are `resquiggledRead`s (genomic `start`, `strand`, read-centric `means`);
    `seq`: the genome sequence the prior blend of get_reads_ref needs, over the region extended
    by fm_offset and the k-mer lags.  Any object with these attributes works."""

    def __init__(self, chrm, strand, start, end, reads, seq=None):
        self.chrm, self.strand, self.start, self.end = chrm, strand, int(start), int(end)
        self.reads, self.seq = reads, seq


def _region_seq_add_read(rd, start, end, bases):
    """one read's bases into the interval's list (intervalData._update_seq, tombo_helper.py:1891-1926) ->
    (bases, covered-so-far).  The slices are the reference's, taken as Python takes them: a read that lies
    outside the interval moves or resizes the list exactly as it does there."""
    if rd.seq is None:
        return bases, max(0, rd.start - start)
    r_seq = rev_comp(rd.seq) if rd.strand == '-' else rd.seq
    if rd.start <= start:
        overlap = rd.end - start
        if rd.end > end:    # the read covers the interval: its slice IS the sequence
            bases = r_seq[-overlap:-(rd.end - end)]
            return bases, len(bases)
        bases[:overlap] = r_seq[-overlap:]
        return bases, overlap
    if rd.end > end:
        overlap = end - rd.start
        bases[-overlap:] = r_seq[:overlap]
        return bases, len(bases)
    r_len, at = rd.end - rd.start, rd.start - start
    bases[at:at + r_len] = r_seq
    return bases, at + r_len


def get_region_seq(reads, start, end):
    """The forward-strand sequence of [start, end) from the reads alone: the reads-only branch of
    intervalData.add_seq (tombo_helper.py:1928-1975).

    The reads are sorted on (start, end).  The first one gives its bases.  Then the reads are walked in
    order, keeping as candidate the one that ends furthest; each time a read's start is at or past the
    covered count, the candidate gives its bases and that read becomes the candidate.  The last candidate
    gives its bases at the end.  A later read writes over an earlier one where they overlap.

    The reference compares the read's GENOMIC start with the covered count, which is relative to the
    interval; that comparison is kept as it is.  Positions no read fills stay '-', so an uncovered flank
    reads '-'.  A minus-strand read gives the reverse complement of its `seq`.  The reads are those of the
    whole region; one that misses the interval is handled as the reference handles it (see
    _region_seq_add_read)."""
    bases = ['-'] * (end - start)
    if reads is None or len(reads) == 0:
        return ''.join(bases)
    rest = sorted(reads, key=lambda r: (r.start, r.end))
    bases, covered = _region_seq_add_read(rest.pop(0), start, end, bases)
    if len(rest) == 0 or covered >= end - start:
        return ''.join(bases)
    curr = rest.pop(0)
    for nxt in rest:
        if nxt.start >= covered:
            bases, covered = _region_seq_add_read(curr, start, end, bases)
            curr = nxt
            if covered >= end - start:
                return ''.join(bases)
            continue
        if nxt.end > curr.end:
            curr = nxt
    bases, _ = _region_seq_add_read(curr, start, end, bases)
    return ''.join(bases)


def get_unique_intervals(plot_intervals, covered_poss=None, num_regions=None):
    """The regions, in order, that do not start inside a region kept before them and, with covered_poss
    ({(chrm, strand): container of positions}), lie on covered positions only; at most num_regions
    (tombo_helper.py:2045-2064).  Regions are the (chrm, start, end, strand, ...) tuples of
    ModelStats.get_most_signif_regions."""
    uniq_p_intervals, used_intervals = [], {}
    for reg_data in plot_intervals:
        chrm, start, end, strand = reg_data[:4]
        interval_poss = list(range(start, end))
        used = used_intervals.setdefault((chrm, strand), set())
        if start not in used and (covered_poss is None or all(
                pos in covered_poss[(chrm, strand)] for pos in interval_poss)):
            uniq_p_intervals.append(reg_data)
            used.update(interval_poss)
        if num_regions is not None and len(uniq_p_intervals) >= num_regions:
            break
    return uniq_p_intervals


class intervalData(object):
    """A genome / transcriptome interval with its reads and sequence (tombo_helper.py:1749-2032): the regions the
    plot data frames of tombo_amd/plot_commands.py are made from.  Every method returns the object, so calls chain
    (`int_data.add_reads(reads_index).add_seq()`).  Reads are in-memory objects with `start`, `end`, `strand`,
    read-centric `means` and, for add_seq without a genome, `seq`."""

    def __setattr__(self, name, value):
        if name == 'chrm':
            if not isinstance(value, str):
                raise TypeError(name + ' must be a string')
        elif name in ('start', 'end'):
            if not isinstance(value, (int, np.integer)):
                raise TypeError(name + ' must be an int')
        elif name == 'strand':
            if value not in (None, '+', '-'):
                raise TypeError('strand must be either None, "+", or "-"')
        elif name in ('reg_id', 'reg_text', 'seq'):
            if value is not None and not isinstance(value, str):
                raise TypeError(name + ' must be a string')
        elif name == 'reads':
            if value is not None and not isinstance(value, list):
                raise TypeError('reads must be a list')
        else:
            raise ValueError(name + ' is an invalid attribute for intervalData')
        super(intervalData, self).__setattr__(name, value)

    def __init__(self, chrm, start, end, strand=None, reg_id=None, reg_text='', reads=None, seq=None):
        self.chrm = str(chrm)
        self.start = start
        self.end = end
        self.strand = str(strand) if strand is not None else None
        self.reg_id = str(reg_id) if reg_id is not None else None
        self.reg_text = str(reg_text)
        self.reads = reads
        self.seq = seq

    def update(self, **kwargs):
        for k, v in kwargs.items():
            self.__setattr__(k, v)
        return self

    def copy(self, include_reads=True):
        return type(self)(self.chrm, self.start, self.end, self.strand, self.reg_id, self.reg_text,
                          self.reads if include_reads else None, self.seq)

    def merge(self, other_reg):
        """a copy with the reads of this interval followed by those of other_reg; all else is this interval's"""
        return self.copy().update(reads=(self.reads if self.reads is not None else []) +
                                  (other_reg.reads if other_reg.reads is not None else []))

    def expand_interval(self, expand_width):
        """start and end only; not seq or reads"""
        return self.update(start=self.start - expand_width, end=self.end + expand_width)

    def add_reads(self, reads_index, require_full_span=False):
        """the reads of reads_index ({(chrm, strand): [reads]}) that overlap the interval, or with require_full_span
        span it (:1860-1889); without a strand the plus reads, then the minus reads"""
        def get_c_s_data(strand):
            if require_full_span:
                return [rd for rd in reads_index.get((self.chrm, strand), [])
                        if rd.start <= self.start and rd.end >= self.end]
            return [rd for rd in reads_index.get((self.chrm, strand), [])
                    if not (rd.start >= self.end or rd.end <= self.start)]
        if self.strand is not None:
            return self.update(reads=get_c_s_data(self.strand))
        return self.update(reads=get_c_s_data('+') + get_c_s_data('-'))

    def add_seq(self, genome_index=None, error_end=True):
        """the forward-strand sequence from genome_index (a Fasta), else from the reads (get_region_seq)"""
        if genome_index is not None:
            return self.update(seq=genome_index.get_seq(self.chrm, self.start, self.end, error_end=error_end))
        return self.update(seq=get_region_seq(self.reads, self.start, self.end))

    def get_base_levels(self, read_rows=False, num_reads=None, engine=None):
        """float64[end - start, reads] (read_rows: transposed) of genome-centric levels, NaN where a read does not
        cover a position (:1976-2032).  With num_reads, `self.reads` is shuffled in place (np.random.shuffle) and the
        first num_reads usable reads are taken.  Reads of the other strand and reads without levels are skipped.
        The reference's four overlap branches place, for every read that overlaps the interval, the read's levels at
        the positions it covers; that is what is built here.  The matrix is a copy of slices without arithmetic, so
        it is made on the host; `engine` is accepted so that every plot-data call takes one, and is not used."""
        if self.reads is None or len(self.reads) == 0:
            raise TomboError('Must annotate region with reads (see `TomboInterval.add_reads`) to extract base levels.')
        if num_reads is not None:
            np.random.shuffle(self.reads)
        reg_events = []
        for rd in self.level_reads():
            r_means = np.asarray(rd.means, dtype=np.float64)
            if rd.strand == '-':
                r_means = r_means[::-1]
            r_reg_means = np.full(self.end - self.start, np.nan)
            lo, hi = max(rd.start, self.start), min(rd.end, self.end)
            if lo < hi:
                r_reg_means[lo - self.start:hi - self.start] = r_means[lo - rd.start:hi - rd.start]
            reg_events.append(r_reg_means)
            if num_reads is not None and len(reg_events) >= num_reads:
                break
        return np.vstack(reg_events) if read_rows else np.column_stack(reg_events)

    def level_reads(self):
        """the reads get_base_levels takes columns from, in order: the interval's strand, with levels"""
        return [rd for rd in self.reads if (self.strand is None or rd.strand == self.strand) and rd.means is not None]


def filter_empty_regions(plot_intervals):
    """the intervals that have reads (tombo_helper.py:2035-2043); none left is the reference's exit, raised here"""
    num_filt = sum(len(p_int.reads) == 0 for p_int in plot_intervals)
    plot_intervals = [p_int for p_int in plot_intervals if len(p_int.reads) > 0]
    if len(plot_intervals) == 0:
        raise TomboError('No reads in any selected regions.')
    if num_filt > 0:
        warnings.warn('Some selected regions contain no reads.')
    return plot_intervals


# ---- genome tracks: coverage, mean signal / SD / dwell per position, sample - control ---------
# (text_output browser_files, iter_cov_regs, get_largest_signal_differences; the pileup kernels
# are csrc/k_tracks.h).  A `reads_index` is the {(chrm, strand): [reads]} mapping `read_index`
# returns; the reads are `resquiggledRead`s or any objects with `start`, `end`, `strand`, `means`.
# Where the reference opens the FAST5 file of a read for an Events column, the column is taken
# from memory: `norm_mean` defaults to `rd.means`, `norm_stdev` and `length` come from `slots`.
TRACK_SLOTS = ('norm_mean', 'norm_stdev', 'length')


def _tracks_engine(engine=None):
    if engine is not None:
        return engine
    from . import resquiggle as rq
    return rq.get_engine()


def _cs_slots(slots, chrm_strand):
    """reads_index-level `slots` ({(chrm, strand): per-list mapping}, or one mapping by read_id for all
    reads) -> the mapping of one (chrm, strand)"""
    if slots is None:
        return None
    if isinstance(slots, dict) and chrm_strand in slots:
        return slots[chrm_strand]
    return slots


def _read_slot(rd, i, slot_name, slots):
    """read-centric `slot_name` of read i of a list, or None (no Events table).  slots: a sequence by position in
    the list, or a mapping by `read_id` or by position"""
    if slots is None:
        if slot_name != 'norm_mean':
            raise ValueError('slot %s needs `slots`: only norm_mean is kept on the reads' % slot_name)
        return getattr(rd, 'means', None)
    if isinstance(slots, dict):
        rid = getattr(rd, 'read_id', None)
        return slots[rid] if rid is not None and rid in slots else slots.get(i)
    return slots[i]


def build_tile_lists(starts, ends, win_start, win_end, tile):
    """Per tile of `tile` positions of the window [win_start, win_end) the reads [starts, ends) that overlap it, in
    input order, in CSR form -> (tile_read_off int64[n_tiles + 1], tile_reads int32).  Vectorised: the (tile, read)
    pairs read by read, then a stable sort by tile."""
    starts, ends = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    n_tiles = -(-(win_end - win_start) // tile)
    lo, hi = np.clip(starts, win_start, win_end) - win_start, np.clip(ends, win_start, win_end) - win_start
    t0 = lo // tile
    cnt = np.where(hi > lo, (hi - 1) // tile - t0 + 1, 0)
    first = np.cumsum(cnt) - cnt
    total = int(cnt.sum())
    reads = np.repeat(np.arange(starts.shape[0], dtype=np.int64), cnt)
    tiles = np.repeat(t0 - first, cnt) + np.arange(total, dtype=np.int64)
    order = np.argsort(tiles, kind='stable')
    off = np.zeros(n_tiles + 1, dtype=np.int64)
    np.cumsum(np.bincount(tiles, minlength=n_tiles), out=off[1:])
    return off, reads[order].astype(np.int32)


class GenomeTracks(object):
    """Per (chromosome, strand) the per-position mean of up to three Events columns over all reads, the number of
    reads behind each mean and the read coverage, computed on the device.

        tracks = GenomeTracks(chrm_sizes, slots=('norm_mean', 'norm_stdev', 'length'))
        tracks.add_reads(chrm, strand, reads, slots={'norm_stdev': [...], 'length': [...]})   # any number of times
        res = tracks.finish()    # {(chrm, strand): TrackSet(means, sums, slot_cov, read_cov)}, arrays of chrm_sizes[chrm]

    add_reads takes batches straight from `read_from_results`; per batch it gathers the reads' arrays (the only
    per-read Python loop) and keeps them.  finish() feeds every (chromosome, strand) to the engine batch by batch,
    in the order the batches came: the device sums stay resident between the batches, and the result has the bits
    of the reference's loop over the reads in that order, however the reads were cut into batches.  A chromosome
    longer than `max_window` is cut into windows on the host (a read that crosses a cut is given to both sides);
    the result does not depend on where the cuts fall.
    slots of add_reads: {slot_name: sequence by position in `reads`, or mapping by read_id / position}; norm_mean
    defaults to `rd.means`.  A read whose column is None (no Events table) is left out of that column's sum and
    coverage and stays in the read coverage.  All columns of a read have one length; `length` (uint32) is added as
    float64, which is exact.  slots=() computes the read coverage alone."""

    def __init__(self, chrm_sizes, slots=('norm_mean',), engine=None, max_window=1 << 26):
        from ._native import TRK_TILE
        slots = tuple(slots)
        if len(slots) > 3 or any(s not in TRACK_SLOTS for s in slots) or len(set(slots)) != len(slots):
            raise ValueError('slots: up to three different names out of %s' % (TRACK_SLOTS,))
        if int(max_window) != max_window or max_window < 1:
            raise ValueError('max_window must be a positive integer')
        self.chrm_sizes, self.slots, self.engine, self.max_window = dict(chrm_sizes), slots, engine, int(max_window)
        self.tile = TRK_TILE
        self._batches = {}      # (chrm, strand) -> [(start, end, flags, off, [values per slot])]
        self.timing = {'lists_s': 0.0, 'engine_s': 0.0, 'kernel_ms': 0.0}

    def add_reads(self, chrm, strand, reads, slots=None):
        if chrm not in self.chrm_sizes:
            raise ValueError('chromosome %r is not in chrm_sizes' % (chrm,))
        slots = slots or {}
        n, ns = len(reads), len(self.slots)
        start, end = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        flags, lens = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int64)
        cols = [[] for _ in range(ns)]
        for i, rd in enumerate(reads):
            start[i], end[i] = rd.start, rd.end
            if rd.strand == '-':
                flags[i] |= 1
            vals = [_read_slot(rd, i, name, slots.get(name)) for name in self.slots]
            have = [v for v in vals if v is not None]
            if have:
                lens[i] = len(have[0])
                if any(len(v) != lens[i] for v in have):
                    raise ValueError('read %d: its slots differ in length' % i)
            for s, v in enumerate(vals):
                if v is None:
                    cols[s].append(None)
                else:
                    flags[i] |= 2 << s
                    cols[s].append(np.asarray(v, dtype=np.float64))
        if n and ((end < start).any() or (start < 0).any() or (end > self.chrm_sizes[chrm]).any() or
                  (start + lens > self.chrm_sizes[chrm]).any()):
            raise ValueError('a read lies outside [0, chrm_sizes[%r])' % (chrm,))
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        values = []
        for s in range(ns):
            v = np.zeros(int(off[-1]), dtype=np.float64)    # (a read without this slot keeps zeros nobody reads)
            for i, c in enumerate(cols[s]):
                if c is not None:
                    v[off[i]:off[i + 1]] = c
            values.append(v)
        self._batches.setdefault((chrm, strand), []).append((start, end, flags, off, values))
        return self

    def _window(self, eng, batches, ws, we, want_sums):
        import time
        eng.tracks_begin(ws, we, max(len(self.slots), 1))
        for start, end, flags, off, values in batches:
            t0 = time.perf_counter()
            reach = np.maximum(end, start + np.diff(off))
            sel = np.flatnonzero((reach > ws) & (start < we))
            if sel.shape[0] < start.shape[0]:       # the reads of this window only, repacked
                ln = np.diff(off)[sel]
                noff = np.zeros(sel.shape[0] + 1, dtype=np.int64)
                np.cumsum(ln, out=noff[1:])
                idx = np.repeat(off[sel] - noff[:-1], ln) + np.arange(int(noff[-1]), dtype=np.int64)
                start, end, flags, off, values = start[sel], end[sel], flags[sel], noff, [v[idx] for v in values]
                reach = reach[sel]
            toff, treads = build_tile_lists(start, reach, ws, we, self.tile)
            t1 = time.perf_counter()
            eng.tracks_add(start, end, flags, off, values or [np.zeros(int(off[-1]))], toff, treads)
            self.timing['lists_s'] += t1 - t0
            self.timing['engine_s'] += time.perf_counter() - t1
        t1 = time.perf_counter()
        res = eng.tracks_finish(want_sums=want_sums)
        self.timing['engine_s'] += time.perf_counter() - t1
        if hasattr(eng, 'tracks_kernel_ms'):
            self.timing['kernel_ms'] += eng.tracks_kernel_ms()
        return res

    def finish(self, want_sums=False):
        """-> {(chrm, strand): TrackSet}: means / sums (None unless want_sums) / slot_cov [len(slots), chrm size],
        read_cov [chrm size]"""
        from ._native import TrackSet
        eng, out, ns = _tracks_engine(self.engine), {}, len(self.slots)
        for (chrm, strand), batches in self._batches.items():
            size = int(self.chrm_sizes[chrm])
            parts = [self._window(eng, batches, ws, min(ws + self.max_window, size), want_sums)
                     for ws in range(0, size, self.max_window)]
            if not parts:
                z = np.zeros((ns, 0))
                parts = [TrackSet(z, z if want_sums else None, z.astype(np.int64), np.zeros(0, dtype=np.int64))]
            cat = (lambda xs: xs[0] if len(xs) == 1 else np.concatenate(xs, axis=-1))
            out[(chrm, strand)] = TrackSet(
                cat([p.means for p in parts])[:ns], cat([p.sums for p in parts])[:ns] if want_sums else None,
                cat([p.slot_cov for p in parts])[:ns], cat([p.read_cov for p in parts]))
        return out


def _iter_index(reads_index):
    return reads_index.items() if hasattr(reads_index, 'items') else iter(reads_index)


def get_chrm_sizes(reads_index, ctrl_reads_index=None):
    """{chrm: the largest read end over both strands (and both indices)} (tombo_helper.py:396-421)"""
    sizes = {}
    for index in (reads_index, ctrl_reads_index):
        if index is None:
            continue
        for (chrm, _), cs_reads in _iter_index(index):
            if len(cs_reads):
                sizes[chrm] = max(sizes.get(chrm, 0), max(rd.end for rd in cs_reads))
    return sizes


def compute_coverage(reads_index, engine=None, max_window=1 << 26):
    """{(chrm, strand): int64 read coverage up to the largest read end of that strand}
    (TomboReads._compute_coverage, tombo_helper.py:1394-1404): every read counts over [start, end), with or
    without an Events table."""
    ends = dict((cs, max(rd.end for rd in rds)) for cs, rds in _iter_index(reads_index) if len(rds))
    tracks = GenomeTracks(get_chrm_sizes(reads_index), slots=(), engine=engine, max_window=max_window)
    for (chrm, strand), cs_reads in _iter_index(reads_index):
        if len(cs_reads):
            tracks.add_reads(chrm, strand, cs_reads)
    res = tracks.finish()
    return dict((cs, res[cs].read_cov[:ends[cs]].copy()) for cs in ends)


def _add_coverages(cov, ctrl_cov):
    """TomboReads._add_coverages (tombo_helper.py:1406-1428): per (chrm, strand) OF THE CONTROL the longer array
    plus the shorter one; what only the sample covers is left out, as in the reference"""
    merged = {}
    for cs, c in ctrl_cov.items():
        if cs in cov:
            a, b = (cov[cs], c) if cov[cs].shape[0] > c.shape[0] else (c, cov[cs])
            m = a.copy()
            m[:b.shape[0]] += b
        else:
            m = c.copy()
        merged[cs] = m
    return merged


def iter_coverage_regions(reads_index, ctrl_reads_index=None, engine=None):
    """Yields (chrm, strand, cs_cov, cs_cov_starts): the read coverage in run-length form
    (TomboReads.iter_coverage_regions, tombo_helper.py:1430-1453): cs_cov_starts holds 0, every position where
    the coverage changes and the length; cs_cov the coverage of each run.  With a control index the coverages are
    added, over the (chrm, strand) of the control only (the reference's behaviour)."""
    eng = _tracks_engine(engine)
    cov = compute_coverage(reads_index, engine=eng)
    if ctrl_reads_index is not None:
        cov = _add_coverages(cov, compute_coverage(ctrl_reads_index, engine=eng))
    for (chrm, strand), cs_cov in cov.items():
        starts, vals = eng.tracks_compact(cs_cov)
        yield chrm, strand, vals, starts


def iter_cov_regs(reads_index, cov_thresh, region_size=None, ctrl_reads_index=None, engine=None):
    """Regions with coverage >= cov_thresh (TomboReads.iter_cov_regs, tombo_helper.py:1457-1485): without
    region_size (chrm, strand, start, end), with it (chrm, strand, start) for starts on multiples of region_size.
    Two habits of the reference are kept:
      * the threshold crossings are paired (1st, 2nd), (2nd, 3rd), ...: the stretch BETWEEN two qualifying runs is
        yielded too, like the runs themselves;
      * with region_size a start is skipped only when it equals the one yielded just before it."""
    for chrm, strand, cov, starts in iter_coverage_regions(reads_index, ctrl_reads_index, engine=engine):
        curr_reg_start = -1
        valid_cov = np.flatnonzero(np.diff(np.concatenate([[False], cov >= cov_thresh, [False]])))
        for i, j in zip(valid_cov[:-1], valid_cov[1:]):
            cov_start, cov_end = starts[i], starts[j]
            if region_size is None:
                yield chrm, strand, cov_start, cov_end
                continue
            first = int(region_size * np.floor(cov_start / float(region_size)))
            last = int(region_size * np.ceil(cov_end / float(region_size)))
            for reg_start in range(first, last, region_size):
                if reg_start != curr_reg_start:
                    yield chrm, strand, reg_start
                    curr_reg_start = reg_start


def get_mean_slot_genome_centric(cs_reads, chrm_len, slot_name, slots=None, engine=None, max_window=1 << 26):
    """float64[chrm_len]: the mean of `slot_name` over the reads of one (chrm, strand) at every position, NaN where
    no read has a value (tombo_helper.py:1661-1676; bit-identical, the reads are added in list order).  slots: the
    column per read, a sequence by position in cs_reads or a mapping by read_id / position (norm_mean: defaults to
    rd.means); None for a read without an Events table."""
    tracks = GenomeTracks({'': chrm_len}, slots=(slot_name,), engine=engine, max_window=max_window)
    tracks.add_reads('', '+', cs_reads, {slot_name: slots})   # (each read's own strand decides the flip)
    return tracks.finish()[('', '+')].means[0]


def iter_mean_slot_values(reads_index, chrm_sizes, slot_name, ctrl_reads_index=None, slots=None, ctrl_slots=None,
                          engine=None):
    """Yields (chrm, strand, cs_mean_values, ctrl_cs_mean_values) over the sorted chromosomes and '+', '-'
    (tombo_helper.py:1678-1712); without a control the fourth value is None, with one a side without reads on that
    (chrm, strand) is None.  slots / ctrl_slots: {(chrm, strand): per-list column mapping}, or one mapping by
    read_id."""
    for chrm, strand in [(c, s) for c in sorted(chrm_sizes) for s in ('+', '-')]:
        cs, vals = (chrm, strand), []
        for index, sl in ((reads_index, slots), (ctrl_reads_index, ctrl_slots)):
            vals.append(None if index is None or cs not in index else get_mean_slot_genome_centric(
                index[cs], chrm_sizes[chrm], slot_name, _cs_slots(sl, cs), engine=engine))
        if ctrl_reads_index is None:
            if vals[0] is not None:
                yield chrm, strand, vals[0], None
        elif vals[0] is not None or vals[1] is not None:
            yield chrm, strand, vals[0], vals[1]


def get_signal_differences(reads_index, ctrl_reads_index, engine=None):
    """{(chrm, strand): nan_to_num(sample mean - control mean)} where both have reads (tombo_helper.py:1730-1742)"""
    eng = _tracks_engine(engine)
    chrm_sizes = get_chrm_sizes(reads_index, ctrl_reads_index)
    return dict(((chrm, strand), eng.tracks_diff(a, b))
                for chrm, strand, a, b in iter_mean_slot_values(reads_index, chrm_sizes, 'norm_mean',
                                                                ctrl_reads_index, engine=eng)
                if a is not None and b is not None)


def get_largest_signal_differences(reads_index, ctrl_reads_index, num_regions, num_bases, engine=None):
    """The num_regions positions with the largest |sample mean - control mean| as (difference,
    max(pos - int(num_bases / 2), 0), chrm, strand), largest first (tombo_helper.py:1714-1728).  The candidates of a
    (chrm, strand) are selected on the device; the difference track is not copied back.
    Ties: the reference takes its candidates from an unstable argsort, so which of several EQUAL differences at the
    cut it keeps is not defined; here the higher position is taken first."""
    eng = _tracks_engine(engine)
    chrm_sizes = get_chrm_sizes(reads_index, ctrl_reads_index)
    found = []
    for chrm, strand, a, b in iter_mean_slot_values(reads_index, chrm_sizes, 'norm_mean', ctrl_reads_index,
                                                    engine=eng):
        if a is None or b is None:
            continue
        vals, poss = eng.tracks_topn(a, b, num_regions)
        found.extend((v, max(int(p) - int(num_bases / 2.0), 0), chrm, strand) for v, p in zip(vals, poss))
    return sorted(found, reverse=True)[:num_regions]

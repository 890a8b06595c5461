"""`tombo text_output browser_files` for reads held in memory: coverage (bedGraph), mean signal, signal SD, dwell
and the sample - control difference (wiggle) per position and strand -- the file names, headers and number
formats of the reference's writers (tombo/_text_output_commands.py:64-93, 230-388) -- and the FASTA of
`tombo text_output signif_sequence_context` (write_most_signif, :395-420).  The per-position numbers come
from the device (tombo_helper.GenomeTracks, csrc/k_tracks.h); the formatting stays in Python.

A `reads_index` is {(chrm, strand): [reads]}.  `slots` / `ctrl_slots`: {slot name: {(chrm, strand): per-list
column sequence or mapping}} for norm_stdev and length (norm_mean defaults to the reads' `means`)."""
import io

import numpy as np

from . import tombo_helper as th

OUT_HEADER = 'track type={0} name="{1}_{2}_{3}{4}" description="{1} {2} {3}{5}"\n'
BG_TYPE, WIG_TYPE = 'bedgraph', 'wig'
OUT_TYPES = {WIG_TYPE: 'wiggle_0', BG_TYPE: 'bedGraph'}
GROUP_NAME, CTRL_NAME = 'sample', 'control'
COV_WIG_TYPE, SIG_WIG_TYPE, DIFF_WIG_TYPE, SD_WIG_TYPE, DWELL_WIG_TYPE = (
    'coverage', 'signal', 'difference', 'signal_sd', 'dwell')
SIG_SLOT, SD_SLOT, DWELL_SLOT = 'norm_mean', 'norm_stdev', 'length'
# these read a statistics file (write_frac_wigs)
FRAC_WIG_TYPE, DFRAC_WIG_TYPE, STAT_WIG_TYPE, VCOV_WIG_TYPE = (
    'fraction', 'dampened_fraction', 'statistic', 'valid_coverage')
STATS_WIG_TYPES = (FRAC_WIG_TYPE, DFRAC_WIG_TYPE, STAT_WIG_TYPE, VCOV_WIG_TYPE)
FRAC_WIG_NAME, DFRAC_WIG_NAME, STAT_WIG_NAME, VCOV_WIG_NAME = (
    'fraction_modified_reads', 'dampened_fraction_modified_reads', 'statistic', 'valid_coverage')


def open_browser_files(wig_base, group_text, type_name, out_type=WIG_TYPE):
    """-> (plus strand file, minus strand file), headers written"""
    fps = []
    for strand_file, strand_name in (('plus', 'fwd_strand'), ('minus', 'rev_strand')):
        fp = io.open('%s.%s%s.%s.%s' % (wig_base, type_name, '.' + group_text if group_text else '', strand_file,
                                        out_type), 'wt')
        fp.write(OUT_HEADER.format(OUT_TYPES[out_type], wig_base, type_name, strand_name,
                                   '_' + group_text if group_text else '', ' ' + group_text if group_text else ''))
        fps.append(fp)
    return tuple(fps)


def _write_cs_data(wig_fp, chrm, cs_poss, cs_vals):
    wig_fp.write('variableStep chrom={} span=1\n'.format(chrm))
    wig_fp.write('\n'.join('{:d} {:.4f}'.format(p + 1, v) for p, v in zip(cs_poss.tolist(), cs_vals.tolist())) + '\n')


def _write_cs_int_data(wig_fp, chrm, cs_poss, cs_vals):
    wig_fp.write('variableStep chrom={} span=1\n'.format(chrm))
    wig_fp.write('\n'.join('{:d} {:d}'.format(p + 1, v) for p, v in zip(cs_poss.tolist(), cs_vals.tolist())) + '\n')


def write_frac_wigs(all_stats, wig_base, do_frac, do_damp, do_stats, do_vcov, fasta_fn=None, motif_descs=None):
    """_text_output_commands.py:95-228: the fraction / dampened fraction / statistic / valid coverage wiggles of a
    statistics container (tombo_stats.ModelStats / LevelStats), block after block in the container's own order,
    one variableStep section per run of blocks of one (chrm, strand)."""
    if fasta_fn is not None and motif_descs is not None:
        raise NotImplementedError('motif filtering of the statistics wiggles needs the genome index: not built')
    slots = [(FRAC_WIG_NAME, lambda b: 1 - b['frac'], _write_cs_data), (DFRAC_WIG_NAME, lambda b: 1 - b['damp_frac'],
             _write_cs_data), (STAT_WIG_NAME, all_stats._stat_transform, _write_cs_data),
             (VCOV_WIG_NAME, lambda b: b['valid_cov'], _write_cs_int_data)]
    slots = [s + (open_browser_files(wig_base, '', s[0]),)
             for s, do in zip(slots, (do_frac, do_damp, do_stats, do_vcov)) if do]

    def write_cs_stats(chrm, strand, poss, vals):
        poss = np.concatenate(poss)
        for (_, _, write, fps), v in zip(slots, vals):
            write(fps[0 if strand == '+' else 1], chrm, poss, np.concatenate(v))

    curr_cs, curr_poss, curr_vals = None, [], [[] for _ in slots]
    for chrm, strand, _, _, block_stats in all_stats:
        if (chrm, strand) != curr_cs:
            if len(curr_poss) > 0:
                write_cs_stats(*curr_cs, curr_poss, curr_vals)
            curr_cs, curr_poss, curr_vals = (chrm, strand), [], [[] for _ in slots]
        curr_poss.append(block_stats['pos'])
        for (_, value, _, _), v in zip(slots, curr_vals):
            v.append(value(block_stats))
    if len(curr_poss) > 0:
        write_cs_stats(*curr_cs, curr_poss, curr_vals)
    for _, _, _, fps in slots:
        for fp in fps:
            fp.close()


def write_cov_wig(reads_index, out_base, group_text, engine=None):
    plus_fp, minus_fp = open_browser_files(out_base, group_text, COV_WIG_TYPE, BG_TYPE)
    for chrm, strand, cs_cov, cs_cov_starts in th.iter_coverage_regions(reads_index, engine=engine):
        starts, cov = cs_cov_starts.tolist(), cs_cov.tolist()
        (plus_fp if strand == '+' else minus_fp).write('\n'.join(
            '%s\t%d\t%d\t%d' % (chrm, starts[i], starts[i + 1], cov[i]) for i in range(len(cov))) + '\n')
    plus_fp.close()
    minus_fp.close()


def write_slot_mean_wig(reads_index, chrm_sizes, wig_base, group_name, wig_type, slot_name, slots=None,
                        engine=None):
    eng = th._tracks_engine(engine)
    plus_fp, minus_fp = open_browser_files(wig_base, group_name, wig_type)
    for chrm, strand, cs_vals, _ in th.iter_mean_slot_values(reads_index, chrm_sizes, slot_name, slots=slots,
                                                             engine=eng):
        _write_cs_data(plus_fp if strand == '+' else minus_fp, chrm, *eng.tracks_compact(cs_vals))
    plus_fp.close()
    minus_fp.close()


def write_signal_and_diff_wigs(reads_index, ctrl_reads_index, chrm_sizes, wig_base, group_name, write_sig,
                               write_diff, slots=None, ctrl_slots=None, engine=None):
    eng = th._tracks_engine(engine)
    fps = []
    if write_sig:
        sig1 = open_browser_files(wig_base, group_name, SIG_WIG_TYPE)
        fps.extend(sig1)
        if ctrl_reads_index is not None:
            sig2 = open_browser_files(wig_base, CTRL_NAME, SIG_WIG_TYPE)
            fps.extend(sig2)
    if write_diff:
        diff = open_browser_files(wig_base, '', DIFF_WIG_TYPE)
        fps.extend(diff)
    for chrm, strand, means1, means2 in th.iter_mean_slot_values(
            reads_index, chrm_sizes, SIG_SLOT, ctrl_reads_index, slots=slots, ctrl_slots=ctrl_slots, engine=eng):
        k = 0 if strand == '+' else 1
        if means1 is not None and write_sig:
            _write_cs_data(sig1[k], chrm, *eng.tracks_compact(means1))
        if means2 is not None:
            if write_sig:
                _write_cs_data(sig2[k], chrm, *eng.tracks_compact(means2))
            if means1 is not None and write_diff:
                # the positions where both have a value (the reference's intersect1d of the two filtered
                # position lists), then the plain difference there
                poss = np.flatnonzero(~np.isnan(means1) & ~np.isnan(means2))
                with np.errstate(all='ignore'):
                    _write_cs_data(diff[k], chrm, poss, means1[poss] - means2[poss])
    for fp in fps:
        fp.close()


def _write_stats_files(all_stats, wig_base, wig_types):
    """the tail of write_all_browser_files (:369-386), the container given instead of a file name"""
    if not all_stats.is_model_stats and any(t in wig_types for t in (FRAC_WIG_TYPE, DFRAC_WIG_TYPE, VCOV_WIG_TYPE)):
        raise th.TomboError('Cannot output --file-type fraction, dampened_fraction or valid_coverage for level '
                            'sample compare statistics.')
    if all_stats.is_model_stats and STAT_WIG_TYPE in wig_types:
        raise th.TomboError('Cannot output `--file-type statistics` for aggregated per-read statistics.')
    write_frac_wigs(all_stats, wig_base, FRAC_WIG_TYPE in wig_types, DFRAC_WIG_TYPE in wig_types,
                    STAT_WIG_TYPE in wig_types, VCOV_WIG_TYPE in wig_types)


def write_all_browser_files(reads_index, ctrl_reads_index, wig_base, wig_types, slots=None, ctrl_slots=None,
                            engine=None, all_stats=None):
    """The files of `tombo text_output browser_files --file-types ...` (write_all_browser_files,
    _text_output_commands.py:322-388; the order of the calls is the reference's).  With a control index the sample's
    files carry `sample` in their names, the control's `control`.  all_stats: an open statistics container
    (tombo_stats.TomboStats(...)), which fraction, dampened_fraction, valid_coverage (ModelStats) and statistic
    (LevelStats) are read from; without it these four types are refused.  reads_index may be None when only those
    are asked for."""
    wig_types = list(wig_types)
    for t in wig_types:
        if t in STATS_WIG_TYPES and all_stats is None:
            raise NotImplementedError('file type %r reads a statistics file: not written by this module' % t)
        if t not in (COV_WIG_TYPE, SIG_WIG_TYPE, DIFF_WIG_TYPE, SD_WIG_TYPE, DWELL_WIG_TYPE) + STATS_WIG_TYPES:
            raise ValueError('unknown file type %r' % (t,))
    if reads_index is None:
        if any(t not in STATS_WIG_TYPES for t in wig_types):
            raise ValueError('file types other than the statistics types need reads')
        return _write_stats_files(all_stats, wig_base, wig_types)
    eng = th._tracks_engine(engine)
    slots, ctrl_slots = slots or {}, ctrl_slots or {}
    sig = dict(slots=slots.get(SIG_SLOT), ctrl_slots=ctrl_slots.get(SIG_SLOT), engine=eng)
    group_name = '' if ctrl_reads_index is None else GROUP_NAME
    per_slot = ((SD_WIG_TYPE, SD_SLOT), (DWELL_WIG_TYPE, DWELL_SLOT))
    if ctrl_reads_index is not None:
        chrm_sizes = th.get_chrm_sizes(reads_index, ctrl_reads_index)
        if COV_WIG_TYPE in wig_types:
            write_cov_wig(ctrl_reads_index, wig_base, CTRL_NAME, engine=eng)
        for wig_type, slot in per_slot:
            if wig_type in wig_types:
                write_slot_mean_wig(ctrl_reads_index, chrm_sizes, wig_base, CTRL_NAME, wig_type, slot,
                                    slots=ctrl_slots.get(slot), engine=eng)
        if SIG_WIG_TYPE in wig_types or DIFF_WIG_TYPE in wig_types:
            write_signal_and_diff_wigs(reads_index, ctrl_reads_index, chrm_sizes, wig_base, group_name,
                                       SIG_WIG_TYPE in wig_types, DIFF_WIG_TYPE in wig_types, **sig)
    else:
        chrm_sizes = th.get_chrm_sizes(reads_index)
        if SIG_WIG_TYPE in wig_types:
            write_signal_and_diff_wigs(reads_index, None, chrm_sizes, wig_base, group_name, True, False, **sig)
    if COV_WIG_TYPE in wig_types:
        write_cov_wig(reads_index, wig_base, group_name, engine=eng)
    for wig_type, slot in per_slot:
        if wig_type in wig_types:
            write_slot_mean_wig(reads_index, chrm_sizes, wig_base, group_name, wig_type, slot,
                                slots=slots.get(slot), engine=eng)
    if any(t in STATS_WIG_TYPES for t in wig_types):
        _write_stats_files(all_stats, wig_base, wig_types)


def write_most_signif(stats, seqs_fp, num_regions, num_bases, reads_index=None, genome_index=None):
    """`tombo text_output signif_sequence_context` (_text_output_commands.py:395-420): one FASTA record
    `>{chrm}:{pos + 1}:{strand} {statistic text}` per most significant region of num_bases bases, the sequence in the
    region's strand orientation.  stats: an open statistics container; seqs_fp: a text file open for writing.  The
    sequence comes from genome_index (a th.Fasta; a region that runs past the chromosome end is cut there, one that
    starts outside raises th.TomboError) or, without one, from the reads of reads_index that overlap the region
    (th.get_region_seq: '-' where no read lies)."""
    if genome_index is None and reads_index is None:
        raise th.TomboError('Must provide either reads or a genome FASTA to output sequences.')
    for chrm, start, end, strand, _, reg_text in stats.get_most_signif_regions(
            num_bases, num_regions, prepend_loc_to_text=True):
        if genome_index is not None:
            seq = genome_index.get_seq(chrm, start, end, error_end=False)
        else:
            seq = th.get_region_seq([rd for rd in reads_index.get((chrm, strand), ())
                                     if not (rd.start >= end or rd.end <= start)], start, end)
        seqs_fp.write('>{0}\n{1}\n'.format(reg_text, seq if strand == '+' else th.rev_comp(seq)))

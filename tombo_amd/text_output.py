"""`tombo text_output browser_files` for reads held in memory: coverage (bedGraph), mean signal, signal SD, dwell
and the sample - control difference (wiggle) per position and strand -- the file names, headers and number
formats of the reference's writers (tombo/_text_output_commands.py:64-93, 230-388).  The per-position numbers come
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
# these read a statistics file: not part of this module
STATS_WIG_TYPES = ('fraction', 'dampened_fraction', 'statistic', 'valid_coverage')


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


def write_all_browser_files(reads_index, ctrl_reads_index, wig_base, wig_types, slots=None, ctrl_slots=None,
                            engine=None):
    """The files of `tombo text_output browser_files --file-types ...` for coverage, signal, signal_sd, dwell and
    difference (write_all_browser_files, _text_output_commands.py:322-388; the order of the calls is the
    reference's).  With a control index the sample's files carry `sample` in their names, the control's `control`."""
    wig_types = list(wig_types)
    for t in wig_types:
        if t in STATS_WIG_TYPES:
            raise NotImplementedError('file type %r reads a statistics file: not written by this module' % t)
        if t not in (COV_WIG_TYPE, SIG_WIG_TYPE, DIFF_WIG_TYPE, SD_WIG_TYPE, DWELL_WIG_TYPE):
            raise ValueError('unknown file type %r' % (t,))
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

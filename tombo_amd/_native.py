"""ctypes binding of libtombo_amd.so (the C ABI in include/tombo_amd.h).

There is no CPU fallback: importing works anywhere (so the symbol table can be checked on a
box without a GPU), but creating an engine raises when no gfx950 device is usable.
"""
import os
import ctypes as C
import subprocess
from collections import namedtuple

import numpy as np

from ._default_parameters import MAX_POINTS_FOR_THEIL_SEN, SIG_MATCH_THRESH

_HERE = os.path.dirname(os.path.abspath(__file__))
# TBA_LIB_PATH: an alternative build of the same library (profiling builds with one of -DTBA_PHASE_DEBUG=<id> /
# -DTBA_SWEEP_STATS / -DTBA_SKIP_STATS / -DTBA_SKIP_CLASS_STATS, A/B comparisons of a kernel variant)
LIB_PATH = os.environ.get('TBA_LIB_PATH') or os.path.join(_HERE, 'libtombo_amd.so')
CSRC = os.path.join(_HERE, 'csrc')
i64, f64, i32 = C.c_int64, C.c_double, C.c_int32

HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC',
               '-shared']


# a second build of the same source for ONE test (tests/test_gpu_determinism.py): the chunk-parallel traceback with a
# deterministic fault in it, which the verifier has to catch.  Never loaded by the product (LIB_PATH is).
INJECT_LIB_PATH = os.path.join(_HERE, 'libtombo_amd_inject.so')
INJECT_FLAGS = ['-DTBA_TB_INJECT=5']


def build(force=False):
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU): libtombo_amd.so and,
    beside it, the fault-injection build one GPU test loads in a child process.  Returns the in-tree library's
    path: a TBA_LIB_PATH build is neither built nor checked here."""
    tree_lib = os.path.join(_HERE, 'libtombo_amd.so')
    srcs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + \
        [os.path.join(_HERE, '..', 'include', 'tombo_amd.h')]
    newest = max(os.path.getmtime(s) for s in srcs)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    jobs = []
    for path, extra in ((tree_lib, os.environ.get('TBA_EXTRA_HIPCC_FLAGS', '').split()), (INJECT_LIB_PATH, INJECT_FLAGS)):
        if force or not os.path.exists(path) or os.path.getmtime(path) < newest:
            jobs.append((path, subprocess.Popen([hipcc] + HIPCC_FLAGS + extra +
                                                ['-o', path, os.path.join(CSRC, 'tba_engine.hip')])))
    for path, p in jobs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, 'hipcc -> ' + path)
    return tree_lib


class Params(C.Structure):
    _fields_ = [(n, f64) for n in ('match_evalue', 'skip_pen', 'max_half_z_score', 'z_shift',
                                   'stay_pen')] + \
               [(n, i64) for n in ('bandwidth', 'running_stat_width', 'min_obs_per_base',
                                   'raw_min_obs_per_base', 'mean_obs_per_event',
                                   'use_t_test_seg', 'band_bound_thresh', 'start_bw',
                                   'start_save_bw', 'start_n_bases', 'do_winsorize_z')]


class Opts(C.Structure):
    _fields_ = [('has_outlier_thresh', i64), ('outlier_thresh', f64),
                ('has_const_scale', i64), ('const_scale', f64),
                ('skip_seq_scaling', i64),
                ('check_start_score', i64), ('sig_match_thresh', f64),
                ('max_raw_cpts', i64), ('min_event_to_seq_ratio', f64),
                ('use_rna_event_scale', i64), ('rna_scale_num_events', i64),
                ('rna_scale_max_frac_events', f64), ('skip_norm_out', i64),
                ('reverse_raw', i64), ('detect_stalls', i64),
                ('stall_window_size', i64), ('stall_n_windows', i64),
                ('stall_mini_window_size', i64), ('stall_min_consecutive_obs', i64),
                ('stall_edge_buffer', i64), ('stall_threshold', f64),
                ('device_subsample', i64), ('subsample_seed', C.c_uint64), ('subsample_first_read', i64),
                ('del_fix_window', i64), ('max_del_fix_window', i64), ('extra_sig_factor', f64)]


class ReadResult(C.Structure):
    """tba_read_result: the scalar part of what resquiggle_read returns, 64 bytes per read"""
    _fields_ = [('status', i32), ('norm_params_changed', i32),
                ('read_start_rel_to_raw', i64), ('norm_len', i64),
                ('shift', f64), ('scale', f64), ('lower_lim', f64), ('upper_lim', f64),
                ('sig_match_score', f64)]


class SynthParams(C.Structure):
    _fields_ = [('mean_dwell', i64), ('min_dwell', i64), ('n_lead', i64), ('n_trail', i64),
                ('scale', f64), ('offset', f64), ('noise_sd', f64), ('dac_per_pa', f64), ('dac_offset', f64),
                ('reverse', i32), ('pad', i32)]


RESULT_DTYPE = np.dtype([
    ('status', np.int32), ('norm_params_changed', np.int32),
    ('read_start_rel_to_raw', np.int64), ('norm_len', np.int64),
    ('shift', np.float64), ('scale', np.float64), ('lower_lim', np.float64),
    ('upper_lim', np.float64), ('sig_match_score', np.float64)])
assert RESULT_DTYPE.itemsize == C.sizeof(ReadResult) == 64

RAW_F64, RAW_F32, RAW_I16 = 0, 1, 2
RAW_DTYPES = {np.dtype(np.float64): RAW_F64, np.dtype(np.float32): RAW_F32,
              np.dtype(np.int16): RAW_I16}


# TBA_GET_* selectors
GET_VALID_CPTS, GET_N_CPTS, GET_EVENT_MEANS, GET_SEG_NORM, GET_SEG_SV, GET_START, \
    GET_BAND_STARTS, GET_READ_TB, GET_DP_SEGS, GET_THEIL_SEN, GET_PATH, GET_LAST_ROW, \
    GET_DP_READ_START, GET_KERNEL_MS, GET_REF_MEANS, GET_REF_SDS, GET_SEGS, GET_STATUS, GET_START_FAIL, \
    GET_STALL_INTS, GET_N_STALL, GET_STALL_OFF, GET_SAMP_IND, GET_TB_PARALLEL, GET_ED_FUSED, GET_ED_TAKEN_POS, GET_ED_N_TAKEN, \
    GET_DP_WORKGROUP, GET_ED_FORM, GET_TB_FORM, GET_TB_VERIFY_FAIL, GET_DP_FORM, GET_NORM_FORM, GET_TS_FORM = range(1, 35)
# TBA_ED_FORM_* / TBA_TB_FORM_*: which kernels produced a read's change points / main traceback
ED_FORM_NONE, ED_FORM_WG_SCAN_PEAKS, ED_FORM_DETECT_PICK, ED_FORM_SCORES_PEAKS, ED_FORM_DETECT_TT_PICK, \
    ED_FORM_TTEST_PEAKS = range(6)
# TBA_NORM_FORM_*: which code found the medians of a read's normalisation
NORM_FORM_NONE, NORM_FORM_SELECT, NORM_FORM_INT_COUNT, NORM_FORM_HIST = range(4)
# TBA_GET_TS_FORM, int32[n][2]: (TBA_TS_FORM_*: what k_theil_sen did with the read, the pairs its one-pass form listed).
# The last four: the generic select ran, and why the one-pass form declined
TS_FORM_NONE, TS_FORM_SMALL, TS_FORM_FAST, TS_FORM_NO_SCRATCH, TS_FORM_NO_WINDOW, TS_FORM_LIST_OVERFLOW, \
    TS_FORM_WINDOW_MISS = range(7)
TB_FORM_NONE, TB_FORM_LANE, TB_FORM_LONG, TB_FORM_PAR16, TB_FORM_PAR64 = 0, 1, 2, 16, 64
# TBA_GET_DP_FORM, int32[n][4]: (TBA_DP_FORM_* of the main forward pass, its cells-per-lane class, TBA_DP_START_* of
# start discovery, class of the retry kernel); derived on the host from the run's launch decisions and per-read state
DP_FORM_NONE, DP_FORM_K_DP, DP_FORM_K_DP8_LOWREG, DP_FORM_MULTI, DP_FORM_WIDE = range(5)
DP_START_NONE, DP_START_FIRST_TRY, DP_START_RETRY_WG, DP_START_RETRY_K_DP = range(4)
# TBA_GET_DP_ONE_SD, int32[n][2]: (the main pass ran on k_dp_c1, bit 0 / 1: the first try / the retry of start discovery did)
GET_DP_ONE_SD = 35
# ReadState.dbg of a profiling build: -DTBA_PHASE_DEBUG=<id>, -DTBA_SWEEP_STATS, -DTBA_SKIP_STATS or
# -DTBA_SKIP_CLASS_STATS (what each leaves in the eight slots: the table in csrc/tba_phase.h)
GET_DEBUG_COUNTERS = 99
STAGE_SEGMENT, STAGE_EVENT_MEANS, STAGE_REF_LEVELS, STAGE_START, STAGE_ASSIGN, STAGE_SKIP, \
    STAGE_RESCALE = range(7)
PUT_VALID_CPTS, PUT_EVENT_MEANS, PUT_NORM, PUT_REF_MEANS, PUT_REF_SDS, PUT_DP_SEGS, \
    PUT_START_STATE = range(1, 8)
MAX_BAND = 3072
MAX_CENTER_READS = 1 << 62   # Engine.center_fit without a limit on the successes that count
ABI_VERSION = 13  # TBA_ABI_VERSION of include/tombo_amd.h
STAGE_NAMES = ["normalize", "cumsum", "scores", "peaks", "event_means", "ref_levels",
               "start_dp", "start_tb", "prep", "main_dp", "main_tb", "skip_resolve", "theil_sen",
               "rescale_score", "stalls", "total"]

# what Engine.get returns per selector: (element type, shape); a name is that count of the uploaded batch
# (n reads, raw samples, ref bases, seg boundaries = bases + reads, ev events -- at least one element)
_GET_SHAPES = {
    GET_N_CPTS: (np.int64, ('n',)), GET_DP_READ_START: (np.int64, ('n',)),
    GET_SEG_SV: (np.float64, ('n', 4)), GET_START: (np.float64, ('n', 4)),
    GET_THEIL_SEN: (np.float64, ('n', 4)), GET_PATH: (np.int32, ('n', 4)), GET_DP_FORM: (np.int32, ('n', 4)),
    GET_TS_FORM: (np.int32, ('n', 2)), GET_DP_ONE_SD: (np.int32, ('n', 2)),
    GET_LAST_ROW: (np.float64, ('n', MAX_BAND)), GET_KERNEL_MS: (np.float32, (32,)),
    GET_DEBUG_COUNTERS: (np.int64, ('n', 8)),
    GET_VALID_CPTS: (np.int64, ('ev',)), GET_EVENT_MEANS: (np.float64, ('ev',)),
    GET_SEG_NORM: (np.float64, ('raw',)),
    GET_BAND_STARTS: (np.int64, ('ref',)), GET_REF_MEANS: (np.float64, ('ref',)), GET_REF_SDS: (np.float64, ('ref',)),
    GET_READ_TB: (np.int64, ('seg',)), GET_DP_SEGS: (np.int64, ('seg',)), GET_SEGS: (np.int64, ('seg',)),
    GET_STATUS: (np.int32, ('n',)), GET_START_FAIL: (np.int32, ('n',)),
    GET_N_STALL: (np.int64, ('n',)), GET_STALL_OFF: (np.int64, ('n',)),
    GET_SAMP_IND: (np.int64, ('n', MAX_POINTS_FOR_THEIL_SEN)),
    GET_TB_PARALLEL: (np.int32, ('n',)), GET_ED_FUSED: (np.int32, ('n',)), GET_DP_WORKGROUP: (np.int32, ('n',)),
    GET_NORM_FORM: (np.int32, ('n',)), GET_ED_FORM: (np.int32, ('n',)), GET_TB_FORM: (np.int32, ('n',)), GET_TB_VERIFY_FAIL: (np.int32, ('n',)),
    GET_ED_TAKEN_POS: (np.int32, ('raw_x2',)), GET_ED_N_TAKEN: (np.int64, ('n',)),
}

class _Ptr(object):
    """argtypes entry of a typed data pointer (`const double *`, `int64_t *`, ...).  Takes None (NULL), a C-contiguous
    numpy array of exactly that element type (writeable unless the header says const), a DeviceArray of that type,
    and any ctypes object as it is (byref, arrays, pointers); ctypes reports anything else as ArgumentError"""
    _CTYPES = (C.c_int.__mro__[-2], type(C.byref(C.c_int())))   # (_ctypes._CData, and what byref makes)

    def __init__(self, dtype, const):
        self.dtype, self.const = np.dtype(dtype), const

    def from_param(self, a):
        if a is None or isinstance(a, self._CTYPES):
            return a
        if isinstance(a, np.ndarray):
            if a.dtype == self.dtype and a.flags.c_contiguous and (self.const or a.flags.writeable):
                return C.c_void_p(a.ctypes.data)
        elif isinstance(a, DeviceArray) and a.dtype == self.dtype:
            return C.c_void_p(a.ptr)
        raise TypeError('expected None, a C-contiguous %s%s array or a ctypes object, got %s' % (
            '' if self.const else 'writeable ', self.dtype, getattr(a, 'dtype', type(a).__name__)))


def _prototypes():
    """entry name -> (restype, argtypes) of every declaration of include/tombo_amd.h, in its order (checked against
    the header by tests/test_abi_and_host.py).  n / q / u / d: int, int64_t, uint64_t, double; v: handles, void * and
    pointers to pointers; D Q I B, with c in front when the header says const: double, int64_t, int32_t, uint8_t *"""
    n, q, u, d, v = C.c_int, i64, C.c_uint64, f64, C.c_void_p
    D, Q, I, B = (_Ptr(t, False) for t in (np.float64, np.int64, np.int32, np.uint8))
    cD, cQ, cI, cB, cS = (_Ptr(t, True) for t in (np.float64, np.int64, np.int32, np.uint8, np.int8))
    P, O, R, SP = (C.POINTER(t) for t in (Params, Opts, ReadResult, SynthParams))
    pileup = [q, cQ, cQ, cS, cQ, q, cQ, cS]     # n_regions .. reg_read_off, n_reads, read_start, read_strand
    site_outs = [D, Q, Q, Q, D, Q, Q]           # out_frac .. out_n_stats
    fwd_pass = [v, D, Q, q, q, Q, cD, q, cD, cD, d, d, d, q, d, n, d]
    return {
        # ---- engine ----
        'tba_engine_create': (n, [n, v]),
        'tba_engine_destroy': (None, [v]),
        'tba_last_error': (C.c_char_p, []),
        'tba_device_count': (n, []),
        'tba_device_mem': (n, [v, Q, Q]),
        'tba_engine_held_bytes': (n, [v, Q]),
        'tba_engine_set_sharing': (n, [v, n]),
        'tba_engine_set_dispatch': (n, [v, q, q]),
        'tba_engine_get_dispatch': (n, [v, Q, Q]),
        'tba_engine_set_side_stream': (n, [v, n]),
        'tba_engine_last_side_stream': (n, [v]),
        'tba_engine_last_dp_lowreg': (n, [v]),
        'tba_engine_last_dp_const_division': (n, [v]),
        'tba_engine_set_dp_const_division': (n, [v, n]),
        'tba_engine_model_const_division': (n, [v]),
        'tba_prove_const_division': (n, [cD, q, I]),
        'tba_one_sd_words': (n, [cD, q, I, D]),
        'tba_c_last_ed_form': (n, [v]),
        'tba_set_model': (n, [v, cD, cD, q, q]),
        # ---- host memory for streaming ----
        'tba_pinned_alloc': (n, [q, v]),
        'tba_pinned_free': (n, [v]),
        # ---- batch pipeline ----
        'tba_batch_upload': (n, [v, P, O, q, cD, cQ, cB, cQ, cD, cI, cQ, cQ, cQ]),
        'tba_batch_upload_async': (n, [v, P, O, q, v, n, cQ, cB, cQ, cD, cI, cQ, cQ, cQ]),
        'tba_batch_footprint': (n, [P, O, q, n, q, cQ, cQ, D]),
        'tba_batch_run': (n, [v]),
        'tba_batch_enqueue': (n, [v]),
        'tba_batch_sync': (n, [v]),
        'tba_batch_wait_for': (n, [v, v]),
        'tba_batch_query': (n, [v]),
        'tba_batch_download': (n, [v, I, Q, Q, D, Q, D, D, I]),
        'tba_batch_download_async': (n, [v, R, I, Q, D]),
        'tba_batch_get': (n, [v, n, v, q]),
        # ---- stepwise execution ----
        'tba_batch_run_stages': (n, [v, n, n]),
        'tba_batch_put': (n, [v, n, v, q, cQ]),
        'tba_set_num_events': (n, [v, cQ, q]),
        'tba_batch_base_stats': (n, [v, D, D, q]),
        'tba_batch_stats': (n, [v, D, D]),
        # ---- per-kernel entry points ----
        'tba_c_adaptive_banded_forward_pass': (n, fwd_pass),
        'tba_c_adaptive_banded_forward_pass_z': (n, fwd_pass + [D]),
        'tba_c_banded_forward_pass': (n, [v, cD, q, q, cQ, d, d, D, Q]),
        'tba_c_banded_forward_pass_adaptive': (n, [v, cD, q, q, Q, q, q, d, d, D, Q, Q]),
        'tba_c_banded_traceback': (n, [v, cQ, q, q, cQ, q, q, Q]),
        'tba_c_base_z_scores': (n, [v, cD, q, d, d, n, d, D]),
        'tba_c_new_means': (n, [v, cD, q, cQ, q, D]),
        'tba_c_apply_outlier_thresh': (n, [v, cD, q, d, d, D]),
        'tba_c_valid_cpts_w_cap': (n, [v, cD, q, q, q, q, Q]),
        'tba_c_valid_cpts_w_cap_t_test': (n, [v, cD, q, q, q, q, Q]),
        'tba_c_new_mean_stds': (n, [v, cD, q, cQ, q, D, D]),
        'tba_c_compute_slopes': (n, [v, cD, cD, q, d, D]),
        'tba_c_reg_z_scores': (n, [v, cD, q, cD, cD, q, cQ, q, q, q, q, q, n, d, Q, Q, D, q]),
        'tba_c_base_forward_pass': (n, [v, cD, q, q, cD, q, q, cD, cQ, q, D, Q]),
        'tba_c_base_traceback': (n, [v, cD, q, q, cD, q, q, q, q, q, Q]),
        # ---- row N4: log-likelihood ratios; per-read p-values ----
        'tba_llh_ratio_windows': (n, [v, n, cD, cD, cD, cD, cD, q, q, cQ, q, cD, D]),
        'tba_read_pvals': (n, [v, cD, cD, cD, cQ, q, q, n, d, D]),
        # ---- level pileups across reads ----
        'tba_group_level_stats': (n, [v, n, n, q, q] + pileup + [cS, cQ, cD, d, D, Q, Q, Q, Q]),
        'tba_reads_ref_levels': (n, [v, n, q, q] + pileup + [cQ, cD, cD, cD, d, d, D, D, Q]),
        # ---- per-site modified fractions ----
        'tba_site_fractions': (n, [v, n, q, cQ, cQ, cD, cD, cD, cQ, q, cQ, cQ, q, n, d,
                                   n, cD, cD, cD, q, q, cQ, q, cD, cQ, cQ, d, cD, cD] + site_outs + [D]),
        'tba_site_fractions_reads': (n, [v, n, q, cQ, cQ, q, cQ, cS, cQ, cD, cB, cQ, cQ, cD, cD, q, d, d, cD, cD] +
                                     site_outs + [I, Q, Q, D, q, D]),
        'tba_site_aggregate': (n, [v, q, cQ, cQ, cQ, v, d, cD, n, cD] + site_outs + [D]),
        # ---- ROC / precision-recall ----
        'tba_roc_motif_labels': (n, [v, q, cB, cQ, cQ, cB, cQ, cQ, cD, q, cI, cB, n, n, D, B, Q, Q, D]),
        'tba_roc_loc_labels': (n, [v, q, cQ, cQ, q, cQ, q, cQ, cQ, cD, D, B, Q, Q, D]),
        'tba_roc_rank_counts': (n, [v, q, cD, cB, q, cQ, Q, Q, Q, D]),
        'tba_roc_sort_tile': (q, []),
        # ---- pairwise distances ----
        'tba_pairwise_window_dists': (n, [v, q, q, q, cD, D, D]),
        'tba_pairwise_nanmean_dists': (n, [v, q, q, cD, D, D]),
        'tba_pdist_tile': (q, []),
        'tba_pdist_lds_row_max': (q, []),
        # ---- alternate-base model estimation ----
        'tba_kmer_levels': (n, [v, cD, cB, cQ, q, q, q, cB, Q, Q, D, q]),
        'tba_kmer_dist': (n, [v, cD, cB, cQ, q, q, q, q, q, n, Q, Q, Q, Q, Q, D, Q, q, D, D]),
        'tba_kde_eval': (n, [v, cD, cQ, q, cD, q, d, D]),
        # ---- genome tracks ----
        'tba_tracks_begin': (n, [v, q, q, n]),
        'tba_tracks_add': (n, [v, q, cQ, cQ, cB, cQ, v, q, cQ, cI]),
        'tba_tracks_finish': (n, [v, D, D, Q, Q]),
        'tba_tracks_kernel_ms': (n, [v, D]),
        'tba_tracks_compact': (n, [v, n, v, q, Q, v, Q]),
        'tba_tracks_diff': (n, [v, cD, cD, q, D]),
        'tba_tracks_topn': (n, [v, cD, cD, q, q, Q, D, Q]),
        # ---- estimate_kmer_model / estimate_motif_alt_model ----
        'tba_region_key_levels': (n, [v, n, q, cQ, cB, cQ, cD, q, cQ, cQ, q, cQ, cQ, q, cQ, cQ, q, Q, Q, D, D]),
        'tba_segment_medians': (n, [v, cD, cQ, q, D]),
        'tba_center_prepare': (n, [v, P, O, q, v, n, cQ, cB, cQ, cQ, cQ, cQ, cQ, I, D]),
        'tba_center_fit': (n, [v, cQ, cD, q, q, I, D, D, Q, D]),
        # ---- region plot data ----
        'tba_region_level_piles': (n, [v, q, cQ, cB, cQ, cD, q, cQ, cQ, cQ, cQ, q, cD, q, cD, Q, D, q, D, D, D]),
        'tba_segment_percentiles': (n, [v, cD, cQ, q, q, cD, q, cD, D, D, D]),
        'tba_region_raw_signal': (n, [v, q, v, n, cQ, cQ, cQ, cQ, cQ, cB, cB, cD, cD, cD, cD, q, cQ, cQ, cQ, n, Q, D, D, Q,
                                      q, D]),
        # ---- read filters ----
        'tba_dwell_pctl_flags': (n, [v, q, cQ, cQ, q, cD, cD, D, B, D]),
        'tba_batch_dwell_pctl_flags': (n, [v, q, cD, cD, D, B, D]),
        'tba_batch_de_novo_stats': (n, [v, q, d, D, q]),
        # ---- the worker's per-read preparation; host-side packing ----
        'tba_identify_stalls': (n, [v, v, n, q, q, q, q, d, q, q, Q, q, Q]),
        # ---- the documented per-read functions of tombo_stats ----
        'tba_normalize_raw_batch': (n, [v, q, v, n, cQ, cQ, cQ, n, cD, cI, cD, n, d, d, D, I, D, I, D]),
        'tba_mom_sums': (n, [v, q, cQ, cD, cD, cD, D]),
        'tba_seg_scores': (n, [v, q, cQ, cD, cD, cD, D]),
        # ---- RNA adapter trimming, the global scale estimate ----
        'tba_trim_rna_batch': (n, [v, q, v, n, cQ, q, q, q, q, q, d, q, Q, I, I, D]),
        'tba_engine_set_trim_budget': (n, [v, q]),
        'tba_raw_med_mad': (n, [v, q, v, n, cQ, D, D, D]),
        'tba_pack_reads': (n, [q, v, n, n, cQ, v, v, cQ, B, n]),
        'tba_unpack_reads': (n, [q, v, q, cQ, cQ, v, n]),
        # ---- synthetic reads made on the device ----
        'tba_synth_create': (n, [n, cD, q, v]),
        'tba_synth_destroy': (None, [v]),
        'tba_synth_generate': (n, [v, SP, u, q, q, cQ, n, Q, Q, v, v]),
        'tba_synth_download': (n, [v, v, B]),
        'tba_synth_dwell_thresholds': (n, [SP, _Ptr(np.uint32, False), q, D]),
        # ---- ABI check, self-tests ----
        'tba_abi_sizes': (n, [Q, q]),
        'tba_selftest_subsample': (n, [v, q, u, q, q, Q]),
        'tba_selftest_division': (n, [v, cD, cD, q, D]),
        'tba_selftest_approx_quotient': (n, [v, cD, cD, q, D]),
        'tba_selftest_const_division': (n, [v, cD, cD, q, d, d, D]),
    }


PROTOTYPES = _prototypes()
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'libtombo_amd.so is not built (run `python -c "import __graft_entry__ as g; '
                'g.build()"`); the resquiggle engine has no CPU fallback')
        L = C.CDLL(LIB_PATH)
        # a stale build (the .so is not tracked by git) must not be driven through newer struct
        # mirrors: the engine would read past tba_opts, or miss fields, without any error
        try:
            for name, (restype, argtypes) in PROTOTYPES.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
            out = (i64 * 4)()
            ok = L.tba_abi_sizes(out, 4) == 0 and list(out) == [
                C.sizeof(Params), C.sizeof(Opts), C.sizeof(ReadResult), ABI_VERSION]
        except AttributeError:
            ok = False
        if not ok:
            raise RuntimeError(
                '%s does not match this binding (struct sizes / TBA_ABI_VERSION %d): rebuild it '
                '(`python -c "import __graft_entry__ as g; g.build()"`)' % (LIB_PATH, ABI_VERSION))
        _lib = L
    return _lib


def _call(L, name, *args):
    """L.name(*args); a return code other than 0 is raised as EngineError with the library's message"""
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise EngineError('%s failed (%d): %s' % (name, rc, L.tba_last_error().decode()))


def prove_const_division(sds):
    """bool[n]: for which of the divisors `sds` the forward pass's two-operation division is proven to be IEEE
    division for every dividend (tba_prove_const_division: host code, no device needed)"""
    sds = np.ascontiguousarray(sds, dtype=np.float64).ravel()
    out = np.zeros(sds.shape[0], dtype=np.int32)
    _call(lib(), 'tba_prove_const_division', sds, sds.shape[0], out)
    return out.astype(bool)


def one_sd_words(sds):
    """(sd, yh, yl) of a level table with one distinct, proven sd -- the words the one-sd forward pass reads
    (tba_one_sd_words: host code, no device needed) -- or None"""
    sds = np.ascontiguousarray(sds, dtype=np.float64).ravel()
    flag, words = np.zeros(1, dtype=np.int32), np.zeros(3, dtype=np.float64)
    _call(lib(), 'tba_one_sd_words', sds, sds.shape[0], flag, words)
    return tuple(float(w) for w in words) if flag[0] else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _check_offsets(off, what):
    off = np.asarray(off)
    if off.dtype != np.int64 or off.ndim != 1 or off.shape[0] < 1:
        raise ValueError('%s must be a one-dimensional int64 array' % what)
    if off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError('%s must start at 0 and be non-decreasing' % what)
    return np.ascontiguousarray(off)


def _check_kmer_levels_args(means, codes, read_off, kmer_width, central_pos, completed):
    """the argument checks of Engine.kmer_levels (shared with the tests' stand-in engine): dtypes are
    checked, not converted -> contiguous (means, codes, read_off, completed)"""
    means, codes, completed = np.asarray(means), np.asarray(codes), np.asarray(completed)
    if means.dtype != np.float64 or codes.dtype != np.uint8 or completed.dtype != np.uint8:
        raise ValueError('means must be float64, codes and completed uint8')
    if int(kmer_width) != kmer_width or not 1 <= kmer_width <= 10:
        raise ValueError('kmer_width must be an integer in [1, 10]')
    if int(central_pos) != central_pos or not 0 <= central_pos < kmer_width:
        raise ValueError('central_pos must be an integer in [0, kmer_width)')
    off = _check_offsets(read_off, 'read_off')
    if means.ndim != 1 or codes.ndim != 1 or not (means.shape[0] == codes.shape[0] == int(off[-1])):
        raise ValueError('per-base arrays and offsets disagree')
    if completed.shape != (4 ** int(kmer_width),):
        raise ValueError('completed must have 4**kmer_width entries')
    return np.ascontiguousarray(means), np.ascontiguousarray(codes), off, np.ascontiguousarray(completed)


KMER_DIST_MAX_WIDTH = 9          # the widest k-mer of tba_kmer_dist
KMER_DIST_TABLE_MAX = 1 << 27    # ... and the most 4**K * n_reads, its dense per-read table


def _check_kmer_dist_args(means, codes, read_off, kmer_width, central_pos, kmer_thresh, num_reads):
    """the argument checks of Engine.kmer_dist (shared with the tests' stand-in engine): dtypes are checked, not
    converted -> contiguous (means, codes, read_off)"""
    means, codes = np.asarray(means), np.asarray(codes)
    if means.dtype != np.float64 or codes.dtype != np.uint8:
        raise ValueError('means must be float64, codes uint8')
    if int(kmer_width) != kmer_width or not 1 <= kmer_width <= KMER_DIST_MAX_WIDTH:
        raise ValueError('kmer_width must be an integer in [1, %d]' % KMER_DIST_MAX_WIDTH)
    if int(central_pos) != central_pos or not 0 <= central_pos < kmer_width:
        raise ValueError('central_pos must be an integer in [0, kmer_width)')
    if int(kmer_thresh) != kmer_thresh or int(num_reads) != num_reads:
        raise ValueError('kmer_thresh and num_reads must be integers')
    off = _check_offsets(read_off, 'read_off')
    if means.ndim != 1 or codes.ndim != 1 or not (means.shape[0] == codes.shape[0] == int(off[-1])):
        raise ValueError('per-base arrays and offsets disagree')
    if int(off[-1]) >= 1 << 31:
        raise ValueError('2**31 bases or more in one batch')
    if 4 ** int(kmer_width) * (off.shape[0] - 1) > KMER_DIST_TABLE_MAX:
        raise ValueError('4**kmer_width * n_reads is above the table limit of 2**27 entries')
    return np.ascontiguousarray(means), np.ascontiguousarray(codes), off


def _check_kde_eval_args(levels, lv_off, x, bandwidth):
    """the argument checks of Engine.kde_eval -> contiguous (levels, lv_off, x)"""
    levels, x = np.asarray(levels), np.asarray(x)
    if levels.dtype != np.float64 or x.dtype != np.float64 or levels.ndim != 1 or x.ndim != 1:
        raise ValueError('levels and x must be one-dimensional float64 arrays')
    off = _check_offsets(lv_off, 'lv_off')
    if levels.shape[0] != int(off[-1]):
        raise ValueError('levels and offsets disagree')
    if not (bandwidth > 0 and np.isfinite(bandwidth)):
        raise ValueError('bandwidth must be positive and finite')
    return np.ascontiguousarray(levels), off, np.ascontiguousarray(x)


KEST_MAX_KEYS = 1 << 24    # the key limit of tba_region_key_levels


def _check_region_key_levels_args(read_start, read_minus, read_off, means, reg_read_off, reg_reads, pos_reg, pos_g,
                                  ent_pos, ent_key, n_keys):
    """the argument checks of Engine.region_key_levels (shared with the tests' stand-in engine): dtypes are checked,
    not converted; every index is checked against the array it points into -> the contiguous arrays, in order"""
    rs, rm, m = np.asarray(read_start), np.asarray(read_minus), np.asarray(means)
    rr, pr, pg, ep, ek = (np.asarray(v) for v in (reg_reads, pos_reg, pos_g, ent_pos, ent_key))
    if rs.dtype != np.int64 or rm.dtype != np.uint8 or m.dtype != np.float64:
        raise ValueError('read_start must be int64, read_minus uint8, means float64')
    if any(v.dtype != np.int64 or v.ndim != 1 for v in (rr, pr, pg, ep, ek)):
        raise ValueError('reg_reads, pos_reg, pos_g, ent_pos and ent_key must be one-dimensional int64 arrays')
    off, roff = _check_offsets(read_off, 'read_off'), _check_offsets(reg_read_off, 'reg_read_off')
    n_reads, n_regions = off.shape[0] - 1, roff.shape[0] - 1
    if rs.shape != (n_reads,) or rm.shape != (n_reads,) or m.shape != (int(off[-1]),):
        raise ValueError('per-read arrays, levels and offsets disagree')
    if n_reads >= 2 ** 31 or ep.shape[0] >= 2 ** 31:
        raise ValueError('a call holds fewer than 2**31 reads and entries')
    if rr.shape[0] != int(roff[-1]) or (rr.shape[0] and (rr.min() < 0 or rr.max() >= n_reads)):
        raise ValueError('reg_reads must hold reg_read_off[-1] indices of reads of the batch')
    if pr.shape != pg.shape or (pr.shape[0] and (pr.min() < 0 or pr.max() >= n_regions)):
        raise ValueError('pos_reg and pos_g must have one entry per position, pos_reg naming a region of the batch')
    if int(n_keys) != n_keys or not 1 <= n_keys <= KEST_MAX_KEYS:
        raise ValueError('n_keys must be an integer in [1, %d]' % KEST_MAX_KEYS)
    if ep.shape != ek.shape or (ep.shape[0] and (ep.min() < 0 or ep.max() >= pr.shape[0] or ek.min() < 0 or
                                                 ek.max() >= n_keys)):
        raise ValueError('ent_pos and ent_key must have one entry per entry, naming a position and a key of the batch')
    return tuple(np.ascontiguousarray(v) for v in (rs, rm, off, m, roff, rr, pr, pg, ep, ek))


def _check_segment_medians_args(values, off):
    """the argument checks of Engine.segment_medians -> contiguous (values, off)"""
    values = np.asarray(values)
    if values.dtype != np.float64 or values.ndim != 1:
        raise ValueError('values must be a one-dimensional float64 array')
    off = _check_offsets(off, 'off')
    if values.shape[0] != int(off[-1]):
        raise ValueError('values and offsets disagree')
    if off.shape[0] > 1 and np.diff(off).max() >= 2 ** 31:
        raise ValueError('a segment holds fewer than 2**31 values')
    return np.ascontiguousarray(values), off


def _check_center_prepare_args(raws, codes, event_starts, read_start_rel_to_raw, num_events, rna):
    """the argument checks of Engine.center_prepare -> (flat samples, raw_off, flat codes, seq_off, flat starts,
    start_off, read_start_rel_to_raw, num_events or None).  The samples: int16 when every read is, else float64"""
    n = len(raws)
    if n == 0:
        raise ValueError('no reads')
    if n > 65535:
        raise ValueError('more than TBA_MAX_BATCH_READS reads in one call')
    if len(codes) != n or len(event_starts) != n:
        raise ValueError('one sequence and one start column per read')
    raws = [np.asarray(r) for r in raws]
    if any(r.ndim != 1 or r.dtype.kind not in 'iuf' for r in raws):
        raise ValueError('the raw signals must be one-dimensional numeric arrays')
    dt = np.dtype(np.int16) if all(r.dtype == np.int16 for r in raws) else np.dtype(np.float64)
    codes = [np.asarray(c) for c in codes]
    if any(c.ndim != 1 or c.dtype != np.uint8 for c in codes):
        raise ValueError('the sequences must be one-dimensional uint8 code arrays')
    starts = [np.asarray(s) for s in event_starts]
    if any(s.ndim != 1 or s.dtype.kind not in 'iu' for s in starts):
        raise ValueError('the start columns must be one-dimensional integer arrays')
    rsr = _i64(read_start_rel_to_raw)
    if rsr.shape != (n,):
        raise ValueError('one read_start_rel_to_raw per read')
    if num_events is not None:
        num_events = _i64(num_events)
        if num_events.shape != (n,) or (num_events < 1).any():
            raise ValueError('one positive num_events per read')
    elif rna:
        raise ValueError('RNA reads need num_events')
    raw = np.concatenate(raws).astype(dt, copy=False) if n else np.zeros(0, dt)
    return (np.ascontiguousarray(raw), _offsets(raws), np.ascontiguousarray(np.concatenate(codes)), _offsets(codes),
            np.ascontiguousarray(np.concatenate(starts), dtype=np.int64), _offsets(starts), rsr, num_events)


def _check_center_fit_args(n_reads, n_points, samp_ind, prior, max_reads):
    """the argument checks of Engine.center_fit -> (samp_ind int64 [n, 1000] or None, prior float64 [m, 2]).
    n_points: the points of every read of the prepared batch (bases - kmer_width + 1)"""
    if n_reads is None:
        raise ValueError('center_prepare has not been called')
    if int(max_reads) < 1:
        raise ValueError('max_reads must be positive')
    if samp_ind is not None:
        samp_ind = _i64(samp_ind)
        if samp_ind.shape != (n_reads, MAX_POINTS_FOR_THEIL_SEN):
            raise ValueError('samp_ind must be int64 [n_reads, %d] (pack_samp_inds)' % MAX_POINTS_FOR_THEIL_SEN)
        # (a row of -1 marks a read without a draw, and the kernel checks every index it takes against the read's
        # points: a bad row fails that read alone)
    elif (np.asarray(n_points) > MAX_POINTS_FOR_THEIL_SEN).any():
        raise ValueError('a read of more than %d points needs samp_ind' % MAX_POINTS_FOR_THEIL_SEN)
    prior = np.zeros((0, 2), np.float64) if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
    if prior.ndim != 2 or prior.shape[1] != 2:
        raise ValueError('prior must be float64 [m, 2]: the factors of the earlier successes')
    return samp_ind, prior


NORMTYPE_NONE, NORMTYPE_PA_RAW, NORMTYPE_MEDIAN, NORMTYPE_MEDIAN_CONST_SCALE, NORMTYPE_ROBUST_MEDIAN = range(5)


def _check_normalize_raw_args(raws, starts, lens, norm_type, sv_in, sv_flags, channel):
    """the argument checks of Engine.normalize_raw_batch -> (dtype, flat samples, raw_off, starts, lens)"""
    n = len(raws)
    if n == 0:
        raise ValueError('no reads')
    raws = [np.asarray(r) for r in raws]
    dt = raws[0].dtype
    if dt not in (np.dtype(np.int16), np.dtype(np.float64)) or any(r.dtype != dt or r.ndim != 1 for r in raws):
        raise ValueError('the raw signals must be one-dimensional arrays, all int16 or all float64')
    if norm_type not in range(5):
        raise ValueError('unknown norm type')
    starts, lens = _i64(starts), _i64(lens)
    sizes = np.array([r.shape[0] for r in raws], dtype=np.int64)
    if starts.shape != (n,) or lens.shape != (n,):
        raise ValueError('one start and one length per read')
    if (starts < 0).any() or (lens < 1).any() or (starts + lens > sizes).any() or (lens >= 2 ** 31).any():
        raise ValueError('a window is empty or does not lie inside its read')
    if (sv_in is None) != (sv_flags is None):
        raise ValueError('scale values and their flags come together')
    if sv_in is not None and (sv_in.dtype != np.float64 or sv_in.shape != (n, 4) or sv_flags.dtype != np.int32
                              or sv_flags.shape != (n,)):
        raise ValueError('sv_in must be float64 [n, 4] and sv_flags int32 [n]')
    if channel is not None and (channel.dtype != np.float64 or channel.shape != (n, 3)):
        raise ValueError('channel must be float64 [n, 3]: offset, range, digitisation')
    if norm_type == NORMTYPE_PA_RAW and channel is None and (sv_flags is None or not (sv_flags & 1).all()):
        raise ValueError('pA_raw needs the channel values')
    return dt, np.ascontiguousarray(np.concatenate(raws)), _offsets(raws), starts, lens


TRIM_TOO_FEW_EVENTS = 23    # TBA_TRIM_TOO_FEW_EVENTS: a read with too few events for the windows of trim_rna
TRIM_MAX_WINDOW = 8192      # the widest moving_window_size tba_trim_rna_batch takes


def _check_raw_reads(raws, min_len=0):
    """the reads of Engine.trim_rna / Engine.raw_med_mad: one-dimensional arrays, all int16 or all float64 (checked,
    not converted) -> (dtype, the arrays)"""
    raws = [np.asarray(r) for r in raws]
    dt = raws[0].dtype if raws else np.dtype(np.float64)
    if dt not in (np.dtype(np.int16), np.dtype(np.float64)) or any(r.dtype != dt or r.ndim != 1 for r in raws):
        raise ValueError('the raw signals must be one-dimensional arrays, all int16 or all float64')
    if any(r.shape[0] < min_len for r in raws):
        raise ValueError('every read needs %d sample(s) or more' % min_len)
    return dt, raws


def _check_trim_rna_args(raws, seg_params, trim_params):
    """the argument checks of Engine.trim_rna (shared with the tests' stand-in engine) -> (dtype, the reads' prefixes,
    (running_stat_width, min_obs_per_base, mean_obs_per_event), (moving_window_size, min_running_values, thresh_scale,
    max_raw_obs))"""
    seg, trim = tuple(seg_params), tuple(trim_params)
    if len(seg) != 3 or any(int(v) != v or v < 1 for v in seg):
        raise ValueError('seg_params must be (running_stat_width, min_obs_per_base, mean_obs_per_event), integers of 1 '
                         'or more')
    if len(trim) != 4 or any(int(v) != v or v < 1 for v in (trim[0], trim[1], trim[3])):
        raise ValueError('trim_params must be (moving_window_size, min_running_values, thresh_scale, max_raw_obs), the '
                         'sizes integers of 1 or more')
    if trim[0] > TRIM_MAX_WINDOW:
        raise ValueError('moving_window_size above %d' % TRIM_MAX_WINDOW)
    thresh_scale = float(trim[2])
    if thresh_scale != thresh_scale:
        raise ValueError('thresh_scale must be a number')
    dt, raws = _check_raw_reads(raws)
    mro = int(trim[3])
    if mro >= 2 ** 31 and any(r.shape[0] >= 2 ** 31 for r in raws):
        raise ValueError('a prefix holds fewer than 2**31 samples')
    return (dt, [r[:mro] for r in raws], tuple(int(v) for v in seg),
            (int(trim[0]), int(trim[1]), thresh_scale, mro))


def _check_point_arrays(off, *arrays):
    """offsets and the float64 arrays they cut into reads -> contiguous (off, *arrays)"""
    off = _check_offsets(off, 'off')
    out = []
    for a in arrays:
        a = np.asarray(a)
        if a.dtype != np.float64 or a.ndim != 1 or a.shape[0] != int(off[-1]):
            raise ValueError('float64 arrays of the length the offsets end at')
        out.append(np.ascontiguousarray(a))
    return (off,) + tuple(out)


def _check_fractions(q, what):
    """quantile fractions (what np.true_divide(q, 100) gives) -> contiguous float64[n]; None: none"""
    if q is None:
        return np.empty(0, dtype=np.float64)
    q = np.asarray(q)
    if q.dtype != np.float64 or q.ndim != 1:
        raise ValueError('%s must be a one-dimensional float64 array of fractions' % what)
    if q.shape[0] and not ((q >= 0.0) & (q <= 1.0)).all():
        raise ValueError('%s must lie in [0, 1]' % what)
    return np.ascontiguousarray(q)


PLOT_COORD_MAX = 1 << 62    # genomic coordinates of the plot entries lie inside (-2**62, 2**62)


def _check_region_level_piles_args(read_start, read_minus, read_off, means, reg_read_off, reg_reads, reg_start, reg_end,
                                   q_linear, q_nearest):
    """the argument checks of Engine.region_level_piles (shared with the tests' stand-in engine): dtypes are checked,
    not converted; every index is checked against the array it points into -> the contiguous arrays, in order, and
    the capacity the levels need (the reads' overlaps with their regions)"""
    rs, rm, m = np.asarray(read_start), np.asarray(read_minus), np.asarray(means)
    rr, st, en = np.asarray(reg_reads), np.asarray(reg_start), np.asarray(reg_end)
    if rs.dtype != np.int64 or rm.dtype != np.uint8 or m.dtype != np.float64:
        raise ValueError('read_start must be int64, read_minus uint8, means float64')
    if any(v.dtype != np.int64 or v.ndim != 1 for v in (rr, st, en)):
        raise ValueError('reg_reads, reg_start and reg_end must be one-dimensional int64 arrays')
    ql, qn = _check_fractions(q_linear, 'q_linear'), _check_fractions(q_nearest, 'q_nearest')
    off, roff = _check_offsets(read_off, 'read_off'), _check_offsets(reg_read_off, 'reg_read_off')
    n_reads, n_regions = off.shape[0] - 1, roff.shape[0] - 1
    if rs.shape != (n_reads,) or rm.shape != (n_reads,) or m.shape != (int(off[-1]),):
        raise ValueError('per-read arrays, levels and offsets disagree')
    if n_reads >= 2 ** 31:
        raise ValueError('a call holds fewer than 2**31 reads')
    if rr.shape[0] != int(roff[-1]) or (rr.shape[0] and (rr.min() < 0 or rr.max() >= n_reads)):
        raise ValueError('reg_reads must hold reg_read_off[-1] indices of reads of the batch')
    if st.shape != (n_regions,) or en.shape != (n_regions,):
        raise ValueError('reg_start and reg_end must have one entry per region')
    if any(v.shape[0] and (v.min() <= -PLOT_COORD_MAX or v.max() >= PLOT_COORD_MAX) for v in (rs, st, en)):
        raise ValueError('coordinates must lie inside (-2**62, 2**62)')
    if n_regions and (en <= st).any():
        raise ValueError('every region needs reg_start < reg_end')
    if n_regions and (np.diff(roff).max() >= 2 ** 31 or int((en - st).sum()) >= 2 ** 31):
        raise ValueError('a pile holds fewer than 2**31 levels and a call fewer than 2**31 positions')
    rep = np.repeat(np.arange(n_regions), np.diff(roff))
    cap = int(np.maximum(np.minimum(rs[rr] + np.diff(off)[rr], en[rep]) - np.maximum(rs[rr], st[rep]), 0).sum())
    return tuple(np.ascontiguousarray(v) for v in (rs, rm, off, m, roff, rr, st, en, ql, qn)) + (cap,)


def _check_segment_percentiles_args(values, off, q_linear, q_nearest):
    """the argument checks of Engine.segment_percentiles -> contiguous (values, off, q_linear, q_nearest)"""
    v, off = _check_segment_medians_args(values, off)
    if off.shape[0] - 1 >= 2 ** 31:
        raise ValueError('a call holds fewer than 2**31 segments')
    return v, off, _check_fractions(q_linear, 'q_linear'), _check_fractions(q_nearest, 'q_nearest')


def _check_dwell_pairs(pairs):
    """[(percentile, threshold), ...] of an observations-per-base filter -> (q float64[n] as numpy divides the
    percentiles out, thresh float64[n]) (shared with the tests' stand-in engine)"""
    pairs = list(pairs)
    if len(pairs) < 1 or any(len(p) != 2 for p in pairs):
        raise ValueError('pairs must be one or more (percentile, threshold)')
    q = np.true_divide(np.array([p[0] for p in pairs], dtype=np.float64), 100)
    thresh = np.array([p[1] for p in pairs], dtype=np.float64)
    if not ((q >= 0.0) & (q <= 1.0)).all() or np.isnan(thresh).any():
        raise ValueError('percentiles must lie in [0, 100] and thresholds must not be NaN')
    return q, thresh


def _check_dwell_pctl_args(segs, seg_off, pairs):
    """the argument checks of Engine.dwell_pctl_flags (shared with the tests' stand-in engine): dtypes are checked,
    not converted -> contiguous (segs, seg_off, q, thresh)"""
    segs = np.asarray(segs)
    if segs.dtype != np.int64 or segs.ndim != 1:
        raise ValueError('segs must be a one-dimensional int64 array')
    off = _check_offsets(seg_off, 'seg_off')
    if segs.shape[0] != int(off[-1]):
        raise ValueError('segs and offsets disagree')
    q, thresh = _check_dwell_pairs(pairs)
    if segs.shape[0] > 1:
        inside = np.ones(segs.shape[0] - 1, dtype=bool)
        inside[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < segs.shape[0])] - 1] = False   # steps from one read to the next
        d = np.diff(segs)[inside]
        if (d < 0).any() or (d >= 2 ** 31).any():
            raise ValueError('the boundaries of a read must not decrease and a length stays below 2**31')
    if off.shape[0] > 1 and np.diff(off).max() >= 2 ** 31:
        raise ValueError('a read holds fewer than 2**31 boundaries')
    return np.ascontiguousarray(segs), off, q, thresh


def raw_signal_fits(segs, read_start_rel_to_raw, n_raw):
    """whether a read's segments (the Events start column and the end) address its raw signal of n_raw samples
    whichever bases are taken: at least one base, non-decreasing from 0 or above, read_start_rel_to_raw >= 0, the
    last end inside the signal.  A read that fails is left out of a region_raw_signal call (the host's form of the
    reference's try / except round th.get_raw_signal)"""
    segs = np.asarray(segs)
    return bool(segs.ndim == 1 and segs.shape[0] >= 2 and segs[0] >= 0 and (np.diff(segs) >= 0).all() and
                0 <= read_start_rel_to_raw and read_start_rel_to_raw + int(segs[-1]) <= n_raw and
                int(segs[-1]) - int(segs[0]) < 2 ** 31)


def _check_region_raw_signal_args(raw, raw_off, segs, segs_off, read_start, rsrtr, minus, rna, shift, scale, lower_lim,
                                  upper_lim, pair_read, pair_start, pair_end):
    """the argument checks of Engine.region_raw_signal (shared with the tests' stand-in engine): dtypes are checked,
    not converted (raw: int16 or int32 as stored); every index and offset is checked against the array it points
    into -> the contiguous arrays, in order, and the samples of every pair"""
    raw, segs = np.asarray(raw), np.asarray(segs)
    if raw.dtype not in (np.dtype(np.int16), np.dtype(np.int32)) or raw.ndim != 1:
        raise ValueError('raw must be a one-dimensional int16 or int32 array')
    i8 = [np.asarray(v) for v in (segs, read_start, rsrtr, pair_read, pair_start, pair_end)]
    u1 = [np.asarray(v) for v in (minus, rna)]
    f8 = [np.asarray(v) for v in (shift, scale, lower_lim, upper_lim)]
    if any(v.dtype != np.int64 or v.ndim != 1 for v in i8) or any(v.dtype != np.uint8 or v.ndim != 1 for v in u1) or \
            any(v.dtype != np.float64 or v.ndim != 1 for v in f8):
        raise ValueError('segs, read_start, rsrtr and the pair arrays must be int64, minus and rna uint8, shift, scale '
                         'and the limits float64, all one-dimensional')
    roff, soff = _check_offsets(raw_off, 'raw_off'), _check_offsets(segs_off, 'segs_off')
    n_reads = roff.shape[0] - 1
    segs, rs, rsr, pr, ps, pe = i8
    if soff.shape[0] != n_reads + 1 or raw.shape[0] != int(roff[-1]) or segs.shape[0] != int(soff[-1]) or \
            any(v.shape != (n_reads,) for v in [rs, rsr] + u1 + f8):
        raise ValueError('per-read arrays, raw signal, segments and offsets disagree')
    if n_reads >= 2 ** 31 or pr.shape[0] >= 2 ** 31:
        raise ValueError('a call holds fewer than 2**31 reads and pairs')
    # raw_signal_fits for every read at once
    if n_reads:
        if np.diff(soff).min() < 2:
            raise ValueError('the segments of a read do not fit its raw signal: a read needs two entries or more')
        inside = np.ones(max(segs.shape[0] - 1, 0), dtype=bool)
        inside[soff[1:-1] - 1] = False                       # the steps from one read's end to the next read's start
        first, last = segs[soff[:-1]], segs[soff[1:] - 1]
        if (np.diff(segs)[inside] < 0).any() or (first < 0).any() or (rsr < 0).any() or \
                (last > np.diff(roff) - rsr).any() or (last - first >= 2 ** 31).any():
            raise ValueError('the segments of a read do not fit its raw signal')
    if pr.shape != ps.shape or pr.shape != pe.shape or (pr.shape[0] and (pr.min() < 0 or pr.max() >= n_reads)):
        raise ValueError('pair_read, pair_start and pair_end must have one entry per pair, pair_read naming a read of '
                         'the batch')
    if any(v.shape[0] and (v.min() <= -PLOT_COORD_MAX or v.max() >= PLOT_COORD_MAX) for v in (rs, ps, pe)):
        raise ValueError('coordinates must lie inside (-2**62, 2**62)')
    nb = np.diff(soff)[pr] - 1
    if pr.shape[0] and ((pe <= ps) | (ps >= rs[pr] + nb) | (pe <= rs[pr])).any():
        raise ValueError('every pair needs pair_start < pair_end and a read that overlaps the region')
    lo, hi = np.maximum(ps - rs[pr], 0), np.minimum(pe - rs[pr] + 1, nb + 1)
    mn = np.asarray(u1[0], dtype=bool)[pr]
    a, b = np.where(mn, nb - hi + 1, lo) + soff[pr], np.where(mn, nb - lo, hi - 1) + soff[pr]
    n_obs = (segs[b] - segs[a]) if pr.shape[0] else np.zeros(0, dtype=np.int64)
    return tuple(np.ascontiguousarray(v) for v in [raw, roff, segs, soff, rs, rsr] + u1 + f8 + [pr, ps, pe]) + (n_obs,)


TRK_TILE = 256      # TBA_TRK_TILE of include/tombo_amd.h: positions per tile of the genome-track pileup
TRK_MAX_SLOTS = 3
# what tracks_finish gives back: means / sums / slot_cov float64 / int64 [n_slots, window], read_cov int64 [window]
TrackSet = namedtuple('TrackSet', 'means sums slot_cov read_cov')


def _check_tracks_begin_args(win_start, win_end, n_slots):
    """the argument checks of Engine.tracks_begin (shared with the tests' stand-in engine)"""
    if int(win_start) != win_start or int(win_end) != win_end or not 0 <= win_start < win_end:
        raise ValueError('the window must be a non-empty integer interval at or above 0')
    if win_end - win_start >= 2 ** 31:
        raise ValueError('a window holds fewer than 2**31 positions')
    if int(n_slots) != n_slots or not 1 <= n_slots <= TRK_MAX_SLOTS:
        raise ValueError('n_slots must be an integer in [1, %d]' % TRK_MAX_SLOTS)


def _check_tracks_add_args(window, n_slots, read_start, read_end, read_flags, read_off, slots, tile_read_off,
                           tile_reads):
    """the argument checks of Engine.tracks_add (shared with the tests' stand-in engine): dtypes are checked, not
    converted -> contiguous (read_start, read_end, read_flags, read_off, slots, tile_read_off, tile_reads)"""
    rs, re_, fl, tr = np.asarray(read_start), np.asarray(read_end), np.asarray(read_flags), np.asarray(tile_reads)
    if rs.dtype != np.int64 or re_.dtype != np.int64 or fl.dtype != np.uint8 or tr.dtype != np.int32:
        raise ValueError('read_start and read_end must be int64, read_flags uint8, tile_reads int32')
    off, toff = _check_offsets(read_off, 'read_off'), _check_offsets(tile_read_off, 'tile_read_off')
    n = off.shape[0] - 1
    if not (rs.shape == re_.shape == fl.shape == (n,)) or tr.ndim != 1:
        raise ValueError('per-read arrays and offsets disagree')
    if n and ((re_ < rs).any() or (rs < 0).any()):
        raise ValueError('a read ends before its start or starts below 0')
    if n and (fl >> (1 + n_slots)).any():
        raise ValueError('read_flags name a slot the track set does not have')
    if toff.shape[0] - 1 != -(-window // TRK_TILE) or int(toff[-1]) != tr.shape[0]:
        raise ValueError('tile_read_off must have one entry per tile of %d positions, plus one, and end at '
                         'len(tile_reads)' % TRK_TILE)
    if tr.shape[0] and (tr.min() < 0 or tr.max() >= n):
        raise ValueError('tile_reads names a read outside the batch')
    slots = [np.asarray(v) for v in slots]
    if len(slots) != n_slots or any(v.dtype != np.float64 or v.shape != (int(off[-1]),) for v in slots):
        raise ValueError('slots must be n_slots float64 arrays of read_off[-1] values')
    return (np.ascontiguousarray(rs), np.ascontiguousarray(re_), np.ascontiguousarray(fl), off,
            [np.ascontiguousarray(v) for v in slots], toff, np.ascontiguousarray(tr))


def _check_track_pair(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float64 or b.dtype != np.float64 or a.ndim != 1 or a.shape != b.shape:
        raise ValueError('a and b must be one-dimensional float64 arrays of one length')
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _check_compact_args(values):
    """-> (contiguous values, mode): float64 -> 0 (the NaN filter), int64 -> 1 (run-length form)"""
    v = np.asarray(values)
    if v.ndim != 1 or v.dtype not in (np.dtype(np.float64), np.dtype(np.int64)):
        raise ValueError('values must be a one-dimensional float64 or int64 array')
    if v.dtype == np.int64 and v.shape[0] == 0:
        raise ValueError('the run-length form needs at least one value')
    return np.ascontiguousarray(v), int(v.dtype == np.int64)


# what one tba_site_fractions call gives back: the per-site arrays compacted per track at pos_off
# (counts[t] records from pos_off[t]), per track the number of statistics, the statistics themselves
SiteFractions = namedtuple('SiteFractions', 'pos_off frac poss cov valid damp counts n_stats per_read')


# the reads table and the (region, read) pairs of one tba_site_fractions_reads call; pos_off: the regions'
# extended positions [reg_start - fm_offset, reg_end + fm_offset); seq (uint8 base codes) None for form 1,
# pos_means / pos_sds (control levels per extended position) None for form 0
SiteReads = namedtuple('SiteReads', 'reg_start reg_end read_start read_strand read_off means seq reg_pair_off '
                                    'pair_read pos_means pos_sds fm_offset pos_off')


def site_reads_stat_bound(form, t, kmer_width=1, central_pos=0):
    """per pair of a SiteReads the number of statistics it yields when it does not fail (the geometry of
    tba_site_fractions_reads, vectorised): an upper bound of what the call produces"""
    rd = t.pair_read
    reg = np.repeat(np.arange(t.reg_start.shape[0], dtype=np.int64), np.diff(t.reg_pair_off))
    s = t.read_start[rd]
    e = s + np.diff(t.read_off)[rd]
    lag_b = lag_e = np.zeros(rd.shape[0], dtype=np.int64)
    if form == 0:
        dn, minus = kmer_width - central_pos - 1, t.read_strand[rd] != 0
        lag_b, lag_e = np.where(minus, dn, central_pos), np.where(minus, central_pos, dn)
    cs = np.maximum(s, t.reg_start[reg] - lag_b - t.fm_offset)
    ce = np.minimum(e, t.reg_end[reg] + lag_e + t.fm_offset)
    return np.maximum(ce - cs - lag_b - lag_e, 0).astype(np.int64)


def _check_site_reads_args(form, reg_start, reg_end, read_start, read_strand, read_off, means, seq, reg_pair_off,
                           pair_read, pos_means, pos_sds, fm_offset):
    """the argument checks of Engine.site_fractions_reads (shared with the tests' stand-in engine), those
    tba_site_fractions_reads makes: dtypes are checked, not converted -> SiteReads of contiguous arrays"""
    if form not in (0, 1):
        raise ValueError('form must be 0 (de_novo) or 1 (sample_compare)')
    if int(fm_offset) != fm_offset or fm_offset < 0 or fm_offset > 64:
        raise ValueError('fm_offset must be an integer in [0, 64]')
    fm = int(fm_offset)
    a = dict(reg_start=(reg_start, np.int64), reg_end=(reg_end, np.int64), read_start=(read_start, np.int64),
             read_strand=(read_strand, np.int8), means=(means, np.float64), pair_read=(pair_read, np.int64))
    if form == 0:
        a.update(seq=(seq, np.uint8))
    else:
        a.update(pos_means=(pos_means, np.float64), pos_sds=(pos_sds, np.float64))
    c = dict(seq=None, pos_means=None, pos_sds=None)
    for name, (arr, dt) in a.items():
        if arr is None:
            raise ValueError('%s is needed for form %d' % (name, form))
        arr = np.asarray(arr)
        if arr.dtype != dt or arr.ndim != 1:
            raise ValueError('%s must be a one-dimensional %s array' % (name, np.dtype(dt).name))
        c[name] = np.ascontiguousarray(arr)
    read_off, pair_off = _check_offsets(read_off, 'read_off'), _check_offsets(reg_pair_off, 'reg_pair_off')
    n_reg, n_reads = c['reg_start'].shape[0], c['read_start'].shape[0]
    if c['reg_end'].shape[0] != n_reg or pair_off.shape[0] != n_reg + 1:
        raise ValueError('reg_start, reg_end must have one entry per region and reg_pair_off one more')
    if c['read_strand'].shape[0] != n_reads or read_off.shape[0] != n_reads + 1:
        raise ValueError('read_start, read_strand must have one entry per read and read_off one more')
    if c['means'].shape[0] != int(read_off[-1]) or (form == 0 and c['seq'].shape[0] != int(read_off[-1])):
        raise ValueError('means%s must have read_off[-1] values' % (' and seq' if form == 0 else ''))
    if c['pair_read'].shape[0] != int(pair_off[-1]):
        raise ValueError('pair_read must have reg_pair_off[-1] values')
    if (c['reg_end'] <= c['reg_start']).any():
        raise ValueError('a region must have end > start')
    if ((c['read_strand'] != 0) & (c['read_strand'] != 1)).any():
        raise ValueError('read_strand must be 0 or 1')
    pos_off = np.concatenate([[0], np.cumsum(c['reg_end'] - c['reg_start'] + 2 * fm)]).astype(np.int64)
    if int(pos_off[-1]) >= 2 ** 31:
        raise ValueError('2^31 positions or more in one call')
    if form == 1 and not (c['pos_means'].shape[0] == c['pos_sds'].shape[0] == int(pos_off[-1])):
        raise ValueError('pos_means and pos_sds must have one value per extended position')
    rd = c['pair_read']
    if ((rd < 0) | (rd >= n_reads)).any():
        raise ValueError('pair_read outside [0, n_reads)')
    reg = np.repeat(np.arange(n_reg, dtype=np.int64), np.diff(pair_off))
    s = c['read_start'][rd]
    if ((s >= c['reg_end'][reg]) | (s + np.diff(read_off)[rd] <= c['reg_start'][reg])).any():
        raise ValueError('a read does not overlap its region')
    return SiteReads(c['reg_start'], c['reg_end'], c['read_start'], c['read_strand'], read_off, c['means'], c['seq'],
                     pair_off, rd, c['pos_means'], c['pos_sds'], fm, pos_off)


# a stored per-read record (PerReadStats block_stats): numpy's packed layout, 16 bytes, the float64 at offset 4
PER_READ_DTYPE = np.dtype([('pos', 'u4'), ('stat', 'f8'), ('read_id', 'u4')])


def _check_site_aggregate_args(blk_start, blk_end, rec_off, records):
    """-> contiguous (blk_start, blk_end, rec_off, records) of site_aggregate, or ValueError"""
    bs, be, off = (np.ascontiguousarray(np.asarray(v, dtype=np.int64)) for v in (blk_start, blk_end, rec_off))
    rec = np.asarray(records)
    if bs.ndim != 1 or be.shape != bs.shape or off.shape != (bs.shape[0] + 1,):
        raise ValueError('blk_start, blk_end must have one entry per block and rec_off one more')
    if rec.dtype != PER_READ_DTYPE or rec.ndim != 1:
        raise ValueError("records must be a one-dimensional array of the stored per-read layout "
                         "[('pos', 'u4'), ('stat', 'f8'), ('read_id', 'u4')] (packed, 16 bytes)")
    if off[0] != 0 or np.any(np.diff(off) < 0) or int(off[-1]) != rec.shape[0]:
        raise ValueError('rec_off must start at 0, not decrease and end at len(records)')
    if np.any(be <= bs):
        raise ValueError('a block must have end > start')
    if int((be - bs).sum()) >= 2 ** 31:
        raise ValueError('2^31 positions or more in one call')
    return bs, be, off, np.ascontiguousarray(rec)


ROC_SORT_TILE = 4096   # ROC_SORT_TILE of csrc/k_roc.h (tba_roc_sort_tile): entries per workgroup and pass of the sort
ROC_MAX_MOTIFS = 64


def _check_roc_recs(rec_off, rec_pos, rec_stat, n_blocks):
    off, pos, stat = np.asarray(rec_off), np.asarray(rec_pos), np.asarray(rec_stat)
    if off.dtype != np.int64 or pos.dtype != np.int64 or stat.dtype != np.float64:
        raise ValueError('rec_off and rec_pos must be int64, rec_stat float64')
    if off.ndim != 1 or off.shape[0] != n_blocks + 1 or pos.ndim != 1 or stat.shape != pos.shape:
        raise ValueError('rec_off must have one entry per block and one more, rec_pos and rec_stat one per record')
    if off[0] != 0 or np.any(np.diff(off) < 0) or int(off[-1]) != pos.shape[0]:
        raise ValueError('rec_off must start at 0, not decrease and end at len(rec_pos)')
    if pos.shape[0] >= 2 ** 31:
        raise ValueError('2^31 records or more in one call')
    return tuple(np.ascontiguousarray(v) for v in (off, pos, stat))


def _check_roc_motif_args(blk_minus, blk_seq_start, seq_off, seq_codes, rec_off, rec_pos, rec_stat, motifs):
    """the argument checks of Engine.roc_motif_labels (shared with the tests' stand-in engine): dtypes are checked,
    not converted -> contiguous (blk_minus, blk_seq_start, seq_off, seq_codes, rec_off, rec_pos, rec_stat, motif table
    int32[n][3], concatenated sets uint8)"""
    minus, ss, s_off, seq = (np.asarray(v) for v in (blk_minus, blk_seq_start, seq_off, seq_codes))
    if minus.dtype != np.uint8 or seq.dtype != np.uint8 or ss.dtype != np.int64 or s_off.dtype != np.int64:
        raise ValueError('blk_minus and seq_codes must be uint8, blk_seq_start and seq_off int64')
    n_blk = minus.shape[0]
    if minus.ndim != 1 or ss.shape != (n_blk,) or s_off.shape != (n_blk + 1,) or seq.ndim != 1:
        raise ValueError('blk_minus, blk_seq_start must have one entry per block and seq_off one more')
    if s_off[0] != 0 or np.any(np.diff(s_off) < 0) or int(s_off[-1]) != seq.shape[0]:
        raise ValueError('seq_off must start at 0, not decrease and end at len(seq_codes)')
    off, pos, stat = _check_roc_recs(rec_off, rec_pos, rec_stat, n_blk)
    if not 1 <= len(motifs) <= ROC_MAX_MOTIFS:
        raise ValueError('between 1 and %d motifs' % ROC_MAX_MOTIFS)
    table, sets = np.empty((len(motifs), 3), dtype=np.int32), []
    for k, (length, mod_pos, mod_base, base_sets) in enumerate(motifs):
        base_sets = np.asarray(base_sets)
        if base_sets.dtype != np.uint8 or base_sets.shape != (length,) or not 1 <= length <= 1024 or \
                np.any(base_sets > 15):
            raise ValueError('a motif needs one 4-bit base set (uint8) per position, 1 to 1024 positions')
        if not 1 <= mod_pos <= length:
            raise ValueError('mod_pos outside the motif')
        table[k] = length, mod_pos, mod_base if 0 <= mod_base <= 3 else 255
        sets.append(base_sets)
    return tuple(np.ascontiguousarray(v) for v in (minus, ss, s_off, seq)) + (off, pos, stat, table,
                                                                              np.ascontiguousarray(np.concatenate(sets)))


def _check_roc_loc_args(blk_loc, mod_locs, unmod_locs, rec_off, rec_pos, rec_stat):
    """-> contiguous (blk_loc int64[n][4], mod_locs, unmod_locs, rec_off, rec_pos, rec_stat) of roc_loc_labels"""
    loc, mod, unmod = np.asarray(blk_loc), np.asarray(mod_locs), np.asarray(unmod_locs)
    if loc.dtype != np.int64 or mod.dtype != np.int64 or unmod.dtype != np.int64:
        raise ValueError('blk_loc, mod_locs and unmod_locs must be int64')
    if loc.ndim != 2 or loc.shape[1] != 4 or mod.ndim != 1 or unmod.ndim != 1:
        raise ValueError('blk_loc must be [n_blocks][4]: mod lo, hi, unmod lo, hi')
    if np.any(loc < 0) or np.any(loc[:, 1] < loc[:, 0]) or np.any(loc[:, 3] < loc[:, 2]) or \
            np.any(loc[:, 1] > mod.shape[0]) or np.any(loc[:, 3] > unmod.shape[0]):
        raise ValueError('location slice outside its list')
    for v, lo, hi in ((mod, loc[:, 0], loc[:, 1]), (unmod, loc[:, 2], loc[:, 3])):
        drops = np.concatenate([[0], np.cumsum(np.diff(v) < 0)])   # drops[i]: descents before element i
        last = v.shape[0] - 1
        if v.shape[0] and np.any(drops[np.minimum(np.maximum(hi - 1, lo), last)] - drops[np.minimum(lo, last)] > 0):
            raise ValueError('a location slice must be ascending')
    off, pos, stat = _check_roc_recs(rec_off, rec_pos, rec_stat, loc.shape[0])
    return (np.ascontiguousarray(loc), np.ascontiguousarray(mod), np.ascontiguousarray(unmod), off, pos, stat)


def _check_roc_rank_args(stats, has_mod, ranks):
    """-> contiguous (stats float64, has_mod as uint8, ranks int64) of roc_rank_counts"""
    st, hm, rk = np.asarray(stats), np.asarray(has_mod), np.asarray(ranks)
    if st.dtype != np.float64 or hm.dtype != np.bool_ or rk.dtype != np.int64:
        raise ValueError('stats must be float64, has_mod bool, ranks int64')
    if st.ndim != 1 or hm.shape != st.shape or rk.ndim != 1:
        raise ValueError('stats and has_mod must be one-dimensional and of one length, ranks one-dimensional')
    n = st.shape[0]
    if n >= 2 ** 31:
        raise ValueError('2^31 entries or more in one call')
    if rk.shape[0] and (rk[0] < 0 or rk[-1] >= n or np.any(np.diff(rk) < 0)):
        raise ValueError('ranks must be non-decreasing and inside [0, n)')
    return np.ascontiguousarray(st), np.ascontiguousarray(hm).view(np.uint8), np.ascontiguousarray(rk)


PDIST_TILE = 16           # PDIST_TILE of csrc/k_pdist.h (tba_pdist_tile): rows per side of a workgroup's tile of pairs
PDIST_LDS_ROW_MAX = 255   # PDIST_LDS_ROW_MAX (tba_pdist_lds_row_max): longer rows are read from global memory
PDIST_MAX_ROWS, PDIST_MAX_ELEMS = 16384, 2 ** 28


def _check_pdist_rows(rows, slide_span=0):
    """the argument checks of Engine.pairwise_window_dists / pairwise_nanmean_dists (shared with the tests' stand-in
    engine): the dtype and the layout are checked, not converted -> rows"""
    rows = np.asarray(rows)
    if rows.dtype != np.float64 or rows.ndim != 2 or not rows.flags.c_contiguous:
        raise ValueError('rows must be a C-contiguous two-dimensional float64 array')
    if rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError('rows must have at least one row and one column')
    if rows.shape[0] > PDIST_MAX_ROWS or rows.size > PDIST_MAX_ELEMS:
        raise ValueError('at most %d rows and 2^28 values in one call' % PDIST_MAX_ROWS)
    if int(slide_span) != slide_span or slide_span < 0 or rows.shape[1] - 2 * int(slide_span) < 1:
        raise ValueError('slide_span must be an integer >= 0 that leaves a window of at least one value')
    return rows


def _site_outputs(starts, ends, damp_counts):
    """both site entries, tracks [starts[t], ends[t]) -> (pos_off, SiteFractions' frac .. n_stats)"""
    pos_off = np.concatenate([[0], np.cumsum(ends - starts)]).astype(np.int64)
    n_trk, n_pos = starts.shape[0], int(pos_off[-1])
    frac = np.empty(n_pos, dtype=np.float64)
    poss, cov, valid = (np.empty(n_pos, dtype=np.int64) for _ in range(3))
    damp = None if damp_counts is None else np.empty(n_pos, dtype=np.float64)
    return pos_off, (frac, poss, cov, valid, damp, np.zeros(n_trk, dtype=np.int64), np.zeros(n_trk, dtype=np.int64))


def _roc_label_outputs(cap, n_counts, return_index):
    """-> (stats, labels, record index or None, counts) of a ROC label entry"""
    return (np.empty(cap, dtype=np.float64), np.empty(cap, dtype=np.uint8),
            np.empty(cap, dtype=np.int64) if return_index else None, np.zeros(n_counts, dtype=np.int64))


def make_params(rp):
    p = Params()
    p.match_evalue, p.skip_pen = rp.match_evalue, rp.skip_pen
    p.do_winsorize_z = 0 if rp.max_half_z_score is None else 1
    p.max_half_z_score = 0.0 if rp.max_half_z_score is None else rp.max_half_z_score
    p.z_shift, p.stay_pen = rp.z_shift, rp.stay_pen
    for n in ('bandwidth', 'running_stat_width', 'min_obs_per_base', 'raw_min_obs_per_base',
              'mean_obs_per_event', 'band_bound_thresh', 'start_bw', 'start_save_bw',
              'start_n_bases'):
        setattr(p, n, int(getattr(rp, n)))
    p.use_t_test_seg = int(bool(rp.use_t_test_seg))
    return p


def make_opts(outlier_thresh=None, const_scale=None, skip_seq_scaling=False,
              sig_match_thresh=None, max_raw_cpts=200, min_event_to_seq_ratio=1.1,
              skip_norm_out=False, reverse_raw=False, stall_params=None, subsample_seed=None,
              del_fix_window=2, max_del_fix_window=10, extra_sig_factor=1.1, subsample_first_read=0,
              seq_samp_type=None):
    """tba_opts.  `seq_samp_type` (a th.seqSampleType): `sig_match_thresh` is that sample type's
    SIG_MATCH_THRESH unless given; `reverse_raw` / `stall_params` (a th.stallParams of the running-window-mean
    method): the worker's RNA preparation on the device (resquiggle.py:1506-1530);
    `subsample_seed` (int): the Theil-Sen subsample is drawn on the device;
    `del_fix_window` / `max_del_fix_window` / `extra_sig_factor`: the keyword arguments of
    resolve_skipped_bases_with_raw (resquiggle.py:405-407)."""
    if sig_match_thresh is None and seq_samp_type is not None:
        sig_match_thresh = SIG_MATCH_THRESH[seq_samp_type.name]
    o = Opts()
    o.del_fix_window, o.max_del_fix_window = int(del_fix_window), int(max_del_fix_window)
    o.extra_sig_factor = float(extra_sig_factor)
    o.reverse_raw = int(bool(reverse_raw))
    if stall_params is not None:
        sp = stall_params
        if sp.n_windows is None or sp.mini_window_size is None or \
                getattr(sp, 'lower_pctl', None) is not None:
            raise NotImplementedError('only the running-window-mean stall detector '
                                      '(MEAN_STALL_PARAMS, the reference default) is on the device')
        o.detect_stalls = 1
        o.stall_window_size, o.stall_n_windows = int(sp.window_size), int(sp.n_windows)
        o.stall_mini_window_size = int(sp.mini_window_size)
        o.stall_min_consecutive_obs, o.stall_edge_buffer = int(sp.min_consecutive_obs), int(sp.edge_buffer)
        o.stall_threshold = float(sp.threshold)
    if subsample_seed is not None:
        o.device_subsample, o.subsample_seed = 1, int(subsample_seed) & 0xffffffffffffffff
        o.subsample_first_read = int(subsample_first_read)   # (the draw of a read is keyed by its index in the JOB)
    o.has_outlier_thresh = int(outlier_thresh is not None)
    o.outlier_thresh = 0.0 if outlier_thresh is None else float(outlier_thresh)
    o.has_const_scale = int(const_scale is not None)
    o.const_scale = 0.0 if const_scale is None else float(const_scale)
    o.skip_seq_scaling = int(bool(skip_seq_scaling))
    o.check_start_score = int(sig_match_thresh is not None)
    o.sig_match_thresh = 0.0 if sig_match_thresh is None else float(sig_match_thresh)
    o.max_raw_cpts = -1 if max_raw_cpts is None else int(max_raw_cpts)
    o.min_event_to_seq_ratio = float(min_event_to_seq_ratio)
    o.use_rna_event_scale, o.rna_scale_num_events, o.rna_scale_max_frac_events = 1, 10000, 0.75
    o.skip_norm_out = int(bool(skip_norm_out))
    return o


class PinnedArray(object):
    """A numpy array over page-locked host memory (tba_pinned_alloc): uploads from it and
    downloads into it are asynchronous DMA transfers.  `.a` is the array; freed on close / GC."""

    def __init__(self, shape, dtype):
        self._L = lib()
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) if not np.isscalar(shape) else int(shape)
        self.nbytes = max(n * dtype.itemsize, 1)
        self._ptr = C.c_void_p()
        _call(self._L, 'tba_pinned_alloc', self.nbytes, C.byref(self._ptr))
        buf = (C.c_char * self.nbytes).from_address(self._ptr.value)
        self.a = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)

    def close(self):
        if getattr(self, '_ptr', None):
            self.a = None
            self._L.tba_pinned_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EngineError(RuntimeError):
    pass


class PinnedPool(object):
    """Process-wide pool of page-locked blocks that RESULTS live in.  `lease(count, dtype)` returns
    a fresh ndarray over a block (or None when the pool's budget is spent); every per-read result array
    is a view of it, and the block goes back to the pool when the last view is gone (the views keep the
    lease array alive; a finalizer on it returns the block).  Blocks are reused, never freed while the
    pool is under its idle cap: hipHostMalloc is slow and hipHostFree waits for all work on the device.

    Budget (bytes of page-locked memory this PROCESS may hold in the pool, leased to live results + idle):
    $TBA_PINNED_POOL_BYTES; default a quarter of the host's memory divided by the ranks of the node
    ($LOCAL_WORLD_SIZE, else $WORLD_SIZE, else 1) and at most 16 GiB -- page-locked memory cannot be swapped,
    and eight ranks with a quarter of the host each would have pinned twice the host.  Beyond the budget
    `lease` returns None and the caller copies into pageable memory, as every result did before round 5.
    NOTE for callers: one retained result keeps its whole batch block alive (segs + signal of every read of
    the batch); copy what is kept for long (`np.array(r.segs)`), or run with TBA_PINNED_POOL_BYTES=0."""

    @staticmethod
    def _alloc_bytes(need):
        return need + need // 16 + 4096         # (what a fresh block really takes: counted against the budget)

    def __init__(self):
        import threading
        self._lock = threading.RLock()   # (a finalizer may run -- and give a block back -- inside lease)
        self._idle = []          # PinnedArray blocks (uint8), by size
        self.leased_bytes = 0
        self.idle_bytes = 0
        env = os.environ.get('TBA_PINNED_POOL_BYTES')
        if env:
            self.budget = int(env)
        else:
            try:
                ranks = max(int(os.environ.get('LOCAL_WORLD_SIZE') or os.environ.get('WORLD_SIZE') or 1), 1)
            except ValueError:
                ranks = 1
            try:
                host = os.sysconf('SC_PHYS_PAGES') * os.sysconf('SC_PAGE_SIZE')
            except (ValueError, OSError):
                host = 32 << 30
            self.budget = min(host // 4 // ranks, 16 << 30)

    def lease(self, count, dtype):
        import weakref
        dtype = np.dtype(dtype)
        need = max(int(count) * dtype.itemsize, 1)
        drop = []
        with self._lock:
            best = None
            for k, pa in enumerate(self._idle):     # smallest idle block that holds it without wasting half
                if need <= pa.nbytes <= 2 * need + (1 << 20) and (best is None or pa.nbytes < self._idle[best].nbytes):
                    best = k
            pa = self._idle.pop(best) if best is not None else None
            fresh = self._alloc_bytes(need)
            if pa is not None:
                self.idle_bytes -= pa.nbytes
                self.leased_bytes += pa.nbytes
            else:
                # make room out of idle blocks of the wrong size before giving up
                while self._idle and self.leased_bytes + self.idle_bytes + fresh > self.budget:
                    old = self._idle.pop()
                    self.idle_bytes -= old.nbytes
                    drop.append(old)
                if self.leased_bytes + self.idle_bytes + fresh > self.budget:
                    fresh = 0
                else:
                    self.leased_bytes += fresh      # reserved before the lock goes: two threads cannot both take the last room
        for old in drop:                            # hipHostFree waits for the device: never under the lock
            old.close()
        if pa is None:
            if fresh == 0:
                return None
            try:
                pa = PinnedArray(fresh, np.uint8)
            except EngineError:
                with self._lock:
                    self.leased_bytes -= fresh
                return None
        buf = (C.c_char * pa.nbytes).from_address(pa._ptr.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(count))
        weakref.finalize(arr, self._give, pa)
        return arr

    def _give(self, pa):
        with self._lock:
            self.leased_bytes -= pa.nbytes
            self._idle.append(pa)
            self.idle_bytes += pa.nbytes

    def trim(self):
        """free the idle blocks (waits for the device: hipHostFree)"""
        with self._lock:
            idle, self._idle, self.idle_bytes = self._idle, [], 0
        for pa in idle:
            pa.close()


_result_pool = None


def result_pool():
    global _result_pool
    if _result_pool is None:
        _result_pool = PinnedPool()
    return _result_pool


class Engine(object):
    """One engine per process per GPU."""

    def __init__(self, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        self.device = int(device)
        self.kmer_width = self.central_pos = None
        self._model_key = None
        self._keep = self._keep_out = None    # the arrays of the upload / the downloads in flight
        self._stage = None                    # page-locked staging, made on first use (host_stage)
        self._ne_override = None              # set_num_events: event counts forced on the next upload
        self.skip_norm_out = False            # of the last upload's options
        _call(self._L, 'tba_engine_create', self.device, C.byref(self._h))

    def _call(self, name, *args):
        _call(self._L, name, self._h, *args)

    def close(self):
        if self._stage is not None:
            self._stage.close()
            self._stage = None
        if self._h:
            self._L.tba_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_model(self, level_means, level_sds, kmer_width, central_pos):
        m = np.ascontiguousarray(level_means, dtype=np.float64)
        s = np.ascontiguousarray(level_sds, dtype=np.float64)
        assert m.shape[0] == 4 ** kmer_width == s.shape[0]
        self._call('tba_set_model', m, s, kmer_width, central_pos)
        self.kmer_width, self.central_pos = int(kmer_width), int(central_pos)
        self._model_key = None

    def ensure_model(self, std_ref):
        """upload std_ref's level table unless the engine already holds the same table (compared
        by content: ids are reused after garbage collection and TomboModel arrays are mutable)"""
        import hashlib
        m = np.ascontiguousarray(std_ref.level_means, dtype=np.float64)
        sd = np.ascontiguousarray(std_ref.level_sds, dtype=np.float64)
        key = (int(std_ref.kmer_width), int(std_ref.central_pos),
               hashlib.blake2b(m.tobytes() + sd.tobytes(), digest_size=16).digest())
        if key != self._model_key:
            self.set_model(m, sd, std_ref.kmer_width, std_ref.central_pos)
            self._model_key = key

    def upload(self, params, opts, raws, seqs, sv_in=None, sv_flags=None, samp_ind=None,
               stall_ints=None):
        """raws: list of sample arrays (all int16, all float32, or anything else -> float64);
        seqs: list of uint8 code arrays."""
        raw, raw_off, seq, seq_off, _ = pack_code_reads(raws, seqs)
        st, sto = pack_stalls(stall_ints)
        self.upload_packed(params, opts, raw, raw_off, seq, seq_off, sv_in=sv_in,
                           sv_flags=sv_flags, samp_ind=samp_ind, stall_ints=st, stall_off=sto,
                           wait=True)

    def _batch_layout(self, params, opts, raw_off, seq_off):
        """the CSR layouts of the batch about to be uploaded (what `get` and the downloads index by) -> the two
        offset arrays as contiguous int64; takes the event counts set_num_events forced on this upload"""
        raw_off = np.ascontiguousarray(raw_off, dtype=np.int64)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        n = raw_off.shape[0] - 1
        self.n = n
        K = self.kmer_width
        self.raw_off, self.seq_off = raw_off, seq_off
        self.B = np.maximum(np.diff(seq_off) - K + 1, 0)
        self.ref_off = np.concatenate([[0], np.cumsum(self.B)]).astype(np.int64)
        self.seg_off = self.ref_off + np.arange(n + 1)
        n_raw = np.diff(raw_off)
        ne = np.maximum(n_raw // int(params.mean_obs_per_event),
                        (self.B * float(opts.min_event_to_seq_ratio)).astype(np.int64))
        ne[(self.B <= 0) | (n_raw <= 0)] = 0
        ov = self._ne_override
        if ov is not None and ov.shape[0] == n:
            ne = np.where((ov > 0) & (self.B > 0) & (n_raw > 0), ov, ne)
        self._ne_override = None
        self.num_events = ne
        self.ev_off = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
        self.n_raw_total = int(raw_off[-1])
        self.skip_norm_out = bool(opts.skip_norm_out)
        return raw_off, seq_off

    def upload_packed(self, params, opts, raw, raw_off, seq, seq_off, sv_in=None, sv_flags=None,
                      samp_ind=None, stall_ints=None, stall_off=None, wait=False):
        """One batch as flat CSR arrays (tba_batch_upload_async): raw (int16 / float32 / float64)
        and seq (uint8 codes) concatenated, offsets int64[n+1].  Enqueue only unless `wait`; the
        arrays are kept referenced until the next upload, but must not be modified before
        `sync()`.  Arrays in PinnedArray memory are transferred by DMA."""
        if not isinstance(raw, DeviceArray):       # (else a Synth batch: copied device to device)
            if raw.dtype not in RAW_DTYPES or not raw.flags.c_contiguous:
                raw = np.ascontiguousarray(raw, dtype=np.float64)
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
        raw_off, seq_off = self._batch_layout(params, opts, raw_off, seq_off)
        n = self.n
        svi = None if sv_in is None else np.ascontiguousarray(sv_in, dtype=np.float64)
        svf = None if sv_flags is None else np.ascontiguousarray(sv_flags, dtype=np.int32)
        si = None if samp_ind is None else np.ascontiguousarray(samp_ind, dtype=np.int64)
        st = None if stall_ints is None else np.ascontiguousarray(stall_ints, dtype=np.int64)
        sto = None if stall_off is None else np.ascontiguousarray(stall_off, dtype=np.int64)
        self._keep = (raw, seq, raw_off, seq_off, svi, svf, si, st, sto)
        self._call('tba_batch_upload_async', params, opts, n, raw.ctypes, RAW_DTYPES[raw.dtype], raw_off, seq, seq_off,
                   svi, svf, si, st, sto)
        if wait:
            self.sync()

    def run(self):
        self._call('tba_batch_run')

    def enqueue(self):
        self._call('tba_batch_enqueue')

    def sync(self):
        # (the targets of the finished downloads belong to the caller alone from here on: a block of
        # the result pool must not stay leased because this engine still points at it)
        self._call('tba_batch_sync')
        self._keep_out = None

    def wait_for(self, other):
        """kernels enqueued next on this engine start after `other`'s last enqueued sequence"""
        self._call('tba_batch_wait_for', other._h)

    def device_mem(self):
        """(free, total) bytes of this engine's device"""
        a, b = i64(0), i64(0)
        self._call('tba_device_mem', C.byref(a), C.byref(b))
        return a.value, b.value

    def held_bytes(self):
        """device bytes of this engine's grow-only batch buffers"""
        a = i64(0)
        self._call('tba_engine_held_bytes', C.byref(a))
        return a.value

    def set_sharing(self, n_engines):
        """scheduling hint: `n_engines` engines are fed concurrently on this device (tba_engine_set_sharing)"""
        self._call('tba_engine_set_sharing', int(n_engines))

    def set_dispatch(self, small_batch_reads=-1, tb_wave_below=-1):
        """read-count thresholds between the latency and the throughput forms of DNA event detection
        and of the main traceback (tba_engine_set_dispatch; identical results; default 1 024 each;
        0: every batch takes the throughput form; negative: unchanged); from the next run"""
        self._call('tba_engine_set_dispatch', int(small_batch_reads), int(tb_wave_below))

    def set_side_stream(self, mode=-1):
        """stall detection and expected levels beside normalisation / event detection on a second stream
        (tba_engine_set_side_stream): -1 while at most two engines are alive on the device, 0 never, 1 always"""
        self._call('tba_engine_set_side_stream', int(mode))

    def last_side_stream(self):
        return bool(self._L.tba_engine_last_side_stream(self._h))

    def last_dp_lowreg(self):
        """whether the last run launched k_dp8_lowreg in place of k_dp<8> (tba_engine_last_dp_lowreg)"""
        return bool(self._L.tba_engine_last_dp_lowreg(self._h))

    def last_dp_const_division(self):
        """(main pass, start discovery): whether the last run's forward passes took k_dp_cdiv, the two-operation
        division by a proven sd (tba_engine_last_dp_const_division)"""
        bits = self._L.tba_engine_last_dp_const_division(self._h)
        return bool(bits & 1), bool(bits & 2)

    def set_dp_const_division(self, auto=True):
        """True (default): batches of a proven model run k_dp_cdiv; False: never (tba_engine_set_dp_const_division)"""
        self._call('tba_engine_set_dp_const_division', 1 if auto else 0)

    def selftest_const_division(self, a, b, z_shift, zcap):
        """float64[3][n] of tba_selftest_const_division: the two-operation quotients a / b, the cell values
        z_shift - min(|q|, zcap) from them, and the same cell values from the general division"""
        a, b = _f64(a), _f64(b)
        assert a.ndim == 1 and a.shape == b.shape and a.shape[0] >= 1
        out = np.empty(3 * a.shape[0], dtype=np.float64)
        self._call('tba_selftest_const_division', a, b, a.shape[0], float(z_shift), float(zcap), out)
        return out.reshape(3, -1)

    def model_const_division(self):
        """whether every sd of the uploaded model is a proven divisor (tba_engine_model_const_division)"""
        return bool(self._L.tba_engine_model_const_division(self._h))

    def get_dispatch(self):
        a, b = i64(0), i64(0)
        self._call('tba_engine_get_dispatch', C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def host_stage(self):
        """this engine's reusable page-locked staging arrays (PinnedStage)"""
        if self._stage is None:
            self._stage = PinnedStage()
        return self._stage

    def query(self):
        """True while work of this engine is still in flight (never blocks)"""
        rc = self._L.tba_batch_query(self._h)
        if rc < 0:
            raise EngineError('tba_batch_query failed (%d): %s' % (rc, self._L.tba_last_error().decode()))
        return rc == 1

    def download_async(self, results=None, segs32=None, segs64=None, norm=None):
        """Enqueue the copies of the finished batch's outputs into the given arrays (ideally
        PinnedArray memory): results RESULT_DTYPE[n], segs32 int32 / segs64 int64 [seg_off[-1]],
        norm float64[n_raw_total].  Valid after sync()."""
        for a, dt, cnt in ((results, RESULT_DTYPE, self.n), (segs32, np.int32, int(self.seg_off[-1])),
                           (segs64, np.int64, int(self.seg_off[-1])),
                           (norm, np.float64, self.n_raw_total)):
            if a is not None and (a.dtype != dt or a.size < cnt or not a.flags.c_contiguous):
                raise ValueError('output array has the wrong dtype / size')
        self._keep_out = (results, segs32, segs64, norm)
        self._call('tba_batch_download_async', None if results is None else (ReadResult * self.n).from_buffer(results),
                   segs32, segs64, norm)

    def footprint(self, params, opts, n_raw, seq_len, raw_dtype=np.float64):
        """device bytes a batch of reads with these lengths would occupy"""
        from .planner import exact_bytes
        return exact_bytes(n_raw, seq_len, params, opts, self.kmer_width, raw_dtype)

    def download(self, want_norm=True):
        n = self.n
        want_norm = want_norm and not self.skip_norm_out
        status = np.zeros(n, np.int32)
        segs = np.zeros(int(self.seg_off[-1]), np.int64)
        rs = np.zeros(n, np.int64)
        norm = np.zeros(self.n_raw_total, np.float64) if want_norm else None
        nl = np.zeros(n, np.int64)
        sv = np.zeros((n, 4))
        score = np.zeros(n)
        changed = np.zeros(n, np.int32)
        self._call('tba_batch_download', status, segs, rs, norm, nl, sv, score, changed)
        return dict(status=status, segs=segs, read_start=rs, norm=norm, norm_len=nl, sv=sv,
                    score=score, changed=changed)

    def get(self, what):
        """tba_batch_get: one intermediate of the uploaded batch (a TBA_GET_* selector) as a fresh array"""
        dims = dict(n=self.n, raw=self.n_raw_total, raw_x2=2 * self.n_raw_total, ref=int(self.ref_off[-1]),
                    seg=int(self.seg_off[-1]), ev=max(int(self.ev_off[-1]), 1))
        dt, shape = _GET_SHAPES[what]
        out = np.zeros([dims.get(d, d) for d in shape], dt)
        self._call('tba_batch_get', what, out.ctypes, out.nbytes)
        return out

    def stall_ints(self):
        """per read the stall intervals in force ([k, 2] int64; given, or detected on the device)"""
        cnt, off = self.get(GET_N_STALL), self.get(GET_STALL_OFF)
        if not cnt.any():
            return [np.zeros((0, 2), np.int64) for _ in range(self.n)]
        flat = np.zeros((int((off + cnt).max()), 2), np.int64)
        self._call('tba_batch_get', GET_STALL_INTS, flat.ctypes, flat.nbytes)
        return [flat[int(o):int(o) + int(c)].copy() for o, c in zip(off, cnt)]

    def run_stages(self, first, last):
        self._call('tba_batch_run_stages', first, last)

    def put(self, what, data, per_read=None):
        data = np.ascontiguousarray(data)
        pr = None if per_read is None else np.ascontiguousarray(per_read, dtype=np.int64)
        self._call('tba_batch_put', what, data.ctypes, data.nbytes, pr)

    def set_num_events(self, num_events):
        ne = None if num_events is None else np.ascontiguousarray(num_events, dtype=np.int64)
        self._call('tba_set_num_events', ne, 0 if ne is None else ne.shape[0])
        self._ne_override = ne

    def base_stats(self):
        """(means, stds) of every base of the finished batch, concatenated by ref_off"""
        nb = int(self.ref_off[-1])
        m, s = np.zeros(nb), np.zeros(nb)
        self._call('tba_batch_base_stats', m, s, nb)
        return m, s

    def de_novo_stats(self, fm_offset, smallest_pval):
        """tba_batch_de_novo_stats: p-values of every base of the finished batch (CSR by ref_off;
        NaN outside the testable part of a read and for failed reads)"""
        nb = int(self.ref_off[-1])
        out = np.full(max(nb, 1), np.nan)
        self._call('tba_batch_de_novo_stats', int(fm_offset), float(smallest_pval), out, nb)
        return out[:nb]

    # ---- statistics over host arrays (numpy in, numpy out; pileup: the CSR bundle of tombo_stats) ----
    def read_pvals(self, means, ref_means, ref_sds, off, fm_offset, floor_out, smallest_pval):
        """tba_read_pvals: z-test p-values (Fisher's method over 2 * fm_offset + 1) of reads concatenated by `off`"""
        m, r, s, off = _f64(means), _f64(ref_means), _f64(ref_sds), _i64(off)
        if not (m.shape[0] == r.shape[0] == s.shape[0] == int(off[-1])):
            raise ValueError('per-base arrays and offsets disagree')
        out = np.empty(m.shape[0], dtype=np.float64)
        self._call('tba_read_pvals', m, r, s, off, off.shape[0] - 1, int(fm_offset), int(floor_out), smallest_pval, out)
        return out

    def llh_ratio_windows(self, kind, means, ref_means, alt_means, ref_vars, starts, width, alt_vars, par):
        """tba_llh_ratio_windows: one ratio per window [start, start + width) of the first array's length"""
        m, r, a, rv, av, st = _f64(means), _f64(ref_means), _f64(alt_means), _f64(ref_vars), _f64(alt_vars), _i64(starts)
        if min(x.shape[0] for x in (r, a, rv, av) if x is not None) < m.shape[0]:
            raise ValueError('window arrays disagree')
        out = np.empty(st.shape[0], dtype=np.float64)
        self._call('tba_llh_ratio_windows', int(kind), m, r, a, rv, av, m.shape[0], int(width), st, st.shape[0],
                   (f64 * 3)(*par), out)
        return out

    def _pileup_args(self, pl, with_ctrl):
        return (pl.reg_start.shape[0], pl.reg_start, pl.reg_end, pl.reg_strand, pl.reg_read_off, pl.read_start.shape[0],
                pl.read_start, pl.read_strand) + ((pl.read_ctrl,) if with_ctrl else ()) + (pl.read_off, pl.means)

    def group_level_stats(self, kind, return_p, fm_offset, min_test_reads, pileup, smallest_pval):
        """-> (stats, positions, coverage, control coverage, counts): counts[r] records from pileup.pos_off[r]"""
        n_pos = int(pileup.pos_off[-1])
        stats = np.empty(n_pos, dtype=np.float64)
        poss, cov, ccov = (np.empty(n_pos, dtype=np.int64) for _ in range(3))
        counts = np.empty(pileup.reg_start.shape[0], dtype=np.int64)
        self._call('tba_group_level_stats', kind, return_p, fm_offset, min_test_reads, *self._pileup_args(pileup, True),
                   smallest_pval, stats, poss, cov, ccov, counts)
        return stats, poss, cov, ccov, counts

    def reads_ref_levels(self, est_mean, fm_offset, min_test_reads, pileup, prior_means, prior_sds, w_mean, w_sd):
        """-> (level means, level sds, coverage) at pileup.pos_off; priors (both or neither) blended in"""
        n_pos = int(pileup.pos_off[-1])
        pm, ps = _f64(prior_means), _f64(prior_sds)
        lm, ls = np.empty(n_pos, dtype=np.float64), np.empty(n_pos, dtype=np.float64)
        cov = np.empty(n_pos, dtype=np.int64)
        self._call('tba_reads_ref_levels', bool(est_mean), fm_offset, min_test_reads, *self._pileup_args(pileup, False),
                   pm, ps, w_mean, w_sd, lm, ls, cov)
        return lm, ls, cov

    # tba_site_fractions' arguments of the form a call leaves out: ref_sds .. smallest_pval / kind .. win_pos
    _NO_Z_FORM = (None, None, 0, None, None, 0, 0, 0.0)
    _NO_WINDOW_FORM = (0, None, None, None, 0, 0, None, 0, None, None, None)

    def _site_fractions(self, form, trk_start, trk_end, z_args, win_args, n_stats, single_read_thresh,
                        lower_thresh, damp_counts, return_per_read):
        trk_start, trk_end = _i64(trk_start), _i64(trk_end)
        pos_off, outs = _site_outputs(trk_start, trk_end, damp_counts)
        per_read = np.empty(n_stats, dtype=np.float64) if return_per_read else None
        self._call('tba_site_fractions', form, trk_start.shape[0], trk_start, trk_end, *z_args, *win_args,
                   float(single_read_thresh), None if lower_thresh is None else (f64 * 1)(float(lower_thresh)),
                   None if damp_counts is None else (f64 * 2)(*damp_counts), *outs, per_read)
        return SiteFractions(pos_off, *outs, per_read)

    def site_fractions_z(self, trk_start, trk_end, means, ref_means, ref_sds, off, read_track, read_pos,
                         fm_offset, floor_out, smallest_pval, single_read_thresh, lower_thresh=None,
                         damp_counts=None, return_per_read=False):
        """tba_site_fractions, z form: the statistics of read_pvals, read r on track read_track[r] from
        position read_pos[r], collated per position of each track -> SiteFractions.  damp_counts: (unmod, mod)"""
        m, r, s = _f64(means), _f64(ref_means), _f64(ref_sds)
        off, r_trk, r_pos = _i64(off), _i64(read_track), _i64(read_pos)
        if not (m.shape[0] == r.shape[0] == s.shape[0] == int(off[-1])) or \
                not (off.shape[0] - 1 == r_trk.shape[0] == r_pos.shape[0]):
            raise ValueError('per-base arrays, offsets and per-read arrays disagree')
        z_args = (m, r, s, off, r_trk.shape[0], r_trk, r_pos, int(fm_offset), int(floor_out), smallest_pval)
        return self._site_fractions(0, trk_start, trk_end, z_args, self._NO_WINDOW_FORM, m.shape[0],
                                    single_read_thresh, lower_thresh, damp_counts, return_per_read)

    def site_fractions_windows(self, trk_start, trk_end, kind, means, ref_means, alt_means, ref_vars, alt_vars,
                               starts, width, win_track, win_pos, par, single_read_thresh, lower_thresh=None,
                               damp_counts=None, return_per_read=False):
        """tba_site_fractions, window form: the statistics of llh_ratio_windows (all value arrays
        of one length), window w on track win_track[w] at position win_pos[w] -> SiteFractions"""
        m, r, a, rv, av = _f64(means), _f64(ref_means), _f64(alt_means), _f64(ref_vars), _f64(alt_vars)
        st, w_trk, w_pos = _i64(starts), _i64(win_track), _i64(win_pos)
        n = m.shape[0]
        if not (r.shape[0] == a.shape[0] == rv.shape[0] == n) or (av is not None and av.shape[0] != n) or \
                not (st.shape[0] == w_trk.shape[0] == w_pos.shape[0]):
            raise ValueError('window arrays disagree')
        win_args = (int(kind), a, rv, av, n, int(width), st, st.shape[0], (f64 * 3)(*par), w_trk, w_pos)
        return self._site_fractions(1, trk_start, trk_end, (m, r) + self._NO_Z_FORM, win_args, st.shape[0],
                                    single_read_thresh, lower_thresh, damp_counts, return_per_read)

    def site_fractions_reads(self, form, reg_start, reg_end, read_start, read_strand, read_off, means, seq,
                             reg_pair_off, pair_read, pos_means, pos_sds, fm_offset, smallest_pval,
                             single_read_thresh, lower_thresh=None, damp_counts=None, return_per_read=False):
        """tba_site_fractions_reads: the z tests (form 0: de_novo under the engine's model, form 1: sample_compare
        under pos_means / pos_sds) of region r on reads pair_read[reg_pair_off[r]:reg_pair_off[r + 1]] of a reads
        table that holds every read once; clip, flip and expected levels are made on the device
        -> (SiteFractions, pair_ok, pair_pos, pair_off): per pair whether it did not fail, the position of its
        first statistic and its offset into per_read.  `last_site_reads_kernel_ms`: device time of the plan,
        scan and gather kernels, and of the kernels behind them."""
        t = _check_site_reads_args(form, reg_start, reg_end, read_start, read_strand, read_off, means, seq,
                                   reg_pair_off, pair_read, pos_means, pos_sds, fm_offset)
        if form == 0 and self.kmer_width is None:
            raise ValueError('form 0 (de_novo) needs a model (set_model)')
        n_pairs = t.pair_read.shape[0]
        pos_off, outs = _site_outputs(t.reg_start - t.fm_offset, t.reg_end + t.fm_offset, damp_counts)
        cap = int(site_reads_stat_bound(form, t, self.kmer_width or 1, self.central_pos or 0).sum()) if return_per_read else 0
        per_read = np.empty(cap, dtype=np.float64) if return_per_read else None
        pair_ok = np.zeros(n_pairs, dtype=np.int32)
        pair_pos, pair_off = np.zeros(n_pairs, dtype=np.int64), np.zeros(n_pairs + 1, dtype=np.int64)
        ms = np.zeros(2, dtype=np.float64)
        self._call('tba_site_fractions_reads', form, t.reg_start.shape[0], t.reg_start, t.reg_end,
                   t.read_start.shape[0], t.read_start, t.read_strand, t.read_off, t.means, t.seq, t.reg_pair_off,
                   t.pair_read, t.pos_means, t.pos_sds, t.fm_offset, smallest_pval, float(single_read_thresh),
                   None if lower_thresh is None else (f64 * 1)(float(lower_thresh)),
                   None if damp_counts is None else (f64 * 2)(*damp_counts), *outs, pair_ok, pair_pos, pair_off,
                   per_read, cap, ms)
        self.last_site_reads_kernel_ms = (float(ms[0]), float(ms[1]))
        if per_read is not None:
            per_read = per_read[:int(pair_off[-1])]
        return SiteFractions(pos_off, *outs, per_read), pair_ok, pair_pos, pair_off

    def site_aggregate(self, blk_start, blk_end, rec_off, records, single_read_thresh, lower_thresh=None,
                       abs_rule=False, damp_counts=None):
        """tba_site_aggregate: the per-site fractions of stored per-read blocks (aggregate_per_read_stats).  Block t
        covers [blk_start[t], blk_end[t]) and owns records[rec_off[t]:rec_off[t + 1]] (PER_READ_DTYPE, uploaded as
        stored) -> SiteFractions (per_read None).  abs_rule: model_compare's |stat| >= single_read_thresh validity
        when no lower threshold is given.  `last_site_aggregate_kernel_ms`: device time of the call's kernels."""
        bs, be, off, rec = _check_site_aggregate_args(blk_start, blk_end, rec_off, records)
        (pos_off, outs), ms = _site_outputs(bs, be, damp_counts), f64(0.0)
        self._call('tba_site_aggregate', bs.shape[0], bs, be, off, rec.ctypes, float(single_read_thresh),
                   None if lower_thresh is None else (f64 * 1)(float(lower_thresh)), bool(abs_rule),
                   None if damp_counts is None else (f64 * 2)(*damp_counts), *outs, C.byref(ms))
        self.last_site_aggregate_kernel_ms = ms.value
        return SiteFractions(pos_off, *outs, None)

    # ---- ROC / precision-recall (csrc/k_roc.h) ----
    def _roc_split(self, stats, labels, index, counts, return_index):
        out, a = [], 0
        for c in counts.tolist():
            item = (stats[a:a + c].copy(), labels[a:a + c].astype(np.bool_))
            out.append(item + (index[a:a + c].copy(),) if return_index else item)
            a += c
        return out

    def roc_motif_labels(self, blk_minus, blk_seq_start, seq_off, seq_codes, rec_off, rec_pos, rec_stat, motifs,
                         ctrl_label=None, return_index=False):
        """tba_roc_motif_labels: records (rec_pos, rec_stat; CSR by block through rec_off) against motifs, each
        (length, mod_pos, mod_base code, uint8 base sets).  Block t: minus strand flag, the genome coordinate of the
        first of its base codes seq_codes[seq_off[t]:seq_off[t + 1]] (0-3 = ACGT, else 4).  ctrl_label None: the rule
        of compute_motif_stats (kept: the record's base is mod_base; label: the motif matches); else that of
        compute_ctrl_motif_stats (kept: the motif matches; label: ctrl_label).  -> per motif (stats float64, has_mod
        bool[, record index int64]) of the kept records in record order.  `last_roc_kernel_ms`: kernel time."""
        minus, ss, s_off, seq, off, pos, stat, table, sets = _check_roc_motif_args(
            blk_minus, blk_seq_start, seq_off, seq_codes, rec_off, rec_pos, rec_stat, motifs)
        n_mot, ms = table.shape[0], f64(0.0)
        outs = _roc_label_outputs(n_mot * pos.shape[0], n_mot, return_index)
        self._call('tba_roc_motif_labels', minus.shape[0], minus, ss, s_off, seq, off, pos, stat, n_mot, table, sets,
                   0 if ctrl_label is None else 1, bool(ctrl_label), *outs, C.byref(ms))
        self.last_roc_kernel_ms = ms.value
        return self._roc_split(*outs, return_index)

    def roc_loc_labels(self, blk_loc, mod_locs, unmod_locs, rec_off, rec_pos, rec_stat, return_index=False):
        """tba_roc_loc_labels: block t owns the ascending slices mod_locs[blk_loc[t, 0]:blk_loc[t, 1]] and
        unmod_locs[blk_loc[t, 2]:blk_loc[t, 3]]; a record is kept when its position is in either, its label is
        whether it is in the first -> (stats, has_mod[, record index]) in record order"""
        loc, mod, unmod, off, pos, stat = _check_roc_loc_args(blk_loc, mod_locs, unmod_locs, rec_off, rec_pos, rec_stat)
        outs, ms = _roc_label_outputs(pos.shape[0], 1, return_index), f64(0.0)
        self._call('tba_roc_loc_labels', loc.shape[0], loc, mod, mod.shape[0], unmod, unmod.shape[0], off, pos, stat,
                   *outs, C.byref(ms))
        self.last_roc_kernel_ms = ms.value
        return self._roc_split(*outs, return_index)[0]

    def roc_rank_counts(self, stats, has_mod, ranks):
        """tba_roc_rank_counts -> (tp_at int64[len(ranks)], tp_total, n_nan): tp_at[j] = True labels among the
        ranks[j] + 1 first entries in ascending (stat, has_mod) order; -0.0 ties with 0.0.  With NaN statistics
        (n_nan > 0) the counts mean nothing.  `last_roc_sort_ms` / `last_roc_gather_ms`: kernel time of the keys and
        the sort / of the label scan and the gather."""
        st, hm, rk = _check_roc_rank_args(stats, has_mod, ranks)
        tp_at = np.zeros(rk.shape[0], dtype=np.int64)
        total, n_nan, ms = i64(0), i64(0), (f64 * 2)()
        self._call('tba_roc_rank_counts', st.shape[0], st, hm, rk.shape[0], rk, tp_at, C.byref(total), C.byref(n_nan),
                   ms)
        self.last_roc_sort_ms, self.last_roc_gather_ms = ms[0], ms[1]
        self.last_roc_kernel_ms = ms[0] + ms[1]
        return tp_at, total.value, n_nan.value

    # ---- pairwise distances between rows (csrc/k_pdist.h) ----
    def pairwise_window_dists(self, rows, slide_span=0):
        """tba_pairwise_window_dists: rows float64[R, L] -> float64[R, R], [i, j] for j <= i the sqrt of the smallest
        sum of squared differences between a window of row i and one of row j (windows of L - 2 slide_span values at
        the starts 0 .. 2 slide_span), 0 above the diagonal.  `last_pdist_kernel_ms`: kernel time."""
        rows = _check_pdist_rows(rows, slide_span)
        n, ms = rows.shape[0], f64(0.0)
        out = np.empty((n, n), dtype=np.float64)
        self._call('tba_pairwise_window_dists', n, rows.shape[1], int(slide_span), rows, out, C.byref(ms))
        self.last_pdist_kernel_ms = ms.value
        return out

    def pairwise_nanmean_dists(self, rows):
        """tba_pairwise_nanmean_dists: rows float64[R, L] -> float64[R (R - 1) / 2], np.nanmean(np.sqrt((u - v)**2)) of
        every pair of rows in scipy's condensed pdist order; NaN where two rows share no number"""
        rows = _check_pdist_rows(rows)
        n, ms = rows.shape[0], f64(0.0)
        out = np.empty(n * (n - 1) // 2, dtype=np.float64)
        self._call('tba_pairwise_nanmean_dists', n, rows.shape[1], rows, out, C.byref(ms))
        self.last_pdist_kernel_ms = ms.value
        return out

    def kmer_levels(self, means, codes, read_off, kmer_width, central_pos, completed):
        """tba_kmer_levels: the levels of a batch of reads (means / codes CSR by read_off) gathered by k-mer
        -> (counts int64[4**K], levels float64, lv_off int64[4**K + 1]); the levels of a k-mer in read order,
        then position order"""
        m, codes, off, done = _check_kmer_levels_args(means, codes, read_off, kmer_width, central_pos, completed)
        n_kmers = 4 ** int(kmer_width)
        counts, lv_off = np.empty(n_kmers, dtype=np.int64), np.empty(n_kmers + 1, dtype=np.int64)
        cap = int(np.maximum(np.diff(off) - (int(kmer_width) - 1), 0).sum())   # every window of the batch
        levels = np.empty(cap, dtype=np.float64)
        self._call('tba_kmer_levels', m, codes, off, off.shape[0] - 1, int(kmer_width), int(central_pos), done, counts,
                   lv_off, levels, cap)
        return counts, levels[:int(lv_off[-1])].copy(), lv_off

    def kmer_dist(self, means, codes, read_off, kmer_width, central_pos, kmer_thresh, num_reads, read_mean):
        """tba_kmer_dist, the count form and then the fill: which reads of the batch (means / codes CSR by read_off,
        in the order given) plot_kmer_dist takes, and their levels by k-mer -> (read_label int64[n_reads] (1, 2, ...;
        0: not taken), n_sel, n_examined, counts int64[4**K], off int64[4**K + 1], values float64, value_label int64,
        kmer_mean float64[4**K]).  The entries of k-mer k are values[off[k]:off[k + 1]] in read order, then position
        order: its levels, or with read_mean np.mean of them per read; value_label: the label of each entry's read;
        kmer_mean: np.mean over the k-mer's entries, NaN where it has none.  `last_kmer_dist_kernel_ms`: kernel time
        of both calls."""
        m, codes, off = _check_kmer_dist_args(means, codes, read_off, kmer_width, central_pos, kmer_thresh, num_reads)
        n_reads, n_kmers = off.shape[0] - 1, 4 ** int(kmer_width)
        label = np.zeros(n_reads, dtype=np.int64)
        counts, voff = np.empty(n_kmers, dtype=np.int64), np.empty(n_kmers + 1, dtype=np.int64)
        n_sel, n_exam, ms0, ms1 = i64(0), i64(0), f64(0.0), f64(0.0)
        head = (m, codes, off, n_reads, int(kmer_width), int(central_pos), int(kmer_thresh), int(num_reads),
                int(bool(read_mean)), label, C.byref(n_sel), C.byref(n_exam), counts, voff)
        self._call('tba_kmer_dist', *(head + (None, None, 0, None, C.byref(ms0))))
        cap = int(voff[-1])
        values, vlabel = np.empty(cap, dtype=np.float64), np.empty(cap, dtype=np.int64)
        kmer_mean = np.empty(n_kmers, dtype=np.float64)
        self._call('tba_kmer_dist', *(head + (values, vlabel, cap, kmer_mean, C.byref(ms1))))
        self.last_kmer_dist_kernel_ms = ms0.value + ms1.value
        return label, int(n_sel.value), int(n_exam.value), counts, voff, values, vlabel, kmer_mean

    def kde_eval(self, levels, lv_off, x, bandwidth):
        """tba_kde_eval: the Gaussian kernel density of every segment of `levels` (CSR by lv_off) on the grid x
        -> float64[n_seg, G]; NaN rows for segments of fewer than two levels or with a NaN level"""
        lv, off, x = _check_kde_eval_args(levels, lv_off, x, bandwidth)
        out = np.empty((off.shape[0] - 1, x.shape[0]), dtype=np.float64)
        self._call('tba_kde_eval', lv, off, off.shape[0] - 1, x, x.shape[0], float(bandwidth), out)
        return out

    # ---- k-mer model estimation (csrc/k_kmer_est.h) ----
    def region_key_levels(self, est_mean, read_start, read_minus, read_off, means, reg_read_off, reg_reads, pos_reg,
                          pos_g, ent_pos, ent_key, n_keys):
        """tba_region_key_levels: get_region_kmer_levels for a batch of regions.  Reads (start, minus-strand flag,
        levels CSR by read_off) are given once; region r uses the reads reg_reads[reg_read_off[r]:reg_read_off[r + 1]]
        in that order; position p is (pos_reg[p], pos_g[p]); entry i files the pair of position ent_pos[i] under key
        ent_key[i].  -> (counts int64[n_keys], off int64[n_keys + 1], levels, sds float64[n_ent]): per key the
        (np.median, np.std) pairs -- est_mean: the c_mean_std pairs -- of its entries, in entry order"""
        rs, rm, off, m, roff, rr, pr, pg, ep, ek = _check_region_key_levels_args(
            read_start, read_minus, read_off, means, reg_read_off, reg_reads, pos_reg, pos_g, ent_pos, ent_key, n_keys)
        n_keys, n_ent = int(n_keys), ep.shape[0]
        counts, koff = np.empty(n_keys, dtype=np.int64), np.empty(n_keys + 1, dtype=np.int64)
        levels, sds = np.empty(n_ent, dtype=np.float64), np.empty(n_ent, dtype=np.float64)
        self._call('tba_region_key_levels', bool(est_mean), rs.shape[0], rs, rm, off, m, roff.shape[0] - 1, roff, rr,
                   pr.shape[0], pr, pg, n_ent, ep, ek, n_keys, counts, koff, levels, sds)
        return counts, koff, levels, sds

    def segment_medians(self, values, off):
        """tba_segment_medians: np.median of every segment of `values` (CSR by off) -> float64[n_seg]; NaN for an
        empty segment or one that holds a NaN.  `values` is not modified"""
        v, off = _check_segment_medians_args(values, off)
        out = np.empty(off.shape[0] - 1, dtype=np.float64)
        self._call('tba_segment_medians', v, off, off.shape[0] - 1, out)
        return out

    # ---- centring a k-mer model on a batch of reads (csrc/k_center.h) ----
    def center_prepare(self, params, opts, raws, codes, event_starts, read_start_rel_to_raw, num_events=None):
        """tba_center_prepare, the first half of center_model_to_median_norm for a batch of reads: every read's
        whole raw signal (int16 or float64: same bits) normalised and kept on the device -- by its medians (DNA
        parameters), or as get_event_scale_values does under RNA parameters (params.use_t_test_seg; opts with
        reverse_raw, stall_params and outlier_thresh; num_events: compute_num_events per read) --, the model's
        levels of `codes` (the reads' `base` columns as uint8 codes), and the reads' own boundaries from their
        `start` columns and read_start_rel_to_raw.  -> status int32 [n]: 0 for a read the fit will take.  The caller
        draws the subsamples of those reads, in read order, and calls center_fit; last_center_kernel_ms: device
        time of the two calls"""
        rna = bool(params.use_t_test_seg)
        raw, raw_off, seq, seq_off, starts, start_off, rsr, ne = _check_center_prepare_args(
            raws, codes, event_starts, read_start_rel_to_raw, num_events, rna)
        n = len(raws)
        # (the entry forces these event counts itself; here they give the layout `get` indexes by)
        self._ne_override = ne if rna else np.full(n, 2, dtype=np.int64)
        raw_off, seq_off = self._batch_layout(params, opts, raw_off, seq_off)
        status, ms = np.zeros(n, np.int32), np.zeros(1, np.float64)
        self._center_n = None
        self._call('tba_center_prepare', params, opts, n, raw.ctypes, RAW_DTYPES[raw.dtype], raw_off, seq, seq_off,
                   starts, start_off, rsr, ne if rna else None, status, ms)
        self._center_n, self.last_center_kernel_ms = n, [float(ms[0]), 0.0]
        return status

    def center_fit(self, samp_ind=None, prior=None, max_reads=MAX_CENTER_READS):
        """tba_center_fit on the batch center_prepare left: samp_ind int64 [n, 1000] (pack_samp_inds; None when no
        read has more than 1000 points), prior float64 [m, 2]: the factors of the successes of earlier calls, in
        order.  -> (status int32 [n], factors float64 [n, 2]: shift_corr_factor and scale_corr_factor, NaN for a
        failed read; medians (shift, scale) of the first max_reads successes -- prior first, then this batch in
        read order -- in np.median's arithmetic, None without a success; how many successes that were)"""
        n = getattr(self, '_center_n', None)
        samp_ind, prior = _check_center_fit_args(n, None if n is None else self.B, samp_ind, prior, max_reads)
        status, factors = np.zeros(n, np.int32), np.zeros((n, 2), np.float64)
        med, used, ms = np.zeros(2, np.float64), np.zeros(1, np.int64), np.zeros(1, np.float64)
        self._center_n = None
        self._call('tba_center_fit', samp_ind, prior if prior.shape[0] else None, prior.shape[0], int(max_reads), status,
                   factors, med, used, ms)
        self.last_center_kernel_ms[1] = float(ms[0])
        return status, factors, (float(med[0]), float(med[1])) if used[0] else None, int(used[0])

    # ---- the documented per-read functions of tombo_stats (csrc/k_norm_api.h) ----
    def normalize_raw_batch(self, raws, starts, lens, norm_type, sv_in=None, sv_flags=None, channel=None,
                            outlier_thresh=None, const_scale=None):
        """tba_normalize_raw_batch: ts.normalize_raw_signal of the windows [starts[i], starts[i] + lens[i]) of the
        one-dimensional arrays `raws`, all int16 or all float64.  norm_type: NORMTYPE_*; sv_in / sv_flags:
        pack_scale_values; channel: float64 [n, 3] offset, range, digitisation.  -> (sv float64 [n, 4]: shift, scale,
        lower_lim, upper_lim; has_lims int32 [n]; the normalised windows as views of one float64 array; status
        int32 [n]: 1 where the scale is exactly 0 and nothing was computed); last_normalize_raw_kernel_ms holds the
        time of the two kernels"""
        n = len(raws)
        dt, raw, raw_off, starts, lens = _check_normalize_raw_args(raws, starts, lens, norm_type, sv_in, sv_flags, channel)
        sv = np.zeros((n, 4), np.float64)
        has_lims, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        out_off = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=out_off[1:])
        norm, ms = np.zeros(int(out_off[-1]), np.float64), np.zeros(1, np.float64)
        self._call('tba_normalize_raw_batch', n, raw.ctypes, RAW_DTYPES[dt], raw_off, starts, lens, int(norm_type),
                   sv_in, sv_flags, channel, int(outlier_thresh is not None),
                   0.0 if outlier_thresh is None else float(outlier_thresh),
                   0.0 if const_scale is None else float(const_scale), sv, has_lims, norm, status, ms)
        self.last_normalize_raw_kernel_ms = float(ms[0])
        return sv, has_lims, [norm[a:b] for a, b in zip(out_off[:-1].tolist(), out_off[1:].tolist())], status

    def mom_sums(self, event_means, model_means, model_inv_vars, off):
        """tba_mom_sums: float64 [n, 5], per read (CSR by off) iv.sum(), (m * iv).sum(), (m * iv * m).sum(),
        (e * iv).sum(), (e * iv * m).sum() in the order of numpy's .sum()"""
        off, e, m, iv = _check_point_arrays(off, event_means, model_means, model_inv_vars)
        out = np.zeros((off.shape[0] - 1, 5), np.float64)
        self._call('tba_mom_sums', off.shape[0] - 1, off, e, m, iv, out)
        return out

    def seg_scores(self, means, ref_means, ref_sds, off):
        """tba_seg_scores: float64 [n], ts.get_read_seg_score of every read (CSR by off)"""
        off, m, rm, rs = _check_point_arrays(off, means, ref_means, ref_sds)
        out = np.zeros(off.shape[0] - 1, np.float64)
        self._call('tba_seg_scores', off.shape[0] - 1, off, m, rm, rs, out)
        return out

    # ---- RNA adapter trimming, the global scale estimate (csrc/k_trim_rna.h) ----
    def trim_rna(self, raws, seg_params, trim_params):
        """tba_trim_rna_batch: ts.trim_rna of the one-dimensional arrays `raws`, all int16 or all float64; only their
        first max_raw_obs samples are handed over.  seg_params: (running_stat_width, min_obs_per_base,
        mean_obs_per_event); trim_params: (moving_window_size, min_running_values, thresh_scale, max_raw_obs).
        -> (adapter ends int64 [n], status int32 [n]: 0, 2 (fewer change points than requested), TRIM_TOO_FEW_EVENTS,
        100); last_trim_ed_form holds ED_FORM_* per read, last_trim_kernel_ms the time of the kernels"""
        dt, pre, (width, mob, mope), (mw, mr, ts_, mro) = _check_trim_rna_args(raws, seg_params, trim_params)
        n = len(pre)
        ends, status, form = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        ms = np.zeros(1, np.float64)
        if n:
            raw = np.ascontiguousarray(np.concatenate(pre))
            self._call('tba_trim_rna_batch', n, raw.ctypes, RAW_DTYPES[dt], _offsets(pre), mob, width, mope, mw, mr, ts_,
                       mro, ends, status, form, ms)
        self.last_trim_ed_form, self.last_trim_kernel_ms = form, float(ms[0])
        return ends, status

    def set_trim_budget(self, samples=0):
        """tba_engine_set_trim_budget: the most prefix samples one device pass of trim_rna holds (0: the default)"""
        self._call('tba_engine_set_trim_budget', int(samples))

    def raw_med_mad(self, raws):
        """tba_raw_med_mad: (np.median(r), np.median(np.abs(r - median))) of the one-dimensional arrays `raws` (one
        sample or more each), all int16 or all float64 -> two float64 [n]; last_med_mad_kernel_ms holds the kernel's
        time"""
        dt, raws = _check_raw_reads(raws, 1)
        n = len(raws)
        med, mad, ms = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(1, np.float64)
        if n:
            raw = np.ascontiguousarray(np.concatenate(raws))
            self._call('tba_raw_med_mad', n, raw.ctypes, RAW_DTYPES[dt], _offsets(raws), med, mad, ms)
        self.last_med_mad_kernel_ms = float(ms[0])
        return med, mad

    # ---- region plot data (csrc/k_plot.h) ----
    def region_level_piles(self, read_start, read_minus, read_off, means, reg_read_off, reg_reads, reg_start, reg_end,
                           q_linear=None, q_nearest=None, want_levels=True):
        """tba_region_level_piles: the level piles of a batch of plot regions.  Reads as in region_key_levels; region
        r is [reg_start[r], reg_end[r]) with the reads reg_reads[reg_read_off[r]:reg_read_off[r + 1]] in that order.
        Positions run region-major, then in genomic order; a pile holds the levels of the covering reads in read
        order, NaN dropped.  q_linear / q_nearest: fractions (np.true_divide(q, 100)).
        -> (off int64[n_pos + 1], levels float64 | None, lin float64[n_pos, n_ql] | None, near float64[n_pos, n_qn] |
        None): np.percentile of every pile, linear and interpolation='nearest'; NaN for an empty pile.
        `last_plot_kernel_ms`: kernel time."""
        rs, rm, off, m, roff, rr, st, en, ql, qn, cap = _check_region_level_piles_args(
            read_start, read_minus, read_off, means, reg_read_off, reg_reads, reg_start, reg_end, q_linear, q_nearest)
        n_pos, ms = int((en - st).sum()), f64(0.0)
        out_off = np.zeros(n_pos + 1, dtype=np.int64)
        levels = np.empty(cap, dtype=np.float64) if want_levels else None
        lin, near = np.empty((n_pos, ql.shape[0]), dtype=np.float64), np.empty((n_pos, qn.shape[0]), dtype=np.float64)
        self._call('tba_region_level_piles', rs.shape[0], rs, rm, off, m, st.shape[0], roff, rr, st, en, ql.shape[0], ql,
                   qn.shape[0], qn, out_off, levels, cap, lin, near, C.byref(ms))
        self.last_plot_kernel_ms = ms.value
        return (out_off, levels[:int(out_off[-1])].copy() if want_levels else None,
                None if q_linear is None else lin, None if q_nearest is None else near)

    def segment_percentiles(self, values, off, q_linear, q_nearest):
        """tba_segment_percentiles: np.percentile of every segment of `values` (CSR by off) at the fractions q_linear
        (linear form) and q_nearest (interpolation='nearest') -> (lin float64[n_seg, n_ql], near float64[n_seg, n_qn]);
        NaN rows for an empty segment or one that holds a NaN.  `values` is not modified"""
        v, off, ql, qn = _check_segment_percentiles_args(values, off, q_linear, q_nearest)
        n_seg, ms = off.shape[0] - 1, f64(0.0)
        lin, near = np.empty((n_seg, ql.shape[0]), dtype=np.float64), np.empty((n_seg, qn.shape[0]), dtype=np.float64)
        self._call('tba_segment_percentiles', v, off, n_seg, ql.shape[0], ql, qn.shape[0], qn, lin, near, C.byref(ms))
        self.last_plot_kernel_ms = ms.value
        return lin, near

    def dwell_pctl_flags(self, segs, seg_off, pairs):
        """tba_dwell_pctl_flags: the observations-per-base rule for reads given by their boundaries (int64 base starts
        and the end, CSR by seg_off); pairs [(percentile, threshold), ...] -> (vals float64[n_reads, n_pairs]:
        np.percentile(np.diff(segs of the read), percentile); flags bool[n_reads]: any value above its threshold).
        A read of fewer than two boundaries: NaN and True.  `last_filter_kernel_ms`: kernel time."""
        segs, off, q, thresh = _check_dwell_pctl_args(segs, seg_off, pairs)
        n, ms = off.shape[0] - 1, f64(0.0)
        vals, flags = np.empty((n, q.shape[0]), dtype=np.float64), np.zeros(n, dtype=np.uint8)
        self._call('tba_dwell_pctl_flags', n, segs, off, q.shape[0], q, thresh, vals, flags, C.byref(ms))
        self.last_filter_kernel_ms = ms.value
        return vals, flags.astype(bool)

    def batch_dwell_pctl_flags(self, pairs):
        """tba_batch_dwell_pctl_flags: the same on the boundaries of the resident batch after a run (nothing but the
        pairs is uploaded) -> (vals float64[n, n_pairs], flags bool[n]); a read that failed: NaN and False"""
        q, thresh = _check_dwell_pairs(pairs)
        ms = f64(0.0)
        vals, flags = np.empty((self.n, q.shape[0]), dtype=np.float64), np.zeros(self.n, dtype=np.uint8)
        self._call('tba_batch_dwell_pctl_flags', q.shape[0], q, thresh, vals, flags, C.byref(ms))
        self.last_filter_kernel_ms = ms.value
        return vals, flags.astype(bool)

    def region_raw_signal(self, raw, raw_off, segs, segs_off, read_start, rsrtr, minus, rna, shift, scale, lower_lim,
                          upper_lim, pair_read, pair_start, pair_end, genome_centric=True):
        """tba_region_raw_signal: th.get_raw_signal, the stored normalisation and the per-base position spread of
        get_r_raw_signal_data for (read, region) pairs.  Reads: raw (int16 or int32, CSR by raw_off), segs (Events
        start column and the end, CSR by segs_off), genomic read_start, rsrtr (read_start_rel_to_raw), minus, rna,
        shift, scale, lower_lim, upper_lim (NaN: no clip).  Pair p: read pair_read[p] over [pair_start[p], pair_end[p]).
        -> (sig_off int64[n_pair + 1], position float64, signal float64, base_i int64), pair-major, sample order.
        `last_plot_kernel_ms`: kernel time."""
        args = _check_region_raw_signal_args(raw, raw_off, segs, segs_off, read_start, rsrtr, minus, rna, shift, scale,
                                             lower_lim, upper_lim, pair_read, pair_start, pair_end)
        (raw, roff, segs, soff, rs, rsr, mn, rn, sh, sc, lo, hi, pr, ps, pe), n_obs = args[:-1], args[-1]
        n_pair, cap, ms = pr.shape[0], int(n_obs.sum()), f64(0.0)
        sig_off = np.zeros(n_pair + 1, dtype=np.int64)
        pos, sig, base = (np.empty(cap, dtype=t) for t in (np.float64, np.float64, np.int64))
        self._call('tba_region_raw_signal', rs.shape[0], C.c_void_p(raw.ctypes.data), raw.dtype.itemsize, roff, segs,
                   soff, rs, rsr, mn, rn, sh, sc, lo, hi, n_pair, pr, ps, pe, bool(genome_centric), sig_off, pos, sig, base,
                   cap, C.byref(ms))
        self.last_plot_kernel_ms = ms.value
        return sig_off, pos, sig, base

    # ---- genome tracks (csrc/k_tracks.h) ----
    def tracks_begin(self, win_start, win_end, n_slots):
        """tba_tracks_begin: open a resident track set over [win_start, win_end) of one (chromosome, strand)"""
        _check_tracks_begin_args(win_start, win_end, n_slots)
        self._call('tba_tracks_begin', int(win_start), int(win_end), int(n_slots))
        self._trk = (int(win_end) - int(win_start), int(n_slots))

    def tracks_add(self, read_start, read_end, read_flags, read_off, slots, tile_read_off, tile_reads):
        """tba_tracks_add: add reads to the open set.  read_flags: bit 0 minus strand, bit 1 + s the read has slot s;
        slots: n_slots float64 arrays, read-centric, CSR by read_off; tile_reads / tile_read_off: per tile of
        TRK_TILE positions the reads that overlap it, in input order"""
        if getattr(self, '_trk', None) is None:
            raise ValueError('no track set is open (tracks_begin)')
        rs, re_, fl, off, sl, toff, tr = _check_tracks_add_args(
            self._trk[0], self._trk[1], read_start, read_end, read_flags, read_off, slots, tile_read_off, tile_reads)
        ptrs = (C.c_void_p * TRK_MAX_SLOTS)(*[v.ctypes.data for v in sl])
        self._call('tba_tracks_add', rs.shape[0], rs, re_, fl, off, ptrs, toff.shape[0] - 1, toff, tr)

    def tracks_finish(self, want_sums=False):
        """tba_tracks_finish -> TrackSet(means, sums or None, slot_cov, read_cov) of the open set"""
        if getattr(self, '_trk', None) is None:
            raise ValueError('no track set is open (tracks_begin)')
        W, ns = self._trk
        means, cov = np.empty((ns, W), dtype=np.float64), np.empty((ns, W), dtype=np.int64)
        sums = np.empty((ns, W), dtype=np.float64) if want_sums else None
        rcov = np.empty(W, dtype=np.int64)
        self._call('tba_tracks_finish', means, sums, cov, rcov)
        return TrackSet(means, sums, cov, rcov)

    def tracks_kernel_ms(self):
        ms = f64(0)
        self._call('tba_tracks_kernel_ms', C.byref(ms))
        return ms.value

    def tracks_compact(self, values):
        """tba_tracks_compact.  float64 values -> (positions, values) that are not NaN (filter_cs_nans);
        int64 values -> (run starts with len(values) behind them, run values) (iter_coverage_regions)"""
        v, mode = _check_compact_args(values)
        n = v.shape[0]
        pos, val, cnt = np.empty(n + 1, dtype=np.int64), np.empty(n, dtype=v.dtype), i64(0)
        self._call('tba_tracks_compact', mode, v.ctypes, n, pos, val.ctypes, C.byref(cnt))
        return pos[:cnt.value + mode].copy(), val[:cnt.value].copy()

    def tracks_diff(self, a, b):
        """tba_tracks_diff: np.nan_to_num(a - b)"""
        a, b = _check_track_pair(a, b)
        out = np.empty(a.shape[0], dtype=np.float64)
        self._call('tba_tracks_diff', a, b, a.shape[0], out)
        return out

    def tracks_topn(self, a, b, n_top):
        """tba_tracks_topn: the min(n_top, len) largest np.nan_to_num(np.abs(a - b)) -> (values, positions), largest
        first; equal values: the higher position first, at the cut as well as in the output"""
        a, b = _check_track_pair(a, b)
        if int(n_top) != n_top or n_top < 0:
            raise ValueError('n_top must be a non-negative integer')
        k = min(int(n_top), a.shape[0])
        pos, val, cnt = np.empty(k, dtype=np.int64), np.empty(k, dtype=np.float64), i64(0)
        self._call('tba_tracks_topn', a, b, a.shape[0], k, pos, val, C.byref(cnt))
        order = np.lexsort((pos[:cnt.value], val[:cnt.value]))[::-1]
        return val[order], pos[order]

    def stats(self):
        a, c = f64(0), f64(0)
        self._call('tba_batch_stats', C.byref(a), C.byref(c))
        return a.value, c.value


class DeviceArray(object):
    """A flat array in device memory owned by someone else (a Synth's last batch): address, element
    type, element count.  Engine.upload_packed takes it in place of a numpy array."""

    def __init__(self, ptr, dtype, size, owner=None):
        self.ptr, self.dtype, self.size, self.owner = int(ptr or 0), np.dtype(dtype), int(size), owner
        self.nbytes = self.size * self.dtype.itemsize
        self.shape = (self.size,)
        self.ctypes = C.c_void_p(self.ptr)     # (what a void * parameter takes, as numpy's .ctypes)


def make_synth_params(mean_dwell=9, min_dwell=2, scale=12.0, offset=90.0, noise_sd=0.25, n_lead=200,
                      n_trail=100, dac_per_pa=1.0 / 0.1709, dac_offset=10.0, reverse=False):
    """tba_synth_params: the keywords of synth.DNA_SYNTH / RNA_SYNTH + the digitisation"""
    return SynthParams(int(mean_dwell), int(min_dwell), int(n_lead), int(n_trail), float(scale), float(offset),
                       float(noise_sd), float(dac_per_pa), float(dac_offset), int(bool(reverse)), 0)


def synth_tables(sp):
    """(dwell thresholds uint32[256], noise constant) of the device generator under `sp` (host only)"""
    thr = np.zeros(256, np.uint32)
    c = f64(0.0)
    _call(lib(), 'tba_synth_dwell_thresholds', sp, thr, 256, C.byref(c))
    return thr, float(c.value)


class Synth(object):
    """Synthetic reads drawn on the device (tba_synth_*, csrc/k_synth.h): a batch is a function of
    (seed, first_read, lengths, parameters) alone."""

    def __init__(self, std_ref, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        km = np.ascontiguousarray(std_ref.level_means, dtype=np.float64)
        self.device = int(device)
        _call(self._L, 'tba_synth_create', self.device, km, int(std_ref.kmer_width), C.byref(self._h))

    def generate(self, sp, seed, n_bases, raw_dtype=np.int16, first_read=0):
        """-> (raw DeviceArray, raw_off int64[n+1], seq DeviceArray, seq_off int64[n+1]); the device
        arrays are valid until the next call"""
        nb = np.ascontiguousarray(n_bases, dtype=np.int64)
        n = nb.shape[0]
        raw_off, seq_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        d_raw, d_seq = C.c_void_p(), C.c_void_p()
        _call(self._L, 'tba_synth_generate', self._h, sp, int(seed) & 0xffffffffffffffff, int(first_read), n, nb,
              RAW_DTYPES[np.dtype(raw_dtype)], raw_off, seq_off, C.byref(d_raw), C.byref(d_seq))
        self._last = (np.dtype(raw_dtype), int(raw_off[-1]), int(seq_off[-1]))
        return (DeviceArray(d_raw.value, raw_dtype, raw_off[-1], self), raw_off,
                DeviceArray(d_seq.value, np.uint8, seq_off[-1], self), seq_off)

    def download(self):
        """the last batch as host arrays (raw, seq codes)"""
        dt, n_raw, n_seq = self._last
        raw, seq = np.empty(n_raw, dt), np.empty(n_seq, np.uint8)
        _call(self._L, 'tba_synth_download', self._h, raw.ctypes, seq)
        return raw, seq

    def close(self):
        if self._h:
            self._L.tba_synth_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def identify_stalls(eng, raw, sp):
    """tba_identify_stalls: ts.identify_stalls (running-window-mean method) of one read on the
    device; returns an int64 [k, 2] array"""
    raw = np.asarray(raw)
    if raw.dtype not in RAW_DTYPES or not raw.flags.c_contiguous:
        raw = np.ascontiguousarray(raw, dtype=np.float64)
    n = raw.shape[0]
    cap = n // (int(sp.min_consecutive_obs) + 1) + 2
    out = np.zeros((cap, 2), np.int64)
    cnt = i64(0)
    if n == 0:
        return out[:0]
    eng._call('tba_identify_stalls', raw.ctypes, RAW_DTYPES[raw.dtype], n, int(sp.window_size), int(sp.n_windows),
              int(sp.mini_window_size), float(sp.threshold), int(sp.min_consecutive_obs), int(sp.edge_buffer), out, cap,
              C.byref(cnt))
    return out[:cnt.value]


def _offsets(items):
    """int64 [n + 1]: where item i starts in the concatenation of `items`"""
    off = np.zeros(len(items) + 1, np.int64)
    np.cumsum(list(map(len, items)), out=off[1:])
    return off


def pack_stalls(stall_ints, or_none=False):
    """per-read stall interval lists (None / empty allowed) -> (int64 [m, 2], int64 offsets[n + 1]),
    or (None, None) for None and, with `or_none`, when no read has an interval (else one zero row)"""
    if stall_ints is None or (or_none and not any(s is not None and len(s) for s in stall_ints)):
        return None, None
    rows = [np.array([[int(a), int(b)] for a, b in s], dtype=np.int64).reshape(-1, 2)
            for s in stall_ints if s is not None and len(s)]
    st = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((1, 2), np.int64)
    return st, _offsets([() if s is None else s for s in stall_ints])


def pack_scale_values(scale_values):
    """per-read th.scaleValues (or None) -> (sv_in float64 [n, 4]: shift, scale, lower_lim, upper_lim;
    sv_flags int32 [n]: 1 given, | 2 with both limits), or (None, None) when no read has any"""
    if all(sv is None for sv in scale_values):
        return None, None
    sv_in = np.zeros((len(scale_values), 4))
    sv_flags = np.zeros(len(scale_values), np.int32)
    for i, sv in enumerate(scale_values):
        if sv is None:
            continue
        sv_in[i, :2] = sv.shift, sv.scale
        sv_flags[i] = 1
        if sv.lower_lim is not None and sv.upper_lim is not None:
            sv_in[i, 2:] = sv.lower_lim, sv.upper_lim
            sv_flags[i] |= 2
    return sv_in, sv_flags


def pack_samp_inds(samp_inds, out=None):
    """per-read Theil-Sen subsamples (MAX_POINTS_FOR_THEIL_SEN indices, or None) -> int64 [n, 1000], filled into
    `out` (reused staging, page-locked memory) when given.  A read of more than 1000 bases needs its row; the
    row of a read without a subsample is set to -1 whatever it held: the kernel rejects a negative index
    (TBA_INTERNAL for that read) instead of fitting a line through an earlier batch's indices -- it cannot tell
    a missing subsample from a given one."""
    si = np.empty((len(samp_inds), MAX_POINTS_FOR_THEIL_SEN), np.int64) if out is None else out
    for i, s in enumerate(samp_inds):
        si[i] = -1 if s is None else s
    return si


class PinnedStage(object):
    """Grow-only page-locked arrays by name (the staging buffers of one batch slot): `get(name,
    count, dtype)` returns a view of `count` elements, reallocating (with 1/8 slack) only when the
    held buffer is too small or of another dtype."""

    def __init__(self):
        self._bufs = {}

    def get(self, name, count, dtype):
        dtype = np.dtype(dtype)
        count = int(count)
        pa = self._bufs.get(name)
        if pa is None or pa.a.dtype != dtype or pa.a.shape[0] < count:
            if pa is not None:
                pa.close()
            pa = PinnedArray(count + count // 8 + 16, dtype)
            self._bufs[name] = pa
        return pa.a[:count]

    def close(self):
        for pa in self._bufs.values():
            pa.close()
        self._bufs.clear()


def _addr(a):
    return a.__array_interface__['data'][0]


_str_ptr = C.pythonapi.PyUnicode_AsUTF8
_str_ptr.argtypes = [C.py_object]
_str_ptr.restype = C.c_void_p


def sample_dtype(raws):
    """the sample type a batch is uploaded in: the reads' own when all share one of RAW_DTYPES, else float64"""
    dts = set(r.dtype if isinstance(r, np.ndarray) else np.asarray(r).dtype for r in raws)
    dt = dts.pop() if len(dts) == 1 else None
    return dt if dt in RAW_DTYPES else np.dtype(np.float64)


def _csr_targets(raw_off, seq_off, dt, pinned=False, stage=None):
    """(raw, seq, keep): the two big arrays of a packed batch -- views of `stage`'s reusable page-locked buffers,
    else `pinned`: fresh page-locked memory (alive while `keep` is referenced), else plain numpy arrays"""
    n_raw, n_seq = int(raw_off[-1]), int(seq_off[-1])
    if stage is not None:
        return stage.get('raw', n_raw, dt), stage.get('seq', n_seq, np.uint8), []
    if pinned:
        pr, ps = PinnedArray(n_raw, dt), PinnedArray(n_seq, np.uint8)
        return pr.a, ps.a, [pr, ps]
    return np.empty(n_raw, dt), np.empty(n_seq, np.uint8), []


def pack_code_reads(raws, seqs, pinned=False):
    """per-read sample arrays and sequences given as uint8 code arrays -> the five-tuple of pack_reads
    (one concatenation each, straight into the target)"""
    dt = sample_dtype(raws)
    raw_off, seq_off = _offsets(raws), _offsets(seqs)
    raw, seq, keep = _csr_targets(raw_off, seq_off, dt, pinned=pinned)
    if len(raws):
        np.concatenate(raws, out=raw, casting='unsafe')
        np.concatenate(seqs, out=seq, casting='unsafe')
    return raw, raw_off, seq, seq_off, keep


def pack_reads(raws, seqs, reverse=False, pinned=False, n_threads=None, stage=None):
    """tba_pack_reads: per-read sample arrays (one dtype of RAW_DTYPES, else float64) and
    sequences (str / bytes of ACGT) -> (raw, raw_off, seq, seq_off, keep) CSR arrays, copied by
    native threads with the GIL released.  `stage` (a PinnedStage): the big arrays are views of its
    reusable page-locked buffers; else `pinned`: fresh page-locked memory (keep it referenced
    through `keep`); else plain numpy arrays."""
    n = len(raws)
    dt = raws[0].dtype if n and isinstance(raws[0], np.ndarray) else None
    as_is = dt in RAW_DTYPES          # (one pass when the reads can be taken as they are)
    for r in raws if as_is else ():
        if not (isinstance(r, np.ndarray) and r.dtype == dt and r.flags.c_contiguous):
            as_is = False
            break
    if not as_is:
        dt = sample_dtype(raws)
        raws = [np.ascontiguousarray(r, dtype=dt) for r in raws]
    # sequences: the UTF-8 view of a str is its own buffer for ASCII text (no copy); the strings
    # themselves stay referenced by the caller's list for the duration of the call
    seq_ptr = [_str_ptr(s) if type(s) is str else None for s in seqs]
    if None in seq_ptr:
        seqs = [s if type(s) is str else bytes(s) for s in seqs]
        seq_ptr = [_str_ptr(s) if type(s) is str else C.cast(C.c_char_p(s), C.c_void_p).value
                   for s in seqs]
    raw_off, seq_off = _offsets(raws), _offsets(seqs)
    if any(not s.isascii() for s in seqs if type(s) is str):
        raise ValueError('sequences must be ASCII')
    raw, seq, keep = _csr_targets(raw_off, seq_off, dt, pinned=pinned, stage=stage)
    rp = (C.c_void_p * n)(*[_addr(r) for r in raws])
    sp = (C.c_void_p * n)(*seq_ptr)
    if n_threads is None:
        n_threads = min(int(os.environ.get('TBA_PACK_THREADS', '16')), os.cpu_count() or 1)
    _call(lib(), 'tba_pack_reads', n, rp, RAW_DTYPES[dt], bool(reverse), raw_off, raw.ctypes, sp, seq_off, seq,
          int(n_threads))
    return raw, raw_off, seq, seq_off, keep


def unpack_reads(src, src_off, count, dtype=None, n_threads=None):
    """tba_unpack_reads: [src[src_off[i]:src_off[i] + count[i]].copy() for i], the copies made
    by native threads.  The per-read arrays are views of ONE fresh allocation (a single large
    mapping takes huge pages where the kernel offers them: first-touch page faults, not the copy,
    bound this step with one malloc per read), so they keep each other's memory alive."""
    n = len(count)
    dt = src.dtype if dtype is None else np.dtype(dtype)
    cnt = np.ascontiguousarray(count, dtype=np.int64)
    if n == 0:
        return []
    off = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    arena = np.empty(int(off[-1]), dt)
    so = np.ascontiguousarray(src_off, dtype=np.int64)
    dp = (np.uint64(_addr(arena)) + off[:-1].astype(np.uint64) * np.uint64(dt.itemsize)).astype(np.uint64)
    if n_threads is None:
        n_threads = min(32, os.cpu_count() or 1)
    _call(lib(), 'tba_unpack_reads', n, src.ctypes, dt.itemsize, so, cnt, dp.ctypes, int(n_threads))
    return np.split(arena, off[1:-1])

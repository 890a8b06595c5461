/* include/tombo_amd.h -- C ABI of the MI355X-native resquiggle engine (libtombo_amd.so).
 *
 * Drop-in boundary for the hot path of nanoporetech/tombo v1.5.1: everything below
 * tombo.resquiggle.resquiggle_read() (tombo/resquiggle.py:1122-1214) -- i.e. the thirteen
 * Python-callable Cython kernels of tombo/_c_dynamic_programming.pyx and tombo/_c_helper.pyx
 * plus the numpy glue between them -- runs as HIP kernels for gfx950 behind these entry points.
 * Plain pointers and sizes only; caller owns every host buffer; no exceptions cross the ABI:
 * every per-read failure is a status code (TBA_* below == the reference's TomboError strings,
 * table in tombo_amd/errors.py).  All arithmetic on the path is IEEE float64 / int64 in the
 * reference's operation order (device code is built with -ffp-contract=off).
 *
 * Two levels:
 *   1. the batch engine (tba_engine_*, tba_batch_*): N reads packed as ragged SoA buffers, one
 *      fixed kernel sequence per batch on one HIP stream; this is what resquiggle_read /
 *      resquiggle_batch call and what bench.py times (inputs resident in HBM).  The same
 *      sequence can be run stage by stage with the caller's intermediates injected
 *      (tba_batch_run_stages / tba_batch_put: the reference's public per-stage functions,
 *      resquiggle.py:63-67), and tba_batch_base_stats adds the per-base statistics of the
 *      Events table (tombo_helper.py:2341-2362).
 *   2. per-kernel entry points (tba_c_*): one call == one call of the Cython function it
 *      cites, same argument meaning, host pointers in / host pointers out, executed by the same
 *      device code (batch of one).  These are what a maintainer binds in place of the Cython
 *      modules (INTEGRATION.md shows the ctypes stubs).
 */
#ifndef TOMBO_AMD_H
#define TOMBO_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (per read) ------------------------------------------------------------ */
enum {
    TBA_OK = 0,
    TBA_TOO_MUCH_SIGNAL = 1,        /* resquiggle.py:1160 */
    TBA_FEWER_CPTS = 2,             /* _c_helper.pyx:118,200 */
    TBA_READ_TOO_SHORT_START = 3,   /* resquiggle.py:704 */
    TBA_MAP_TOO_SHORT_START = 4,    /* resquiggle.py:706 */
    TBA_POOR_START = 5,             /* resquiggle.py:745 */
    TBA_INVALID_START_PATH = 6,     /* tombo_stats.py:2356 */
    TBA_OPEN_PORE = 7,              /* resquiggle.py:1009 */
    TBA_STARTS_TOO_FAR = 8,         /* resquiggle.py:612 */
    TBA_MASK_TOO_FEW = 9,           /* resquiggle.py:672 */
    TBA_ADAPT_BEYOND = 10,          /* _c_dynamic_programming.pyx:354 */
    TBA_BEYOND_BANDWIDTH = 11,      /* _c_dynamic_programming.pyx:305 */
    TBA_DISCORDANT = 12,            /* resquiggle.py:976 */
    TBA_NOT_ENOUGH_DEL_SIGNAL = 13, /* resquiggle.py:490 */
    TBA_TOO_MANY_DELS = 14,         /* resquiggle.py:495 */
    TBA_INVALID_SEG = 15,           /* resquiggle.py:530 */
    TBA_ZERO_LEN = 16,              /* resquiggle.py:534 */
    TBA_NEG_START = 17,             /* resquiggle.py:536 */
    TBA_PAST_END = 18,              /* resquiggle.py:538 */
    TBA_RESCALE_FAIL = 19,          /* tombo_stats.py:421 */
    TBA_SEQ_SEG_MISMATCH = 20,      /* resquiggle.py:1201 */
    TBA_NO_RAW = 21,                /* resquiggle.py:1148 */
    TBA_INVALID_SEQ = 22,           /* tombo_stats.py:858 */
    TBA_TRIM_TOO_FEW_EVENTS = 23,   /* tombo_stats.py:250,258: numpy's ValueError, too few events for the windows */
    TBA_INTERNAL = 100,             /* the reference would raise a non-Tombo exception here */
    TBA_UNSUPPORTED = 101           /* valid in the reference, outside this engine's limits
                                       (band wider than TBA_MAX_BAND, scratch arena exhausted) */
};
/* call-level return values of the functions below (0 == success) */
enum { TBA_E_ARG = -1, TBA_E_HIP = -2, TBA_E_NOMEM = -3, TBA_E_STATE = -4 };

#define TBA_MAX_BAND 3072 /* widest DP band (cells per row) the wave-per-read kernel carries */
#define TBA_MAX_BATCH_READS 65535 /* reads per batch (a launch-grid dimension); longer lists are
                                     cut into batches by the host (tombo_amd/planner.py) */

/* th.resquiggleParams (tombo/tombo_helper.py:173-198) */
typedef struct {
    double match_evalue, skip_pen, max_half_z_score, z_shift, stay_pen;
    int64_t bandwidth, running_stat_width, min_obs_per_base, raw_min_obs_per_base,
        mean_obs_per_event, use_t_test_seg, band_bound_thresh, start_bw, start_save_bw,
        start_n_bases;
    int64_t do_winsorize_z; /* max_half_z_score is not None */
} tba_params;

/* remaining arguments of resquiggle_read (resquiggle.py:1122-1127) that apply to a whole batch */
typedef struct {
    int64_t has_outlier_thresh; double outlier_thresh;
    int64_t has_const_scale;    double const_scale;
    int64_t skip_seq_scaling;
    int64_t check_start_score;  double sig_match_thresh; /* seq_samp_type given */
    int64_t max_raw_cpts;                                 /* < 0: None */
    double  min_event_to_seq_ratio;
    int64_t use_rna_event_scale, rna_scale_num_events;    /* _default_parameters.py:78-80 */
    double  rna_scale_max_frac_events;
    int64_t skip_norm_out; /* engine option: do not materialise the final normalised signal (the
                              caller recomputes it from raw + scale_values, as Tombo does when it
                              reads a resquiggled FAST5 back: tombo_helper.py get_raw_read_slot /
                              tombo_stats.normalize_raw_signal); norm_signal downloads are refused */
    /* ---- the worker's per-read preparation (_resquiggle_worker.adjust_map_res,
     * resquiggle.py:1506-1530), on the device, part of the upload / of tba_batch_enqueue ---- */
    int64_t reverse_raw;   /* the samples arrive in acquisition order (direct RNA: 3'->5') and are
                              flipped in place once after the upload: raw_signal[::-1], :1516 */
    int64_t detect_stalls; /* ts.identify_stalls(raw_signal, MEAN_STALL_PARAMS) (tombo_stats.py:
                              269-368, the running-window-mean method; :1524-1528) over the
                              (flipped) raw samples; its intervals take the place of stall_ints,
                              which must then be NULL */
    int64_t stall_window_size, stall_n_windows, stall_mini_window_size,
        stall_min_consecutive_obs, stall_edge_buffer; /* th.stallParams, tombo_helper.py:200-214 */
    double  stall_threshold;
    int64_t device_subsample; /* draw the Theil-Sen subsample of reads with more than 1000 bases
                              (np.random.choice(B, 1000, replace=False), tombo_stats.py:411-416)
                              on the device instead of taking samp_ind: the first 1000 images of
                              a keyed pseudo-random permutation of [0, B) (counter based: a
                              function of subsample_seed and the read's index in the batch) */
    uint64_t subsample_seed;
    int64_t subsample_first_read; /* index, in the caller's job, of the batch's first read: read i of the batch
                              draws under the key of (subsample_seed, subsample_first_read + i), so the subsample
                              of a read does not depend on how its list was cut into batches */
    /* keyword arguments of resolve_skipped_bases_with_raw (resquiggle.py:405-407): bases a window
     * around a skipped base starts with / may grow to, and the signal a window must hold relative to
     * its bases.  All three zero (a zero-initialised struct): the reference's defaults 2 / 10 / 1.1
     * (_default_parameters.py:72,73,67). */
    int64_t del_fix_window, max_del_fix_window;
    double  extra_sig_factor;
} tba_opts;

typedef struct tba_engine tba_engine;

/* ---- engine ----------------------------------------------------------------------------- */
/* One engine per process per GPU (reads shard across GPUs by process; no collective).
 * device: HIP ordinal.  Fails with TBA_E_HIP when no gfx950 device is usable: there is no CPU
 * fallback in this library. */
int  tba_engine_create(int device, tba_engine **out);
void tba_engine_destroy(tba_engine *e);
const char *tba_last_error(void);
int  tba_device_count(void);
/* free / total bytes of the engine's device (hipMemGetInfo): what a batch planner budgets against */
int  tba_device_mem(tba_engine *e, int64_t *free_bytes, int64_t *total_bytes);

/* device bytes held by this engine's (grow-only) batch buffers */
int  tba_engine_held_bytes(tba_engine *e, int64_t *bytes);
/* Scheduling hint, no effect on results: n_engines = how many engines are fed concurrently on this
 * engine's device (the slots of a streaming pipeline; 1 = this engine has the device to itself, the
 * default).  With n_engines > 1 a batch whose work is mostly outside the banded DP (RNA) runs the
 * register-capped build of the DP kernel so that the other engines' kernels fit beside it. */
int  tba_engine_set_sharing(tba_engine *e, int n_engines);
/* (ABI 9: tba_engine_set_dp_workgroup_batch is gone with the workgroup-per-read form of the main forward pass it
 * switched on -- measured slower in round 4, profiles/r04_dp_workgroup_form.txt; TBA_GET_DP_WORKGROUP reads zeros.) */
/* Event detection (c_valid_cpts_w_cap, _c_helper.pyx:89-120) and the main traceback
 * (c_banded_traceback, _c_dynamic_programming.pyx:281-310) each have a LATENCY and a THROUGHPUT
 * form with identical results; which one a batch takes depends on its read count alone:
 *   - DNA event detection: batches of at most small_batch_reads reads scan a workgroup per read
 *     and keep the score array (k_cumsum_scores_long + k_peaks); larger ones run the score-free
 *     pipeline k_detect + k_pick (with the last pass of the normalisation in its loader);
 *   - traceback: batches of at most tb_wave_below reads give every read a wavefront
 *     (k_main_tb_par<64>), larger ones 16 lanes (k_main_tb_par<16>).
 * Both thresholds default to 1 024 reads; a negative argument leaves a threshold as it is, 0 sends
 * every batch through the throughput form.  Applied from the next tba_batch_enqueue /
 * tba_batch_run_stages.  The parity tests run through both forms by this entry; the environment
 * variables TBA_SMALL_BATCH_READS / TBA_TB_WAVE_BELOW set the same at engine creation.
 * TBA_GET_ED_FORM / TBA_GET_TB_FORM report which kernels actually produced each read's result. */
int  tba_engine_set_dispatch(tba_engine *e, int64_t small_batch_reads, int64_t tb_wave_below);
int  tba_engine_get_dispatch(tba_engine *e, int64_t *small_batch_reads, int64_t *tb_wave_below);
/* The side stream.  A full run (tba_batch_enqueue / tba_batch_run) puts what does not depend on the
 * signal's normalisation -- the stall detector (ts.identify_stalls, RNA) and the expected levels of the
 * sequences (get_exp_levels_from_seq) -- on a second stream of the engine, beside normalisation and
 * event detection, and joins it where the reference's order needs the results; identical results (an
 * invalid base still loses to an earlier segmentation error of the same read).  mode -1 (default):
 * used while at most two engines are alive on the device in this process (TBA_SIDE_STREAM_MAX_ENGINES)
 * and tba_engine_set_sharing says no more -- more streams than hardware queues serialise behind each
 * other; 0: never; 1: always.  tba_engine_last_side_stream: whether the last full run used it. */
int  tba_engine_set_side_stream(tba_engine *e, int mode);
int  tba_engine_last_side_stream(tba_engine *e);
/* whether the last run launched k_dp8_lowreg, the register-capped build of the 8-cell forward pass, in place of
 * k_dp<8> (the choice tba_engine_set_sharing describes; per read: TBA_GET_DP_FORM) */
int  tba_engine_last_dp_lowreg(tba_engine *e);
/* The forward pass divides by the level's sd.  Where every sd of the model (tba_set_model) is a divisor for which
 * the two-operation form fma(a, yh, a * yl) -- yh + yl the reciprocal as a pair -- is proven to BE IEEE division,
 * for every dividend, the batch form of the forward pass uses it (k_dp_cdiv: same results bit for bit, fewer float64
 * operations); a batch whose sds came through TBA_PUT_REF_SDS, a main pass on k_dp8_lowreg and the per-kernel C
 * entries keep the general division.
 * tba_engine_last_dp_const_division: bit 0 -- the last run's main forward pass took it, bit 1 -- start discovery did.
 * tba_engine_set_dp_const_division: mode 1 (default) as above, 0 never; from the next run.
 * tba_engine_model_const_division: 1 when the model's table is proven.
 * tba_prove_const_division: host only, no device needed: proven[i] = 1 when the form is proven for sd[i], else 0
 * (not finite, not positive, subnormal, outside [2^-256, 2^256], an all-ones significand: 0). */
int  tba_engine_last_dp_const_division(tba_engine *e);
int  tba_engine_set_dp_const_division(tba_engine *e, int mode);
int  tba_engine_model_const_division(tba_engine *e);
int  tba_prove_const_division(const double *sd, int64_t n, int32_t *proven);
/* A level table whose sd column holds ONE value (Tombo's DNA and RNA models), that value a proven divisor: the
 * reciprocal pair is the same in every row of every read, so tba_set_model makes it once on the host and the forward
 * pass gets it as two kernel arguments (k_dp_c1: k_dp_cdiv with the pair the same in every lane instead of a lane
 * per row, the level mean as the only per-row load, and no arg-max in the static rows whose arg-max nobody reads; same results bit for bit).  It runs wherever
 * k_dp_cdiv would (above) and the table has one sd; tba_engine_last_dp_const_division and TBA_GET_DP_FORM report it as
 * the two-operation form it is, TBA_GET_DP_ONE_SD tells the two apart per read (ABI 13.1).
 * tba_one_sd_words: host only, no device needed: *one_sd = 1 and words[0..2] = sd, yh = RN(1 / sd),
 * yl = RN(RN(1 - sd yh) yh) when the n values of sd are one bit pattern and proven, else *one_sd = 0 and zeros. */
int  tba_one_sd_words(const double *sd, int64_t n, int32_t *one_sd, double *words);
/* TBA_ED_FORM_* of the last tba_c_valid_cpts_w_cap / tba_c_valid_cpts_w_cap_t_test call on this engine
 * (those entries follow the engine's dispatch like a batch of one read) */
int  tba_c_last_ed_form(tba_engine *e);

/* canonical k-mer level table, lexicographic k-mer order (TomboModel, tombo_stats.py:580-919;
 * lookup replaces get_exp_levels_from_seq :834-862) */
int tba_set_model(tba_engine *e, const double *kmer_means, const double *kmer_sds,
                  int64_t kmer_width, int64_t central_pos);

/* ---- host memory for streaming -----------------------------------------------------------
 * Page-locked host buffers: uploads from / downloads into them are true DMA transfers that
 * overlap with kernels of other engines (one engine == one batch slot == one HIP stream; a
 * streaming caller keeps 2-3 engines per GPU busy: upload N+1 || compute N || download N-1,
 * the analogue of the reference's reader -> worker -> writer processes,
 * resquiggle.py:1859-1950).  Pageable buffers work everywhere too, but make the "async" calls
 * block while HIP stages them. */
int tba_pinned_alloc(int64_t bytes, void **out);
int tba_pinned_free(void *p);

/* raw sample types accepted at the boundary: float64 (the reference's in-memory type), float32,
 * or the int16 DAC values as the FAST5 file stores them (`Signal`, resquiggle.py:1397).  Widening
 * to float64 happens on the device and is exact: results are bit-identical for the same values. */
enum { TBA_RAW_F64 = 0, TBA_RAW_F32 = 1, TBA_RAW_I16 = 2 };

/* ---- batch pipeline == resquiggle_read() for n_reads reads -------------------------------
 * raw_off[n+1], seq_off[n+1]: CSR offsets into raw (float64 pA / DAC values) and seq (uint8
 * codes 0..3 = ACGT, genome_seq including the k-mer flanks).
 * Optional per-read inputs (NULL to omit):
 *   sv_in[n][4] + sv_flags[n]: map_res.scale_values (shift, scale, lower, upper); flag bit0 =
 *       scale values given, bit1 = limits given (second and later run_rsqgl_iters passes,
 *       resquiggle.py:1498-1503);
 *   samp_ind[n][1000]: the np.random.choice subsample of calc_kmer_fitted_shift_scale
 *       (tombo_stats.py:411-416); required for reads with more than 1000 bases unless
 *       skip_seq_scaling;
 *   stall_off[n+1], stall_ints[][2]: map_res.stall_ints (RNA).
 */
int tba_batch_upload(tba_engine *e, const tba_params *p, const tba_opts *o, int64_t n_reads,
                     const double *raw, const int64_t *raw_off,
                     const uint8_t *seq, const int64_t *seq_off,
                     const double *sv_in, const int32_t *sv_flags,
                     const int64_t *samp_ind,
                     const int64_t *stall_ints, const int64_t *stall_off);
/* Same with a typed raw buffer (TBA_RAW_*), enqueue only: every copy is issued on the engine's
 * stream and the call returns; the caller's buffers (raw, seq, sv_in, samp_ind, stall_ints) must
 * stay valid and unchanged until tba_batch_sync / tba_batch_query reports the engine idle.
 * tba_batch_upload == this with TBA_RAW_F64 followed by tba_batch_sync.
 * raw and seq may also be device memory of the engine's GPU (a batch made by tba_synth_generate):
 * the copy kind is taken from the pointers. */
int tba_batch_upload_async(tba_engine *e, const tba_params *p, const tba_opts *o, int64_t n_reads,
                           const void *raw, int raw_dtype, const int64_t *raw_off,
                           const uint8_t *seq, const int64_t *seq_off,
                           const double *sv_in, const int32_t *sv_flags,
                           const int64_t *samp_ind,
                           const int64_t *stall_ints, const int64_t *stall_off);
/* device bytes a batch of these reads would occupy (what tba_batch_upload* allocates): lets a
 * host planner cut a read list into batches that fit a memory budget before uploading */
int tba_batch_footprint(const tba_params *p, const tba_opts *o, int64_t kmer_width, int raw_dtype,
                        int64_t n_reads, const int64_t *n_raw, const int64_t *seq_len,
                        double *bytes);
/* runs the whole kernel sequence on the uploaded batch; returns after the stream is idle */
int tba_batch_run(tba_engine *e);
/* same, but only enqueues (for timing with events / overlapping); pair with tba_batch_sync */
int tba_batch_enqueue(tba_engine *e);
int tba_batch_sync(tba_engine *e);
/* the kernel sequence enqueued NEXT on e starts after the one last enqueued on `other` has
 * finished (copies are not ordered): a streaming caller keeps the batches' kernels back to back
 * instead of interleaved while uploads and downloads of other slots overlap them */
int tba_batch_wait_for(tba_engine *e, tba_engine *other);
/* 0: the engine's stream is idle; 1: work still in flight (never blocks) */
int tba_batch_query(tba_engine *e);
/* Outputs (any pointer may be NULL):
 *   status[n]; segs (CSR by seg_off[i] = seq_off[i] - i*(K-1) + i, B_i+1 entries per read);
 *   read_start_rel_to_raw[n]; norm_signal (same CSR as raw; first norm_len[i] entries valid);
 *   scale_values[n][4]; sig_match_score[n]; norm_params_changed[n] */
int tba_batch_download(tba_engine *e, int32_t *status, int64_t *segs,
                       int64_t *read_start_rel_to_raw, double *norm_signal, int64_t *norm_len,
                       double *scale_values, double *sig_match_score,
                       int32_t *norm_params_changed);
/* Compact per-read record + enqueue-only download: results[n] (64 bytes per read: what
 * resquiggle_read returns besides the arrays), the base boundaries as int32 (segs32) and / or
 * int64 (segs64), CSR by seg_off like tba_batch_download, and the normalised signal (refused
 * under tba_opts.skip_norm_out).  The records and int32 boundaries are packed by a kernel on the
 * engine's stream, the copies follow on the same stream; the outputs are valid after
 * tba_batch_sync.  lower_lim / upper_lim are NaN where scale_values has None. */
typedef struct {
    int32_t status, norm_params_changed;
    int64_t read_start_rel_to_raw, norm_len;
    double shift, scale, lower_lim, upper_lim, sig_match_score;
} tba_read_result;
int tba_batch_download_async(tba_engine *e, tba_read_result *results, int32_t *segs32,
                             int64_t *segs64, double *norm_signal);
/* stage-wise intermediates of the last run, for parity tests (what: TBA_GET_*; CSR layouts in
 * tombo_amd/_native.py) */
enum {
    TBA_GET_VALID_CPTS = 1,   /* int64, CSR by ev_off (capacity num_events per read) */
    TBA_GET_N_CPTS = 2,       /* int64[n] */
    TBA_GET_EVENT_MEANS = 3,  /* float64, CSR by ev_off */
    TBA_GET_SEG_NORM = 4,     /* float64, CSR by raw_off: normalised signal before trimming */
    TBA_GET_SEG_SV = 5,       /* float64[n][4] */
    TBA_GET_START = 6,        /* float64[n][4]: (loc, events_per_base) of call 0 and call 1 */
    TBA_GET_BAND_STARTS = 7,  /* int64, CSR by ref_off (B per read) */
    TBA_GET_READ_TB = 8,      /* int64, CSR by seg_off */
    TBA_GET_DP_SEGS = 9,      /* int64, CSR by seg_off */
    TBA_GET_THEIL_SEN = 10,   /* float64[n][4] */
    TBA_GET_PATH = 11,        /* int32[n][4]: path (1 adaptive, 2 static), n_static, W, n_start_calls */
    TBA_GET_LAST_ROW = 12,    /* float64[n][TBA_MAX_BAND]: last forward-pass row */
    TBA_GET_DP_READ_START = 13, /* int64[n] */
    TBA_GET_KERNEL_MS = 14,   /* float32[32]: per-stage GPU time of the last run (events) */
    TBA_GET_REF_MEANS = 15,   /* float64, CSR by ref_off: expected levels of every base */
    TBA_GET_REF_SDS = 16,
    TBA_GET_SEGS = 17,        /* int64, CSR by seg_off: boundaries after skipped-base resolution */
    TBA_GET_STATUS = 18,      /* int32[n] */
    TBA_GET_START_FAIL = 19,  /* int32[n]: status that failed the first start-discovery try (0: none) */
    TBA_GET_STALL_INTS = 20,  /* int64[][2]: the stall intervals in force (given, or detected under
                                 tba_opts.detect_stalls), read i at STALL_OFF[i], N_STALL[i] of them */
    TBA_GET_N_STALL = 21,     /* int64[n] */
    TBA_GET_STALL_OFF = 22,   /* int64[n] */
    TBA_GET_SAMP_IND = 23,    /* int64[n][1000]: the Theil-Sen subsamples used (as uploaded, or as
                                 drawn under tba_opts.device_subsample; reads of <= 1000 bases: unused) */
    TBA_GET_TB_PARALLEL = 24, /* int32[n]: 1 where the chunk-parallel traceback walked the read (performance
                               * diagnostics: 0 on an adaptive read means the lane-per-read walk had to) */
    TBA_GET_ED_FUSED = 25,    /* int32[n]: 1 where the score-free event detection (k_detect / k_pick) finished the
                               * read, 0 where the kernels that keep the score array had to (diagnostics) */
    TBA_GET_ED_TAKEN_POS = 26, /* int32, two slots per sample (CSR by 2 * raw_off): positions of the taken list k_detect
                                * left, valid right after stage TBA_STAGE_SEGMENT only (later stages reuse the buffer) */
    TBA_GET_ED_N_TAKEN = 27,  /* int64[n]: its length per read */
    TBA_GET_DP_WORKGROUP = 28, /* int32[n]: zeros since ABI 9 (was: 1 where the removed workgroup-per-read form ran the main forward pass) */
    TBA_GET_ED_FORM = 29,     /* int32[n]: TBA_ED_FORM_*: the kernels that produced the read's change points
                               * (0: none did -- the read had failed before) */
    TBA_GET_TB_FORM = 30,     /* int32[n]: TBA_TB_FORM_*: the kernel that walked the read's main traceback */
    TBA_GET_TB_VERIFY_FAIL = 31, /* int32[n]: rows of the read where the verifier of the chunk-parallel traceback
                               * (k_tb_par_verify) found something else than its own walk; such a read was walked again
                               * by the lane-per-read kernel, so its result is the serial walk's either way.  Zero for
                               * every read is the expected state: a binding should treat anything else as a fault of
                               * the machine or the build worth reporting (ABI 9) */
    TBA_GET_DP_FORM = 32,     /* int32[n][4]: the forward-pass kernels that took the read (ABI 11): TBA_DP_FORM_* of the
                               * main pass, its cells-per-lane class (0: wide, none), TBA_DP_START_* of start discovery,
                               * the class of the retry kernel (0: no retry).  DERIVED on the host, not written by the
                               * kernels: the launch decisions the engine recorded when it enqueued the run, and per read
                               * the predicates by which the kernels select their reads (k_dp.h, k_dp_multi.h, k_dp_wg.h)
                               * over the state the run left (TBA_GET_PATH, TBA_GET_START_FAIL, start state) */
    TBA_GET_NORM_FORM = 33,   /* int32[n]: TBA_NORM_FORM_*: the code that found the medians of the read's normalisation */
    TBA_GET_TS_FORM = 34,     /* int32[n][2]: what k_theil_sen did with the read (ABI 13): TBA_TS_FORM_*, and the entries of
                               * the one-pass form's list of pairs (0 where its pass over the pairs did not run; the pairs
                               * inside the window or too close to tell, and for points beyond the float range some
                               * partners of the padding to 64, dropped later).  Written by the kernel */
    TBA_GET_DP_ONE_SD = 35,   /* int32[n][2]: whether the read's forward passes ran on k_dp_c1, the one-sd form of the
                               * two-operation division (tba_one_sd_words; ABI 13.1): [0] 1 -- the main pass did; [1] bit 0
                               * -- the first try of start discovery did, bit 1 -- its retry did (a retry by k_dp_wg never
                               * does).  Derived on the host like TBA_GET_DP_FORM, which reports these reads as before */
    TBA_GET_DEBUG_COUNTERS = 99 /* int64[n][8]: ReadState.dbg, only filled by the profiling builds (one of
                                   -DTBA_PHASE_DEBUG=<id>, -DTBA_SWEEP_STATS, -DTBA_SKIP_STATS, -DTBA_SKIP_CLASS_STATS;
                                   the slots of each: csrc/tba_phase.h), zeros otherwise */
};
enum {
    TBA_ED_FORM_NONE = 0,
    TBA_ED_FORM_WG_SCAN_PEAKS = 1,  /* latency form: workgroup-per-read scan (k_cumsum_scores_long) + k_peaks */
    TBA_ED_FORM_DETECT_PICK = 2,    /* throughput form: k_detect + k_pick, no score array */
    TBA_ED_FORM_SCORES_PEAKS = 3,   /* pipelined k_cumsum_scores (or k_cumsum + k_scores_dna) + k_peaks: reads
                                     * k_detect / k_pick flagged, parameter sets outside their limits */
    TBA_ED_FORM_DETECT_TT_PICK = 4, /* RNA: k_detect_tt + k_pick */
    TBA_ED_FORM_TTEST_PEAKS = 5     /* RNA: k_scores_ttest + k_peaks */
};
enum {
    TBA_NORM_FORM_NONE = 0,         /* no medians: scale values given or taken from the events (RNA), or the read had failed */
    TBA_NORM_FORM_SELECT = 1,       /* k_normalize: one pass per median through a sampled window, or the generic bucket select */
    TBA_NORM_FORM_INT_COUNT = 2,    /* k_normalize, int16 samples: both medians from one counting pass */
    TBA_NORM_FORM_HIST = 3          /* k_normalize_hist, float samples: all medians from one histogram pass and one list pass */
};
enum {                              /* TBA_GET_TS_FORM column 0: the Theil-Sen fit's median slope (k_theil_sen) */
    TBA_TS_FORM_NONE = 0,           /* no fit: the read had failed before, or skip_seq_scaling */
    TBA_TS_FORM_SMALL = 1,          /* fewer than 256 points: the generic two-pass select over all slopes, by design */
    TBA_TS_FORM_FAST = 2,           /* one pass over the pairs against a sampled window, exact select among the listed ones */
    /* the generic select ran because the one-pass form declined: */
    TBA_TS_FORM_NO_SCRATCH = 3,     /* room for fewer than 4096 listed pairs in the read's scratch slices */
    TBA_TS_FORM_NO_WINDOW = 4,      /* the sampled median slope is outside (0.5, 1.5) */
    TBA_TS_FORM_LIST_OVERFLOW = 5,  /* more pairs listed than the scratch holds */
    TBA_TS_FORM_WINDOW_MISS = 6     /* the window did not hold the middle ranks of all slopes */
};
enum {
    TBA_TB_FORM_NONE = 0,
    TBA_TB_FORM_LANE = 1,           /* k_main_tb: a lane per read, the serial walk on the chunk kernels' row-block walker
                                     * (static bands, reads the chunk kernels or their verifier handed back) */
    TBA_TB_FORM_LONG = 2,           /* k_main_tb_long */
    TBA_TB_FORM_PAR16 = 16,         /* k_main_tb_par<16>: throughput form */
    TBA_TB_FORM_PAR64 = 64          /* k_main_tb_par<64>: latency form, and the long reads of any batch */
};
enum {                              /* TBA_GET_DP_FORM column 0 */
    TBA_DP_FORM_NONE = 0,           /* no main forward pass: the read had failed before */
    TBA_DP_FORM_K_DP = 1,           /* k_dp<CPL>: a wavefront per read */
    TBA_DP_FORM_K_DP8_LOWREG = 2,   /* k_dp8_lowreg: the 8-cell class under 112 registers (tba_engine_set_sharing) */
    TBA_DP_FORM_MULTI = 3,          /* k_dp_multi: narrow adaptive bands, several reads per wavefront */
    TBA_DP_FORM_WIDE = 4            /* k_dp_wide: a static band wider than every class */
};
enum {                              /* TBA_GET_DP_FORM column 2 */
    TBA_DP_START_NONE = 0,          /* no start discovery: static whole-read assignment (short read), or failed before */
    TBA_DP_START_FIRST_TRY = 1,     /* the first try (k_dp<class of start_bw>) only */
    TBA_DP_START_RETRY_WG = 2,      /* ... and the retry over start_save_bw by k_dp_wg<CPL>: a workgroup per read */
    TBA_DP_START_RETRY_K_DP = 3     /* ... and the retry by k_dp<CPL> (start_n_bases beyond k_dp_wg's rows) */
};
int tba_batch_get(tba_engine *e, int what, void *out, int64_t out_bytes);
/* ---- stepwise execution (the reference's public per-stage API, resquiggle.py:63-67) ---------
 * The pipeline in stages; tba_batch_run_stages runs first..last on the uploaded batch (starting
 * at TBA_STAGE_SEGMENT resets the per-read state).  tba_batch_put injects the inputs of a later
 * stage so that it can run without the earlier ones:
 *   segment_signal                 = stage SEGMENT   (get VALID_CPTS, SEG_NORM, SEG_SV)
 *   find_seq_start_in_events       = put EVENT_MEANS/VALID_CPTS/REF_*, stage START (get START)
 *   find_adaptive_base_assignment  = put VALID_CPTS + EVENT_MEANS, stages REF_LEVELS..ASSIGN
 *   find_static_base_assignment    = same with put START_STATE = 4 (get READ_TB)
 *   resolve_skipped_bases_with_raw = put NORM, REF_*, DP_SEGS, stage SKIP (get SEGS) */
enum {
    TBA_STAGE_SEGMENT = 0,      /* normalisation + event detection (+ stall removal) */
    TBA_STAGE_EVENT_MEANS = 1,  /* compute_base_means over the change points */
    TBA_STAGE_REF_LEVELS = 2,   /* get_exp_levels_from_seq */
    TBA_STAGE_START = 3,        /* find_seq_start_in_events (+ retry) */
    TBA_STAGE_ASSIGN = 4,       /* masked start / static fallback, adaptive DP, traceback */
    TBA_STAGE_SKIP = 5,         /* resolve_skipped_bases_with_raw */
    TBA_STAGE_RESCALE = 6       /* Theil-Sen rescale + final score */
};
enum {
    TBA_PUT_VALID_CPTS = 1,   /* int64, CSR by ev_off; per_read[i] = count */
    TBA_PUT_EVENT_MEANS = 2,  /* float64, CSR by ev_off */
    TBA_PUT_NORM = 3,         /* float64, CSR by raw_off: normalised signal */
    TBA_PUT_REF_MEANS = 4,    /* float64, CSR by ref_off */
    TBA_PUT_REF_SDS = 5,
    TBA_PUT_DP_SEGS = 6,      /* int64, CSR by seg_off; per_read[2i], [2i+1] = read_start, length */
    TBA_PUT_START_STATE = 7   /* per_read[i] = 4: force the static whole-read assignment */
};
int tba_batch_run_stages(tba_engine *e, int first_stage, int last_stage);
int tba_batch_put(tba_engine *e, int what, const void *data, int64_t bytes,
                  const int64_t *per_read);
/* per-read num_events for the NEXT tba_batch_upload (segment_signal's argument); NULL clears */
int tba_set_num_events(tba_engine *e, const int64_t *num_events, int64_t n_reads);

/* Per-base event statistics of the finished batch (the compute part of the Events table that
 * write_new_fast5_group stores, tombo_helper.py:2341-2362): c_new_mean_stds (_c_helper.pyx:38-57)
 * over every successful read's final signal and boundaries, on the device.  means / stds: CSR by
 * the reads' base counts (same layout as the ref_means of tba_batch_get), B_tot doubles each;
 * entries of failed reads are left untouched. */
int tba_batch_base_stats(tba_engine *e, double *means, double *stds, int64_t n_values);

/* bytes of algorithmic traffic / cell updates of the last uploaded batch */
int tba_batch_stats(tba_engine *e, double *algorithmic_bytes, double *dp_cells);

/* ---- per-kernel entry points (one call == one Cython call; host buffers) -----------------
 * These are the parity surface, not the throughput path: every call allocates and frees its
 * device temporaries (hipMalloc / hipFree) and synchronises the stream. */
/* c_adaptive_banded_forward_pass, _c_dynamic_programming.pyx:314-412: fwd_pass[(n_bases+1)*bw],
 * fwd_pass_tb[(n_bases+1)*bw] (int64 moves) and event_starts[n_bases] are updated in place
 * from row start_seq_pos. */
int tba_c_adaptive_banded_forward_pass(tba_engine *e, double *fwd_pass, int64_t *fwd_pass_tb,
    int64_t n_bases, int64_t bandwidth, int64_t *event_starts, const double *event_means,
    int64_t n_events, const double *r_ref_means, const double *r_ref_sds, double z_shift,
    double skip_pen, double stay_pen, int64_t start_seq_pos, double mask_fill_z_score,
    int do_winsorize_z, double max_half_z_score);
/* ... with return_z_scores=True (pyx:324,339,387-388,409-410): z_scores[(n_bases - start_seq_pos) * bw]
 * receives the shifted z-scores of every row the pass computed (NULL: as above) */
int tba_c_adaptive_banded_forward_pass_z(tba_engine *e, double *fwd_pass, int64_t *fwd_pass_tb,
    int64_t n_bases, int64_t bandwidth, int64_t *event_starts, const double *event_means,
    int64_t n_events, const double *r_ref_means, const double *r_ref_sds, double z_shift,
    double skip_pen, double stay_pen, int64_t start_seq_pos, double mask_fill_z_score,
    int do_winsorize_z, double max_half_z_score, double *z_scores);
/* c_banded_forward_pass, pyx:240-279 */
int tba_c_banded_forward_pass(tba_engine *e, const double *shifted_z_scores, int64_t n_bases,
    int64_t bandwidth, const int64_t *event_starts, double skip_pen, double stay_pen,
    double *fwd_pass, int64_t *fwd_pass_tb);
/* ... with adaptive rows behind the first n_static ones (1 <= n_static <= n_bases): from row n_static on a row's
 * band start follows the arg-max of the row before (pyx:342-358, against n_events) and is written to
 * event_starts[n_static..]; the row's band cells are its row of shifted_z_scores wherever the band lies.
 * top_pos: the arg-max of the last row.
 * FOR THE TESTS of the forward pass's kernel (a z matrix of the caller's making reaches rows the event path cannot
 * be made to hold); no counterpart in the reference, not part of the drop-in surface, may change without notice. */
int tba_c_banded_forward_pass_adaptive(tba_engine *e, const double *shifted_z_scores, int64_t n_bases,
    int64_t bandwidth, int64_t *event_starts, int64_t n_static, int64_t n_events, double skip_pen,
    double stay_pen, double *fwd_pass, int64_t *fwd_pass_tb, int64_t *top_pos);
/* c_banded_traceback, pyx:281-310 */
int tba_c_banded_traceback(tba_engine *e, const int64_t *fwd_pass_tb, int64_t n_bases,
    int64_t bandwidth, const int64_t *event_starts, int64_t band_pos,
    int64_t band_boundary_thresh, int64_t *seq_poss);
/* c_base_z_scores, pyx:17-32 */
int tba_c_base_z_scores(tba_engine *e, const double *b_sig, int64_t n, double ref_mean,
    double ref_sd, int do_winsorize_z, double max_half_z_score, double *out);
/* c_new_means, _c_helper.pyx:59-71 */
int tba_c_new_means(tba_engine *e, const double *norm_signal, int64_t n_sig,
    const int64_t *new_segs, int64_t n_segs, double *means);
/* c_apply_outlier_thresh, _c_helper.pyx:73-87 */
int tba_c_apply_outlier_thresh(tba_engine *e, const double *sig, int64_t n, double lower_lim,
    double upper_lim, double *out);
/* c_valid_cpts_w_cap, _c_helper.pyx:89-120 (+ the sort of tombo_helper.py:76-82);
 * returns a TBA_* status (TBA_FEWER_CPTS ...) */
int tba_c_valid_cpts_w_cap(tba_engine *e, const double *sig, int64_t n, int64_t min_base_obs,
    int64_t running_stat_width, int64_t num_cpts, int64_t *cpts);
/* c_valid_cpts_w_cap_t_test, _c_helper.pyx:144-202 (+ sort) */
int tba_c_valid_cpts_w_cap_t_test(tba_engine *e, const double *sig, int64_t n,
    int64_t min_base_obs, int64_t running_stat_width, int64_t num_cpts, int64_t *cpts);

/* c_new_mean_stds, _c_helper.pyx:38-57: segment means and population standard deviations */
int tba_c_new_mean_stds(tba_engine *e, const double *norm_signal, int64_t n_sig,
    const int64_t *new_segs, int64_t n_segs, double *means, double *stds);
/* c_compute_slopes, _c_helper.pyx:362-377: all i<j slopes in itertools.combinations order;
 * slopes[n*(n-1)/2] */
int tba_c_compute_slopes(tba_engine *e, const double *r_event_means,
    const double *r_model_means, int64_t n, double max_slope, double *slopes);
/* c_reg_z_scores, _c_dynamic_programming.pyx:34-97: per base of [reg_start, reg_end) the
 * admissible signal interval and the negative half z-scores over it.  r_b_starts has
 * n_b_starts entries (indices up to reg_end are read).  bounds[2*i..] = (start, end) relative
 * to r_b_starts[reg_start]; z_off[reg_len+1] = offsets of each base's scores inside z (capacity
 * z_cap doubles; TBA_E_ARG if too small -- reg_len * (r_b_starts[reg_end] -
 * r_b_starts[reg_start]) always suffices). */
int tba_c_reg_z_scores(tba_engine *e, const double *r_sig, int64_t n_sig,
    const double *r_ref_means, const double *r_ref_sds, int64_t n_bases,
    const int64_t *r_b_starts, int64_t n_b_starts, int64_t reg_start, int64_t reg_end,
    int64_t max_base_shift, int64_t min_obs_per_base, int do_winsorize_z,
    double max_half_z_score, int64_t *bounds, int64_t *z_off, double *z, int64_t z_cap);
/* c_base_forward_pass, _c_dynamic_programming.pyx:99-163: b_data has b_end - b_start entries,
 * the prev_* arrays prev_b_end - prev_b_start; outputs b_fwd_data / b_last_diag of b_end -
 * b_start entries.  TBA_INTERNAL where the reference raises IndexError. */
int tba_c_base_forward_pass(tba_engine *e, const double *b_data, int64_t b_start, int64_t b_end,
    const double *prev_b_data, int64_t prev_b_start, int64_t prev_b_end,
    const double *prev_b_fwd_data, const int64_t *prev_b_last_diag, int64_t min_obs_per_base,
    double *b_fwd_data, int64_t *b_last_diag);
/* c_base_traceback, _c_dynamic_programming.pyx:165-182: *sig_pos = the new base boundary, or
 * -1 where the reference returns None */
int tba_c_base_traceback(tba_engine *e, const double *curr_b_data, int64_t curr_len,
    int64_t curr_start, const double *next_b_data, int64_t next_len, int64_t next_start,
    int64_t next_end, int64_t sig_start, int64_t min_obs_per_base, int64_t *sig_pos);

/* ---- row N4: per-position log-likelihood ratios of the model-comparison statistics ---------
 * c_calc_llh_ratio (kind 0), c_calc_llh_ratio_const_var (1), c_calc_scaled_llh_ratio_const_var (2)
 * (_c_helper.pyx:277-358) for n_windows windows of `width` values starting at starts[i] of the
 * per-base arrays (n_values entries each), the slicing of tombo_stats.py:4042-4074.  kind 1 / 2
 * take the constant variance from ref_vars[starts[i]] and ignore alt_vars (may be NULL);
 * kind 2: par = {scale_factor, density_height_factor, density_height_power}.  One call with
 * one window == one call of the Cython function.  Transcendental functions are the device
 * library's: results match the reference to ~1e-13 relative, kind 1 bit for bit. */
int tba_llh_ratio_windows(tba_engine *e, int kind, const double *means, const double *ref_means,
    const double *alt_means, const double *ref_vars, const double *alt_vars, int64_t n_values,
    int64_t width, const int64_t *starts, int64_t n_windows, const double *par, double *out);

/* compute_sample_compare_read_stats / compute_de_novo_read_stats (tombo_stats.py:3675-3873)
 * after their file access: per-base p-values 2 * Phi(-|mean - ref_mean| / ref_sd), combined by
 * Fisher's method over windows of 2 * fm_offset + 1 positions when fm_offset > 0
 * (calc_window_fishers_method :2252-2271, SMALLEST_PVAL floor; the first / last fm_offset
 * positions of a read are NaN), NaN wherever an input is NaN (control positions without
 * coverage).  floor_out != 0: the de novo form (result floored at smallest_pval).  n_reads reads
 * as CSR slices off[n_reads + 1] of the three arrays and of pvals.  erfc / log / exp are the
 * device library's: ~1e-14 relative to scipy. */
int tba_read_pvals(tba_engine *e, const double *means, const double *ref_means,
    const double *ref_sds, const int64_t *off, int64_t n_reads, int64_t fm_offset, int floor_out,
    double smallest_pval, double *pvals);
/* ---- level pileups across reads: level_sample_compare and the control reference levels ------
 * A batch of regions in one call.  Region r: genomic [reg_start[r], reg_end[r]), strand
 * reg_strand[r] (0 '+', 1 '-', 2 none: no strand filter), its reads reg_read_off[r] ..
 * reg_read_off[r + 1] - 1 of the read arrays; read q: genomic start read_start[q], strand
 * read_strand[q] (0 / 1), read-centric levels means[read_off[q] .. read_off[q + 1]) (NaN: no
 * level); read_ctrl[q] != 0 puts it in the control group.  Reads of the other strand are skipped.
 * Outputs are laid out by the extended regions [reg_start - fm_offset, reg_end + fm_offset): region
 * r owns entries from P_r = sum over earlier regions of their extended lengths.
 *
 * tba_group_level_stats: compute_group_reg_stats (tombo_stats.py:4236-4398).  stat_kind 0 KS, 1 U,
 * 2 t; return_p 1: p-values (Fisher's method over 2 fm_offset + 1 positions when fm_offset > 0,
 * floored at smallest_pval), 0: statistics (window means).  Per region out_counts[r] tested
 * positions, compacted at P_r: out_stats, out_poss (genomic), out_cov / out_ctrl_cov (sample /
 * control coverage).  U ranks equal values sample first. */
int tba_group_level_stats(tba_engine *e, int stat_kind, int return_p, int64_t fm_offset,
    int64_t min_test_reads, int64_t n_regions, const int64_t *reg_start, const int64_t *reg_end,
    const int8_t *reg_strand, const int64_t *reg_read_off, int64_t n_reads,
    const int64_t *read_start, const int8_t *read_strand, const int8_t *read_ctrl,
    const int64_t *read_off, const double *means, double smallest_pval, double *out_stats,
    int64_t *out_poss, int64_t *out_cov, int64_t *out_ctrl_cov, int64_t *out_counts);
/* get_reads_ref (tombo_stats.py:3627-3673): every read is one group.  Per extended position:
 * out_cov, and where out_cov >= min_test_reads the median (est_mean: mean) and population sd of
 * the levels, else NaN.  prior_means / prior_sds (both or neither; per extended position): the
 * posterior blend with weights prior_w_mean / prior_w_sd (compute_posterior_samp_dists).  Zero
 * sd becomes NaN in both outputs. */
int tba_reads_ref_levels(tba_engine *e, int est_mean, int64_t fm_offset, int64_t min_test_reads,
    int64_t n_regions, const int64_t *reg_start, const int64_t *reg_end, const int8_t *reg_strand,
    const int64_t *reg_read_off, int64_t n_reads, const int64_t *read_start,
    const int8_t *read_strand, const int64_t *read_off, const double *means,
    const double *prior_means, const double *prior_sds, double prior_w_mean, double prior_w_sd,
    double *out_means, double *out_sds, int64_t *out_cov);

/* ---- per-site modified fractions of the model-based tests ------------------------------------
 * compute_reg_stats / collate_reg_stats / apply_per_read_thresh (tombo_stats.py:4084-4229) and
 * calc_damp_fraction (:2537-2552) for a batch of n_tracks tracks in one call.  A track is one
 * (region, statistic name): genomic interval [trk_start[t], trk_end[t]) in which its statistics
 * lie; outputs are laid out by the tracks: track t owns entries from P_t = sum over earlier tracks
 * of their lengths.  The per-read statistics are computed on the device by the code of
 * tba_read_pvals / tba_llh_ratio_windows (same results) and stay there.
 *   form 0 (de_novo, sample_compare): means / ref_means / ref_sds / off / n_reads / fm_offset /
 *     floor_out / smallest_pval as tba_read_pvals; read r belongs to track read_track[r] and its
 *     first value lies at genomic position read_pos[r].  The window arguments are ignored.
 *   form 1 (model_compare): kind / means / ref_means / alt_means / ref_vars / alt_vars / n_values /
 *     width / starts / n_windows / par as tba_llh_ratio_windows; window w belongs to track
 *     win_track[w] at genomic position win_pos[w].  The read arguments are ignored.
 * Every non-NaN statistic counts as coverage of its (track, position); it is valid coverage when
 * stat <= *lower_thresh || stat >= single_read_thresh (lower_thresh given), else in form 1 when
 * |stat| >= single_read_thresh, else always.  Per track out_counts[t] positions with coverage, in
 * ascending order, compacted at P_t: out_frac = (valid statistics >= single_read_thresh) /
 * valid coverage (NaN without valid coverage), out_pos (genomic), out_cov, out_valid_cov;
 * out_n_stats[t] = the track's non-NaN statistics.  damp_counts = {unmod, mod} pseudo-counts and
 * out_damp_frac (both or neither): (rint(frac * valid) + unmod) / (valid + unmod + mod).
 * out_per_read (may be NULL): the statistics themselves, in the layout of tba_read_pvals' pvals
 * (form 0) or tba_llh_ratio_windows' out (form 1); without it nothing per read is copied back.
 * TBA_E_ARG: NULL pointers, offsets that do not start at 0 or decrease, a read / window whose
 * positions leave its track, fm_offset outside [0, 64]. */
int tba_site_fractions(tba_engine *e, int form, int64_t n_tracks, const int64_t *trk_start,
    const int64_t *trk_end, const double *means, const double *ref_means, const double *ref_sds,
    const int64_t *off, int64_t n_reads, const int64_t *read_track, const int64_t *read_pos,
    int64_t fm_offset, int floor_out, double smallest_pval, int kind, const double *alt_means,
    const double *ref_vars, const double *alt_vars, int64_t n_values, int64_t width,
    const int64_t *starts, int64_t n_windows, const double *par, const int64_t *win_track,
    const int64_t *win_pos, double single_read_thresh, const double *lower_thresh,
    const double *damp_counts, double *out_frac, int64_t *out_pos, int64_t *out_cov,
    int64_t *out_valid_cov, double *out_damp_frac, int64_t *out_counts, int64_t *out_n_stats,
    double *out_per_read);

/* The z tests (form 0: de_novo, form 1: sample_compare) of tba_site_fractions straight from a READS
 * TABLE: the per-read preparation of compute_reg_stats (region clip, strand flip, expected levels)
 * runs on the device, every read is uploaded once however many regions it spans.
 *   regions   track r is [reg_start[r] - fm_offset, reg_end[r] + fm_offset); outputs are laid out by
 *             P_r = sum of the earlier tracks' lengths, as in tba_site_fractions.
 *   reads     read q covers genomic [read_start[q], read_start[q] + n_q), n_q = read_off[q + 1] -
 *             read_off[q], on strand read_strand[q] (0: '+', 1: '-'); `means` and, form 0, `seq`
 *             (base codes, 0..3 = ACGT, anything else invalid) are read-centric, CSR by read_off.
 *   pairs     region r tests reads pair_read[reg_pair_off[r] .. reg_pair_off[r + 1]), in that order.
 *   form 0    expected levels from the engine's model (tba_set_model: K, cp, dn = K - cp - 1);
 *             floor_out of tba_read_pvals is 1.  pos_means / pos_sds are ignored.
 *   form 1    pos_means / pos_sds[P_r + g - (reg_start[r] - fm_offset)]: the control levels per
 *             extended position (the layout of tba_reads_ref_levels' outputs, NaN: no level);
 *             floor_out is 0.  seq is ignored.
 * A pair, read [s, e) in region [a, b), fm = fm_offset:
 *   form 0    (lag_b, lag_e) = (cp, dn) on '+', (dn, cp) on '-'; cs = max(s, a - lag_b - fm), ce =
 *             min(e, b + lag_e + fm); statistics at genomic g in [cs + lag_b, ce - lag_e).  The pair
 *             fails when ce - cs < K, when a base code of the clipped part (read indices [cs - s,
 *             ce - s) on '+', [e - ce, e - cs) on '-') is invalid, or when fm > 0 and it has fewer
 *             than 2 fm + 1 statistics.  The level at g is means[i], i = g - s on '+', e - 1 - g on
 *             '-'; the expected level is the model's row of the k-mer at read indices [i - cp, i - cp + K).
 *   form 1    cs = max(s, a - fm), ce = min(e, b + fm); statistics at g in [cs, ce), same i.  The pair
 *             fails when no g has level, pos_means and pos_sds all non-NaN, or when fm > 0 and
 *             ce - cs < 2 fm + 1.
 * A failed pair contributes nothing (the TomboError of the reference's per-read function).  The
 * statistics of the pairs, in pair order, then go through the kernels of tba_site_fractions form 0
 * unchanged.  Outputs: those of tba_site_fractions, and per pair out_pair_ok (1: not failed),
 * out_pair_pos (genomic position of its first statistic), out_pair_off[n_pairs + 1] (its first
 * statistic's index; a failed pair has none).  out_per_read (may be NULL; per_read_cap values): the
 * statistics in that layout.  out_kernel_ms (may be NULL; 2 values): device time (hipEvents) of the
 * plan, scan and gather kernels, and of the statistic and collation kernels behind them.
 * TBA_E_ARG, before anything is launched: NULL pointers, offsets that do not start at 0 or decrease,
 * a region with end <= start, pair_read outside [0, n_reads), a strand that is not 0 or 1, a read
 * that does not overlap [reg_start, reg_end) of its region, fm_offset outside [0, 64], 2^31
 * positions or more, form 0 without a model.  TBA_E_ARG after the plan: per_read_cap below the
 * number of statistics (no output is written). */
int tba_site_fractions_reads(tba_engine *e, int form, int64_t n_regions, const int64_t *reg_start,
    const int64_t *reg_end, int64_t n_reads, const int64_t *read_start, const int8_t *read_strand,
    const int64_t *read_off, const double *means, const uint8_t *seq, const int64_t *reg_pair_off,
    const int64_t *pair_read, const double *pos_means, const double *pos_sds, int64_t fm_offset,
    double smallest_pval, double single_read_thresh, const double *lower_thresh,
    const double *damp_counts, double *out_frac, int64_t *out_pos, int64_t *out_cov,
    int64_t *out_valid_cov, double *out_damp_frac, int64_t *out_counts, int64_t *out_n_stats,
    int32_t *out_pair_ok, int64_t *out_pair_pos, int64_t *out_pair_off, double *out_per_read,
    int64_t per_read_cap, double *out_kernel_ms);

/* The same per-site outputs from STORED per-read statistics (aggregate_per_read_stats,
 * tombo_stats.py:4699-4777): n_blocks blocks of a per-read statistics file, block t covering
 * genomic [blk_start[t], blk_end[t]) and owning records rec_off[t] .. rec_off[t + 1] of `records`,
 * which holds the blocks' records concatenated in the layout they are stored in: numpy's packed
 * [('pos','u4'),('stat','f8'),('read_id','u4')], 16 bytes per record with the float64 at byte
 * offset 4 (no repack on the host; the read id is not used).  Any order inside a block.
 * Validity as above: lower_thresh given; else form 1 (model_compare): |stat| >= single_read_thresh;
 * else (form 0) every statistic.  NaN statistics are dropped.  Outputs as tba_site_fractions, a
 * block being a track: block t owns entries from P_t = sum of the earlier blocks' lengths, a block
 * without records gives out_counts[t] = 0.  Only the outputs are copied back.  out_kernel_ms (may
 * be NULL): device time of the call's kernels (hipEvents).
 * TBA_E_ARG: NULL pointers, offsets that do not start at 0 or decrease, a block with
 * end <= start, 2^31 positions or more in one call (nothing is launched for any of these); a
 * record whose position lies outside its block (found on the device: such a record is counted
 * and otherwise ignored, no output is written). */
int tba_site_aggregate(tba_engine *e, int64_t n_blocks, const int64_t *blk_start,
    const int64_t *blk_end, const int64_t *rec_off, const void *records, double single_read_thresh,
    const double *lower_thresh, int form, const double *damp_counts, double *out_frac,
    int64_t *out_pos, int64_t *out_cov, int64_t *out_valid_cov, double *out_damp_frac,
    int64_t *out_counts, int64_t *out_n_stats, double *out_kernel_ms);

/* ---- ROC / precision-recall from stored statistics (tombo_stats.py:2377-2535) -----------------
 * Records are (rec_pos, rec_stat) pairs, CSR by block: block t owns rec_off[t] .. rec_off[t + 1].
 *
 * tba_roc_motif_labels: compute_motif_stats (mode 0) / compute_ctrl_motif_stats (mode 1).  Block t
 * lies on the minus strand when blk_minus[t] != 0 and carries the base codes seq[seq_off[t] ..
 * seq_off[t + 1]) (0..3 = ACGT, anything else: not a base) of the genome from coordinate
 * blk_seq_start[t] on; a minus-strand block is read as the complement, backwards.  Motif k is
 * motifs[3k .. 3k + 2] = (length, 1-based modified position, base code of the modified position or
 * a value above 3 for a letter that is not a base) and `length` 4-bit base sets (bit c: code c
 * allowed) in motif_sets, all motifs concatenated.  A motif matches at a record when all of its
 * positions, the modified one on the record, lie inside the block's sequence and hold an allowed
 * base.  mode 0: a (record, motif) pair is kept when the base under the record, in strand
 * orientation, is the motif's modified base; its label is whether the motif matches.  mode 1: a
 * pair is kept when the motif matches; its label is `label`.
 * Outputs: the kept pairs of motif 0 in record order, then those of motif 1, ...: out_stats,
 * out_has_mod (0 / 1) and, unless NULL, out_index (the record) -- capacity n_motifs * n_records
 * each; out_counts[n_motifs].  out_kernel_ms (may be NULL): device time of the kernels.
 *
 * tba_roc_loc_labels: compute_ground_truth_stats.  Block t owns mod_locs[blk_loc[4t] ..
 * blk_loc[4t + 1]) and unmod_locs[blk_loc[4t + 2] .. blk_loc[4t + 3]), each slice ascending.  A
 * record is kept when its position is in either slice; its label is whether it is in the first.
 * Outputs as above with one motif (capacity n_records).
 *
 * tba_roc_rank_counts: out_tp_at[j] = entries with has_mod != 0 among the ranks[j] + 1 first
 * entries in ascending (statistic, has_mod) order (-0.0 equals 0.0; of equal statistics the
 * unmodified come first); out_tp_total: all of them; out_n_nan: NaN statistics (the counts mean
 * nothing when there is one).  n < 2^31; ranks non-decreasing inside [0, n).  out_kernel_ms (may be
 * NULL): two values, the device time of the keys and the sort, and of the label scan and the gather.
 * tba_roc_sort_tile: entries per workgroup and pass of that call's sort.
 *
 * TBA_E_ARG: NULL pointers, offsets that do not start at 0 or decrease, 2^31 records or more, no
 * motif or more than 64, a motif with length outside [1, 1024] or its modified position outside
 * it, a location slice outside its list, bad ranks.  Nothing is launched for any of these. */
int tba_roc_motif_labels(tba_engine *e, int64_t n_blocks, const uint8_t *blk_minus,
    const int64_t *blk_seq_start, const int64_t *seq_off, const uint8_t *seq, const int64_t *rec_off,
    const int64_t *rec_pos, const double *rec_stat, int64_t n_motifs, const int32_t *motifs,
    const uint8_t *motif_sets, int mode, int label, double *out_stats, uint8_t *out_has_mod,
    int64_t *out_index, int64_t *out_counts, double *out_kernel_ms);
int tba_roc_loc_labels(tba_engine *e, int64_t n_blocks, const int64_t *blk_loc, const int64_t *mod_locs,
    int64_t n_mod, const int64_t *unmod_locs, int64_t n_unmod, const int64_t *rec_off, const int64_t *rec_pos,
    const double *rec_stat, double *out_stats, uint8_t *out_has_mod, int64_t *out_index, int64_t *out_count,
    double *out_kernel_ms);
int tba_roc_rank_counts(tba_engine *e, int64_t n, const double *stats, const uint8_t *has_mod,
    int64_t n_ranks, const int64_t *ranks, int64_t *out_tp_at, int64_t *out_tp_total, int64_t *out_n_nan,
    double *out_kernel_ms);
int64_t tba_roc_sort_tile(void);

/* ---- pairwise distances between the rows of a matrix (tombo_stats.py:142-196) ------------------
 * rows: dense row-major float64[n_rows][row_len].  Every sum is numpy's float64 add.reduce of a
 * contiguous vector, so the outputs equal numpy's bit for bit.
 *
 * tba_pairwise_window_dists: get_pairwise_dists.  out[n_rows][n_rows]; for j <= i
 *   out[i][j] = sqrt(min over i1, i2 in [0, 2 slide_span] of
 *                    sum((rows[i][i1 : i1 + nb] - rows[j][i2 : i2 + nb])^2)),  nb = row_len - 2 slide_span
 * (Python's min over i1 outer, i2 inner: a NaN sum stays only when it is the first), and 0 for
 * j > i.  slide_span 0 is euclidian_dist.
 *
 * tba_pairwise_nanmean_dists: the metric of order_reads, np.nanmean(np.sqrt((u - v)**2)), for
 * every i < j in scipy's condensed pdist order (k = n i - i (i + 1) / 2 + j - i - 1):
 * out_condensed[n_rows (n_rows - 1) / 2]; NaN for a pair without a position where both rows hold a
 * number.  n_rows == 1 writes nothing (out_condensed may then be NULL).
 *
 * out_kernel_ms (may be NULL): device time of the call's kernel.
 * tba_pdist_tile: rows per side of the tile of pairs one workgroup owns; tba_pdist_lds_row_max:
 * the longest row the workgroup keeps in LDS (longer rows are read from global memory).
 * Limits of one call: n_rows <= 16384 (a 2 GiB matrix out) and n_rows * row_len <= 2^28 (2 GiB in).
 * TBA_E_ARG: NULL pointers, n_rows < 1, row_len < 1, slide_span < 0, row_len - 2 slide_span < 1,
 * a size above the limits.  Nothing is launched for any of these. */
int tba_pairwise_window_dists(tba_engine *e, int64_t n_rows, int64_t row_len, int64_t slide_span,
    const double *rows, double *out, double *out_kernel_ms);
int tba_pairwise_nanmean_dists(tba_engine *e, int64_t n_rows, int64_t row_len, const double *rows,
    double *out_condensed, double *out_kernel_ms);
int64_t tba_pdist_tile(void);
int64_t tba_pdist_lds_row_max(void);

/* ---- alternate-base model estimation (estimate_alt_model, tombo_stats.py:1747-2098) -----------
 * The base levels of a batch of reads gathered by k-mer (_parse_base_levels_worker, :1747-1776).
 * means / codes: read-centric levels and base codes (0..3 = ACGT, anything else: not a base) of
 * the reads, both CSR by read_off[n_reads + 1].  Window i of a read is bases i .. i + kmer_width - 1
 * and pairs with the read's level central_pos + i; a window with a non-ACGT code and a window
 * whose k-mer (index: first base most significant) has completed[kmer] set are skipped; a NaN
 * level is kept; a read shorter than kmer_width contributes nothing.
 * out_counts[4^K]: levels per k-mer.  out_lv_off[4^K + 1] (may be NULL in the count form): their
 * exclusive prefix.  out_levels NULL: the count form, nothing else is written.  Else the fill
 * form: out_levels[out_lv_off[k] .. out_lv_off[k + 1]) = the levels of k-mer k in read order and,
 * inside a read, position order -- bit-identical from run to run; levels_cap is the capacity of
 * out_levels (the windows of the batch, sum of max(len - K + 1, 0), always suffice).
 * TBA_E_ARG: NULL pointers, offsets that do not start at 0 or decrease, kmer_width outside
 * [1, 10], central_pos outside [0, kmer_width), 2^31 bases or more, levels_cap too small. */
int tba_kmer_levels(tba_engine *e, const double *means, const uint8_t *codes,
    const int64_t *read_off, int64_t n_reads, int64_t kmer_width, int64_t central_pos,
    const uint8_t *completed, int64_t *out_counts, int64_t *out_lv_off, double *out_levels,
    int64_t levels_cap);
/* K-mer level distributions (plot_kmer_dist, _plot_commands.py:451-559): which reads of a batch the plot
 * takes, their levels grouped by k-mer and read, and the means the plot orders the k-mers by.
 * means / codes / read_off and the windows as in tba_kmer_levels (a window with a code above 3 is skipped; a NaN
 * level propagates); the reads are taken in the order given.  kmer_width K in [1, 9].
 * A read is valid if kmer_thresh == 0, or if it shows all 4^K k-mers and (kmer_thresh == 1 or its rarest k-mer
 * occurs MORE than kmer_thresh times -- the reference's comparison).  A read is examined while fewer than
 * num_reads valid reads stand before it (the first read always is); an examined valid read is taken and gets
 * the label 1, 2, ...: out_read_label[n_reads] (0: not taken), *out_n_sel the reads taken, *out_n_examined the
 * reads examined.  A read shorter than K is valid under kmer_thresh == 0 and contributes nothing.
 * Entries of a k-mer (index: first base most significant), in read order and inside a read in position order:
 *   read_mean == 0  every level of the k-mer in the taken reads
 *   read_mean != 0  per taken read that shows the k-mer, np.mean of its levels of the k-mer (np.add.reduce in
 *                   numpy's order -- 8192-value blocks, pairwise from 8 values on -- divided by the count)
 * out_counts[4^K]: entries per k-mer; out_off[4^K + 1]: their exclusive prefix.
 * out_values NULL: the count form, nothing else is written (out_value_label and out_kmer_mean may be NULL).
 * Else the fill form: out_values / out_value_label [out_off[k] .. out_off[k + 1]) = the entries of k-mer k and
 * the labels of their reads; out_kmer_mean[4^K] = np.mean over the k-mer's entries as they stand in out_values
 * (one contiguous run), NaN where there is none.  values_cap: the capacity of out_values and out_value_label
 * (the windows of the batch, sum of max(len - K + 1, 0), always suffice); it is compared after the counting
 * kernels, before any value is written.  No floating-point atomics: the same call gives the same bytes.
 * out_kernel_ms (may be NULL): device time of the call's kernels.
 * n_reads == 0 is valid: every count is 0, nothing is launched.
 * TBA_E_ARG: NULL pointers other than those named optional, offsets that do not start at 0 or decrease, kmer_width
 * outside [1, 9], central_pos outside [0, kmer_width), 2^31 bases or more, 4^K * n_reads above 2^27 (the dense
 * per-read table), values_cap too small.  Nothing is launched for any of these but the last. */
int tba_kmer_dist(tba_engine *e, const double *means, const uint8_t *codes, const int64_t *read_off,
    int64_t n_reads, int64_t kmer_width, int64_t central_pos, int64_t kmer_thresh, int64_t num_reads,
    int read_mean, int64_t *out_read_label, int64_t *out_n_sel, int64_t *out_n_examined, int64_t *out_counts,
    int64_t *out_off, double *out_values, int64_t *out_value_label, int64_t values_cap, double *out_kmer_mean,
    double *out_kernel_ms);
/* Gaussian kernel densities (est_kernel_density, :1914-1939).  levels: n_seg segments, CSR by
 * lv_off[n_seg + 1] (any order inside a segment; the input is not changed).
 * out_dens[s * n_x + g] = sum_i exp(-0.5 ((x[g] - l_i) / bandwidth)^2) / (n bandwidth sqrt(2 pi))
 * over the n levels of segment s: scipy.stats.gaussian_kde(l, bw_method=bandwidth /
 * l.std(ddof=1)).evaluate(x).  The sum runs over the sorted levels in a fixed order: the output
 * is bit-identical from run to run.  A segment of fewer than two levels (scipy raises) or with a
 * NaN level gives a row of NaN.
 * TBA_E_ARG: NULL pointers, offsets that do not start at 0 or decrease, a bandwidth that is not
 * positive and finite, more than 65535 * 256 grid points. */
int tba_kde_eval(tba_engine *e, const double *levels, const int64_t *lv_off, int64_t n_seg,
    const double *x, int64_t n_x, double bandwidth, double *out_dens);

/* ---- genome tracks (text_output browser_files, iter_cov_regs, get_largest_signal_differences) ---
 * The pileup of per-base values over the reads of one (chromosome, strand):
 * get_mean_slot_genome_centric (tombo_helper.py:1661-1676) and TomboReads._compute_coverage
 * (:1394-1404).  The reference adds the reads to a float64 array one after the other, so a
 * position's sum is the left-to-right sum of its values in read order; these entries keep that
 * order (no floating-point atomics, one thread per position) and are bit-identical to it.
 *
 * tba_tracks_begin opens a track set over the window [win_start, win_end) of the chromosome:
 * n_slots (1..3) float64 sum arrays at +0.0, one int64 coverage per slot and one int64 read
 * coverage, all in device memory until the next tba_tracks_begin.  An engine holds one set.
 * TBA_E_ARG: an empty window, one of 2^31 positions or more, n_slots outside [1, 3]. */
#define TBA_TRK_TILE 256
int tba_tracks_begin(tba_engine *e, int64_t win_start, int64_t win_end, int n_slots);
/* Adds n_reads reads to the open set.  Read q lies at genomic [read_start[q], read_end[q]): that
 * interval counts into the read coverage.  Its slot values, read-centric (5'->3' of the read),
 * are slots[s][read_off[q] .. read_off[q + 1]) for every slot s with bit 1 + s of read_flags[q]
 * set (a read without an Events table has none); bit 0: minus strand, value i lies at genomic
 * read_start + len - 1 - i instead of read_start + i.  Positions outside the window are ignored.
 * The window is cut into tiles of TBA_TRK_TILE positions, n_tiles = ceil(window / TBA_TRK_TILE);
 * tile_reads[tile_read_off[t] .. tile_read_off[t + 1]) lists, in input order, the reads that
 * overlap tile t (a listed read that does not overlap adds nothing; an overlapping read that is
 * not listed is missed).  The values of a position are added in list order, continuing the sums
 * of earlier calls: reads fed batch by batch in index order give the bits of one call.
 * NaN and +-inf pass through ordinary IEEE addition.
 * TBA_E_ARG: no open set, NULL pointers, offsets that do not start at 0 or decrease, n_tiles that
 * is not the window's, a listed read outside [0, n_reads), end < start, a flag for a slot the
 * set does not have. */
int tba_tracks_add(tba_engine *e, int64_t n_reads, const int64_t *read_start, const int64_t *read_end,
    const uint8_t *read_flags, const int64_t *read_off, const double *const *slots, int64_t n_tiles,
    const int64_t *tile_read_off, const int32_t *tile_reads);
/* The open set's results, each may be NULL: means_out[s * window + p] = sum / (double)coverage
 * (NaN where nothing was added: 0 / 0), sums_out and slot_cov_out in the same layout,
 * read_cov_out[window].  The set stays open: further reads may be added. */
int tba_tracks_finish(tba_engine *e, double *means_out, double *sums_out, int64_t *slot_cov_out,
    int64_t *read_cov_out);
/* kernel time (hipEvents) of the open set's tba_tracks_add / tba_tracks_finish calls so far */
int tba_tracks_kernel_ms(tba_engine *e, double *ms);
/* Ordered compaction of n 64-bit values (flag, scan, scatter on the device; order kept).
 * mode 0 (filter_cs_nans, _text_output_commands.py:230-233): values float64; out_pos / out_val =
 *   the indices and values that are not NaN.
 * mode 1 (iter_coverage_regions, tombo_helper.py:1430-1453): values int64; out_pos = 0, every i
 *   with values[i] != values[i - 1], and n behind them (*out_count + 1 entries); out_val = the
 *   value at each of those starts.
 * out_pos holds n + 1 entries, out_val n; *out_count: the kept values. */
int tba_tracks_compact(tba_engine *e, int mode, const void *values, int64_t n, int64_t *out_pos,
    void *out_val, int64_t *out_count);
/* out = np.nan_to_num(a - b): NaN -> 0, +-inf -> +-the largest double (get_signal_differences) */
int tba_tracks_diff(tba_engine *e, const double *a, const double *b, int64_t n, double *out);
/* The min(n_top, n) largest values of np.nan_to_num(np.abs(a - b)) and their positions
 * (get_largest_signal_differences, tombo_helper.py:1714-1728), selected on the device: a radix
 * select over the whole grid on the values' bit patterns, then compaction; only the selected
 * pairs are copied back.  Output: first the values above the n_top-th largest in position
 * order, then those that equal it.  Of equal values at the cut the HIGHEST positions are taken
 * (the reference's unstable argsort leaves that choice open). */
int tba_tracks_topn(tba_engine *e, const double *a, const double *b, int64_t n, int64_t n_top,
    int64_t *out_pos, double *out_val, int64_t *out_count);

/* ---- estimate_kmer_model / estimate_motif_alt_model (csrc/k_kmer_est.h) ----
 * get_region_kmer_levels (tombo_stats.py:1242-1359) for a batch of regions, the arithmetic only:
 * the host has done the region sequences, the coverage intervals, the motif search and the keys.
 *   reads      read_start, read_minus (1: minus strand, its levels are reversed to genome order),
 *              means CSR by read_off[n_reads + 1]; a read is uploaded once per call
 *   regions    reg_reads CSR by reg_read_off[n_regions + 1]: indices of the region's reads in the
 *              region's read order (the order the levels of a position are taken in)
 *   positions  pos_reg / pos_g [n_pos]: region and genomic position of every wanted position
 *   entries    ent_pos / ent_key [n_ent]: a position index and a key in [0, n_keys), n_keys <= 2^24
 * Per position the levels of the region's reads that cover it, NaN levels included, give the pair
 * (np.median, np.std), or with est_mean the pair of c_mean_std (left-to-right sums).  The entries
 * are then stably partitioned by key: out_counts[n_keys], out_off[n_keys + 1], and out_levels /
 * out_sds [n_ent] hold per key its entries' pairs in entry order.  No floating-point atomics:
 * the same call gives the same bits. */
int tba_region_key_levels(tba_engine *e, int est_mean, int64_t n_reads, const int64_t *read_start,
    const uint8_t *read_minus, const int64_t *read_off, const double *means, int64_t n_regions,
    const int64_t *reg_read_off, const int64_t *reg_reads, int64_t n_pos, const int64_t *pos_reg,
    const int64_t *pos_g, int64_t n_ent, const int64_t *ent_pos, const int64_t *ent_key, int64_t n_keys,
    int64_t *out_counts, int64_t *out_off, double *out_levels, double *out_sds);
/* np.median of every segment of values (CSR by off[n_seg + 1]): the mean of the two middle values
 * for an even count, NaN for an empty segment or one that holds a NaN.  values is not modified. */
int tba_segment_medians(tba_engine *e, const double *values, const int64_t *off, int64_t n_seg,
    double *out_medians);
/* center_model_to_median_norm (tombo_stats.py:1599-1705) for a batch of reads, in two calls (csrc/k_center.h; ABI
 * minor 2).  The reference draws the Theil-Sen subsample of a read of more than 1000 points with np.random.choice, in
 * read order, and only for a read that got as far as the fit: the caller draws between the two calls, for the reads
 * whose status after the first is TBA_OK.
 * tba_center_prepare: the batch as tba_batch_upload_async takes it (raw int16 / float32 / float64, same bits for the
 * same values; seq = the `base` column as codes), plus the `start` column of every read's Events table (starts, CSR
 * by start_off[n_reads + 1]) and read_start_rel_to_raw[n_reads].  It normalises every read's whole raw signal and
 * keeps it on the device -- p->use_t_test_seg == 0 (DNA): ts.normalize_raw_signal alone; otherwise (RNA) what
 * get_event_scale_values does: the samples are reversed (o->reverse_raw), stalls detected on them
 * (o->detect_stalls), t-test change points with num_events[read] of compute_num_events, stall change points
 * removed, scale values from the events (o->use_rna_event_scale, limits +-o->outlier_thresh), normalisation
 * with them.  num_events is required for RNA and ignored for DNA.  Then the expected levels of seq under the
 * model of tba_set_model, and the read's own boundaries: with up = central_pos, dn = kmer_width - up - 1 >= 1 a read
 * of n rows gets read_start = read_start_rel_to_raw + start[up] and the n - kmer_width + 2 boundaries
 * start[up .. n - dn] - start[up].  status[n_reads]: TBA_SEQ_SEG_MISMATCH where rows and bases differ in number or
 * are fewer than kmer_width + 1, TBA_ZERO_LEN where the boundaries do not strictly increase, TBA_NEG_START /
 * TBA_PAST_END where they leave the raw signal, TBA_INVALID_SEQ, TBA_FEWER_CPTS and the other codes of the steps
 * above; TBA_INTERNAL for a signal of fewer than 4 * running_stat_width + 2 samples.  kernel_ms (may be NULL): device
 * time of the call's kernels.
 * tba_center_fit, on the batch tba_center_prepare left: samp_ind[n_reads][1000] as in tba_batch_upload (NULL when no
 * read of the batch has more than 1000 points), k_theil_sen over the boundaries, then the pick: the successes of
 * the calls before (prior[n_prior][2], their factors in order) followed by this batch's in read order, the first
 * max_reads of them counted.  status[n_reads] (TBA_RESCALE_FAIL for a slope of 0), factors[n_reads][2] =
 * (shift_corr_factor, scale_corr_factor) = (-inter / slope, 1 / slope), NaN for a failed read; medians[2] =
 * np.median of the counted factors (untouched when none counted); *n_used = how many counted. */
int tba_center_prepare(tba_engine *e, const tba_params *p, const tba_opts *o, int64_t n_reads,
    const void *raw, int raw_dtype, const int64_t *raw_off, const uint8_t *seq, const int64_t *seq_off,
    const int64_t *starts, const int64_t *start_off, const int64_t *read_start_rel_to_raw,
    const int64_t *num_events, int32_t *status, double *kernel_ms);
int tba_center_fit(tba_engine *e, const int64_t *samp_ind, const double *prior, int64_t n_prior,
    int64_t max_reads, int32_t *status, double *factors, double *medians, int64_t *n_used, double *kernel_ms);

/* ---- region plot data (csrc/k_plot.h): the numbers behind the frames of tombo/_plot_commands.py:784-984 ----
 * Level piles of a batch of plot regions: get_r_boxplot_data, get_r_quant_data and get_r_event_data over
 * intervalData.get_base_levels (tombo_helper.py:1976-2032).  Reads as in tba_region_key_levels (read_start,
 * read_minus, means CSR by read_off[n_reads + 1]); region r is [reg_start[r], reg_end[r]) with the reads
 * reg_reads[reg_read_off[r] .. reg_read_off[r + 1]) in that order.  Positions run region-major, then in
 * genomic order: n_pos = sum(reg_end - reg_start).  The pile of a position holds, in the region's read
 * order, the levels of the reads that cover it; a NaN level is DROPPED (the frames remove NaN; the k-mer
 * estimation above keeps it).
 *   out_off[n_pos + 1]      the piles' offsets
 *   out_levels              NULL, or the piles themselves (levels_cap values of room; the reads' overlaps
 *                           with their regions always suffice)
 *   out_lin[n_pos * n_ql]   np.percentile(pile, 100 q_linear[j]), the default linear form
 *   out_near[n_pos * n_qn]  np.percentile(pile, 100 q_nearest[j], interpolation='nearest')
 * q_linear / q_nearest are the fractions numpy divides out (np.true_divide(q, 100)), in [0, 1].  On the
 * pile sorted ascending, v of n values: nearest is v[rint((n - 1) q)] (round half to even); linear is
 * numpy's _lerp of a = v[floor(vi)], b = v[min(floor(vi) + 1, n - 1)], t = vi - floor(vi), vi = (n - 1) q:
 * a + (b - a) t, and b - (b - a) (1 - t) where t >= 0.5, no operation fused.  An empty pile: NaN.
 * No floating-point atomics: the same call gives the same bits.  out_kernel_ms (may be NULL): kernel time.
 * TBA_E_ARG: NULL pointers, offsets that do not start at 0 or decrease, a region that names a read outside
 * the batch, reg_end <= reg_start, a coordinate outside (-2^62, 2^62), a fraction outside [0, 1], a region
 * with 2^31 reads or more (a pile of 2^31 levels), 2^31 positions or more, levels_cap too small.  Zero
 * regions write out_off[0] = 0 and launch nothing. */
int tba_region_level_piles(tba_engine *e, int64_t n_reads, const int64_t *read_start,
    const uint8_t *read_minus, const int64_t *read_off, const double *means, int64_t n_regions,
    const int64_t *reg_read_off, const int64_t *reg_reads, const int64_t *reg_start, const int64_t *reg_end,
    int64_t n_ql, const double *q_linear, int64_t n_qn, const double *q_nearest, int64_t *out_off,
    double *out_levels, int64_t levels_cap, double *out_lin, double *out_near, double *out_kernel_ms);
/* The two percentile forms alone, of every segment of values (CSR by off[n_seg + 1]; values is not
 * modified): out_lin[n_seg * n_ql], out_near[n_seg * n_qn].  An empty segment and one that holds a NaN give
 * NaN, as np.percentile does.  Zero segments or zero fractions launch nothing. */
int tba_segment_percentiles(tba_engine *e, const double *values, const int64_t *off, int64_t n_seg,
    int64_t n_ql, const double *q_linear, int64_t n_qn, const double *q_nearest, double *out_lin, double *out_near,
    double *out_kernel_ms);
/* The raw-signal frame: th.get_raw_signal (tombo_helper.py:2090-2137), normalize_raw_signal with the read's
 * stored scale values and the per-base position spread of get_r_raw_signal_data (_plot_commands.py:946-966)
 * for n_pair (read, region) pairs.
 *   reads  raw: the stored DAC values, int16_t (raw_bytes 2) or int32_t (raw_bytes 4), CSR by raw_off;
 *          segs: the Events start column and the end, CSR by segs_off (bases + 1 entries a read);
 *          read_start (genomic), rsrtr (read_start_rel_to_raw), minus, rna, shift, scale, lower_lim,
 *          upper_lim (a NaN limit: no clip)
 *   pairs  pair_read, and the region [pair_start, pair_end), which the read must overlap
 * Per pair: the overlap slice of the segments (reversed for '-' as segs[-1] - segs[::-1]), its window of
 * the signal (the whole signal reversed first for RNA, the window reversed for '-'), (raw - shift) / scale,
 * the clip of c_apply_outlier_thresh; genome_centric == 0 applies the minus-strand flip of :946-952.  Then
 * for sample i of n of overlap base b: Position = (pair_start + b + start_offset) + i * (1.0 / n).
 *   out_sig_off[n_pair + 1]; out_position, out_signal, out_base_i [samples_cap]: pair-major, sample order
 * TBA_E_ARG: NULL pointers, bad offsets, raw_bytes not 2 or 4, a read with fewer than two segment entries,
 * with decreasing or negative segments, a negative rsrtr or segments that end past its signal, a pair that
 * names no read of the batch, pair_end <= pair_start, no overlap, samples_cap too small.  Zero pairs write
 * out_sig_off[0] = 0 and launch nothing. */
int tba_region_raw_signal(tba_engine *e, int64_t n_reads, const void *raw, int raw_bytes,
    const int64_t *raw_off, const int64_t *segs, const int64_t *segs_off, const int64_t *read_start,
    const int64_t *rsrtr, const uint8_t *minus, const uint8_t *rna, const double *shift, const double *scale,
    const double *lower_lim, const double *upper_lim, int64_t n_pair, const int64_t *pair_read,
    const int64_t *pair_start, const int64_t *pair_end, int genome_centric, int64_t *out_sig_off,
    double *out_position, double *out_signal, int64_t *out_base_i, int64_t samples_cap, double *out_kernel_ms);

/* ---- read filters: dwell percentiles (csrc/k_filter.h) -------------------------------------------
 * The "stuck read" rule of tombo filter stuck (_filter_reads.py:58-96) and of the worker loop's
 * --obs-per-base-filter (resquiggle.py:1449-1456) for n_reads reads: any(np.percentile(base_lens, pctl) >
 * thresh for pctl, thresh in obs_filter).  segs: per read its base starts and its end (int64, CSR by
 * seg_off[n_reads + 1]); the lengths are the successive differences, so a read of n bases has n + 1 entries
 * and a read of 0 or 1 entries has no lengths.  Per pair j: q[j] the fraction numpy divides out
 * (np.true_divide(pctl, 100)) and thresh[j].
 *   out_vals[n_reads * n_pairs]  (may be NULL) np.percentile(lens, pctl) in the default linear form, bit for
 *                                bit: the _lerp of tba_region_level_piles on the two order statistics, which
 *                                are found by counting (an LDS histogram of the lengths, an exact radix select
 *                                for a rank among the lengths of 4095 and more); nothing is sorted
 *   out_flags[n_reads]           1 where any out_vals[i][j] > thresh[j] (strict)
 * A read without lengths: NaN and flag 1 (np.percentile raises on an empty array and the reference's
 * read_is_stuck answers True to any exception).  No floating-point atomics: the same call gives the same
 * bits.  out_kernel_ms (may be NULL): kernel time.
 * TBA_E_ARG: NULL pointers, offsets that do not start at 0 or decrease, n_pairs < 1, a fraction outside
 * [0, 1], a NaN threshold, a decreasing boundary inside a read, a length of 2^31 or more, a read of 2^31
 * entries or more.  Zero reads launch nothing. */
int tba_dwell_pctl_flags(tba_engine *e, int64_t n_reads, const int64_t *segs, const int64_t *seg_off,
    int64_t n_pairs, const double *q, const double *thresh, double *out_vals, uint8_t *out_flags,
    double *out_kernel_ms);
/* The same kernel on the boundaries of the resident batch after a run (what tba_batch_download returns as
 * segs; nothing is uploaded except the pairs): out_vals[n * n_pairs] (may be NULL), out_flags[n] for the n
 * reads of the batch.  A read whose status is not 0 gets NaN and flag 0: such a read is never indexed.
 * TBA_E_STATE without a run batch. */
int tba_batch_dwell_pctl_flags(tba_engine *e, int64_t n_pairs, const double *q, const double *thresh,
    double *out_vals, uint8_t *out_flags, double *out_kernel_ms);

/* The de novo statistic of every read of the finished resident batch, nothing uploaded: per-base
 * means (c_new_means over the final signal and boundaries, as tba_batch_base_stats) against the
 * batch's own expected levels, which are the canonical model's levels of the read sequence --
 * compute_de_novo_read_stats (tombo_stats.py:3771-3873) for a read tested over its whole length.
 * pvals: CSR by the reads' base counts (layout of tba_batch_base_stats), n_values >= B_tot;
 * per read only [central_pos, B - (K - central_pos - 1)) is tested (k-mers inside the read),
 * the rest and failed reads are NaN. */
int tba_batch_de_novo_stats(tba_engine *e, int64_t fm_offset, double smallest_pval,
                            double *pvals, int64_t n_values);

/* ---- the worker's per-read preparation (row P10) ---------------------------------------------
 * ts.identify_stalls(all_raw_signal, stall_params) (tombo_stats.py:269-368), running-window-mean
 * method, for one read in host memory (raw_dtype: TBA_RAW_*): ints[2 i], ints[2 i + 1] = the
 * i-th (widened, merged) stall interval, *n_ints of them (cap = capacity of ints in intervals;
 * TBA_E_ARG with *n_ints set when it is too small).  Inside a batch the same kernels run under
 * tba_opts.detect_stalls. */
int tba_identify_stalls(tba_engine *e, const void *raw, int raw_dtype, int64_t n,
    int64_t window_size, int64_t n_windows, int64_t mini_window_size, double threshold,
    int64_t min_consecutive_obs, int64_t edge_buffer, int64_t *ints, int64_t cap, int64_t *n_ints);

/* ---- the documented per-read functions of tombo_stats, for a batch of reads (csrc/k_norm_api.h) ----
 * ts.normalize_raw_signal (tombo_stats.py:482-573) of n_reads reads in host memory.  raw: the reads'
 * samples one after the other (raw_dtype: TBA_RAW_I16 or TBA_RAW_F64), read i at raw_off[i] ..
 * raw_off[i + 1]; its window is start[i] .. start[i] + len[i] of them (len >= 1).  norm_type:
 * TBA_NORMTYPE_*.  sv_flags (or NULL) bit 0: read i takes shift and scale from sv_in[4 i], sv_in[4 i + 1]
 * whatever the norm type, bit 1: and the limits sv_in[4 i + 2], sv_in[4 i + 3] (an outlier threshold
 * overrides them).  channel (or NULL; TBA_NORMTYPE_PA_RAW needs it): offset, range, digitisation per read.
 * has_outlier_thresh: the limits are median -/+ MAD * outlier_thresh of the normalised window.
 * const_scale: the scale of TBA_NORMTYPE_MEDIAN_CONST_SCALE.  Out: status[i] 0, or 1 for a scale of exactly
 * 0 (the reference's FloatingPointError; nothing else is written for that read); sv_out[4 i ..] shift,
 * scale, lower, upper, the limits valid where has_lims[i]; norm: the normalised windows one after the
 * other, read i at sum(len[0 .. i)); *out_kernel_ms (or NULL): the time of the two kernels. */
enum { TBA_NORMTYPE_NONE = 0, TBA_NORMTYPE_PA_RAW = 1, TBA_NORMTYPE_MEDIAN = 2,
       TBA_NORMTYPE_MEDIAN_CONST_SCALE = 3, TBA_NORMTYPE_ROBUST_MEDIAN = 4 };
int tba_normalize_raw_batch(tba_engine *e, int64_t n_reads, const void *raw, int raw_dtype,
    const int64_t *raw_off, const int64_t *start, const int64_t *len, int norm_type,
    const double *sv_in, const int32_t *sv_flags, const double *channel, int has_outlier_thresh,
    double outlier_thresh, double const_scale, double *sv_out, int32_t *has_lims, double *norm,
    int32_t *status, double *out_kernel_ms);
/* The five sums of the method-of-moments fit (ts.calc_kmer_fitted_shift_scale, tombo_stats.py:427-437), each
 * in the order of numpy's .sum(): sums[5 i ..] = iv.sum(), (m * iv).sum(), (m * iv * m).sum(), (e * iv).sum(),
 * (e * iv * m).sum() over the points off[i] .. off[i + 1] of read i (e event means, m model means, iv model
 * inverse variances). */
int tba_mom_sums(tba_engine *e, int64_t n_reads, const int64_t *off, const double *event_means,
    const double *model_means, const double *model_inv_vars, double *sums);
/* ts.get_read_seg_score (tombo_stats.py:2327-2338) of n_reads reads: scores[i] = np.mean(np.abs((means -
 * ref_means) / ref_sds)) over the bases off[i] .. off[i + 1]. */
int tba_seg_scores(tba_engine *e, int64_t n_reads, const int64_t *off, const double *means,
    const double *ref_means, const double *ref_sds, double *scores);

/* ---- RNA adapter trimming and the global scale estimate (csrc/k_trim_rna.h) ----
 * ts.trim_rna (tombo_stats.py:235-267) of n_reads reads in host memory.  raw: the reads' samples one after the
 * other (raw_dtype: TBA_RAW_I16 or TBA_RAW_F64), read i at raw_off[i] .. raw_off[i + 1]; only its first max_raw_obs
 * samples are uploaded and touched.  min_obs_per_base, running_stat_width, mean_obs_per_event: th.resquiggleParams;
 * moving_window_size, min_running_values, thresh_scale, max_raw_obs: th.trimRnaParams.  The change points come from
 * the batch kernels of event detection (th.valid_cpts_w_cap: the plain detector, sorted; equal scores as
 * INTEGRATION.md section 6 states), in the form tba_engine_set_dispatch selects: above small_batch_reads reads, with
 * 2 * running_stat_width <= 32 and min_obs_per_base 3, k_detect + k_pick, else the kernels that keep the scores.
 * Out: adapter_end[i] (0 where status[i] is not TBA_OK); status[i]: TBA_OK, TBA_FEWER_CPTS (the detector's
 * TomboError), TBA_TRIM_TOO_FEW_EVENTS (fewer than moving_window_size + min_running_values - 2 event SDs: numpy's
 * ValueError 'negative dimensions are not allowed'), TBA_INTERNAL (a prefix without a score or an event: the
 * reference indexes an empty array); ed_form (or NULL): TBA_ED_FORM_* of the kernels that produced each read's
 * change points; *out_kernel_ms (or NULL): the time of the kernels.  No read count or max_raw_obs is refused for
 * its size: reads with more event SDs than the LDS form holds take the global-memory form of the window kernel,
 * batches are cut inside the call by a budget of uploaded samples (tba_engine_set_trim_budget), and zero reads
 * launch nothing.  The same call gives the same bytes (no floating-point atomics).
 * TBA_E_ARG: NULL pointers, offsets that do not start at 0 or decrease, a raw dtype other than the two, a parameter
 * below 1, a thresh_scale that is NaN, a prefix of 2^31 samples or more, a moving_window_size above 8192 (a row of
 * the window stage is one block of numpy's pairwise sum: wider rows are refused, not answered differently). */
int tba_trim_rna_batch(tba_engine *e, int64_t n_reads, const void *raw, int raw_dtype, const int64_t *raw_off,
    int64_t min_obs_per_base, int64_t running_stat_width, int64_t mean_obs_per_event, int64_t moving_window_size,
    int64_t min_running_values, double thresh_scale, int64_t max_raw_obs, int64_t *adapter_end, int32_t *status,
    int32_t *ed_form, double *out_kernel_ms);
/* the most prefix samples one device pass of tba_trim_rna_batch holds (a read above it goes alone); samples < 1:
 * back to the default, TBA_TRIM_BUDGET_DEFAULT */
#define TBA_TRIM_BUDGET_DEFAULT (1ll << 26)
int tba_engine_set_trim_budget(tba_engine *e, int64_t samples);
/* np.median(raw) and np.median(np.abs(raw - median)) of n_reads reads (one sample or more each), by exact
 * selection on int16 or float64 samples: what ts.estimate_global_scale (tombo_stats.py:452-480) takes of a read.
 * No normalised signal is made.  *out_kernel_ms (or NULL): the time of the kernel. */
int tba_raw_med_mad(tba_engine *e, int64_t n_reads, const void *raw, int raw_dtype, const int64_t *raw_off,
    double *med, double *mad, double *out_kernel_ms);

/* Host-side, no GPU involved: pack n_reads per-read sample arrays (raw_ptrs[i], raw_off[i+1] -
 * raw_off[i] samples of type raw_dtype; reverse != 0: copied back to front) and sequences
 * (seq_ptrs[i]: ASCII A/C/G/T, seq_off[i+1] - seq_off[i] letters, stored as codes 0..3, anything
 * else as 255 -> TBA_INVALID_SEQ) into the CSR buffers tba_batch_upload_async takes, with
 * n_threads threads.  This is the reader of the reference's worker pool (resquiggle.py:1385-1486)
 * for callers that hold one array per read. */
int tba_pack_reads(int64_t n_reads, const void *const *raw_ptrs, int raw_dtype, int reverse,
    const int64_t *raw_off, void *raw_out, const char *const *seq_ptrs, const int64_t *seq_off,
    uint8_t *seq_out, int n_threads);

/* ... and back: count[i] elements of elem_bytes bytes from src + src_off[i] (elements) into
 * dst_ptrs[i], n_threads threads (per-read result arrays out of one flat download) */
int tba_unpack_reads(int64_t n_reads, const void *src, int64_t elem_bytes, const int64_t *src_off,
    const int64_t *count, void *const *dst_ptrs, int n_threads);

/* ---- synthetic reads made on the device (bench / test support) ---------------------------------
 * No counterpart in the reference: its benchmark input is a directory of FAST5 files.  The
 * multi-GPU job of BASELINE.json (a million distinct 10 kb reads through a host work queue) cannot
 * be synthesised on the host cores inside a benchmark's set-up, so every batch of that job is
 * drawn on the device from a counter-based generator keyed by (seed, first_read + read, element):
 * the reads of tombo_amd/synth.py (uniform ACGT, level = the model's k-mer mean, dwell =
 * max(min_dwell, Geometric(1 / mean_dwell)), level + noise per sample, n_lead / n_trail samples
 * of open-pore-like signal around them), reproducible on any rank and bit for bit by the numpy
 * restatement tombo_amd.synth.device_reads_reference (csrc/k_synth.h states the draws). */
typedef struct tba_synth tba_synth;
typedef struct {
    int64_t mean_dwell, min_dwell, n_lead, n_trail;
    double scale, offset, noise_sd;   /* pA = (level + noise * noise_sd) * scale + offset */
    double dac_per_pa, dac_offset;    /* TBA_RAW_I16: rint(pA * dac_per_pa + dac_offset) */
    int32_t reverse, pad;             /* reverse: samples in acquisition order of a 3'->5' (RNA) run */
} tba_synth_params;
int tba_synth_create(int device, const double *kmer_means, int64_t kmer_width, tba_synth **out);
void tba_synth_destroy(tba_synth *g);
/* n_reads reads of n_bases[i] bases (sequence: n_bases[i] + kmer_width - 1 codes), raw_dtype
 * TBA_RAW_I16 or TBA_RAW_F64.  Returns when the batch is in device memory: raw_off / seq_off
 * (n_reads + 1, host) get its CSR offsets, *d_raw / *d_seq the device arrays (owned by the
 * generator, valid until its next call) -- tba_batch_upload_async takes them in place of host
 * arrays. */
int tba_synth_generate(tba_synth *g, const tba_synth_params *p, uint64_t seed, int64_t first_read,
    int64_t n_reads, const int64_t *n_bases, int raw_dtype, int64_t *raw_off, int64_t *seq_off,
    const void **d_raw, const uint8_t **d_seq);
/* the last generated batch to host memory (either may be NULL) */
int tba_synth_download(tba_synth *g, void *raw, uint8_t *seq);
/* host only: the generator's dwell thresholds (n <= 256) and noise constant under p */
int tba_synth_dwell_thresholds(const tba_synth_params *p, uint32_t *thr, int64_t n, double *noise_norm);

/* out[0..2] = sizeof(tba_params), sizeof(tba_opts), sizeof(tba_read_result) of this build, out[3]
 * (n >= 4) = TBA_ABI_VERSION: lets a binding without a C compiler (ctypes) check its struct mirrors
 * and refuse a stale build of the library */
#define TBA_ABI_VERSION 13
/* additions that leave every struct, every entry and every selector of TBA_ABI_VERSION as it was (not part of
 * tba_abi_sizes: a binding asks for what it needs by name).  1: tba_one_sd_words, TBA_GET_DP_ONE_SD;
 * 2: tba_center_prepare, tba_center_fit; 3: tba_site_fractions_reads; 4: tba_trim_rna_batch,
 * tba_engine_set_trim_budget, tba_raw_med_mad, TBA_TRIM_TOO_FEW_EVENTS */
#define TBA_ABI_MINOR 4
int tba_abi_sizes(int64_t *out, int64_t n);

/* self-test: out[t] = index t of the subsample tba_opts.device_subsample draws for read
 * `read_index` of a batch under `seed`, for a read of n bases (t < count <= n) */
int tba_selftest_subsample(tba_engine *e, int64_t n, uint64_t seed, int64_t read_index,
                           int64_t count, int64_t *out);
/* self-test: out[i] = the row-constant division used inside the DP kernel (reciprocal + two
 * residual corrections) for a[i] / b[i]; must equal the IEEE quotient bit for bit */
int tba_selftest_division(tba_engine *e, const double *a, const double *b, int64_t n,
                          double *out);
/* self-test: out[i] = the approximate quotient a[i] * r, r = v_rcp_f64(b[i]) + one Newton step,
 * that the Theil-Sen kernel classifies slope pairs with (calc_kmer_fitted_shift_scale,
 * tombo_stats.py:401-425); its relative error must stay far inside the 1e-5 guard band */
int tba_selftest_approx_quotient(tba_engine *e, const double *a, const double *b, int64_t n,
                                 double *out);
/* self-test of the two-operation division (tba_engine_last_dp_const_division), the reciprocal pair of b[i] made
 * as the forward pass makes it; out has 3 n values: out[i] the quotient of a[i] by b[i], out[n + i] the cell's
 * z_shift - min(|quotient|, zcap) from it, out[2 n + i] the same from the general division */
int tba_selftest_const_division(tba_engine *e, const double *a, const double *b, int64_t n,
                                double z_shift, double zcap, double *out);

#ifdef __cplusplus
}
#endif
#endif

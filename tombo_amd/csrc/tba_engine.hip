// tba_engine.hip -- batch engine + C ABI (include/tombo_amd.h) of the gfx950 resquiggle path.
// One engine == one GPU == one HIP stream; a batch is a fixed sequence of kernels over ragged
// SoA buffers that stay resident in HBM between upload and download.
#include <atomic>
#include "tba_common.h"
#include "div_const_proof.h"
#include "k_scan.h"
#include "k_select.h"
#include "k_segment.h"
#include "k_detect.h"
#include "k_prep_raw.h"
#include "k_dp.h"
#include "k_tb_par.h"
#include "k_dp_multi.h"
#include "k_long.h"
#include "k_dp_wg.h"
#include "k_tail.h"
#include "k_cabi.h"
#include "k_synth.h"
#include "k_group.h"
#include "k_site.h"
#include "k_kde.h"
#include "k_kmer_dist.h"
#include "k_tracks.h"
#include "k_kmer_est.h"
#include "k_roc.h"
#include "k_pdist.h"
#include "k_plot.h"
#include "k_filter.h"
#include "k_norm_api.h"
#include "k_center.h"
#include "k_trim_rna.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <unordered_set>
#include <vector>

static thread_local std::string g_last_error;
static int set_err(int code, const std::string &msg) { g_last_error = msg; return code; }

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return set_err(TBA_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

// A grow-only buffer: device memory (DevBuf), or page-locked host memory (PinBuf: engine-owned staging of the
// small per-batch records, so that the "async" upload never falls back to HIP's blocking pageable path).
template <bool PINNED>
struct GrowBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        release();
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = PINNED ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return set_err(TBA_E_NOMEM, std::string(PINNED ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e)); }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};
typedef GrowBuf<false> DevBuf; typedef GrowBuf<true> PinBuf;

// timing slots (TBA_GET_KERNEL_MS, tba_stage_name): one per pipeline step (STEPS, below), then these two
enum { N_STEP = 14, SLOT_STALLS = N_STEP, SLOT_TOTAL, N_STAGE };

#define WIDE_BLOCKS 64 // workgroups of k_dp_wide (each owns two scratch rows)
#define TB_LANES 16    // reads per wavefront of the latency-bound lane-per-read kernels
#ifndef TBA_SMALL_BATCH
#define TBA_SMALL_BATCH 1024 // up to this many reads the scan of event detection runs a workgroup per read
                             // (k_detect costs ~7 us per 128 samples whatever the batch: 10 kb reads, event detection
                             // 384 reads 5.1 -> 1.4 ms, 1 024 reads 5.1 -> 3.2, 2 048 reads 5.4 -> 6.2: profiles/r04_small_batch_scan.txt)
#endif

// k_peaks is compiled per exclusion radius (min_obs_per_base - 1): 2 and 5 are the defaults of
// the DNA / RNA parameter sets, anything else takes the generic kernel
static void launch_peaks(i64 min_obs_per_base, unsigned n_blocks, hipStream_t s, ReadState *rs, const DevParams *dp, const double *score,
                         unsigned char *state, double *dense, i64 *valid_cpts, int ttest, int only_flagged = 0, int form = TBA_ED_FORM_SCORES_PEAKS)
{
    const i64 r = min_obs_per_base - 1;
    (r == 2 ? k_peaks<2> : r == 5 ? k_peaks<5> : k_peaks<0>)<<<n_blocks, SEL_NT, 0, s>>>(rs, dp, score, state, dense, valid_cpts, ttest, only_flagged, form);
}

// Everything the device buffers of a batch depend on, from the per-read lengths alone: plan_batch's
// output, kept by the engine for the uploaded batch.
struct BatchSizes {
    i64 S_tot = 0, seq_tot = 0, B_tot = 0, E_tot = 0, max_raw = 0, max_B = 0, max_nev = 0;
    i64 moves_need = 0, start_moves_stride = 0, moves_arena = 0, skip_arena = 0, wide_w = 0, n_stall = 0;
    double algo_bytes = 0, cells = 0;
};

// Every device buffer of the engine, once: the members, release_all() and tba_engine_held_bytes() are made
// from this list (the sizes of a batch: for_each_batch_buffer).  Its order is the order of release.
#define TBA_ENGINE_DEVBUFS(X)                                                                                         \
    X(d_rs); X(d_dp);                 /* ReadState[n] / DevParams */                                                  \
    X(d_kmeans); X(d_ksds);           /* the model's level table (tba_set_model) */                                   \
    /* the batch as uploaded (d_raw, d_seq, d_sv_in, d_samp, d_stall: or as detected) and what the steps hand on */   \
    X(d_raw); X(d_norm); X(d_norm_out); X(d_csum); X(d_score); X(d_state); X(d_cpts); X(d_evm); X(d_seq); X(d_refm); X(d_refs); X(d_bst); \
    X(d_lo); X(d_hi); X(d_readtb); X(d_dpsegs); X(d_segs); X(d_win); X(d_absz); X(d_sv_in); X(d_samp); X(d_stall); X(d_lastrow);          \
    X(d_startvals); X(d_smoves); X(d_moves); X(d_dscr); X(d_wide);                                                    \
    X(d_stat);                        /* per-base means / stds of a finished batch (launch_base_stats) */             \
    X(d_res); X(d_segs32);            /* packed results of tba_batch_download_async */                                \
    X(d_skipq);                       /* window queues of k_skip_dp_wave */                                           \
    X(d_order); X(d_long);            /* read indices by decreasing length (k_dp_multi's grouping); the long reads (k_long.h) */ \
    X(d_stall_csum); X(d_stall_bits); /* the stall detector's own scratch (it runs beside event detection) */ \
    X(d_trk_sum); X(d_trk_cov); X(d_trk_rcov); /* the resident genome tracks (tba_tracks_begin .. tba_tracks_finish) */ \
    X(d_cstart); X(d_cout); X(d_csel); /* centring (tba_center_prepare / tba_center_fit): the `start` columns, the results, the pick's lists */

struct tba_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    // Side stream of a full pipeline run: what does not depend on event detection -- the worker's
    // stall detection over the raw samples (RNA) and the expected levels of the sequence -- runs
    // beside the normalisation / event detection kernels of the main stream and is joined before its
    // first consumer (k_remove_stalls; start discovery).  Both groups wait on memory most of their time
    // (SQ_WAIT_ANY 60-80 % of their wave cycles): together they fill what each leaves idle.
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_stalls = nullptr, ev_levels = nullptr, ev_st0 = nullptr, ev_st1 = nullptr, ev_skip0 = nullptr, ev_skip1 = nullptr;
    hipEvent_t ev[N_STAGE + 1] = {}; // ev[i], ev[i + 1]: around step i of the pipeline; ev[N_STEP]: its end, ev[SLOT_TOTAL]: its start
    float stage_ms[32] = {};
    bool have_model = false, have_batch = false, ran = false;
    bool finished = false; // the last stage (rescale + score) has run on the uploaded batch
    bool center_ready = false; // tba_center_prepare has left the uploaded batch for tba_center_fit
    DevParams hp;
    i64 n_reads = 0;
    BatchSizes z;                 // of the uploaded batch
    size_t n_segs() const { return (size_t)(z.B_tot + n_reads); } // segment boundaries of the batch: B + 1 per read
    bool any_stall = false, have_samp = false, have_sv = false;
    std::vector<i64> ne_override; // per-read num_events for the next upload (stepwise API)
    // The two-operation division of the forward pass (k_dp_cdiv, k_dp.h): model_cdiv -- every sd of the level table
    // is proven (div_const_proof.h, tba_set_model); refs_put -- the batch's d_refs came from the caller
    // (TBA_PUT_REF_SDS), not from the table; cdiv_auto -- tba_engine_set_dp_const_division
    bool model_cdiv = false, refs_put = false, cdiv_auto = true;
    // ... and its one-sd form (k_dp_c1): the model's table has ONE sd, proven; one_sd_w -- that sd, yh = RN(1 / sd),
    // yl = recip_low(sd, yh) (one_sd_words, tba_set_model): model state, handed to the kernels as arguments
    bool one_sd = false;
    double one_sd_w[3] = {0.0, 0.0, 0.0};
    int n_sharing = 1;            // engines fed concurrently on this device (tba_engine_set_sharing)
    int side_mode = -1;           // tba_engine_set_side_stream: -1 by the engines alive, 0 never, 1 always
    bool last_side = false;       // the last full run used the side stream
    // The forward-pass launches of the last run (TBA_GET_DP_FORM, tba_engine_last_dp_lowreg): a run from the first
    // stage clears them, a stage that runs records its own.
    struct DpLaunches {
        bool start = false, main = false, lowreg = false, wide = false;
        bool cdiv_main = false, cdiv_start = false; // k_dp_cdiv took the main pass / start discovery (dp_cdiv)
        // ... in its one-sd form, k_dp_c1 (dp_one_sd): the main pass, the first try, a retry that went through k_dp
        bool c1_main = false, c1_start = false, c1_retry = false;
        int retry_wcpl = 0;       // class of the retry's k_dp_wg; 0: k_dp<class of start_save_bw> in retry mode
    } last_dp;
    // latency / throughput forms of event detection and traceback (tba_engine_set_dispatch)
    i64 small_batch = TBA_SMALL_BATCH, tb_wave_below = TBP_WAVE_BELOW;
    int last_c_ed_form = 0;       // tba_c_last_ed_form
    i64 trim_budget = TBA_TRIM_BUDGET_DEFAULT; // tba_engine_set_trim_budget
    int raw_dtype = TBA_RAW_F64;
    // the open genome-track set (k_tracks.h): window [trk_start, trk_start + trk_W), trk_slots sum arrays (0: none open)
    i64 trk_start = 0, trk_W = 0;
    int trk_slots = 0;
    double trk_kernel_ms = 0;     // kernel time of the open set so far (tba_tracks_kernel_ms)
    PinBuf h_rs, h_dp;            // ReadState[n] / DevParams as uploaded (pinned)
#define DEVBUF_MEMBER(name_) DevBuf name_
    TBA_ENGINE_DEVBUFS(DEVBUF_MEMBER)
    template <class F> void for_each_devbuf(F f) { TBA_ENGINE_DEVBUFS(f) }
    PinBuf h_order, h_long;       // d_order / d_long as uploaded (pinned)
    i64 n_long = 0;
    void release_all()
    {
        for_each_devbuf([](DevBuf &b) { b.release(); });
        for (PinBuf *h : {&h_order, &h_long, &h_rs, &h_dp}) h->release();
    }
};

extern "C" const char *tba_last_error(void) { return g_last_error.c_str(); }

extern "C" int tba_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// engines alive per device in this process: the side stream (run_prelude) is only used while the
// process's streams fit the device's hardware queues (four by default) -- beyond that streams share
// a queue, and a side stream queued behind ANOTHER engine's half-second forward pass holds its own
// engine's main stream at the join (measured: eight resident long-tail batches 37.8 k -> 31.4 k reads/s)
#define TBA_MAX_DEVICES 64
static std::atomic<int> g_live_engines[TBA_MAX_DEVICES];

extern "C" int tba_engine_create(int device, tba_engine **out)
{
    if (!out) return set_err(TBA_E_ARG, "out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_err(TBA_E_HIP, "no HIP device visible: the resquiggle engine has no CPU fallback");
    if (device < 0 || device >= n) return set_err(TBA_E_ARG, "bad device ordinal");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return set_err(TBA_E_HIP, std::string("device is ") + prop.gcnArchName +
                                      ", this library carries gfx950 code only");
    tba_engine *e = new tba_engine();
    e->device = device;
    if (const char *v = getenv("TBA_SMALL_BATCH_READS")) e->small_batch = std::max<i64>(atoll(v), 0);
    if (const char *v = getenv("TBA_TB_WAVE_BELOW")) e->tb_wave_below = std::max<i64>(atoll(v), 0);
    HIP_TRY(hipStreamCreate(&e->stream));
    if (device < TBA_MAX_DEVICES) g_live_engines[device]++;
    for (hipEvent_t *x : {&e->ev_fork, &e->ev_stalls, &e->ev_levels, &e->ev_st0, &e->ev_st1, &e->ev_skip0, &e->ev_skip1}) HIP_TRY(hipEventCreate(x));
    for (int i = 0; i <= N_STAGE; i++) HIP_TRY(hipEventCreate(&e->ev[i]));
    *out = e;
    return 0;
}

extern "C" void tba_engine_destroy(tba_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    if (e->stream2) (void)hipStreamSynchronize(e->stream2);
    e->release_all();
    for (int i = 0; i <= N_STAGE; i++) if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
    for (hipEvent_t x : {e->ev_fork, e->ev_stalls, e->ev_levels, e->ev_st0, e->ev_st1, e->ev_skip0, e->ev_skip1}) if (x) (void)hipEventDestroy(x);
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->device < TBA_MAX_DEVICES) g_live_engines[e->device]--;
    delete e;
}

// Whether every value of a level table's sd column is a proven divisor of the two-operation division.  The
// prover runs once per DISTINCT value (Tombo's DNA and RNA models have one each: microseconds); a table with more
// than TBA_CDIV_MAX_DISTINCT of them is left unproven rather than paid for.
#define TBA_CDIV_MAX_DISTINCT 4096
static bool sds_all_proven(const double *sds, size_t n)
{
    std::unordered_set<u64> seen; // (bit patterns: -0.0, NaNs and the like stay apart and fail the prover one by one)
    u64 last = 0;
    for (size_t i = 0; i < n; i++) {
        u64 b;
        memcpy(&b, sds + i, 8);
        if (i > 0 && b == last) continue;
        last = b;
        if (seen.count(b)) continue;
        if (seen.size() >= TBA_CDIV_MAX_DISTINCT || !div_const_proof::proven(sds[i])) return false;
        seen.insert(b);
    }
    return n > 0;
}

extern "C" int tba_prove_const_division(const double *sd, int64_t n, int32_t *proven)
{
    if (n < 0 || (n > 0 && (!sd || !proven))) return set_err(TBA_E_ARG, "bad arguments");
    for (int64_t i = 0; i < n; i++) proven[i] = div_const_proof::proven(sd[i]);
    return 0;
}

// The words of a level table with ONE distinct sd (by bit pattern), a proven divisor: the sd, yh = RN(1 / sd) and
// yl = recip_low(sd, yh) -- the division and the function the rows of k_dp_cdiv make them with (k_dp.h,
// load_levels), so the same bits.  false: the table has several sds, or its one sd is not proven.
static bool one_sd_words(const double *sds, size_t n, double (&w)[3])
{
    if (n == 0 || !sds_all_proven(sds, n)) return false;
    for (size_t i = 1; i < n; i++) if (memcmp(sds + i, sds, 8) != 0) return false;
    w[0] = sds[0];
    w[1] = 1.0 / w[0];
    w[2] = recip_low(w[0], w[1]);
    return true;
}

extern "C" int tba_one_sd_words(const double *sd, int64_t n, int32_t *one_sd, double *words)
{
    if (n < 0 || (n > 0 && !sd) || !one_sd || !words) return set_err(TBA_E_ARG, "bad arguments");
    double w[3] = {0.0, 0.0, 0.0};
    *one_sd = one_sd_words(sd, (size_t)n, w) ? 1 : 0;
    memcpy(words, w, sizeof(w));
    return 0;
}

extern "C" int tba_set_model(tba_engine *e, const double *kmer_means, const double *kmer_sds,
                             int64_t kmer_width, int64_t central_pos)
{
    if (!e || !kmer_means || !kmer_sds || kmer_width < 1 || kmer_width > 12)
        return set_err(TBA_E_ARG, "bad model arguments");
    HIP_TRY(hipSetDevice(e->device));
    size_t n = (size_t)1 << (2 * kmer_width);
    if (e->d_kmeans.ensure(n * 8) || e->d_ksds.ensure(n * 8)) return TBA_E_NOMEM;
    HIP_TRY(hipMemcpyAsync(e->d_kmeans.p, kmer_means, n * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_ksds.p, kmer_sds, n * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->hp.kmer_width = kmer_width;
    e->hp.central_pos = central_pos;
    e->have_model = true;
    e->model_cdiv = sds_all_proven(kmer_sds, n);
    double w[3] = {0.0, 0.0, 0.0};
    e->one_sd = one_sd_words(kmer_sds, n, w);
    memcpy(e->one_sd_w, w, sizeof(w));
    // a batch uploaded under another model has stale per-read geometry (B depends on K)
    e->have_batch = e->ran = e->finished = false;
    return 0;
}

extern "C" int tba_device_mem(tba_engine *e, int64_t *free_bytes, int64_t *total_bytes)
{
    if (!e) return set_err(TBA_E_ARG, "engine is NULL");
    HIP_TRY(hipSetDevice(e->device));
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return 0;
}

extern "C" int tba_pinned_alloc(int64_t bytes, void **out)
{
    if (!out || bytes < 0) return set_err(TBA_E_ARG, "bad arguments");
    void *p = nullptr;
    hipError_t rc = hipHostMalloc(&p, (size_t)(bytes > 0 ? bytes : 1), hipHostMallocDefault);
    if (rc != hipSuccess) return set_err(TBA_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(rc));
    *out = p;
    return 0;
}
extern "C" int tba_pinned_free(void *p)
{
    if (p && hipHostFree(p) != hipSuccess) return set_err(TBA_E_HIP, "hipHostFree failed");
    return 0;
}

// launch a kernel template instantiated for the batch's raw sample type
#define RAW_DISPATCH(dt_, call_)                                                               \
    do {                                                                                       \
        if ((dt_) == TBA_RAW_I16) { typedef int16_t RT; call_; }                               \
        else if ((dt_) == TBA_RAW_F32) { typedef float RT; call_; }                            \
        else { typedef double RT; call_; }                                                     \
    } while (0)

// ---- batch sizing -----------------------------------------------------------------------------
// (BatchSizes: shared by tba_batch_upload_async and tba_batch_footprint)
static size_t raw_elem_bytes(int dt) { return dt == TBA_RAW_I16 ? 2 : dt == TBA_RAW_F32 ? 4 : 8; }

// per-read geometry; rs may be NULL (footprint only).  Returns 0 or TBA_E_ARG.
static int plan_batch(const tba_params *p, const tba_opts *o, i64 K, i64 n, const i64 *raw_off,
                      const i64 *n_raw_arr, const i64 *seq_off, const i64 *seq_len_arr,
                      const std::vector<i64> &ne_override, const int32_t *sv_flags,
                      const i64 *stall_off, ReadState *rs, BatchSizes &z)
{
    const int cpl_main = cpl_class(p->bandwidth);
    if (cpl_class(p->start_bw) == 0 || cpl_class(p->start_save_bw) == 0 || cpl_main == 0)
        return set_err(TBA_E_ARG, "bandwidth / start bandwidth above TBA_MAX_BAND");
    i64 ref_acc = 0, ev_acc = 0, raw_acc = 0, seq_acc = 0, stall_acc = 0;
    for (i64 i = 0; i < n; i++) {
        const i64 n_raw = raw_off ? raw_off[i + 1] - raw_off[i] : n_raw_arr[i];
        const i64 seq_len = seq_off ? seq_off[i + 1] - seq_off[i] : seq_len_arr[i];
        if (n_raw < 0 || seq_len < 0) return set_err(TBA_E_ARG, "negative read length");
        ReadState tmp;
        ReadState &r = rs ? rs[i] : tmp;
        memset(&r, 0, sizeof(r));
        r.raw_off = raw_acc; r.n_raw = n_raw; raw_acc += n_raw;
        r.seq_off = seq_acc; r.seq_len = seq_len; seq_acc += seq_len;
        const i64 B = seq_len - K + 1;
        r.ref_off = ref_acc;
        r.seg_off = ref_acc + i;
        r.B = B > 0 ? B : 0;
        ref_acc += r.B;
        r.ev_off = ev_acc;
        r.status = TBA_OK;
        r.sv_flags = sv_flags ? sv_flags[i] : 0;
        if (stall_off) { r.stall_off = stall_off[i]; r.n_stall = stall_off[i + 1] - stall_off[i]; }
        else if (o->detect_stalls) { // capacity of k_stall_runs: a run is longer than min_consecutive_obs
            r.stall_off = stall_acc;
            stall_acc += (n_raw > 0 ? n_raw : 0) / (o->stall_min_consecutive_obs + 1) + 2;
        }
        if (B <= 0 || n_raw <= 0) {
            r.status = n_raw <= 0 ? TBA_NO_RAW : TBA_INTERNAL;
            continue;
        }
        // ts.compute_num_events (tombo_stats.py:1558-1574) and the guard of resquiggle.py:1159
        i64 num_events = std::max(n_raw / p->mean_obs_per_event,
                                  (i64)((double)B * o->min_event_to_seq_ratio));
        const bool forced = (i64)ne_override.size() == n && ne_override[(size_t)i] > 0;
        if (forced) num_events = ne_override[(size_t)i]; // caller-chosen (segment_signal)
        r.num_events = num_events; // event space is reserved for every read with B > 0
        ev_acc += num_events;
        if (!forced && (double)num_events / (double)p->bandwidth > (double)B) { r.status = TBA_TOO_MUCH_SIGNAL; continue; }
        if (num_events <= 1 || n_raw < 4 * p->running_stat_width + 2) { r.status = TBA_INTERNAL; continue; }
        z.max_raw = std::max(z.max_raw, n_raw);
        z.max_B = std::max(z.max_B, B);
        r.is_long = n_raw > TBA_LONG_RAW || B > TBA_LONG_BASES;
        const i64 n_ev = num_events - 1;
        const bool short_read = n_ev < p->start_bw + p->start_n_bases || B < p->start_n_bases;
        // packed move rows: the adaptive band, or the whole-read static band of a short read
        // (n_ev - mask_len cells, any width: k_dp_wide beyond the widest class)
        i64 row_bytes = mv_row_bytes(p->bandwidth);
        if (short_read) row_bytes = std::max(row_bytes, mv_row_bytes(n_ev));
        z.moves_need += (B + 1) * (row_bytes + MV_STRIP_BYTES); // (+ the centre strip of the adaptive rows, k_dp.h)
        z.max_nev = std::max(z.max_nev, n_ev);
        // algorithmic traffic: raw in + seq + norm out + segs + band starts +
        // 2-bit moves + scalars
        z.algo_bytes += 8.0 * n_raw + (double)seq_len + 8.0 * n_raw + 8.0 * (B + 1) + 8.0 * B +
                        (double)((B * p->bandwidth + 3) / 4) + 64.0;
        z.cells += (double)B * p->bandwidth + (short_read ? 0.0 : (double)p->start_n_bases * p->start_bw);
    }
    z.S_tot = raw_acc; z.seq_tot = seq_acc; z.B_tot = ref_acc; z.E_tot = ev_acc;
    z.wide_w = z.max_nev > TBA_MAX_BAND ? ((z.max_nev + 63) / 64) * 64 : 0;
    const i64 start_w = std::max(p->start_bw, p->start_save_bw);
    z.start_moves_stride = (p->start_n_bases + 1) * (i64)mv_class_rowb(cpl_class(start_w));
    z.moves_arena = z.moves_need + z.moves_need / 8 + (64ll << 20);
    // raw-DP scratch arena (8-byte units): windows are a few bases x tens of samples; reads that
    // do not fit the arena get TBA_UNSUPPORTED
    z.skip_arena = n * 32768 + (32ll << 20);
    z.n_stall = stall_off ? stall_off[n] : stall_acc;
    return 0;
}

// the device buffers of a batch: (buffer, bytes) through `f`
template <class F>
static void for_each_batch_buffer(tba_engine *e, const tba_params *p, const tba_opts *o, i64 n,
                                  const BatchSizes &z, int raw_dtype, F f)
{
    const size_t S = (size_t)std::max<i64>(z.S_tot, 1), Bt = (size_t)std::max<i64>(z.B_tot, 1),
                 Et = (size_t)std::max<i64>(z.E_tot, 1), N = (size_t)n;
#define BUF(name_, bytes_) f(e ? &e->name_ : (DevBuf *)nullptr, (size_t)(bytes_)) // (e == NULL: sizes only)
    BUF(d_rs, N * sizeof(ReadState));
    BUF(d_dp, sizeof(DevParams));
    // (+ 64 bytes: the 16-byte accesses of a pass over a signal may touch the element past an odd end)
    BUF(d_raw, S * raw_elem_bytes(raw_dtype) + 64);
    BUF(d_norm, S * 8 + 64);
    if (!o->skip_norm_out) BUF(d_norm_out, S * 8 + 64);
    BUF(d_csum, (S + N) * 8 + 64);
    BUF(d_score, S * 8 + 64);
    BUF(d_state, std::max(S, S / 8 + 8 * N + 64)); // (also the stall detector's bit words)
    BUF(d_cpts, Et * 8);
    BUF(d_evm, Et * 8);
    BUF(d_seq, (size_t)std::max<i64>(z.seq_tot, 1));
    BUF(d_refm, Bt * 8);
    BUF(d_refs, Bt * 8);
    BUF(d_bst, Bt * 8);
    BUF(d_lo, Bt * 4);
    BUF(d_hi, Bt * 4);
    BUF(d_readtb, (Bt + N) * 8);
    BUF(d_dpsegs, (Bt + N) * 8);
    BUF(d_segs, (Bt + N) * 8);
    BUF(d_win, (Bt + N) * 24);
    BUF(d_absz, Bt * 8);
    BUF(d_sv_in, N * 32);
    BUF(d_samp, N * MAX_TS_POINTS * 8);
    BUF(d_lastrow, N * TBA_MAX_BAND * 8);
    BUF(d_startvals, N * (size_t)p->start_n_bases * 8);
    BUF(d_smoves, N * (size_t)z.start_moves_stride);
    BUF(d_moves, (size_t)z.moves_arena);
    BUF(d_dscr, (size_t)z.skip_arena * 8);
    if (z.wide_w) BUF(d_wide, (size_t)WIDE_BLOCKS * 2 * (size_t)z.wide_w * 8);
    if (z.n_stall > 0) BUF(d_stall, (size_t)z.n_stall * 16);
    if (o->detect_stalls) { // (its scratch is its own: the detector runs beside event detection, which owns csum / state)
        BUF(d_stall_bits, S / 8 + 8 * N + 64);
        if (!(raw_dtype == TBA_RAW_I16 && o->stall_window_size <= SI_MAXW)) BUF(d_stall_csum, (S + N) * 8 + 64);
    }
    BUF(d_skipq, 64 + 3 * (N * 32 + 4096) * 8);
    BUF(d_order, N * 4);
    BUF(d_long, N * 4);
    BUF(d_res, N * sizeof(tba_read_result));
    BUF(d_segs32, (Bt + N) * 4);
#undef BUF
}

extern "C" int tba_batch_footprint(const tba_params *p, const tba_opts *o, int64_t kmer_width,
                                   int raw_dtype, int64_t n_reads, const int64_t *n_raw,
                                   const int64_t *seq_len, double *bytes)
{
    if (!p || !o || !n_raw || !seq_len || !bytes || n_reads <= 0 || kmer_width < 1)
        return set_err(TBA_E_ARG, "bad arguments");
    if (raw_dtype < TBA_RAW_F64 || raw_dtype > TBA_RAW_I16) return set_err(TBA_E_ARG, "unknown raw dtype");
    BatchSizes z;
    std::vector<i64> none;
    if (int rc = plan_batch(p, o, kmer_width, n_reads, nullptr, n_raw, nullptr, seq_len, none, nullptr,
                            nullptr, nullptr, z))
        return rc;
    double tot = 0;
    for_each_batch_buffer(nullptr, p, o, n_reads, z, raw_dtype,
                          [&](DevBuf *, size_t b) { tot += (double)(b + b / 8 + 256); });
    *bytes = tot;
    return 0;
}

extern "C" int tba_batch_upload_async(tba_engine *e, const tba_params *p, const tba_opts *o,
                                      int64_t n_reads, const void *raw, int raw_dtype,
                                      const int64_t *raw_off, const uint8_t *seq,
                                      const int64_t *seq_off, const double *sv_in,
                                      const int32_t *sv_flags, const int64_t *samp_ind,
                                      const int64_t *stall_ints, const int64_t *stall_off)
{
    // the forced event counts apply to this upload only, whatever its outcome
    std::vector<i64> ne_override;
    if (e) ne_override.swap(e->ne_override);
    if (!e || !p || !o || n_reads <= 0 || !raw || !raw_off || !seq || !seq_off)
        return set_err(TBA_E_ARG, "bad batch arguments");
    if (raw_dtype < TBA_RAW_F64 || raw_dtype > TBA_RAW_I16) return set_err(TBA_E_ARG, "unknown raw dtype");
    // several kernels index the read with the y dimension of the grid
    if (n_reads > TBA_MAX_BATCH_READS) return set_err(TBA_E_ARG, "more than TBA_MAX_BATCH_READS reads in one batch");
    if (!e->have_model) return set_err(TBA_E_STATE, "tba_set_model has not been called");
    if (o->del_fix_window < 0 || o->max_del_fix_window < 0 || !(o->extra_sig_factor >= 0.0))
        return set_err(TBA_E_ARG, "bad skipped-base window parameters");
    if (p->bandwidth < 2 || p->running_stat_width < 1 || p->min_obs_per_base < 1 ||
        p->raw_min_obs_per_base < 1 || p->mean_obs_per_event < 1 || p->start_n_bases < 1)
        return set_err(TBA_E_ARG, "bad resquiggle parameters");
    // CSR offsets: start at 0, never decrease (a foreign caller's mistake must not become an
    // out-of-bounds device access)
    if (raw_off[0] != 0 || seq_off[0] != 0) return set_err(TBA_E_ARG, "offset arrays must start at 0");
    for (i64 i = 0; i < n_reads; i++)
        if (raw_off[i + 1] < raw_off[i] || seq_off[i + 1] < seq_off[i])
            return set_err(TBA_E_ARG, "offset arrays must be non-decreasing");
    const bool stalls = stall_ints && stall_off;
    if (o->detect_stalls) {
        if (stalls) return set_err(TBA_E_ARG, "stall_ints given together with tba_opts.detect_stalls");
        // th.stallParams of the running-window-mean method (tombo_stats.py:317-323)
        if (o->stall_n_windows < 2 || o->stall_n_windows > 16 || o->stall_mini_window_size < 1 ||
            o->stall_window_size != o->stall_n_windows * o->stall_mini_window_size ||
            o->stall_min_consecutive_obs < 0 || !(o->stall_threshold == o->stall_threshold))
            return set_err(TBA_E_ARG, "bad stall detection parameters");
    }
    if (stalls) {
        if (stall_off[0] != 0) return set_err(TBA_E_ARG, "offset arrays must start at 0");
        for (i64 i = 0; i < n_reads; i++) {
            if (stall_off[i + 1] < stall_off[i]) return set_err(TBA_E_ARG, "offset arrays must be non-decreasing");
            // interval ends ascend (k_remove_stalls binary-searches them; the values themselves are
            // only compared, never used as indices: identify_stalls widens past the signal ends)
            for (i64 k = stall_off[i] + 1; k < stall_off[i + 1]; k++)
                if (stall_ints[2 * k + 1] < stall_ints[2 * k - 1])
                    return set_err(TBA_E_ARG, "stall interval ends must ascend");
        }
    }
    HIP_TRY(hipSetDevice(e->device));
    // the previous batch of this engine must be done with the buffers (and with h_rs)
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_batch = e->ran = e->finished = e->center_ready = false;
    e->hp.p = *p;
    e->hp.o = *o;
    e->hp.fill_masked = (MASK_FILL_Z_SCORE - p->z_shift) + p->z_shift;
    if (o->del_fix_window == 0 && o->max_del_fix_window == 0 && o->extra_sig_factor == 0.0) {
        // a zero-initialised tba_opts: the reference's defaults
        e->hp.o.del_fix_window = DEL_FIX_WINDOW; e->hp.o.max_del_fix_window = MAX_DEL_FIX_WINDOW;
        e->hp.o.extra_sig_factor = EXTRA_SIG_FACTOR;
    }
    const i64 n = n_reads;
    if (e->h_rs.ensure((size_t)n * sizeof(ReadState)) || e->h_dp.ensure(sizeof(DevParams))) return TBA_E_NOMEM;
    BatchSizes &z = e->z = BatchSizes();
    if (int rc = plan_batch(p, o, e->hp.kmer_width, n, raw_off, nullptr, seq_off, nullptr, ne_override,
                            sv_flags, stalls ? stall_off : nullptr, e->h_rs.as<ReadState>(), z))
        return rc;
    e->n_reads = n, e->raw_dtype = raw_dtype;
    e->any_stall = (stalls && stall_off[n] > 0) || o->detect_stalls;
    e->have_samp = samp_ind != nullptr;
    e->have_sv = sv_in != nullptr && sv_flags != nullptr;
    int rc = 0;
    const size_t norm_out_was = e->d_norm_out.cap;
    for_each_batch_buffer(e, p, o, n, z, raw_dtype, [&](DevBuf *b, size_t bytes) { rc |= b->ensure(bytes); });
    if (rc) return TBA_E_NOMEM;
    // a new d_norm_out starts as zeros: a download of it holds samples no kernel writes (past a read's norm_len, the
    // reads that failed), and those must not be whatever the allocation held before (NaN left by another call's scratch)
    if (e->d_norm_out.p && e->d_norm_out.cap != norm_out_was)
        HIP_TRY(hipMemsetAsync(e->d_norm_out.p, 0, e->d_norm_out.cap, e->stream));

    hipStream_t s = e->stream;
    const size_t N = (size_t)n;
    { // reads by decreasing length (stable): the groups of a k_dp_multi wavefront finish together
        if (e->h_order.ensure(N * 4)) return TBA_E_NOMEM;
        i32 *ord = e->h_order.as<i32>();
        const ReadState *hrs = e->h_rs.as<ReadState>();
        for (i64 i = 0; i < n; i++) ord[i] = (i32)i;
        std::stable_sort(ord, ord + n, [hrs](i32 a, i32 b) { return hrs[a].B > hrs[b].B; });
        HIP_TRY(hipMemcpyAsync(e->d_order.p, ord, N * 4, hipMemcpyHostToDevice, s));
        // the long reads, longest first (is_long was set by plan_batch)
        if (e->h_long.ensure(N * 4)) return TBA_E_NOMEM;
        i32 *lg = e->h_long.as<i32>();
        e->n_long = 0;
        for (i64 i = 0; i < n; i++) if (hrs[ord[i]].is_long) lg[e->n_long++] = ord[i];
        if (e->n_long > 0) HIP_TRY(hipMemcpyAsync(e->d_long.p, lg, (size_t)e->n_long * 4, hipMemcpyHostToDevice, s));
    }
    e->hp.dp_wg_mode = 0;
    memcpy(e->h_dp.p, &e->hp, sizeof(DevParams));
    HIP_TRY(hipMemcpyAsync(e->d_rs.p, e->h_rs.p, N * sizeof(ReadState), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->d_dp.p, e->h_dp.p, sizeof(DevParams), hipMemcpyHostToDevice, s));
    // (raw / seq may be device memory -- a batch made by tba_synth_generate: the kind is taken from the pointer)
    HIP_TRY(hipMemcpyAsync(e->d_raw.p, raw, (size_t)z.S_tot * raw_elem_bytes(raw_dtype), hipMemcpyDefault, s));
    HIP_TRY(hipMemcpyAsync(e->d_seq.p, seq, (size_t)z.seq_tot, hipMemcpyDefault, s));
    if (e->have_sv) HIP_TRY(hipMemcpyAsync(e->d_sv_in.p, sv_in, N * 32, hipMemcpyHostToDevice, s));
    if (e->have_samp)
        HIP_TRY(hipMemcpyAsync(e->d_samp.p, samp_ind, N * MAX_TS_POINTS * 8, hipMemcpyHostToDevice, s));
    if (stalls && stall_off[n] > 0)
        HIP_TRY(hipMemcpyAsync(e->d_stall.p, stall_ints, (size_t)stall_off[n] * 16, hipMemcpyHostToDevice, s));
    if (o->reverse_raw) { // once per upload, in stream order behind the copy
        const unsigned gr = (unsigned)std::min<i64>(std::max<i64>((z.max_raw / 2 + 1023) / 1024, 1), 64);
        RAW_DISPATCH(raw_dtype, (k_reverse_raw<RT><<<dim3(gr, (unsigned)n), 256, 0, s>>>(e->d_rs.as<ReadState>(), e->d_raw.as<RT>())));
        HIP_TRY(hipGetLastError());
    }
    e->have_batch = true;
    e->refs_put = false;
    return 0;
}

extern "C" int tba_batch_upload(tba_engine *e, const tba_params *p, const tba_opts *o,
                                int64_t n_reads, const double *raw, const int64_t *raw_off,
                                const uint8_t *seq, const int64_t *seq_off, const double *sv_in,
                                const int32_t *sv_flags, const int64_t *samp_ind,
                                const int64_t *stall_ints, const int64_t *stall_off)
{
    if (int rc = tba_batch_upload_async(e, p, o, n_reads, raw, TBA_RAW_F64, raw_off, seq, seq_off, sv_in,
                                        sv_flags, samp_ind, stall_ints, stall_off)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int tba_set_num_events(tba_engine *e, const int64_t *num_events, int64_t n_reads)
{
    if (!e || n_reads < 0) return set_err(TBA_E_ARG, "bad arguments");
    if (!num_events) { e->ne_override.clear(); return 0; }
    e->ne_override.assign(num_events, num_events + n_reads);
    return 0;
}

// k_dp<8> or its 112-register build (k_dp.h): the latter when other engines run their kernels beside
// this one (streaming slots) and the batch has more than 0.04 samples per DP cell, i.e. event
// detection and normalisation, not the DP, are most of the work (RNA 3 kb: 0.087, DNA 10 kb: 0.018)
static bool dp_lowreg(const tba_engine *e) { return e->n_sharing > 1 && e->z.cells > 0 && (double)e->z.S_tot > 0.04 * e->z.cells; }
// k_dp<CPL> or k_dp_cdiv<CPL>, the two-operation division: the latter when every sd the rows can meet is a proven
// divisor, i.e. the model's table is and d_refs was filled from it (k_ref_levels copies the table's values)
static bool dp_cdiv(const tba_engine *e) { return e->cdiv_auto && e->model_cdiv && !e->refs_put; }
// ... or k_dp_c1<CPL>, its form for a table with ONE sd (the reciprocal pair comes from one_sd_w as kernel arguments, not from d_refs)
static bool dp_one_sd(const tba_engine *e) { return dp_cdiv(e) && e->one_sd; }

// ---- the pipeline -----------------------------------------------------------------------------
// One run over the uploaded batch, as its steps see it: the engine, its streams, the grid sizes, the kernel
// forms, and the device buffers as typed pointers (each cast made here, once).
struct Run {
    tba_engine *const e;
    const tba_params &P = e->hp.p;
    const tba_opts &O = e->hp.o;
    const hipStream_t s = e->stream;
    hipStream_t s2 = s; // (run_prelude) the side stream of a full run, else the main stream
    bool side = false;  // ... which implies the whole stage range
    const i64 n = e->n_reads;
    const unsigned nb = (unsigned)n, tpr = (unsigned)((n + 63) / 64); // (tpr: blocks for thread-per-read kernels)
    // workgroups per read of the (blocks, reads) kernels: 256 items per workgroup when the batch is
    // small (parallelism), up to 4096 when the reads alone fill the machine -- short-lived
    // workgroups cost more in launches than they win in balance (RNA, 10 k reads: 113 -> 107 ms)
    unsigned gx(i64 items) const
    {
        const i64 fine = (items + 255) / 256, coarse = (items + 4095) / 4096;
        const i64 want = (16384 + n - 1) / n; // enough workgroups in all for ~8 per CU-slot
        return (unsigned)std::min<i64>(std::max<i64>(std::max<i64>(coarse, std::min<i64>(fine, want)), 1), 128);
    }
    const unsigned gS = gx(e->z.max_raw), gB = gx(e->z.max_B), gE = gx(e->z.max_raw / std::max<i64>(P.mean_obs_per_event, 1) + 1);
    const bool rna = P.use_t_test_seg != 0;
    const bool fused_scores = 2 * P.running_stat_width <= 64; // cumsum + scores in one kernel
    // DNA defaults: the scores never reach memory (k_detect.h); what that form leaves (flagged reads)
    // goes through the kernels of the other forms as before
    const bool fused_detect = !rna && 2 * P.running_stat_width <= DT_W2MAX && P.min_obs_per_base == 3;
    // A handful of reads cannot hide the scan's serial chain behind each other: k_detect /
    // k_cumsum_scores pay a pipeline step (barrier, memory round trip, greedy: ~7 us) per 128 samples
    // whatever the batch, 5 ms for a 10 kb read; a workgroup per read (k_long.h: the step is 1 856
    // dependent adds long) does the same in 0.5 ms.  (resquiggle_read, a batch of one: 20.4 -> 16 ms.)
    const bool wg_scan = !rna && fused_scores && n <= e->small_batch && (size_t)n * 4 <= e->d_order.cap;
    const bool fused_tt = rna && P.min_obs_per_base == 6 && P.running_stat_width <= TT_MAXW; // RNA defaults: radius 5
    const int only_flagged = (fused_detect && !wg_scan) || fused_tt ? 1 : 0;
    const int rdt = e->raw_dtype;
    void *raw = e->d_raw.p; // samples of that type: (RT *) under RAW_DISPATCH(c.rdt, ...)
    ReadState *rs = e->d_rs.as<ReadState>();
    const DevParams *dp = e->d_dp.as<DevParams>();
    uint8_t *seq = e->d_seq.as<uint8_t>();
    unsigned char *state = e->d_state.as<unsigned char>(), *smoves = e->d_smoves.as<unsigned char>(), *moves = e->d_moves.as<unsigned char>();
    i32 *order = e->d_order.as<i32>(), *lng = e->d_long.as<i32>(), *lo = e->d_lo.as<i32>(), *hi = e->d_hi.as<i32>();
    i64 *cpts = e->d_cpts.as<i64>(), *samp = e->d_samp.as<i64>(), *stall = e->d_stall.as<i64>(), *bst = e->d_bst.as<i64>(), *readtb = e->d_readtb.as<i64>(),
        *dpsegs = e->d_dpsegs.as<i64>(), *segs = e->d_segs.as<i64>(), *win = e->d_win.as<i64>(), *skipq = e->d_skipq.as<i64>();
    u64 *stall_bits = e->d_stall_bits.as<u64>();
    double *kmeans = e->d_kmeans.as<double>(), *ksds = e->d_ksds.as<double>(), *sv_in = e->d_sv_in.as<double>(), *norm = e->d_norm.as<double>(),
           *norm_out = e->d_norm_out.as<double>(), *csum = e->d_csum.as<double>(), *score = e->d_score.as<double>(), *evm = e->d_evm.as<double>(),
           *refm = e->d_refm.as<double>(), *refs = e->d_refs.as<double>(), *lastrow = e->d_lastrow.as<double>(), *startvals = e->d_startvals.as<double>(),
           *wide = e->d_wide.as<double>(), *dscr = e->d_dscr.as<double>(), *absz = e->d_absz.as<double>(), *stall_csum = e->d_stall_csum.as<double>();
};
template <int CPL>
static void launch_dp_t(Run &c, int mode)
{
    // (a main pass under k_dp8_lowreg's selector stays on the general division in every class: step_main_dp)
    const bool lowreg = mode == DP_MAIN && dp_lowreg(c.e);
    unsigned char *const mv = mode == DP_MAIN ? c.moves : c.smoves;
    if (dp_one_sd(c.e) && !lowreg) {
        k_dp_c1<CPL><<<dim3(c.nb), dim3(64), 0, c.s>>>(c.rs, c.dp, mode, c.evm, c.refm, c.refs, c.bst, c.lo, c.hi, mv, c.e->z.start_moves_stride, c.lastrow, nullptr,
                                                       c.e->one_sd_w[1], c.e->one_sd_w[2]);
        return;
    }
    const auto k = CPL == 8 && lowreg ? k_dp8_lowreg : dp_cdiv(c.e) && !lowreg ? k_dp_cdiv<CPL> : k_dp<CPL, false>;
    k<<<dim3(c.nb), dim3(64), 0, c.s>>>(c.rs, c.dp, mode, c.evm, c.refm, c.refs, c.bst, c.lo, c.hi, mode == DP_MAIN ? c.moves : c.smoves, c.e->z.start_moves_stride, c.lastrow, nullptr);
}
template <int CPL, int RPW>
static void launch_dp_multi_t(Run &c)
{
    k_dp_multi<CPL, RPW><<<dim3((unsigned)((c.n + RPW - 1) / RPW)), dim3(64), 0, c.s>>>(c.rs, c.n, c.order, c.dp, c.evm, c.refm, c.refs, c.bst, c.lo, c.hi, c.moves, c.lastrow);
}
// the band classes of k_dp (cpl_class, k_dp.h): `list` in the order the main DP launches them;
// dispatch(cpl, f) calls f(std::integral_constant<int, CPL>()) for the run-time class (nothing for 0)
template <int... CPL>
struct CplClasses {
    static constexpr int list[] = {CPL...};
    template <class F> static void dispatch(int cpl, F f)
    {
        (void)((cpl == CPL && (f(std::integral_constant<int, CPL>()), true)) || ...);
    }
};
typedef CplClasses<4, 5, 8, 12, 16, 24, 32, 48> DpClasses;

static void launch_dp(Run &c, int cpl, int mode) { DpClasses::dispatch(cpl, [&](auto cls) { launch_dp_t<decltype(cls)::value>(c, mode); }); }

// Before the first step: a run from the top starts from the uploaded state; the `total` bracket opens; a
// full run forks the side stream, which takes stall detection and the expected levels.
static int run_prelude(Run &c, int first, int last)
{
    tba_engine *e = c.e;
    const hipStream_t s = c.s;
    // starting from the top discards the state of a previous run of the same batch
    if (first == TBA_STAGE_SEGMENT) {
        HIP_TRY(hipMemcpyAsync(e->d_rs.p, e->h_rs.p, (size_t)c.n * sizeof(ReadState), hipMemcpyHostToDevice, s));
        e->last_dp = tba_engine::DpLaunches();
    }
    HIP_TRY(hipEventRecord(e->ev[SLOT_TOTAL], s));         // start of the sequence (the `total` bracket)
    // A full run forks the side stream here (TBA_NO_SIDE_STREAM=1: everything on the main stream, in
    // this order); a partial run (stepwise API) stays on one stream.
    static const bool side_off = getenv("TBA_NO_SIDE_STREAM") != nullptr;
    static const int max_engines = [] { const char *x = getenv("TBA_SIDE_STREAM_MAX_ENGINES"); return x ? atoi(x) : 2; }();
    c.side = !side_off && first == TBA_STAGE_SEGMENT && last == TBA_STAGE_RESCALE && e->side_mode != 0 &&
             (e->side_mode == 1 || (e->device < TBA_MAX_DEVICES &&
              std::max(e->n_sharing, g_live_engines[e->device].load()) <= max_engines));
    e->last_side = c.side;
    if (c.side && !e->stream2) HIP_TRY(hipStreamCreate(&e->stream2)); // (created on first use: a stream takes a queue slot)
    const hipStream_t s2 = c.s2 = c.side ? e->stream2 : s;
    if (c.side) {
        HIP_TRY(hipEventRecord(e->ev_fork, s));
        HIP_TRY(hipStreamWaitEvent(s2, e->ev_fork, 0));
    }
    // caller-side preparation: ts.identify_stalls over the raw samples (its own scratch: it runs beside
    // event detection)
    HIP_TRY(hipEventRecord(e->ev_st0, s2));
    if (first == TBA_STAGE_SEGMENT && c.O.detect_stalls) {
        const unsigned gq = c.gx(e->z.max_raw / 8 + 1); // chunks of SI_T positions
        if (c.rdt == TBA_RAW_I16 && c.O.stall_window_size <= SI_MAXW) { // exact integer sums: no cumulative sum in memory
            (c.O.stall_n_windows == 7 ? k_stall_metric_i16<7> : k_stall_metric_i16<0>)<<<dim3(gq, c.nb), 256, 0, s2>>>(c.rs, c.dp, (int16_t *)c.raw, c.stall_bits);
        } else {
            if (cs_reads_for(c.n) == 20) RAW_DISPATCH(c.rdt, (k_cumsum_scores<20, RT, 1><<<(unsigned)((c.n + 19) / 20), 256, 0, s2>>>(c.rs, c.n, c.dp, (RT *)c.raw, c.stall_csum)));
            else RAW_DISPATCH(c.rdt, (k_cumsum_scores<32, RT, 1><<<(unsigned)((c.n + 31) / 32), 256, 0, s2>>>(c.rs, c.n, c.dp, (RT *)c.raw, c.stall_csum)));
            if (e->n_long > 0) RAW_DISPATCH(c.rdt, (k_cumsum_scores_long<RT, 1><<<(unsigned)e->n_long, 256, 0, s2>>>(c.rs, c.lng, c.dp, (RT *)c.raw, c.stall_csum)));
            (c.O.stall_n_windows == 7 ? k_stall_metric<7> : k_stall_metric<0>)<<<dim3(gq, c.nb), 256, 0, s2>>>(c.rs, c.dp, c.stall_csum, c.stall_bits);
        }
        k_stall_runs<<<dim3(c.gx(e->z.max_raw / 64 + 1), c.nb), 256, 0, s2>>>(c.rs, c.dp, c.stall_bits, c.stall);
        k_stall_merge<<<c.tpr, 64, 0, s2>>>(c.rs, c.n, c.dp, c.stall);
    }
    HIP_TRY(hipEventRecord(e->ev_st1, s2));
    if (c.side) {
        HIP_TRY(hipEventRecord(e->ev_stalls, s2));
        // the expected levels need the sequence and the model only
        k_ref_levels<<<dim3(c.gB, c.nb), 256, 0, s2>>>(c.rs, c.dp, c.seq, c.kmeans, c.ksds, c.refm, c.refs, 1);
        e->refs_put = false;
        HIP_TRY(hipEventRecord(e->ev_levels, s2));
    }
    return 0;
}

// ts.normalize_raw_signal: float samples go through k_normalize_hist first (the medians of the reads it takes,
// two passes over the signal), then k_normalize (every other read's medians, and the normalised signal).  A batch
// with a const scale, or RNA with its scale values from the events, has no medians for the first kernel: not launched.
static void launch_normalize(Run &c, int mode, int write_norm)
{
    if (batch_has_medians(c.O, mode)) {
        if (c.rdt == TBA_RAW_F32) k_normalize_hist<float><<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, (float *)c.raw, c.norm, mode);
        else if (c.rdt != TBA_RAW_I16) k_normalize_hist<double><<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, (double *)c.raw, c.norm, mode);
    }
    RAW_DISPATCH(c.rdt, (k_normalize<RT><<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, (RT *)c.raw, c.norm, c.sv_in, mode, write_norm)));
}

// The steps: what runs between the timing events ev[i] and ev[i + 1], in the order of STEPS below.
static int step_normalize(Run &c)
{
    // (with k_detect on the way its loader writes the normalised signal: k_normalize only finds the
    // scale values then, and normalises the long reads, which k_detect leaves to k_long.h)
    if (!c.rna) launch_normalize(c, 0, c.fused_detect && !c.wg_scan ? 2 : 1);
    return 0;
}
static int step_cumsum(Run &c)
{
    const i64 n = c.n;
    if (c.rna) return 0;
    if (c.wg_scan) {
        k_cumsum_scores_long<double, 0><<<c.nb, 256, 0, c.s>>>(c.rs, c.order, c.dp, c.norm, c.score);
        return 0;
    }
    if (c.fused_detect) {
        RAW_DISPATCH(c.rdt, (k_detect<2, RT><<<(unsigned)((n + DT_READS - 1) / DT_READS), 256, 0, c.s>>>(c.rs, n, c.dp, (RT *)c.raw, c.norm, c.csum, c.score, c.e->z.S_tot)));
        k_pick<<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, c.csum, c.score, c.cpts, 0);
    }
    if (c.fused_scores) {
        if (cs_reads_for(n) == 20) k_cumsum_scores<20><<<(unsigned)((n + 19) / 20), 256, 0, c.s>>>(c.rs, n, c.dp, c.norm, c.score, c.only_flagged);
        else k_cumsum_scores<32><<<(unsigned)((n + 31) / 32), 256, 0, c.s>>>(c.rs, n, c.dp, c.norm, c.score, c.only_flagged);
        if (c.e->n_long > 0) k_cumsum_scores_long<double, 0><<<(unsigned)c.e->n_long, 256, 0, c.s>>>(c.rs, c.lng, c.dp, c.norm, c.score);
    }
    else k_cumsum<<<c.tpr, 64, 0, c.s>>>(c.rs, n, c.norm, c.csum);
    return 0;
}
static int step_scores(Run &c)
{
    if (!c.rna) {
        if (!c.fused_scores) k_scores_dna<<<dim3(c.gS, c.nb), 256, 0, c.s>>>(c.rs, c.dp, c.csum, c.score);
        return 0;
    }
    if (c.fused_tt) {
        if (c.P.running_stat_width == 12) RAW_DISPATCH(c.rdt, (k_detect_tt<5, 12, RT><<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, (RT *)c.raw, c.csum, c.score)));
        else RAW_DISPATCH(c.rdt, (k_detect_tt<5, 0, RT><<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, (RT *)c.raw, c.csum, c.score)));
        k_pick<<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, c.csum, c.score, c.cpts, 1);
    }
    RAW_DISPATCH(c.rdt, (k_scores_ttest<RT><<<dim3(c.gS, c.nb), 256, 0, c.s>>>(c.rs, c.dp, (RT *)c.raw, c.score, c.only_flagged)));
    return 0;
}
static int step_peaks(Run &c)
{
    launch_peaks(c.P.min_obs_per_base, c.nb, c.s, c.rs, c.dp, c.score, c.state, c.csum, c.cpts, c.rna ? 1 : 0, c.only_flagged,
                 c.rna ? TBA_ED_FORM_TTEST_PEAKS : c.wg_scan ? TBA_ED_FORM_WG_SCAN_PEAKS : TBA_ED_FORM_SCORES_PEAKS);
    if (c.side) HIP_TRY(hipStreamWaitEvent(c.s, c.e->ev_stalls, 0)); // the stall intervals (and nothing else of the side stream)
    if (c.e->any_stall) k_remove_stalls<<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.n, c.stall, c.cpts, c.csum);
    if (c.rna) { // RNA normalises after event detection (segment_signal, resquiggle.py:1073-1098)
        RAW_DISPATCH(c.rdt, (k_event_means<RT, 1280><<<dim3(c.gE, c.nb), 256, 0, c.s>>>(c.rs, c.dp, (RT *)c.raw, c.cpts, c.evm, 1)));
        k_rna_event_scale<<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, c.evm);
        launch_normalize(c, 1, 1);
    }
    return 0;
}
static int step_event_means(Run &c)
{
    // long events (RNA: mean_obs_per_event 15): the wide staging slice
    (c.P.mean_obs_per_event >= 10 ? k_event_means<double, 1280> : k_event_means<double>)<<<dim3(c.gE, c.nb), 256, 0, c.s>>>(c.rs, c.dp, c.norm, c.cpts, c.evm, 0);
    return 0;
}
static int step_ref_levels(Run &c)
{
    if (c.side) {                                                  // (computed on the side stream)
        HIP_TRY(hipStreamWaitEvent(c.s, c.e->ev_levels, 0));
        k_seq_status<<<c.tpr, 64, 0, c.s>>>(c.rs, c.n);
    } else {
        k_ref_levels<<<dim3(c.gB, c.nb), 256, 0, c.s>>>(c.rs, c.dp, c.seq, c.kmeans, c.ksds, c.refm, c.refs);
        c.e->refs_put = false;                                     // (d_refs holds the table's values again)
    }
    return 0;
}
static void launch_start_tb(Run &c, int mode)
{
    k_start_tb<<<(unsigned)((c.n + TB_LANES - 1) / TB_LANES), TB_LANES, 0, c.s>>>(c.rs, c.n, c.dp, mode, c.evm, c.refm, c.refs, c.smoves, c.e->z.start_moves_stride, c.readtb, c.startvals);
}
// start_dp + start_tb: find_seq_start_in_events, first try then retry
static int step_start_dp(Run &c)
{
    k_path0<<<c.tpr, 64, 0, c.s>>>(c.rs, c.n, c.dp);
    c.e->last_dp.cdiv_start = dp_cdiv(c.e);
    c.e->last_dp.c1_start = dp_one_sd(c.e);
    launch_dp(c, cpl_class(c.P.start_bw), DP_START_TRY);
    launch_start_tb(c, DP_START_TRY);
    return 0;
}
static int step_start_tb(Run &c)
{
    // the retry of the few reads whose first try failed: one workgroup per read (k_dp_wg.h)
    const int wcpl = c.P.start_n_bases <= WG_MAX_ROWS ? dp_wg_cpl(c.P.start_save_bw) : 0;
    c.e->last_dp.start = true, c.e->last_dp.retry_wcpl = wcpl;
    c.e->last_dp.c1_retry = wcpl == 0 && dp_one_sd(c.e); // (k_dp_wg has the general division only)
    const auto wg = wcpl == 4 ? k_dp_wg<4> : wcpl == 8 ? k_dp_wg<8> : wcpl == 12 ? k_dp_wg<12> : nullptr;
    if (wg) wg<<<c.nb, 256, 0, c.s>>>(c.rs, c.dp, c.evm, c.refm, c.refs, c.smoves, c.e->z.start_moves_stride, c.lastrow);
    else launch_dp(c, cpl_class(c.P.start_save_bw), DP_START_RETRY);
    launch_start_tb(c, DP_START_RETRY);
    return 0;
}
static int step_prep(Run &c)
{
    k_prep<<<c.tpr, 64, 0, c.s>>>(c.rs, c.n, c.dp, c.bst, c.lo, c.hi);
    k_scan_arena<0><<<1, 256, 0, c.s>>>(c.rs, c.n, c.e->z.moves_arena);
    return 0;
}
static int step_main_dp(Run &c)
{
    const i64 wide_w = c.e->z.wide_w;
    c.e->last_dp.main = true, c.e->last_dp.wide = wide_w != 0;
    c.e->last_dp.lowreg = dp_lowreg(c.e); // (launch_dp_t's choice for the 8-cell class)
    c.e->last_dp.cdiv_main = dp_cdiv(c.e) && !dp_lowreg(c.e); // (... and for every class)
    c.e->last_dp.c1_main = dp_one_sd(c.e) && !dp_lowreg(c.e);
    for (int cls : DpClasses::list) launch_dp(c, cls, DP_MAIN);
    const DpMultiClass m = dp_multi_class(c.P.bandwidth); // narrow adaptive bands: several reads per wavefront
    if (m.cpl == 4 && m.rpw == 2) launch_dp_multi_t<4, 2>(c);
    if (wide_w) // a static band wider than every class is possible in this batch
        k_dp_wide<<<WIDE_BLOCKS, 64, 0, c.s>>>(c.rs, c.n, c.dp, c.evm, c.refm, c.refs, c.bst, c.moves, c.wide, wide_w);
    return 0;
}
static int step_main_tb(Run &c)
{
    const i64 n = c.n, n_long = c.e->n_long;
    // rows of a read over several lanes (k_tb_par.h): 16 lanes per read when the reads fill the
    // machine, a wavefront per read for small batches and for the long reads; what it leaves
    // (static bands, failed verification) is walked by the lane-per-read kernels below
    const bool lanes16 = n > c.e->tb_wave_below;
    auto per_chunk = [&](auto k16, auto k64) {
        if (lanes16) k16<<<(unsigned)((n + 3) / 4), 64, 0, c.s>>>(c.rs, n, nullptr, c.dp, c.moves, c.bst, c.readtb);
        else k64<<<c.nb, 64, 0, c.s>>>(c.rs, n, nullptr, c.dp, c.moves, c.bst, c.readtb);
        if (n_long > 0 && lanes16) k64<<<(unsigned)n_long, 64, 0, c.s>>>(c.rs, n_long, c.lng, c.dp, c.moves, c.bst, c.readtb);
    };
    per_chunk(k_main_tb_par<16>, k_main_tb_par<64>);
#ifndef TBA_NO_TB_VERIFY
    // behind the kernel boundary: the first block of rows under every chunk top walked again, compare
    // only; what disagrees is the serial kernels' (counted: TBA_GET_TB_VERIFY_FAIL), the rest is trimmed
    per_chunk(k_tb_par_verify<16>, k_tb_par_verify<64>);
#endif
    k_main_tb<<<(unsigned)((n + TB_LANES - 1) / TB_LANES), TB_LANES, 0, c.s>>>(c.rs, n, c.dp, c.moves, c.bst, c.readtb);
    if (n_long > 0) k_main_tb_long<<<(unsigned)n_long, 64, 0, c.s>>>(c.rs, c.lng, c.dp, c.moves, c.bst, c.readtb);
    k_tb_gather<<<dim3(c.gB, c.nb), 256, 0, c.s>>>(c.rs, c.cpts, c.readtb, c.dpsegs);
    return 0;
}
static int step_skip_resolve(Run &c)
{
    // window queues of the wave-per-window kernels: counters + three (read, window) lists
    const i64 qcap = c.n * 32 + 4096;
    i32 *lists = (i32 *)(c.skipq + 8);
    HIP_TRY(hipMemsetAsync(c.skipq, 0, 64, c.s));
    k_skip_plan<<<c.nb, 64, 0, c.s>>>(c.rs, c.n, c.dp, c.dpsegs, c.segs, c.win, c.skipq, lists, qcap);
    k_scan_arena<1><<<1, 256, 0, c.s>>>(c.rs, c.n, c.e->z.skip_arena);
    if (c.P.raw_min_obs_per_base > 1) { // (k_skip_plan queues nothing otherwise)
        // The three classes own disjoint windows and each is a queue drained by lone wavefronts whose time is
        // one lane's stay recurrence: a kernel is as long as its slowest chain of windows, not as its work.
        // With the side stream the middle class runs beside the big one instead of behind it: 5.0 -> 4.1 ms for
        // the three on cfg4 (tools/skip_timeline.sh; before the kernels' LDS diet 7.5 -> 5.7; all three at once
        // on three streams: 3.7-4.1, no better for the stage).  TBA_SKIP_FORK=0: one after the other, as before
        // round 6.
        static const bool fork_off = getenv("TBA_SKIP_FORK") != nullptr && getenv("TBA_SKIP_FORK")[0] == '0';
        const bool fork = c.side && !fork_off;
        if (fork) {
            HIP_TRY(hipEventRecord(c.e->ev_skip0, c.s));
            HIP_TRY(hipStreamWaitEvent(c.s2, c.e->ev_skip0, 0));
        }
        auto wave = [&](auto k, int cls, unsigned n_blocks, hipStream_t st) { // (the class's list is the cls-th)
            k<<<n_blocks, 64, 0, st>>>(c.rs, c.dp, c.norm, c.refm, c.refs, c.dpsegs, c.segs, c.win, c.skipq, lists + 2 * qcap * cls, qcap);
        };
        wave(k_skip_dp_wave<SKIP_LEN_B, SKIP_BITS_B, 2>, 2, 512, c.s);
        wave(k_skip_dp_wave<SKIP_LEN_M, SKIP_BITS_M, 1>, 1, 1024, fork ? c.s2 : c.s);
        wave(k_skip_dp_wave<SKIP_LEN_S, SKIP_BITS_S, 0>, 0, 2048, c.s);
        if (fork) {
            HIP_TRY(hipEventRecord(c.e->ev_skip1, c.s2));
            HIP_TRY(hipStreamWaitEvent(c.s, c.e->ev_skip1, 0));
        }
    }
    // (raw_min_obs_per_base == 1, DNA: the small windows out of LDS -- k_tail.h)
    (c.P.raw_min_obs_per_base == 1 ? k_skip_dp<true> : k_skip_dp<false>)<<<c.nb, 64, 0, c.s>>>(c.rs, c.dp, c.norm, c.refm, c.refs, c.dpsegs, c.segs, c.win, c.dscr);
    return 0;
}
static int step_theil_sen(Run &c)
{
    k_theil_sen<<<c.nb, SEL_NT, 0, c.s>>>(c.rs, c.dp, c.norm, c.segs, c.refm, c.e->have_samp || c.O.device_subsample ? c.samp : nullptr, c.csum, c.score);
    return 0;
}
static int step_rescale_score(Run &c)
{
    const bool out = !c.O.skip_norm_out;
    (out ? k_rescale_absz<true> : k_rescale_absz<false>)<<<dim3(c.gB, c.nb), 256, 0, c.s>>>(c.rs, c.dp, c.norm, out ? c.norm_out : nullptr, c.segs, c.refm, c.refs, c.absz);
    k_final_score<<<c.nb, 64, 0, c.s>>>(c.rs, c.n, c.absz);
    return 0;
}

// The schedule: step i runs between the events ev[i] and ev[i + 1] of the main stream (timing slot i, named
// here), in a run whose stage range holds its public stage.
static const struct Step { const char *name; int stage; int (*enqueue)(Run &); } STEPS[] = {
    {"normalize", TBA_STAGE_SEGMENT, step_normalize},
    {"cumsum", TBA_STAGE_SEGMENT, step_cumsum},
    {"scores", TBA_STAGE_SEGMENT, step_scores},
    {"peaks", TBA_STAGE_SEGMENT, step_peaks},
    {"event_means", TBA_STAGE_EVENT_MEANS, step_event_means},
    {"ref_levels", TBA_STAGE_REF_LEVELS, step_ref_levels},
    {"start_dp", TBA_STAGE_START, step_start_dp},
    {"start_tb", TBA_STAGE_START, step_start_tb},
    {"prep", TBA_STAGE_ASSIGN, step_prep},
    {"main_dp", TBA_STAGE_ASSIGN, step_main_dp},
    {"main_tb", TBA_STAGE_ASSIGN, step_main_tb},
    {"skip_resolve", TBA_STAGE_SKIP, step_skip_resolve},
    {"theil_sen", TBA_STAGE_RESCALE, step_theil_sen},
    {"rescale_score", TBA_STAGE_RESCALE, step_rescale_score},
};
static_assert(sizeof(STEPS) / sizeof(STEPS[0]) == N_STEP, "one step per timing slot");

// Every event is recorded in every run, whether or not its step runs: tba_batch_sync reads them all.
static int enqueue_stages(tba_engine *e, int first, int last)
{
    if (!e || !e->have_batch) return set_err(TBA_E_STATE, "no batch uploaded");
    if (first < 0 || last > TBA_STAGE_RESCALE || first > last) return set_err(TBA_E_ARG, "bad stage range");
    if (first > 0 && !e->ran) return set_err(TBA_E_STATE, "stages before `first` have not been run or injected");
    HIP_TRY(hipSetDevice(e->device));
    Run c{e};
    if (int rc = run_prelude(c, first, last)) return rc;
    for (int i = 0; i < N_STEP; i++) {
        HIP_TRY(hipEventRecord(e->ev[i], c.s));
        if (STEPS[i].stage >= first && STEPS[i].stage <= last)
            if (int rc = STEPS[i].enqueue(c)) return rc;
    }
    HIP_TRY(hipEventRecord(e->ev[N_STEP], c.s)); // the end of the last step
    HIP_TRY(hipGetLastError());
    e->ran = true;
    e->finished = last == TBA_STAGE_RESCALE;
    return 0;
}

extern "C" int tba_batch_enqueue(tba_engine *e) { return enqueue_stages(e, TBA_STAGE_SEGMENT, TBA_STAGE_RESCALE); }

// The kernels this engine enqueues next start only after `other`'s last enqueued kernel sequence has
// finished (its transfers are not waited for): a streaming caller keeps the kernel sequences of its
// slots back to back instead of interleaved, while their copies still overlap.
extern "C" int tba_batch_wait_for(tba_engine *e, tba_engine *other)
{
    if (!e || !other) return set_err(TBA_E_ARG, "engine is NULL");
    if (!other->ran || e == other) return 0; // nothing enqueued there yet
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamWaitEvent(e->stream, other->ev[N_STEP], 0));
    return 0;
}

extern "C" int tba_batch_run_stages(tba_engine *e, int first_stage, int last_stage)
{
    if (int rc = enqueue_stages(e, first_stage, last_stage)) return rc;
    return tba_batch_sync(e);
}

// inject stage inputs of the uploaded batch (stepwise API): see include/tombo_amd.h
extern "C" int tba_batch_put(tba_engine *e, int what, const void *data, int64_t bytes,
                             const int64_t *per_read)
{
    if (!e || !e->have_batch || !data) return set_err(TBA_E_STATE, "no batch uploaded");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t N = (size_t)e->n_reads;
    auto put = [&](DevBuf &b, size_t cap_bytes) -> int {
        if ((size_t)bytes > cap_bytes) return set_err(TBA_E_ARG, "input larger than the batch buffer");
        HIP_TRY(hipMemcpy(b.p, data, (size_t)bytes, hipMemcpyHostToDevice));
        return 0;
    };
    std::vector<ReadState> rs(N);
    // the first injection of a fresh batch starts from the uploaded state
    if (!e->ran) HIP_TRY(hipMemcpy(e->d_rs.p, e->h_rs.p, N * sizeof(ReadState), hipMemcpyHostToDevice));
    e->ran = true;
    HIP_TRY(hipMemcpy(rs.data(), e->d_rs.p, N * sizeof(ReadState), hipMemcpyDeviceToHost));
    int rc = 0;
    switch (what) {
    case TBA_PUT_VALID_CPTS: // per_read[i] = number of change points of read i
        if (!per_read) return set_err(TBA_E_ARG, "per_read counts required");
        // the kernels index the signal with these values: strictly increasing inside [0, n_raw]
        for (size_t i = 0; i < N; i++) {
            if (per_read[i] > rs[i].num_events || per_read[i] < 2) return set_err(TBA_E_ARG, "change point count outside the reserved space");
            if ((size_t)(rs[i].ev_off + per_read[i]) * 8 > (size_t)bytes) return set_err(TBA_E_ARG, "change point array shorter than the counts");
            const i64 *c = (const i64 *)data + rs[i].ev_off;
            for (i64 k = 0; k < per_read[i]; k++)
                if (c[k] < 0 || c[k] > rs[i].n_raw || (k > 0 && c[k] <= c[k - 1]))
                    return set_err(TBA_E_ARG, "change points must be strictly increasing inside [0, n_raw]");
        }
        rc = put(e->d_cpts, (size_t)e->z.E_tot * 8);
        for (size_t i = 0; i < N && !rc; i++) { rs[i].n_cpts = per_read[i]; rs[i].n_ev = per_read[i] - 1; }
        break;
    case TBA_PUT_EVENT_MEANS: rc = put(e->d_evm, (size_t)e->z.E_tot * 8); break;
    case TBA_PUT_NORM: rc = put(e->d_norm, (size_t)e->z.S_tot * 8); break;
    case TBA_PUT_REF_MEANS: rc = put(e->d_refm, (size_t)e->z.B_tot * 8); break;
    case TBA_PUT_REF_SDS: rc = put(e->d_refs, (size_t)e->z.B_tot * 8); e->refs_put = true; break; // (dp_cdiv: any divisor now)
    case TBA_PUT_DP_SEGS: // per_read[2i] = read_start_rel_to_raw, per_read[2i+1] = trimmed signal length
        if (!per_read) return set_err(TBA_E_ARG, "per_read (read_start, norm_len) required");
        if ((size_t)bytes < e->n_segs() * 8) return set_err(TBA_E_ARG, "segment array shorter than the batch");
        for (size_t i = 0; i < N; i++) { // boundaries index the signal: non-decreasing inside [0, norm_len]
            const i64 rstart = per_read[2 * i], nl = per_read[2 * i + 1];
            if (rstart < 0 || nl < 0 || rstart + nl > rs[i].n_raw) return set_err(TBA_E_ARG, "segments outside the signal");
            const i64 *sg = (const i64 *)data + rs[i].seg_off;
            for (i64 k = 0; k <= rs[i].B; k++)
                if (sg[k] < 0 || sg[k] > nl || (k > 0 && sg[k] < sg[k - 1]))
                    return set_err(TBA_E_ARG, "segment boundaries must be non-decreasing inside [0, norm_len]");
        }
        rc = put(e->d_dpsegs, e->n_segs() * 8);
        for (size_t i = 0; i < N && !rc; i++) {
            rs[i].read_start = rs[i].dp_read_start = per_read[2 * i];
            rs[i].norm_len = per_read[2 * i + 1];
        }
        break;
    case TBA_PUT_START_STATE: // per_read[i]: 4 = force the static whole-read path
        if (!per_read) return set_err(TBA_E_ARG, "per_read states required");
        for (size_t i = 0; i < N; i++) rs[i].start_state = (i32)per_read[i];
        break;
    default: return set_err(TBA_E_ARG, "unknown TBA_PUT_* selector");
    }
    if (rc) return rc;
    HIP_TRY(hipMemcpy(e->d_rs.p, rs.data(), N * sizeof(ReadState), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int tba_batch_sync(tba_engine *e)
{
    if (!e) return set_err(TBA_E_ARG, "engine is NULL");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->ran) {
        memset(e->stage_ms, 0, sizeof(e->stage_ms));
        for (int i = 0; i < N_STEP; i++) (void)hipEventElapsedTime(&e->stage_ms[i], e->ev[i], e->ev[i + 1]);
        (void)hipEventElapsedTime(&e->stage_ms[SLOT_STALLS], e->ev_st0, e->ev_st1); // stall detection (side stream: overlaps the steps above)
        (void)hipEventElapsedTime(&e->stage_ms[SLOT_TOTAL], e->ev[SLOT_TOTAL], e->ev[N_STEP]);
    }
    return 0;
}

extern "C" int tba_batch_run(tba_engine *e) { return tba_batch_run_stages(e, TBA_STAGE_SEGMENT, TBA_STAGE_RESCALE); }

extern "C" int tba_batch_download(tba_engine *e, int32_t *status, int64_t *segs,
                                  int64_t *read_start_rel_to_raw, double *norm_signal,
                                  int64_t *norm_len, double *scale_values,
                                  double *sig_match_score, int32_t *norm_params_changed)
{
    if (!e || !e->ran) return set_err(TBA_E_STATE, "no batch has been run");
    if (norm_signal && e->hp.o.skip_norm_out)
        return set_err(TBA_E_STATE, "the batch was run with skip_norm_out: there is no normalised signal to download");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t N = (size_t)e->n_reads;
    std::vector<ReadState> rs(N);
    HIP_TRY(hipMemcpy(rs.data(), e->d_rs.p, N * sizeof(ReadState), hipMemcpyDeviceToHost));
    if (segs) HIP_TRY(hipMemcpy(segs, e->d_segs.p, e->n_segs() * 8, hipMemcpyDeviceToHost));
    if (norm_signal) HIP_TRY(hipMemcpy(norm_signal, e->d_norm_out.p, (size_t)e->z.S_tot * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; i++) {
        const ReadState &r = rs[i];
        if (status) status[i] = r.status;
        if (read_start_rel_to_raw) read_start_rel_to_raw[i] = r.read_start;
        if (norm_len) norm_len[i] = r.status == TBA_OK ? r.norm_len : 0;
        if (scale_values) {
            scale_values[4 * i + 0] = r.shift; scale_values[4 * i + 1] = r.scale;
            scale_values[4 * i + 2] = r.has_lims ? r.lower : NAN;
            scale_values[4 * i + 3] = r.has_lims ? r.upper : NAN;
        }
        if (sig_match_score) sig_match_score[i] = r.score;
        if (norm_params_changed) norm_params_changed[i] = r.changed;
    }
    return 0;
}

// per-read records + int32 boundaries, packed on the device so that the download is a few
// contiguous copies (grid: (blocks, reads))
__global__ __launch_bounds__(256) void k_pack_results(const ReadState *rs, const i64 *segs,
    tba_read_result *res, i32 *segs32)
{
    const ReadState &r = rs[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        tba_read_result o;
        o.status = r.status; o.norm_params_changed = r.changed;
        o.read_start_rel_to_raw = r.read_start;
        o.norm_len = r.status == TBA_OK ? r.norm_len : 0;
        o.shift = r.shift; o.scale = r.scale;
        o.lower_lim = r.has_lims ? r.lower : NAN;
        o.upper_lim = r.has_lims ? r.upper : NAN;
        o.sig_match_score = r.score;
        res[blockIdx.y] = o;
    }
    if (segs32 == nullptr) return;
    const i64 *sg = segs + r.seg_off;
    i32 *o32 = segs32 + r.seg_off;
    const bool ok = r.status == TBA_OK;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i <= r.B; i += (i64)gridDim.x * 256)
        o32[i] = ok ? (i32)sg[i] : 0;
}

extern "C" int tba_batch_download_async(tba_engine *e, tba_read_result *results, int32_t *segs32,
                                        int64_t *segs64, double *norm_signal)
{
    if (!e || !e->ran) return set_err(TBA_E_STATE, "no batch has been run");
    if (norm_signal && e->hp.o.skip_norm_out)
        return set_err(TBA_E_STATE, "the batch was run with skip_norm_out: there is no normalised signal to download");
    if (segs32 && e->z.max_raw > 0x7fffffffll) return set_err(TBA_E_ARG, "signal too long for int32 boundaries");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t N = (size_t)e->n_reads;
    const unsigned gB = (unsigned)std::min<i64>(std::max<i64>((e->z.max_B + 1 + 255) / 256, 1), 64);
    if (results || segs32) {
        k_pack_results<<<dim3(segs32 ? gB : 1, (unsigned)N), 256, 0, s>>>(e->d_rs.as<ReadState>(),
            e->d_segs.as<i64>(), e->d_res.as<tba_read_result>(), segs32 ? e->d_segs32.as<i32>() : nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (results) HIP_TRY(hipMemcpyAsync(results, e->d_res.p, N * sizeof(tba_read_result), hipMemcpyDeviceToHost, s));
    if (segs32) HIP_TRY(hipMemcpyAsync(segs32, e->d_segs32.p, e->n_segs() * 4, hipMemcpyDeviceToHost, s));
    if (segs64) HIP_TRY(hipMemcpyAsync(segs64, e->d_segs.p, e->n_segs() * 8, hipMemcpyDeviceToHost, s));
    if (norm_signal) HIP_TRY(hipMemcpyAsync(norm_signal, e->d_norm_out.p, (size_t)e->z.S_tot * 8, hipMemcpyDeviceToHost, s));
    return 0;
}

extern "C" int tba_batch_query(tba_engine *e)
{
    if (!e) return set_err(TBA_E_ARG, "engine is NULL");
    HIP_TRY(hipSetDevice(e->device));
    const hipError_t rc = hipStreamQuery(e->stream);
    if (rc == hipSuccess) return 0;
    if (rc == hipErrorNotReady) return 1;
    return set_err(TBA_E_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(rc));
}

template <class T, size_t K> static std::array<T, K> to_array(const T (&a)[K])
{
    std::array<T, K> v;
    std::copy(a, a + K, v.begin());
    return v;
}

extern "C" int tba_batch_get(tba_engine *e, int what, void *out, int64_t out_bytes)
{
    if (!e || !e->ran || !out) return set_err(TBA_E_STATE, "no batch has been run");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t N = (size_t)e->n_reads;
    auto copy = [&](const DevBuf &b, size_t bytes) -> int {
        if ((size_t)out_bytes < bytes) return set_err(TBA_E_ARG, "output buffer too small");
        HIP_TRY(hipMemcpy(out, b.p, bytes, hipMemcpyDeviceToHost));
        return 0;
    };
    switch (what) {
    case TBA_GET_VALID_CPTS: return copy(e->d_cpts, (size_t)e->z.E_tot * 8);
    case TBA_GET_EVENT_MEANS: return copy(e->d_evm, (size_t)e->z.E_tot * 8);
    case TBA_GET_SEG_NORM: return copy(e->d_norm, (size_t)e->z.S_tot * 8);
    case TBA_GET_ED_TAKEN_POS: return copy(e->d_score, (size_t)e->z.S_tot * 8);
    case TBA_GET_BAND_STARTS: return copy(e->d_bst, (size_t)e->z.B_tot * 8);
    case TBA_GET_READ_TB: return copy(e->d_readtb, e->n_segs() * 8);
    case TBA_GET_DP_SEGS: return copy(e->d_dpsegs, e->n_segs() * 8);
    case TBA_GET_LAST_ROW: return copy(e->d_lastrow, N * TBA_MAX_BAND * 8);
    case TBA_GET_REF_MEANS: return copy(e->d_refm, (size_t)e->z.B_tot * 8);
    case TBA_GET_REF_SDS: return copy(e->d_refs, (size_t)e->z.B_tot * 8);
    case TBA_GET_SEGS: return copy(e->d_segs, e->n_segs() * 8);
    case TBA_GET_SAMP_IND: return copy(e->d_samp, N * MAX_TS_POINTS * 8);
    case TBA_GET_STALL_INTS:
        if (!e->any_stall) return set_err(TBA_E_STATE, "the batch has no stall intervals");
        // (the caller sizes `out` by the intervals in use: max(STALL_OFF + N_STALL))
        return copy(e->d_stall, std::min((size_t)e->z.n_stall * 16, (size_t)out_bytes));
    case TBA_GET_KERNEL_MS:
        if ((size_t)out_bytes < sizeof(e->stage_ms)) return set_err(TBA_E_ARG, "output buffer too small");
        memcpy(out, e->stage_ms, sizeof(e->stage_ms));
        return 0;
    default: break;
    }
    std::vector<ReadState> rs(N);
    HIP_TRY(hipMemcpy(rs.data(), e->d_rs.p, N * sizeof(ReadState), hipMemcpyDeviceToHost));
    // the per-read selectors: one T per read, from the read's ReadState `r`
    auto per_read = [&](auto get) -> int {
        typedef decltype(get(rs[0])) T;
        if ((size_t)out_bytes < N * sizeof(T)) return set_err(TBA_E_ARG, "output buffer too small");
        for (size_t i = 0; i < N; i++) {
            const T v = get(rs[i]);
            memcpy((char *)out + i * sizeof(T), &v, sizeof(T));
        }
        return 0;
    };
#define PER_READ(T, ...) per_read([](const ReadState &r) -> T { return __VA_ARGS__; })
    typedef std::array<double, 4> D4;
    typedef std::array<i32, 4> I4;
    typedef std::array<i32, 2> I2;
    typedef std::array<i64, 8> I8;
    switch (what) {
    case TBA_GET_START_FAIL: return PER_READ(i32, r.pad0);
    case TBA_GET_STATUS: return PER_READ(i32, r.status);
    // (by the form the kernels recorded, not by the absence of a flag)
    case TBA_GET_ED_FUSED: return PER_READ(i32, r.ed_form == TBA_ED_FORM_DETECT_PICK || r.ed_form == TBA_ED_FORM_DETECT_TT_PICK);
    case TBA_GET_TB_PARALLEL: return PER_READ(i32, r.tb_done);
    case TBA_GET_ED_FORM: return PER_READ(i32, r.ed_form);
    case TBA_GET_TB_FORM: return PER_READ(i32, r.tb_form);
    case TBA_GET_NORM_FORM: return PER_READ(i32, r.norm_form);
    case TBA_GET_TB_VERIFY_FAIL: return PER_READ(i32, r.tb_verify_fail);
    case TBA_GET_DP_WORKGROUP: return PER_READ(i32, r.dp_wg);
    case TBA_GET_ED_N_TAKEN: return PER_READ(i64, r.n_taken);
    case TBA_GET_N_CPTS: return PER_READ(i64, r.n_cpts);
    case TBA_GET_DP_READ_START: return PER_READ(i64, r.dp_read_start);
    case TBA_GET_N_STALL: return PER_READ(i64, r.n_stall);
    case TBA_GET_STALL_OFF: return PER_READ(i64, r.stall_off);
    case TBA_GET_SEG_SV: return PER_READ(D4, D4{r.shift, r.scale, r.lower, r.upper});
    case TBA_GET_START: return PER_READ(D4, to_array(r.start_res));
    case TBA_GET_THEIL_SEN: return PER_READ(D4, to_array(r.ts));
    case TBA_GET_TS_FORM: return PER_READ(I2, to_array(r.ts_form));
    case TBA_GET_PATH: return PER_READ(I4, I4{r.path, (i32)r.n_static, (i32)r.W, r.n_start_calls});
    case TBA_GET_DEBUG_COUNTERS: return PER_READ(I8, to_array(r.dbg)); // phase cycle / sweep counters of a profiling build
    case TBA_GET_DP_FORM: {
        // Derived: what the steps of the last run launched (last_dp), and per read the kernels' own selection predicates over the
        // state the run left -- k_prep / k_scan_arena leave a path only on reads that go into the main pass,
        // and nothing after start discovery touches start_state, n_start_calls or the first try's failure.
        const tba_params &P = e->hp.p;
        const tba_engine::DpLaunches L = e->last_dp;
        const int multi_cpl = dp_multi_class(P.bandwidth).cpl;
        const int retry_cpl = L.retry_wcpl ? L.retry_wcpl : cpl_class(P.start_save_bw);
        return per_read([&](const ReadState &r) -> I4 {
            I4 f{TBA_DP_FORM_NONE, 0, TBA_DP_START_NONE, 0};
            if (L.main && r.path != PATH_NONE) {
                const int c = cpl_class(r.W);
                if (r.path == PATH_ADAPTIVE && r.W == P.bandwidth && multi_cpl != 0) // k_dp_multi.h:89, k_dp.h:296
                    f[0] = TBA_DP_FORM_MULTI, f[1] = multi_cpl;
                else if (c != 0)                                                     // k_dp.h:294
                    f[0] = c == 8 && L.lowreg ? TBA_DP_FORM_K_DP8_LOWREG : TBA_DP_FORM_K_DP, f[1] = c;
                else if (r.path == PATH_STATIC && L.wide)                            // k_dp.h:789
                    f[0] = TBA_DP_FORM_WIDE;
            }
            // the retry took the reads in ST_RETRY (k_dp.h:304, k_dp_wg.h:34): it left ST_OK and two calls, or
            // its status and the state as it was; the first try those in ST_TRY: one call, the reason it failed
            // (TBA_GET_START_FAIL), or -- an internal error -- the state as it was
            const bool retried = r.n_start_calls == 2 || r.start_state == ST_RETRY;
            const bool tried = retried || r.n_start_calls == 1 || r.pad0 != 0 || r.start_state == ST_TRY;
            if (L.start && retried)
                f[2] = L.retry_wcpl ? TBA_DP_START_RETRY_WG : TBA_DP_START_RETRY_K_DP, f[3] = retry_cpl;
            else if (L.start && tried)
                f[2] = TBA_DP_START_FIRST_TRY;
            return f;
        });
    }
    case TBA_GET_DP_ONE_SD: {
        // Derived like TBA_GET_DP_FORM, whose predicates these are: the reads a k_dp launch of the last run took, where
        // that launch was k_dp_c1
        const tba_params &P = e->hp.p;
        const tba_engine::DpLaunches L = e->last_dp;
        const int multi_cpl = dp_multi_class(P.bandwidth).cpl;
        return per_read([&](const ReadState &r) -> I2 {
            I2 f{0, 0};
            if (L.main && L.c1_main && r.path != PATH_NONE && cpl_class(r.W) != 0 &&
                !(r.path == PATH_ADAPTIVE && r.W == P.bandwidth && multi_cpl != 0)) f[0] = 1;
            const bool retried = r.n_start_calls == 2 || r.start_state == ST_RETRY;
            const bool tried = retried || r.n_start_calls == 1 || r.pad0 != 0 || r.start_state == ST_TRY;
            if (L.start && tried && L.c1_start) f[1] |= 1;
            if (L.start && retried && L.c1_retry) f[1] |= 2;
            return f;
        });
    }
    default: break;
    }
#undef PER_READ
    return set_err(TBA_E_ARG, "unknown TBA_GET_* selector");
}

// workgroups per read of the per-base kernels over a finished batch
static unsigned base_blocks(const tba_engine *e) { return (unsigned)std::min<i64>(std::max<i64>((e->z.max_B + 255) / 256, 1), 128); }

// per-base means and stds of the final signal into e->d_stat (B_tot means, then B_tot stds)
static int launch_base_stats(tba_engine *e)
{
    if (e->d_stat.ensure((size_t)e->z.B_tot * 16)) return set_err(TBA_E_NOMEM, "hipMalloc failed");
    double *d_m = e->d_stat.as<double>();
    k_base_stats<<<dim3(base_blocks(e), (unsigned)e->n_reads), 256, 0, e->stream>>>(e->d_rs.as<ReadState>(),
        e->d_dp.as<DevParams>(), e->hp.o.skip_norm_out ? nullptr : e->d_norm_out.as<double>(),
        e->d_norm.as<double>(), e->d_segs.as<i64>(), d_m, d_m + e->z.B_tot);
    return 0;
}

extern "C" int tba_batch_base_stats(tba_engine *e, double *means, double *stds, int64_t n_values)
{
    if (!e || !e->have_batch || !e->finished) return set_err(TBA_E_STATE, "no finished batch");
    if (!means || !stds || n_values < e->z.B_tot) return set_err(TBA_E_ARG, "output buffers too small");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->z.B_tot == 0) return 0;
    if (int rc = launch_base_stats(e)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    const double *d_m = e->d_stat.as<double>();
    HIP_TRY(hipMemcpy(means, d_m, (size_t)e->z.B_tot * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(stds, d_m + e->z.B_tot, (size_t)e->z.B_tot * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tba_batch_stats(tba_engine *e, double *algorithmic_bytes, double *dp_cells)
{
    if (!e || !e->have_batch) return set_err(TBA_E_STATE, "no batch uploaded");
    if (algorithmic_bytes) *algorithmic_bytes = e->z.algo_bytes;
    if (dp_cells) *dp_cells = e->z.cells;
    return 0;
}

extern "C" const char *tba_stage_name(int i) { return i < 0 || i >= N_STAGE ? "" : i < N_STEP ? STEPS[i].name : i == SLOT_STALLS ? "stalls" : "total"; }

// ---------------------------------------------------------------------------------------------
// per-kernel entry points (tba_c_*): host buffers in, host buffers out, batch of one
namespace {
// The device scratch of one call on its engine's device and stream, freed on return.  The first
// failure is kept (its code in `rc`, its message through set_err) and turns every later step into
// a no-op, so an entry checks `rc` once, after its buffers.  Copies block: inputs are on the device
// before the launches that read them, outputs are read back after sync().
struct Scratch {
    int rc = 0;
    hipStream_t stream;
    std::vector<void *> bufs;
    explicit Scratch(tba_engine *e) : stream(e->stream) { hip(hipSetDevice(e->device), "hipSetDevice(e->device)"); }
    ~Scratch() { for (void *p : bufs) (void)hipFree(p); }
    int hip(hipError_t err, const char *what)
    {
        if (err != hipSuccess && !rc) rc = set_err(TBA_E_HIP, std::string(what) + ": " + hipGetErrorString(err));
        return rc;
    }
    // n elements of T (at least 8 bytes); NULL after a failure
    template <class T> T *out(size_t n)
    {
        void *p = nullptr;
        if (rc) return nullptr;
        if (hipMalloc(&p, std::max<size_t>(n * sizeof(T), 8)) != hipSuccess) {
            rc = set_err(TBA_E_NOMEM, "hipMalloc failed");
            return nullptr;
        }
        bufs.push_back(p);
        return (T *)p;
    }
    // n elements copied in from the host, followed by `pad` zeroed bytes; n == 0 never touches `host`
    template <class T> T *in(const T *host, size_t n, size_t pad = 0)
    {
        char *p = out<char>(n * sizeof(T) + pad);
        if (p && pad) hip(hipMemset(p + n * sizeof(T), 0, pad), "hipMemset");
        if (p && n && !rc) hip(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
        return rc ? nullptr : (T *)p;
    }
    // `bytes` of p zeroed on the stream, before the launches that follow; returns rc
    int zero(void *p, size_t bytes)
    {
        return rc || !p ? rc : hip(hipMemsetAsync(p, 0, bytes, stream), "hipMemsetAsync");
    }
    // a zeroed status word for a kernel of k_cabi.h that reports one (read back by sync)
    i32 *status()
    {
        i32 *p = out<i32>(1);
        zero(p, 4);
        return p;
    }
    // after the launches: their errors, then the stream.  Returns rc after a failure, else the
    // status word (0 without one).
    int sync(const i32 *d_status = nullptr)
    {
        if (rc || hip(hipGetLastError(), "hipGetLastError") || hip(hipStreamSynchronize(stream), "hipStreamSynchronize")) return rc;
        i32 st = 0;
        if (d_status && get(&st, d_status, 1)) return rc;
        return st;
    }
    // n elements back to the host (after sync); returns rc
    template <class T> int get(T *host, const T *dev, size_t n)
    {
        return rc ? rc : hip(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy");
    }
};

// Kernel time of one span of launches on the call's stream: from construction to stop(), through
// two events made for the call and destroyed with it.  Switched off, or after a failure in `sc`,
// every step is a no-op and ms() is 0.
struct KernelTimer {
    Scratch &sc;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool stopped = false;
    explicit KernelTimer(Scratch &sc_, bool on = true) : sc(sc_)
    {
        if (!on || sc.rc || sc.hip(hipEventCreate(&ev0), "hipEventCreate") || sc.hip(hipEventCreate(&ev1), "hipEventCreate")) return;
        sc.hip(hipEventRecord(ev0, sc.stream), "hipEventRecord");
    }
    ~KernelTimer() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }
    void stop() { stopped = ev1 && !sc.rc && !sc.hip(hipEventRecord(ev1, sc.stream), "hipEventRecord"); }
    // the span's time; waits for its end, so it is safe before sc.sync() too (and costs nothing after it)
    double ms()
    {
        float t = 0;
        if (!stopped || sc.rc || hipEventSynchronize(ev1) != hipSuccess || hipEventElapsedTime(&t, ev0, ev1) != hipSuccess) return 0.0;
        return t;
    }
};
static unsigned grid_for(i64 n) { return (unsigned)std::min<i64>(std::max<i64>((n + 255) / 256, 1), 4096); }

static void launch_direct(tba_engine *e, int cpl, DpJob *job)
{
    DpClasses::dispatch(cpl, [&](auto c) {
        k_dp<decltype(c)::value, true><<<dim3(1), dim3(64), 0, e->stream>>>(
            e->d_rs.as<ReadState>(), e->d_dp.as<DevParams>(), DP_DIRECT, nullptr, nullptr, nullptr,
            nullptr, nullptr, nullptr, nullptr, 0, nullptr, job);
    });
}

// shared by the two forward-pass entry points
static int run_direct_dp(tba_engine *e, DpJob hj, int cpl, i64 n_rows, i64 W, i64 row0,
                         double *fwd_host, int64_t *tb_host, int64_t *starts_host, i64 starts_from,
                         int64_t *top_pos_host = nullptr)
{
    const i64 stride = (i64)cpl * 64;            // forward rows
    const i64 mstride = mv_class_rowb(cpl);      // packed 2-bit move rows
    Scratch sc(e);
    double *d_fwd = sc.out<double>((size_t)(n_rows + 1) * stride);
    unsigned char *d_mv = sc.out<unsigned char>((size_t)(n_rows + 1) * mstride);
    hj.fwd_out = d_fwd;
    hj.mv = d_mv;
    hj.status = TBA_OK;
    DpJob *d_job = sc.in(&hj, 1);
    if (sc.rc) return sc.rc;
    // the kernel needs *some* ReadState / DevParams to bind its references to
    if (e->d_rs.ensure(sizeof(ReadState)) || e->d_dp.ensure(sizeof(DevParams))) return TBA_E_NOMEM;
    launch_direct(e, cpl, d_job);
    if (sc.sync() || sc.get(&hj, d_job, 1)) return sc.rc;
    if (hj.status != TBA_OK) return hj.status;
    if (top_pos_host) *top_pos_host = hj.top_pos;
    std::vector<unsigned char> mv((size_t)(n_rows + 1) * mstride);
    std::vector<double> fw((size_t)(n_rows + 1) * stride);
    if (sc.get(mv.data(), d_mv, mv.size()) || sc.get(fw.data(), d_fwd, fw.size())) return sc.rc;
    // rows row0+1 .. n_rows are new (row 0 too when starting from scratch); device rows are
    // padded to the moves stride
    for (i64 r = row0 == 0 ? 0 : row0 + 1; r <= n_rows; r++)
        memcpy(fwd_host + r * W, fw.data() + r * stride, (size_t)W * 8);
    for (i64 r = row0 + 1; r <= n_rows; r++)
        for (i64 b = 0; b < W; b++)
            tb_host[r * W + b] = (mv[(size_t)(r * mstride + (b >> 2))] >> (2 * (b & 3))) & 3;
    if (starts_host) return sc.get(starts_host + starts_from, hj.starts + starts_from, (size_t)(n_rows - starts_from));
    return TBA_OK;
}

// boundaries of n_segs segments: non-decreasing inside [0, n_sig]
static int check_segs(const int64_t *segs, i64 n_segs, i64 n_sig)
{
    for (i64 i = 0; i <= n_segs; i++)
        if (segs[i] < 0 || segs[i] > n_sig || (i > 0 && segs[i] < segs[i - 1]))
            return set_err(TBA_E_ARG, "segment boundaries outside the signal");
    return 0;
}
} // namespace

extern "C" int tba_c_adaptive_banded_forward_pass_z(tba_engine *e, double *fwd_pass,
    int64_t *fwd_pass_tb, int64_t n_bases, int64_t bandwidth, int64_t *event_starts,
    const double *event_means, int64_t n_events, const double *r_ref_means,
    const double *r_ref_sds, double z_shift, double skip_pen, double stay_pen,
    int64_t start_seq_pos, double mask_fill_z_score, int do_winsorize_z, double max_half_z_score,
    double *z_scores)
{
    if (!e || !fwd_pass || !fwd_pass_tb || !event_starts || !event_means || !r_ref_means ||
        !r_ref_sds || n_bases < 1 || bandwidth < 2 || start_seq_pos < 1 || start_seq_pos > n_bases)
        return set_err(TBA_E_ARG, "bad arguments");
    const int cpl = cpl_class(bandwidth);
    if (!cpl) return TBA_UNSUPPORTED;
    if (n_events < 1) return set_err(TBA_E_ARG, "no events");
    for (i64 i = 0; i < start_seq_pos; i++) // the given (static) rows' band starts index the events
        if (event_starts[i] < 0 || event_starts[i] >= n_events || (i > 0 && event_starts[i] < event_starts[i - 1]))
            return set_err(TBA_E_ARG, "event_starts must be non-decreasing inside [0, n_events)");
    const size_t n_z = (size_t)(n_bases - start_seq_pos) * (size_t)bandwidth;
    DpJob j;
    memset(&j, 0, sizeof(j));
    Scratch sc(e);
    j.z_out = z_scores && n_z ? sc.out<double>(n_z) : nullptr;
    j.ev = sc.in(event_means, n_events);
    j.mu = sc.in(r_ref_means, n_bases);
    j.sd = sc.in(r_ref_sds, n_bases);
    j.starts = sc.in(event_starts, n_bases);
    j.init_row = sc.in(fwd_pass + start_seq_pos * bandwidth, bandwidth);
    if (sc.rc) return sc.rc;
    j.W = bandwidth; j.n_rows = n_bases; j.row0 = start_seq_pos; j.n_static = start_seq_pos;
    j.n_ev = n_events; j.zmat = nullptr;
    j.z_shift = z_shift; j.skip_pen = skip_pen; j.stay_pen = stay_pen; j.max_half_z = max_half_z_score;
    j.fill = mask_fill_z_score; j.winsor = do_winsorize_z ? 1 : 0;
    const int rc = run_direct_dp(e, j, cpl, n_bases, bandwidth, start_seq_pos, fwd_pass, fwd_pass_tb,
                                 event_starts, start_seq_pos);
    if (rc == TBA_OK && j.z_out) return sc.get(z_scores, j.z_out, n_z);
    return rc;
}

extern "C" int tba_c_adaptive_banded_forward_pass(tba_engine *e, double *fwd_pass,
    int64_t *fwd_pass_tb, int64_t n_bases, int64_t bandwidth, int64_t *event_starts,
    const double *event_means, int64_t n_events, const double *r_ref_means,
    const double *r_ref_sds, double z_shift, double skip_pen, double stay_pen,
    int64_t start_seq_pos, double mask_fill_z_score, int do_winsorize_z, double max_half_z_score)
{
    return tba_c_adaptive_banded_forward_pass_z(e, fwd_pass, fwd_pass_tb, n_bases, bandwidth, event_starts,
        event_means, n_events, r_ref_means, r_ref_sds, z_shift, skip_pen, stay_pen, start_seq_pos,
        mask_fill_z_score, do_winsorize_z, max_half_z_score, nullptr);
}


extern "C" int tba_c_banded_forward_pass(tba_engine *e, const double *shifted_z_scores,
    int64_t n_bases, int64_t bandwidth, const int64_t *event_starts, double skip_pen,
    double stay_pen, double *fwd_pass, int64_t *fwd_pass_tb)
{
    if (!e || !shifted_z_scores || !event_starts || !fwd_pass || !fwd_pass_tb || n_bases < 1 ||
        bandwidth < 2)
        return set_err(TBA_E_ARG, "bad arguments");
    const int cpl = cpl_class(bandwidth);
    if (!cpl) return TBA_UNSUPPORTED;
    for (i64 i = 0; i < n_bases; i++)
        if (event_starts[i] < 0 || (i > 0 && event_starts[i] < event_starts[i - 1]))
            return set_err(TBA_E_ARG, "event_starts must be non-negative and non-decreasing");
    DpJob j;
    memset(&j, 0, sizeof(j));
    Scratch sc(e);
    j.zmat = sc.in(shifted_z_scores, (size_t)n_bases * bandwidth);
    j.starts = sc.in(event_starts, n_bases);
    if (sc.rc) return sc.rc;
    j.W = bandwidth; j.n_rows = n_bases; j.row0 = 0; j.n_static = n_bases; j.n_ev = 0;
    j.init_row = nullptr;
    j.skip_pen = skip_pen; j.stay_pen = stay_pen;
    int rc = run_direct_dp(e, j, cpl, n_bases, bandwidth, 0, fwd_pass, fwd_pass_tb, nullptr, 0);
    if (rc == TBA_OK) // row 0 of the move matrix is never read; the reference leaves it empty
        for (i64 b = 0; b < bandwidth; b++) fwd_pass_tb[b] = 0;
    return rc;
}

// The forward pass over a given z matrix with adaptive rows behind the static ones: k_dp<CPL, true>'s zmat form
// with n_static < n_rows (a row's band cells are its z row whatever its start; the start moves the previous row)
extern "C" int tba_c_banded_forward_pass_adaptive(tba_engine *e, const double *shifted_z_scores,
    int64_t n_bases, int64_t bandwidth, int64_t *event_starts, int64_t n_static, int64_t n_events,
    double skip_pen, double stay_pen, double *fwd_pass, int64_t *fwd_pass_tb, int64_t *top_pos)
{
    if (!e || !shifted_z_scores || !event_starts || !fwd_pass || !fwd_pass_tb || !top_pos || n_bases < 1 ||
        bandwidth < 2 || n_static < 1 || n_static > n_bases || n_events < 1 || n_events > 0x7fffffff)
        return set_err(TBA_E_ARG, "bad arguments");
    const int cpl = cpl_class(bandwidth);
    if (!cpl) return TBA_UNSUPPORTED;
    for (i64 i = 0; i < n_static; i++)
        if (event_starts[i] < 0 || event_starts[i] >= n_events || (i > 0 && event_starts[i] < event_starts[i - 1]))
            return set_err(TBA_E_ARG, "event_starts must be non-decreasing inside [0, n_events)");
    DpJob j;
    memset(&j, 0, sizeof(j));
    Scratch sc(e);
    j.zmat = sc.in(shifted_z_scores, (size_t)n_bases * bandwidth);
    j.starts = sc.in(event_starts, n_bases);
    if (sc.rc) return sc.rc;
    j.W = bandwidth; j.n_rows = n_bases; j.row0 = 0; j.n_static = n_static; j.n_ev = n_events;
    j.init_row = nullptr;
    j.skip_pen = skip_pen; j.stay_pen = stay_pen;
    int rc = run_direct_dp(e, j, cpl, n_bases, bandwidth, 0, fwd_pass, fwd_pass_tb, event_starts, n_static, top_pos);
    if (rc == TBA_OK)
        for (i64 b = 0; b < bandwidth; b++) fwd_pass_tb[b] = 0;
    return rc;
}

extern "C" int tba_c_banded_traceback(tba_engine *e, const int64_t *fwd_pass_tb, int64_t n_bases,
    int64_t bandwidth, const int64_t *event_starts, int64_t band_pos,
    int64_t band_boundary_thresh, int64_t *seq_poss)
{
    if (!e || !fwd_pass_tb || !event_starts || !seq_poss || n_bases < 1 || bandwidth < 1 ||
        band_pos < 0 || band_pos >= bandwidth)
        return set_err(TBA_E_ARG, "bad arguments");
    const size_t cells = (size_t)(n_bases + 1) * bandwidth;
    std::vector<unsigned char> mv(cells);
    for (size_t i = 0; i < cells; i++) mv[i] = (unsigned char)fwd_pass_tb[i];
    Scratch sc(e);
    const unsigned char *d_mv = sc.in(mv.data(), cells);
    const i64 *d_st = sc.in(event_starts, n_bases);
    i64 *d_out = sc.out<i64>(n_bases + 1);
    i32 *d_status = sc.status();
    if (sc.rc) return sc.rc;
    k_c_traceback<<<1, 64, 0, e->stream>>>(d_mv, bandwidth, n_bases, bandwidth, d_st, band_pos,
                                           band_boundary_thresh, d_out, d_status);
    const int st = sc.sync(d_status);
    if (st == TBA_OK) return sc.get(seq_poss, d_out, n_bases + 1);
    return st;
}

extern "C" int tba_c_base_z_scores(tba_engine *e, const double *b_sig, int64_t n, double ref_mean,
    double ref_sd, int do_winsorize_z, double max_half_z_score, double *out)
{
    if (!e || !b_sig || !out || n < 0) return set_err(TBA_E_ARG, "bad arguments");
    if (n == 0) return TBA_OK;
    Scratch sc(e);
    const double *d_in = sc.in(b_sig, n);
    double *d_out = sc.out<double>(n);
    if (sc.rc) return sc.rc;
    k_c_base_z_scores<<<grid_for(n), 256, 0, e->stream>>>(d_in, n, ref_mean, ref_sd,
                                                          do_winsorize_z, max_half_z_score, d_out);
    if (sc.sync()) return sc.rc;
    return sc.get(out, d_out, n);
}

extern "C" int tba_c_new_means(tba_engine *e, const double *norm_signal, int64_t n_sig,
    const int64_t *new_segs, int64_t n_segs, double *means)
{
    if (!e || !norm_signal || !new_segs || !means || n_segs < 0 || n_sig < 0)
        return set_err(TBA_E_ARG, "bad arguments");
    if (n_segs == 0) return TBA_OK;
    if (int rc = check_segs(new_segs, n_segs, n_sig)) return rc;
    // the batch pipeline's own kernel on a one-read batch (k_event_means: wave-cooperative, software-
    // pipelined segment sums, k_select.h) -- the slice size picked as the batch pipeline picks it,
    // by the mean segment length (+ 64 bytes: a 16-byte access may touch the element past an odd end)
    ReadState r;
    memset(&r, 0, sizeof(r));
    r.n_raw = n_sig; r.n_cpts = n_segs + 1; r.status = TBA_OK;
    DevParams dp;
    memset(&dp, 0, sizeof(dp));
    Scratch sc(e);
    const double *d_sig = sc.in(norm_signal, n_sig, 64);
    const i64 *d_segs = sc.in(new_segs, n_segs + 1);
    double *d_out = sc.out<double>(n_segs);
    ReadState *d_rs = sc.in(&r, 1);
    const DevParams *d_dp = sc.in(&dp, 1);
    if (sc.rc) return sc.rc;
    const unsigned g = (unsigned)std::min<i64>(std::max<i64>((n_segs + 255) / 256, 1), 128);
    if (n_sig >= 10 * n_segs)
        k_event_means<double, 1280><<<dim3(g, 1), 256, 0, e->stream>>>(d_rs, d_dp, d_sig, d_segs, d_out, 0);
    else
        k_event_means<double><<<dim3(g, 1), 256, 0, e->stream>>>(d_rs, d_dp, d_sig, d_segs, d_out, 0);
    if (sc.sync()) return sc.rc;
    return sc.get(means, d_out, n_segs);
}

extern "C" int tba_c_apply_outlier_thresh(tba_engine *e, const double *sig, int64_t n,
    double lower_lim, double upper_lim, double *out)
{
    if (!e || !sig || !out || n < 0) return set_err(TBA_E_ARG, "bad arguments");
    if (n == 0) return TBA_OK;
    Scratch sc(e);
    const double *d_in = sc.in(sig, n);
    double *d_out = sc.out<double>(n);
    if (sc.rc) return sc.rc;
    k_c_clip<<<grid_for(n), 256, 0, e->stream>>>(d_in, n, lower_lim, upper_lim, d_out);
    if (sc.sync()) return sc.rc;
    return sc.get(out, d_out, n);
}

// the two change-point detectors run the batch kernels on a one-read batch
static int c_valid_cpts(tba_engine *e, const double *sig, int64_t n, int64_t min_base_obs,
                        int64_t width, int64_t num_cpts, int64_t *cpts, int ttest)
{
    if (!e || !sig || !cpts || n < 1 || min_base_obs < 1 || width < 1 || num_cpts < 1)
        return set_err(TBA_E_ARG, "bad arguments");
    if ((ttest ? n - 2 * width : n + 1 - 2 * width) <= 0) return TBA_INTERNAL;
    // The score-free kernels of the batch pipeline (k_detect.h) when the engine's dispatch sends a
    // batch of one read through the throughput form (tba_engine_set_dispatch(0, ...): the parity tests
    // of this entry in both forms) and for the t-test scores at RNA's defaults; the kernels that keep
    // the scores then run on what those left (flagged reads) -- exactly the batch pipeline's sequence.
    const bool detect = !ttest && e->small_batch < 1 && 2 * width <= DT_W2MAX && min_base_obs == 3;
    const bool detect_tt = ttest && e->small_batch < 1 && min_base_obs == 6 && width <= TT_MAXW;
    ReadState r;
    memset(&r, 0, sizeof(r));
    r.n_raw = n; r.num_events = num_cpts; r.status = TBA_OK;
    if (detect) { // (shift 0, scale 1, no limits: the loader's normalised copy of the signal is the signal)
        r.shift = 0.0; r.scale = 1.0;
        r.is_long = n > TBA_LONG_RAW;
    }
    DevParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.p.running_stat_width = width; dp.p.min_obs_per_base = min_base_obs;
    Scratch sc(e);
    const double *d_sig = sc.in(sig, n);
    double *d_csum = sc.out<double>(n + 1);
    double *d_score = sc.out<double>(n);
    unsigned char *d_state = sc.out<unsigned char>(n);
    i64 *d_cpts = sc.out<i64>(num_cpts);
    ReadState *d_rs = sc.in(&r, 1);
    const DevParams *d_dp = sc.in(&dp, 1);
    if (sc.rc) return sc.rc;
    hipStream_t s = e->stream;
    const unsigned g = grid_for(n) > 128 ? 128 : grid_for(n);
    if (detect) {
        Scratch norm(e); // (released at the end of this scope, before the launches below)
        double *d_norm = norm.out<double>(n + 2 + 8); // (+ 64 bytes past the n + 2 values)
        if (norm.rc) return norm.rc;
        k_detect<2, double><<<1, 256, 0, s>>>(d_rs, 1, d_dp, d_sig, d_norm, d_csum, d_score, n);
        k_pick<<<1, SEL_NT, 0, s>>>(d_rs, d_dp, d_csum, d_score, d_cpts, 0);
        if (norm.sync()) return norm.rc;
    } else if (detect_tt) {
        if (width == 12) k_detect_tt<5, 12, double><<<1, SEL_NT, 0, s>>>(d_rs, d_dp, d_sig, d_csum, d_score);
        else k_detect_tt<5, 0, double><<<1, SEL_NT, 0, s>>>(d_rs, d_dp, d_sig, d_csum, d_score);
        k_pick<<<1, SEL_NT, 0, s>>>(d_rs, d_dp, d_csum, d_score, d_cpts, 1);
    }
    const int only_flagged = detect || detect_tt ? 1 : 0;
    if (!ttest && 2 * width <= 64) { // the batch pipeline's fused form
        k_cumsum_scores<32><<<1, 256, 0, s>>>(d_rs, 1, d_dp, d_sig, d_score, only_flagged);
    } else if (!ttest) {
        k_cumsum<<<1, 64, 0, s>>>(d_rs, 1, d_sig, d_csum);
        k_scores_dna<<<dim3(g, 1), 256, 0, s>>>(d_rs, d_dp, d_csum, d_score);
    } else {
        k_scores_ttest<double><<<dim3(g, 1), 256, 0, s>>>(d_rs, d_dp, d_sig, d_score, only_flagged);
    }
    launch_peaks(min_base_obs, 1, s, d_rs, d_dp, d_score, d_state, d_csum, d_cpts, ttest, only_flagged,
                 ttest ? TBA_ED_FORM_TTEST_PEAKS : TBA_ED_FORM_SCORES_PEAKS);
    if (sc.sync() || sc.get(&r, d_rs, 1)) return sc.rc;
    if (r.status == TBA_OK && sc.get(cpts, d_cpts, num_cpts)) return sc.rc;
    e->last_c_ed_form = r.ed_form;
    return r.status;
}

// which kernels produced the result of the last tba_c_valid_cpts_w_cap[_t_test] call (TBA_ED_FORM_*)
extern "C" int tba_c_last_ed_form(tba_engine *e) { return e ? e->last_c_ed_form : 0; }

extern "C" int tba_c_valid_cpts_w_cap(tba_engine *e, const double *sig, int64_t n,
    int64_t min_base_obs, int64_t running_stat_width, int64_t num_cpts, int64_t *cpts)
{
    return c_valid_cpts(e, sig, n, min_base_obs, running_stat_width, num_cpts, cpts, 0);
}

extern "C" int tba_c_valid_cpts_w_cap_t_test(tba_engine *e, const double *sig, int64_t n,
    int64_t min_base_obs, int64_t running_stat_width, int64_t num_cpts, int64_t *cpts)
{
    return c_valid_cpts(e, sig, n, min_base_obs, running_stat_width, num_cpts, cpts, 1);
}

extern "C" int tba_c_new_mean_stds(tba_engine *e, const double *norm_signal, int64_t n_sig,
    const int64_t *new_segs, int64_t n_segs, double *means, double *stds)
{
    if (!e || !norm_signal || !new_segs || !means || !stds || n_segs < 0 || n_sig < 0)
        return set_err(TBA_E_ARG, "bad arguments");
    if (n_segs == 0) return TBA_OK;
    if (int rc = check_segs(new_segs, n_segs, n_sig)) return rc;
    Scratch sc(e);
    const double *d_sig = sc.in(norm_signal, n_sig);
    const i64 *d_segs = sc.in(new_segs, n_segs + 1);
    double *d_m = sc.out<double>(n_segs);
    double *d_s = sc.out<double>(n_segs);
    if (sc.rc) return sc.rc;
    k_c_new_mean_stds<<<grid_for(n_segs), 256, 0, e->stream>>>(d_sig, d_segs, n_segs, d_m, d_s);
    if (sc.sync() || sc.get(means, d_m, n_segs)) return sc.rc;
    return sc.get(stds, d_s, n_segs);
}

extern "C" int tba_c_compute_slopes(tba_engine *e, const double *r_event_means,
    const double *r_model_means, int64_t n, double max_slope, double *slopes)
{
    if (!e || !r_event_means || !r_model_means || !slopes || n < 0)
        return set_err(TBA_E_ARG, "bad arguments");
    if (n < 2) return TBA_OK;
    if (n > 65535) return set_err(TBA_E_ARG, "too many points");
    const size_t ns = (size_t)n * (size_t)(n - 1) / 2;
    Scratch sc(e);
    const double *d_ev = sc.in(r_event_means, n);
    const double *d_md = sc.in(r_model_means, n);
    double *d_out = sc.out<double>(ns);
    if (sc.rc) return sc.rc;
    k_c_compute_slopes<<<dim3((unsigned)(n - 1)), 256, 0, e->stream>>>(d_ev, d_md, n, max_slope, d_out);
    if (sc.sync()) return sc.rc;
    return sc.get(slopes, d_out, ns);
}

extern "C" int tba_c_reg_z_scores(tba_engine *e, const double *r_sig, int64_t n_sig,
    const double *r_ref_means, const double *r_ref_sds, int64_t n_bases,
    const int64_t *r_b_starts, int64_t n_b_starts, int64_t reg_start, int64_t reg_end,
    int64_t max_base_shift, int64_t min_obs_per_base, int do_winsorize_z,
    double max_half_z_score, int64_t *bounds, int64_t *z_off, double *z, int64_t z_cap)
{
    if (!e || !r_sig || !r_ref_means || !r_ref_sds || !r_b_starts || !bounds || !z_off || !z ||
        n_sig < 0 || z_cap < 0)
        return set_err(TBA_E_ARG, "bad arguments");
    const i64 reg_len = reg_end - reg_start;
    if (reg_start < 0 || reg_len <= 0 || reg_end > n_bases || reg_end >= n_b_starts ||
        max_base_shift < 0)
        return set_err(TBA_E_ARG, "region outside the bases / base starts");
    Scratch sc(e);
    const double *d_sig = sc.in(r_sig, n_sig);
    const double *d_mu = sc.in(r_ref_means, n_bases);
    const double *d_sd = sc.in(r_ref_sds, n_bases);
    const i64 *d_bs = sc.in(r_b_starts, n_b_starts);
    i64 *d_ss = sc.out<i64>(reg_len);
    i64 *d_se = sc.out<i64>(reg_len);
    i64 *d_off = sc.out<i64>(reg_len + 1);
    double *d_z = sc.out<double>(z_cap);
    i32 *d_st = sc.status();
    if (sc.rc) return sc.rc;
    k_c_reg_bounds<<<1, 64, 0, e->stream>>>(d_bs, reg_start, reg_end, max_base_shift,
        min_obs_per_base, d_ss, d_se, d_off);
    k_c_reg_z<<<dim3((unsigned)reg_len), 64, 0, e->stream>>>(d_sig, n_sig, d_mu, d_sd, reg_start,
        d_ss, d_se, d_off, z_cap, do_winsorize_z, max_half_z_score, d_z, d_st);
    std::vector<i64> ss(reg_len), se(reg_len);
    const int st = sc.sync(d_st);
    if (sc.rc || sc.get(ss.data(), d_ss, reg_len) || sc.get(se.data(), d_se, reg_len) ||
        sc.get(z_off, d_off, reg_len + 1))
        return sc.rc;
    if (z_off[reg_len] > z_cap) return set_err(TBA_E_ARG, "z-score buffer too small");
    if (st != 0) return set_err(TBA_E_ARG, "base intervals outside the signal");
    const i64 base = r_b_starts[reg_start];
    for (i64 i = 0; i < reg_len; i++) { bounds[2 * i] = ss[i] - base; bounds[2 * i + 1] = se[i] - base; }
    if (z_off[reg_len] > 0) return sc.get(z, d_z, z_off[reg_len]);
    return TBA_OK;
}

extern "C" int tba_c_base_forward_pass(tba_engine *e, const double *b_data, int64_t b_start,
    int64_t b_end, const double *prev_b_data, int64_t prev_b_start, int64_t prev_b_end,
    const double *prev_b_fwd_data, const int64_t *prev_b_last_diag, int64_t min_obs_per_base,
    double *b_fwd_data, int64_t *b_last_diag)
{
    if (!e || !b_data || !prev_b_data || !prev_b_fwd_data || !prev_b_last_diag || !b_fwd_data ||
        !b_last_diag)
        return set_err(TBA_E_ARG, "bad arguments");
    const i64 b_len = b_end - b_start, plen = prev_b_end - prev_b_start;
    if (b_len <= 0 || plen <= 0) return set_err(TBA_E_ARG, "empty base interval");
    Scratch sc(e);
    const double *d_b = sc.in(b_data, b_len);
    const double *d_pb = sc.in(prev_b_data, plen);
    const double *d_pf = sc.in(prev_b_fwd_data, plen);
    const i64 *d_pl = sc.in(prev_b_last_diag, plen);
    double *d_cum = sc.out<double>(plen);
    double *d_f = sc.out<double>(b_len);
    i64 *d_l = sc.out<i64>(b_len);
    i32 *d_st = sc.status();
    if (sc.rc) return sc.rc;
    k_c_base_forward_pass<<<1, 64, 0, e->stream>>>(d_b, b_start, b_end, d_pb, prev_b_start, prev_b_end,
        d_pf, d_pl, min_obs_per_base, d_cum, d_f, d_l, d_st);
    if (int st = sc.sync(d_st)) return st;
    if (sc.get(b_fwd_data, d_f, b_len)) return sc.rc;
    return sc.get(b_last_diag, d_l, b_len);
}

extern "C" int tba_c_base_traceback(tba_engine *e, const double *curr_b_data, int64_t curr_len,
    int64_t curr_start, const double *next_b_data, int64_t next_len, int64_t next_start,
    int64_t next_end, int64_t sig_start, int64_t min_obs_per_base, int64_t *sig_pos)
{
    if (!e || !curr_b_data || !next_b_data || !sig_pos || curr_len <= 0 || next_len <= 0)
        return set_err(TBA_E_ARG, "bad arguments");
    Scratch sc(e);
    const double *d_c = sc.in(curr_b_data, curr_len);
    const double *d_n = sc.in(next_b_data, next_len);
    i64 *d_out = sc.out<i64>(1);
    i32 *d_st = sc.status();
    if (sc.rc) return sc.rc;
    k_c_base_traceback<<<1, 64, 0, e->stream>>>(d_c, curr_len, curr_start, d_n, next_len, next_start,
        next_end, sig_start, min_obs_per_base, d_out, d_st);
    if (int st = sc.sync(d_st)) return st;
    return sc.get(sig_pos, d_out, 1);
}

static int check_csr_off(const int64_t *off, i64 n)   // (this and check_windows: shared with tba_site_fractions)
{
    if (n > 0 && off[0] != 0) return set_err(TBA_E_ARG, "offset arrays must start at 0");
    for (i64 i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return set_err(TBA_E_ARG, "offset arrays must be non-decreasing");
    return TBA_OK;
}
static int check_windows(int kind, const int64_t *starts, i64 n_windows, i64 width, i64 n_values)
{
    for (i64 i = 0; i < n_windows; i++)
        if (starts[i] < 0 || starts[i] + width > n_values || (kind != 0 && starts[i] >= n_values))
            return set_err(TBA_E_ARG, "window outside the arrays");
    return TBA_OK;
}

extern "C" int tba_llh_ratio_windows(tba_engine *e, int kind, const double *means,
    const double *ref_means, const double *alt_means, const double *ref_vars,
    const double *alt_vars, int64_t n_values, int64_t width, const int64_t *starts,
    int64_t n_windows, const double *par, double *out)
{
    if (!e || !means || !ref_means || !alt_means || !ref_vars || !starts || !out || kind < 0 ||
        kind > 2 || (kind == 0 && !alt_vars) || (kind == 2 && !par) || n_values < 0 || width < 0 ||
        n_windows < 0)
        return set_err(TBA_E_ARG, "bad arguments");
    if (n_windows == 0) return TBA_OK;
    if (const int rc = check_windows(kind, starts, n_windows, width, n_values)) return rc;
    Scratch sc(e);
    const double *d_m = sc.in(means, n_values);
    const double *d_r = sc.in(ref_means, n_values);
    const double *d_a = sc.in(alt_means, n_values);
    const double *d_rv = sc.in(ref_vars, n_values);
    const double *d_av = alt_vars ? sc.in(alt_vars, n_values) : sc.out<double>(n_values);
    const i64 *d_s = sc.in(starts, n_windows);
    double *d_o = sc.out<double>(n_windows);
    if (sc.rc) return sc.rc;
    k_c_llh_windows<<<grid_for(n_windows), 256, 0, e->stream>>>(kind, d_m, d_r, d_a, d_rv, d_av, width,
        d_s, n_windows, par ? par[0] : 0.0, par ? par[1] : 0.0, par ? par[2] : 0.0, d_o);
    if (sc.sync()) return sc.rc;
    return sc.get(out, d_o, n_windows);
}

extern "C" int tba_read_pvals(tba_engine *e, const double *means, const double *ref_means,
    const double *ref_sds, const int64_t *off, int64_t n_reads, int64_t fm_offset, int floor_out,
    double smallest_pval, double *pvals)
{
    if (!e || !means || !ref_means || !ref_sds || !off || !pvals || n_reads < 0 || fm_offset < 0 ||
        fm_offset > 64)
        return set_err(TBA_E_ARG, "bad arguments");
    if (n_reads == 0) return TBA_OK;
    if (const int rc = check_csr_off(off, n_reads)) return rc;
    const i64 total = off[n_reads];
    if (total == 0) return TBA_OK;
    Scratch sc(e);
    const double *d_m = sc.in(means, total);
    const double *d_r = sc.in(ref_means, total);
    const double *d_s = sc.in(ref_sds, total);
    const i64 *d_off = sc.in(off, n_reads + 1);
    double *d_o = sc.out<double>(total);
    if (sc.rc) return sc.rc;
    k_read_pvals<<<grid_for(total), 256, 0, e->stream>>>(d_m, d_r, d_s, d_off, n_reads, total, fm_offset,
        floor_out, smallest_pval, d_o);
    if (sc.sync()) return sc.rc;
    return sc.get(pvals, d_o, total);
}

// ---- level pileups across reads (k_group.h): level_sample_compare and get_reads_ref ----------
namespace {
// the device side of one pileup call: inputs checked and uploaded, pileup, scan, fill and sort
// enqueued.  Host work is O(regions + reads): the level buffer of region r starts at the sum of
// its reads' overlaps with the earlier regions' extended intervals (an upper bound of their
// valid levels), so no coverage comes back to the host between the steps.
struct Pileup {
    GrpArgs a{};
    i32 *cov = nullptr, *run_a = nullptr, *run_b = nullptr;
    i64 *lv_off = nullptr, *out_idx = nullptr, *counts = nullptr;
    double *levels = nullptr;
};

// Segments of `levels` (sizes cov, starts lv_off) sorted in place, one kernel per size class.  The classify
// kernel in front has filled the three lists of segments (`stride` apart) and their three lengths cls.
static void launch_sort_classes(hipStream_t s, const i64 *lists, i64 stride, const u32 *cls, const i32 *cov,
                                const i64 *lv_off, double *levels)
{
    k_grp_sort_wave<<<1024, 256, 0, s>>>(lists, cls, cov, lv_off, levels);
    k_grp_sort_wg<<<1024, 256, 0, s>>>(lists + stride, cls + 1, cov, lv_off, levels, 0);
    k_grp_sort_wg<<<256, 256, 0, s>>>(lists + 2 * stride, cls + 2, cov, lv_off, levels, 1);
}

// the levels of every position sorted in place (a failure stays in sc.rc)
static void grp_sort_levels(Scratch &sc, const Pileup &P)
{
    i64 *lists = sc.out<i64>(6 * P.a.n_pos);
    u32 *cls = sc.out<u32>(3);
    if (sc.zero(cls, 3 * sizeof(u32))) return;
    k_grp_classify<<<grid_for(2 * P.a.n_pos), 256, 0, sc.stream>>>(P.a.n_pos, P.cov, P.out_idx, lists, cls);
    launch_sort_classes(sc.stream, lists, 2 * P.a.n_pos, cls, P.cov, P.lv_off, P.levels);
}

static int grp_pileup(Scratch &sc, Pileup &P, i64 fm, i64 min_reads, int two_groups,
    i64 min_run, bool sort, i64 n_regions, const int64_t *reg_start, const int64_t *reg_end,
    const int8_t *reg_strand, const int64_t *reg_read_off, i64 n_reads, const int64_t *read_start,
    const int8_t *read_strand, const int8_t *read_ctrl, const int64_t *read_off, const double *means)
{
    if (reg_read_off[0] != 0 || reg_read_off[n_regions] > n_reads || read_off[0] != 0)
        return set_err(TBA_E_ARG, "offset arrays must start at 0 and stay inside the reads");
    std::vector<i64> pos_off(n_regions + 1, 0), lvl_base(n_regions + 1, 0);
    for (i64 r = 0; r < n_regions; r++) {
        if (reg_end[r] <= reg_start[r] || reg_strand[r] < 0 || reg_strand[r] > 2 ||
            reg_read_off[r + 1] < reg_read_off[r])
            return set_err(TBA_E_ARG, "bad region");
        const i64 lo = reg_start[r] - fm, hi = reg_end[r] + fm;
        pos_off[r + 1] = pos_off[r] + (hi - lo);
        i64 acc = 0;
        for (i64 q = reg_read_off[r]; q < reg_read_off[r + 1]; q++) {
            const i64 s = read_start[q], t = s + (read_off[q + 1] - read_off[q]);
            const i64 ov = std::min(t, hi) - std::max(s, lo);
            acc += ov > 0 ? ov : 0;
        }
        lvl_base[r + 1] = lvl_base[r] + acc;
    }
    for (i64 q = 0; q < n_reads; q++)
        if (read_off[q + 1] < read_off[q] || read_strand[q] < 0 || read_strand[q] > 1)
            return set_err(TBA_E_ARG, "bad read");
    const i64 n_pos = pos_off[n_regions], n_lv = lvl_base[n_regions], n_means = read_off[n_reads];
    GrpArgs &a = P.a;
    a.n_regions = n_regions; a.n_pos = n_pos; a.fm = fm;
    a.reg_start = sc.in(reg_start, n_regions);
    a.reg_end = sc.in(reg_end, n_regions);
    a.reg_read_off = sc.in(reg_read_off, n_regions + 1);
    a.pos_off = sc.in(pos_off.data(), n_regions + 1);
    a.lvl_base = sc.in(lvl_base.data(), n_regions + 1);
    a.reg_strand = sc.in(reg_strand, n_regions);
    a.read_start = sc.in(read_start, n_reads);
    a.read_off = sc.in(read_off, n_reads + 1);
    a.read_strand = sc.in(read_strand, n_reads);
    a.read_ctrl = read_ctrl ? sc.in(read_ctrl, n_reads) : nullptr;
    if (!read_ctrl) { int8_t *z = sc.out<int8_t>(n_reads); sc.zero(z, n_reads); a.read_ctrl = z; }
    a.means = sc.in(means, n_means);
    P.cov = sc.out<i32>(2 * n_pos);
    P.run_a = sc.out<i32>(n_pos);
    P.run_b = sc.out<i32>(n_pos);
    P.lv_off = sc.out<i64>(2 * n_pos);
    P.out_idx = sc.out<i64>(n_pos);
    P.counts = sc.out<i64>(n_regions);
    P.levels = sc.out<double>(n_lv);
    if (sc.rc) return sc.rc;
    k_grp_pileup<false><<<grid_for(n_pos), 256, 0, sc.stream>>>(a, P.cov, nullptr, nullptr);
    k_grp_scan<<<(unsigned)n_regions, 64, 0, sc.stream>>>(a, P.cov, min_reads, two_groups, min_run,
        P.lv_off, P.run_a, P.run_b, P.out_idx, P.counts);
    k_grp_pileup<true><<<grid_for(n_pos), 256, 0, sc.stream>>>(a, P.cov, P.lv_off, P.levels);
    if (sort) grp_sort_levels(sc, P);
    return sc.hip(hipGetLastError(), "launch");
}
}  // namespace

extern "C" int tba_group_level_stats(tba_engine *e, int stat_kind, int return_p, int64_t fm_offset,
    int64_t min_test_reads, int64_t n_regions, const int64_t *reg_start, const int64_t *reg_end,
    const int8_t *reg_strand, const int64_t *reg_read_off, int64_t n_reads,
    const int64_t *read_start, const int8_t *read_strand, const int8_t *read_ctrl,
    const int64_t *read_off, const double *means, double smallest_pval, double *out_stats,
    int64_t *out_poss, int64_t *out_cov, int64_t *out_ctrl_cov, int64_t *out_counts)
{
    if (!e || stat_kind < 0 || stat_kind > 2 || fm_offset < 0 || fm_offset > 64 || min_test_reads < 1 ||
        n_regions < 0 || n_reads < 0 || !reg_start || !reg_end || !reg_strand || !reg_read_off ||
        !read_start || !read_strand || !read_ctrl || !read_off || !means || !out_stats || !out_poss ||
        !out_cov || !out_ctrl_cov || !out_counts)
        return set_err(TBA_E_ARG, "bad arguments");
    if (n_regions == 0) return TBA_OK;
    Scratch sc(e);
    Pileup P;
    if (const int rc = grp_pileup(sc, P, fm_offset, min_test_reads, 1, 2 * fm_offset + 1, true,
            n_regions, reg_start, reg_end, reg_strand, reg_read_off, n_reads, read_start, read_strand,
            read_ctrl, read_off, means))
        return rc;
    const i64 n_pos = P.a.n_pos;
    double *raw = sc.out<double>(n_pos), *d_stats = sc.out<double>(n_pos);
    i64 *d_poss = sc.out<i64>(n_pos), *d_cov = sc.out<i64>(n_pos), *d_ccov = sc.out<i64>(n_pos);
    if (sc.rc) return sc.rc;
    k_grp_test<<<grid_for(n_pos), 256, 0, e->stream>>>(n_pos, stat_kind, return_p, P.cov, P.lv_off,
        P.out_idx, P.levels, raw);
    k_grp_window<<<grid_for(n_pos), 256, 0, e->stream>>>(P.a, return_p, smallest_pval, P.cov, P.run_a,
        P.run_b, P.out_idx, raw, d_stats, d_poss, d_cov, d_ccov);
    if (sc.sync()) return sc.rc;
    // the compacted outputs of region r start at its first extended position (unused tails are
    // left as they are)
    if (sc.get(out_counts, P.counts, n_regions) || sc.get(out_stats, d_stats, n_pos) ||
        sc.get(out_poss, d_poss, n_pos) || sc.get(out_cov, d_cov, n_pos))
        return sc.rc;
    return sc.get(out_ctrl_cov, d_ccov, n_pos);
}

extern "C" int tba_reads_ref_levels(tba_engine *e, int est_mean, int64_t fm_offset,
    int64_t min_test_reads, int64_t n_regions, const int64_t *reg_start, const int64_t *reg_end,
    const int8_t *reg_strand, const int64_t *reg_read_off, int64_t n_reads,
    const int64_t *read_start, const int8_t *read_strand, const int64_t *read_off,
    const double *means, const double *prior_means, const double *prior_sds, double prior_w_mean,
    double prior_w_sd, double *out_means, double *out_sds, int64_t *out_cov)
{
    if (!e || fm_offset < 0 || min_test_reads < 1 || n_regions < 0 || n_reads < 0 || !reg_start ||
        !reg_end || !reg_strand || !reg_read_off || !read_start || !read_strand || !read_off ||
        !means || !out_means || !out_sds || !out_cov || (!prior_means) != (!prior_sds))
        return set_err(TBA_E_ARG, "bad arguments");
    if (n_regions == 0) return TBA_OK;
    Scratch sc(e);
    Pileup P;
    if (const int rc = grp_pileup(sc, P, fm_offset, min_test_reads, 0, 1, false, n_regions, reg_start,
            reg_end, reg_strand, reg_read_off, n_reads, read_start, read_strand, nullptr, read_off, means))
        return rc;
    const i64 n_pos = P.a.n_pos;
    double *mean = sc.out<double>(n_pos), *sd = sc.out<double>(n_pos), *d_m = sc.out<double>(n_pos), *d_s = sc.out<double>(n_pos);
    i64 *d_c = sc.out<i64>(n_pos);
    const double *d_pm = prior_means ? sc.in(prior_means, n_pos) : nullptr;
    const double *d_ps = prior_sds ? sc.in(prior_sds, n_pos) : nullptr;
    if (sc.rc) return sc.rc;
    // moments in read order first, then the sort for the median
    k_ref_moments<<<grid_for(n_pos), 256, 0, e->stream>>>(n_pos, P.cov, P.lv_off, P.out_idx, P.levels, mean, sd);
    if (!est_mean) grp_sort_levels(sc, P);
    k_ref_finish<<<grid_for(n_pos), 256, 0, e->stream>>>(n_pos, est_mean, P.cov, P.lv_off, P.out_idx,
        P.levels, mean, sd, d_pm, d_ps, prior_w_mean, prior_w_sd, d_m, d_s, d_c);
    if (sc.sync()) return sc.rc;
    if (sc.get(out_means, d_m, n_pos) || sc.get(out_sds, d_s, n_pos)) return sc.rc;
    return sc.get(out_cov, d_c, n_pos);
}

// ---- per-site modified fractions (k_site.h): compute_reg_stats for a batch of tracks -----------
namespace {
// The collation both site entries share: the tracks and their counters on the device, the per-site outputs,
// k_site_finish over them and the read-back.  An entry zeroes the counters, runs its own kernels that fill
// them, then finish(); a failure stays in sc.rc.
struct SiteCollate {
    Scratch &sc;
    SiteArgs a{};
    i64 n_pos;
    double damp_num = 0.0, damp_den = 0.0;
    double *d_frac, *d_damp = nullptr;
    i64 *d_pos, *d_cov, *d_valid, *d_counts, *d_ns;
    SiteCollate(Scratch &sc_, i64 n_tracks, const int64_t *starts, const std::vector<i64> &pos_off, double single_read_thresh,
                const double *lower_thresh, int form, const double *damp_counts) : sc(sc_), n_pos(pos_off[n_tracks])
    {
        a.n_tracks = n_tracks;
        a.trk_start = sc.in(starts, n_tracks);
        a.pos_off = sc.in(pos_off.data(), n_tracks + 1);
        a.valid_mode = lower_thresh ? 0 : form == 1 ? 1 : 2;
        a.single = single_read_thresh;
        a.lower = lower_thresh ? *lower_thresh : 0.0;
        a.cnt = sc.out<i32>(3 * n_pos);
        d_frac = sc.out<double>(n_pos);
        if (damp_counts) { d_damp = sc.out<double>(n_pos); damp_num = damp_counts[0]; damp_den = damp_counts[0] + damp_counts[1]; }
        d_pos = sc.out<i64>(n_pos); d_cov = sc.out<i64>(n_pos); d_valid = sc.out<i64>(n_pos);
        d_counts = sc.out<i64>(n_tracks); d_ns = sc.out<i64>(n_tracks);
    }
    int zero_counters() { return sc.zero(a.cnt, 3 * n_pos * sizeof(i32)); }
    void finish()
    {
        if (sc.rc) return;
        k_site_finish<<<(unsigned)a.n_tracks, 64, 0, sc.stream>>>(a, damp_num, damp_den, d_frac, d_pos, d_cov, d_valid,
            d_damp, d_counts, d_ns);
    }
    // after sc.sync(): the compacted outputs of track t start at its first position (unused tails are left
    // as they are); returns rc
    int read_back(double *out_frac, int64_t *out_pos, int64_t *out_cov, int64_t *out_valid_cov, double *out_damp_frac,
                  int64_t *out_counts, int64_t *out_n_stats)
    {
        if (sc.get(out_counts, d_counts, a.n_tracks) || sc.get(out_n_stats, d_ns, a.n_tracks) ||
            sc.get(out_frac, d_frac, n_pos) || sc.get(out_pos, d_pos, n_pos) ||
            sc.get(out_cov, d_cov, n_pos) || sc.get(out_valid_cov, d_valid, n_pos))
            return sc.rc;
        return d_damp ? sc.get(out_damp_frac, d_damp, n_pos) : sc.rc;
    }
};
} // namespace

extern "C" int tba_site_fractions(tba_engine *e, int form, int64_t n_tracks, const int64_t *trk_start,
    const int64_t *trk_end, const double *means, const double *ref_means, const double *ref_sds,
    const int64_t *off, int64_t n_reads, const int64_t *read_track, const int64_t *read_pos,
    int64_t fm_offset, int floor_out, double smallest_pval, int kind, const double *alt_means,
    const double *ref_vars, const double *alt_vars, int64_t n_values, int64_t width,
    const int64_t *starts, int64_t n_windows, const double *par, const int64_t *win_track,
    const int64_t *win_pos, double single_read_thresh, const double *lower_thresh,
    const double *damp_counts, double *out_frac, int64_t *out_pos, int64_t *out_cov,
    int64_t *out_valid_cov, double *out_damp_frac, int64_t *out_counts, int64_t *out_n_stats,
    double *out_per_read)
{
    if (!e || (form != 0 && form != 1) || n_tracks < 0 || !trk_start || !trk_end || !means ||
        !ref_means || !out_frac || !out_pos || !out_cov || !out_valid_cov || !out_counts ||
        !out_n_stats || (!damp_counts) != (!out_damp_frac))
        return set_err(TBA_E_ARG, "bad arguments");
    if (form == 0 && (!ref_sds || !off || !read_track || !read_pos || n_reads < 0 || fm_offset < 0 ||
                      fm_offset > 64))
        return set_err(TBA_E_ARG, "bad arguments (z form)");
    if (form == 1 && (!alt_means || !ref_vars || !starts || !win_track || !win_pos || kind < 0 ||
                      kind > 2 || (kind == 0 && !alt_vars) || (kind == 2 && !par) || n_values < 0 ||
                      width < 0 || n_windows < 0))
        return set_err(TBA_E_ARG, "bad arguments (window form)");
    if (n_tracks == 0) return TBA_OK;
    std::vector<i64> pos_off(n_tracks + 1, 0);
    for (i64 t = 0; t < n_tracks; t++) {
        if (trk_end[t] < trk_start[t]) return set_err(TBA_E_ARG, "bad track");
        pos_off[t + 1] = pos_off[t] + (trk_end[t] - trk_start[t]);
    }
    const i64 total = form == 0 && n_reads > 0 ? off[n_reads] : 0;
    if (form == 0) {
        if (const int rc = check_csr_off(off, n_reads)) return rc;
        for (i64 r = 0; r < n_reads; r++) {
            const i64 t = read_track[r];
            if (t < 0 || t >= n_tracks) return set_err(TBA_E_ARG, "read outside the tracks");
            if (off[r + 1] > off[r] && (read_pos[r] < trk_start[t] || read_pos[r] + (off[r + 1] - off[r]) > trk_end[t]))
                return set_err(TBA_E_ARG, "statistic position outside its track");
        }
    } else {
        if (const int rc = check_windows(kind, starts, n_windows, width, n_values)) return rc;
        for (i64 w = 0; w < n_windows; w++) {
            const i64 t = win_track[w];
            if (t < 0 || t >= n_tracks) return set_err(TBA_E_ARG, "window outside the tracks");
            if (win_pos[w] < trk_start[t] || win_pos[w] >= trk_end[t])
                return set_err(TBA_E_ARG, "statistic position outside its track");
        }
    }
    Scratch sc(e);
    SiteCollate S(sc, n_tracks, trk_start, pos_off, single_read_thresh, lower_thresh, form, damp_counts);
    const SiteArgs &a = S.a;
    S.zero_counters();
    double *d_pr = nullptr;
    const i64 n_stats = form == 0 ? total : n_windows;
    if (form == 0 && total > 0) {
        const double *d_m = sc.in(means, total);
        const double *d_r = sc.in(ref_means, total);
        const double *d_s = sc.in(ref_sds, total);
        const i64 *d_off = sc.in(off, n_reads + 1);
        const i64 *d_rt = sc.in(read_track, n_reads);
        const i64 *d_rp = sc.in(read_pos, n_reads);
        if (out_per_read || fm_offset > 0) d_pr = sc.out<double>(total);
        if (sc.rc) return sc.rc;
        if (fm_offset == 0)
            k_site_z<<<grid_for(total), 256, 0, e->stream>>>(a, d_m, d_r, d_s, d_off, n_reads, total, d_rt,
                d_rp, floor_out, smallest_pval, d_pr);
        else {
            k_read_pvals<<<grid_for(total), 256, 0, e->stream>>>(d_m, d_r, d_s, d_off, n_reads, total,
                fm_offset, floor_out, smallest_pval, d_pr);
            k_site_stat<<<grid_for(total), 256, 0, e->stream>>>(a, d_pr, d_off, n_reads, total, d_rt, d_rp);
        }
    } else if (form == 1 && n_windows > 0) {
        const double *d_m = sc.in(means, n_values);
        const double *d_r = sc.in(ref_means, n_values);
        const double *d_a = sc.in(alt_means, n_values);
        const double *d_rv = sc.in(ref_vars, n_values);
        const double *d_av = alt_vars ? sc.in(alt_vars, n_values) : sc.out<double>(n_values);
        const i64 *d_st = sc.in(starts, n_windows);
        const i64 *d_wt = sc.in(win_track, n_windows);
        const i64 *d_wp = sc.in(win_pos, n_windows);
        if (out_per_read) d_pr = sc.out<double>(n_windows);
        if (sc.rc) return sc.rc;
        k_site_win<<<grid_for(n_windows), 256, 0, e->stream>>>(a, kind, d_m, d_r, d_a, d_rv, d_av, width,
            d_st, n_windows, par ? par[0] : 0.0, par ? par[1] : 0.0, par ? par[2] : 0.0, d_wt, d_wp, d_pr);
    }
    S.finish();
    if (sc.sync() || S.read_back(out_frac, out_pos, out_cov, out_valid_cov, out_damp_frac, out_counts, out_n_stats))
        return sc.rc;
    if (out_per_read && d_pr) return sc.get(out_per_read, d_pr, n_stats);
    return TBA_OK;
}

// ---- per-site fractions of the z tests from a reads table: the per-read preparation on the device --
extern "C" int tba_site_fractions_reads(tba_engine *e, int form, int64_t n_regions, const int64_t *reg_start,
    const int64_t *reg_end, int64_t n_reads, const int64_t *read_start, const int8_t *read_strand,
    const int64_t *read_off, const double *means, const uint8_t *seq, const int64_t *reg_pair_off,
    const int64_t *pair_read, const double *pos_means, const double *pos_sds, int64_t fm_offset,
    double smallest_pval, double single_read_thresh, const double *lower_thresh,
    const double *damp_counts, double *out_frac, int64_t *out_pos, int64_t *out_cov,
    int64_t *out_valid_cov, double *out_damp_frac, int64_t *out_counts, int64_t *out_n_stats,
    int32_t *out_pair_ok, int64_t *out_pair_pos, int64_t *out_pair_off, double *out_per_read,
    int64_t per_read_cap, double *out_kernel_ms)
{
    if (!e || (form != 0 && form != 1) || n_regions < 0 || n_reads < 0 || !reg_start || !reg_end ||
        !read_start || !read_strand || !read_off || !means || !reg_pair_off || !pair_read ||
        !out_frac || !out_pos || !out_cov || !out_valid_cov || !out_counts || !out_n_stats ||
        !out_pair_ok || !out_pair_pos || !out_pair_off || (!damp_counts) != (!out_damp_frac) ||
        fm_offset < 0 || fm_offset > 64 || (out_per_read && per_read_cap < 0))
        return set_err(TBA_E_ARG, "bad arguments");
    if (form == 0 && !seq) return set_err(TBA_E_ARG, "bad arguments (de_novo form: no base codes)");
    if (form == 1 && (!pos_means || !pos_sds)) return set_err(TBA_E_ARG, "bad arguments (sample_compare form: no control levels)");
    if (form == 0 && (!e->have_model || e->hp.central_pos < 0 || e->hp.central_pos >= e->hp.kmer_width))
        return set_err(TBA_E_ARG, "the de_novo form needs a model (tba_set_model)");
    if (const int rc = check_csr_off(read_off, n_reads)) return rc;
    if (const int rc = check_csr_off(reg_pair_off, n_regions)) return rc;
    for (i64 q = 0; q < n_reads; q++)
        if (read_strand[q] < 0 || read_strand[q] > 1) return set_err(TBA_E_ARG, "read strand must be 0 or 1");
    const i64 n_pairs = n_regions > 0 ? reg_pair_off[n_regions] : 0;
    std::vector<i64> pos_off(n_regions + 1, 0), pair_reg(n_pairs);
    for (i64 r = 0; r < n_regions; r++) {
        if (reg_end[r] <= reg_start[r] || reg_end[r] - reg_start[r] >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "bad region");
        pos_off[r + 1] = pos_off[r] + (reg_end[r] - reg_start[r]) + 2 * fm_offset;
        if (pos_off[r + 1] >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "2^31 positions or more in one call");
        for (i64 p = reg_pair_off[r]; p < reg_pair_off[r + 1]; p++) {
            const i64 q = pair_read[p];
            if (q < 0 || q >= n_reads) return set_err(TBA_E_ARG, "pair_read outside the reads");
            const i64 s = read_start[q], t = s + (read_off[q + 1] - read_off[q]);
            if (s >= reg_end[r] || t <= reg_start[r]) return set_err(TBA_E_ARG, "a read does not overlap its region");
            pair_reg[p] = r;
        }
    }
    if (n_pairs == 0) {   // no region, or nothing to test: every track is empty
        if (out_kernel_ms) out_kernel_ms[0] = out_kernel_ms[1] = 0.0;
        out_pair_off[0] = 0;
        std::fill_n(out_counts, n_regions, 0);
        std::fill_n(out_n_stats, n_regions, 0);
        return TBA_OK;
    }
    const i64 n_bases = read_off[n_reads], n_pos = pos_off[n_regions];
    std::vector<i64> trk_start(n_regions);
    for (i64 r = 0; r < n_regions; r++) trk_start[r] = reg_start[r] - fm_offset;
    Scratch sc(e);
    SiteCollate S(sc, n_regions, trk_start.data(), pos_off, single_read_thresh, lower_thresh, 0, damp_counts);
    SitePairArgs a{};
    a.form = form; a.fm = fm_offset; a.n_pairs = n_pairs;
    a.K = form == 0 ? (int)e->hp.kmer_width : 1;
    a.cp = form == 0 ? (int)e->hp.central_pos : 0;
    a.reg_start = sc.in(reg_start, n_regions);
    a.reg_end = sc.in(reg_end, n_regions);
    a.pos_off = S.a.pos_off;
    a.pair_reg = sc.in(pair_reg.data(), n_pairs);
    a.pair_read = sc.in(pair_read, n_pairs);
    a.read_start = sc.in(read_start, n_reads);
    a.read_off = sc.in(read_off, n_reads + 1);
    a.read_strand = sc.in(read_strand, n_reads);
    a.means = sc.in(means, n_bases);
    if (form == 0) {
        a.seq = sc.in(seq, n_bases);
        a.kmeans = e->d_kmeans.as<double>();
        a.ksds = e->d_ksds.as<double>();
    } else {
        a.pos_means = sc.in(pos_means, n_pos);
        a.pos_sds = sc.in(pos_sds, n_pos);
    }
    i32 *d_ok = sc.out<i32>(n_pairs);
    i64 *d_ppos = sc.out<i64>(n_pairs), *d_cnt = sc.out<i64>(n_pairs), *d_poff = sc.out<i64>(n_pairs + 1);
    if (sc.rc) return sc.rc;
    // the plan and the scan; the number of statistics comes back before the buffers for them are made
    KernelTimer t_plan(sc, out_kernel_ms != nullptr);
    k_site_pair_plan<<<grid_for(64 * n_pairs), 256, 0, sc.stream>>>(a, d_ok, d_ppos, d_cnt);
    k_exclusive_prefix<i64><<<1, 256, 0, sc.stream>>>(n_pairs, d_cnt, d_poff, d_poff + n_pairs);
    t_plan.stop();
    i64 total = 0;
    if (sc.sync() || sc.get(&total, d_poff + n_pairs, 1)) return sc.rc;
    if (out_per_read && per_read_cap < total) return set_err(TBA_E_ARG, "per_read_cap is smaller than the number of statistics");
    double *d_pr = nullptr;
    KernelTimer t_gather(sc, out_kernel_ms != nullptr);
    KernelTimer t_stat(sc, out_kernel_ms != nullptr);
    S.zero_counters();
    if (total > 0) {
        double *d_m = sc.out<double>(total), *d_r = sc.out<double>(total), *d_s = sc.out<double>(total);
        if (out_per_read || fm_offset > 0) d_pr = sc.out<double>(total);
        if (sc.rc) return sc.rc;
        k_site_gather<<<grid_for(total), 256, 0, sc.stream>>>(a, d_poff, d_ppos, total, d_m, d_r, d_s);
        t_gather.stop();
        const int floor_out = form == 0 ? 1 : 0;
        if (fm_offset == 0)
            k_site_z<<<grid_for(total), 256, 0, sc.stream>>>(S.a, d_m, d_r, d_s, d_poff, n_pairs, total, a.pair_reg,
                d_ppos, floor_out, smallest_pval, d_pr);
        else {
            k_read_pvals<<<grid_for(total), 256, 0, sc.stream>>>(d_m, d_r, d_s, d_poff, n_pairs, total,
                fm_offset, floor_out, smallest_pval, d_pr);
            k_site_stat<<<grid_for(total), 256, 0, sc.stream>>>(S.a, d_pr, d_poff, n_pairs, total, a.pair_reg, d_ppos);
        }
    } else
        t_gather.stop();
    S.finish();
    t_stat.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) {
        const double g = t_gather.ms();
        out_kernel_ms[0] = t_plan.ms() + g;
        out_kernel_ms[1] = t_stat.ms() - g;
    }
    if (S.read_back(out_frac, out_pos, out_cov, out_valid_cov, out_damp_frac, out_counts, out_n_stats) ||
        sc.get(out_pair_ok, d_ok, n_pairs) || sc.get(out_pair_pos, d_ppos, n_pairs) ||
        sc.get(out_pair_off, d_poff, n_pairs + 1))
        return sc.rc;
    if (out_per_read && total > 0) return sc.get(out_per_read, d_pr, total);
    return TBA_OK;
}

// ---- per-site fractions from stored per-read records: aggregate_per_read_stats -----------------
extern "C" int tba_site_aggregate(tba_engine *e, int64_t n_blocks, const int64_t *blk_start,
    const int64_t *blk_end, const int64_t *rec_off, const void *records, double single_read_thresh,
    const double *lower_thresh, int form, const double *damp_counts, double *out_frac,
    int64_t *out_pos, int64_t *out_cov, int64_t *out_valid_cov, double *out_damp_frac,
    int64_t *out_counts, int64_t *out_n_stats, double *out_kernel_ms)
{
    if (!e || (form != 0 && form != 1) || n_blocks < 0 || !blk_start || !blk_end || !rec_off ||
        !out_frac || !out_pos || !out_cov || !out_valid_cov || !out_counts || !out_n_stats ||
        (!damp_counts) != (!out_damp_frac))
        return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (n_blocks == 0) return TBA_OK;
    if (const int rc = check_csr_off(rec_off, n_blocks)) return rc;
    const i64 n_recs = rec_off[n_blocks];
    if (n_recs > 0 && !records) return set_err(TBA_E_ARG, "bad arguments");
    std::vector<i64> pos_off(n_blocks + 1, 0);
    for (i64 t = 0; t < n_blocks; t++) {
        if (blk_end[t] <= blk_start[t] || blk_end[t] - blk_start[t] >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "bad block");
        pos_off[t + 1] = pos_off[t] + (blk_end[t] - blk_start[t]);
        if (pos_off[t + 1] >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "2^31 positions or more in one call");
    }
    Scratch sc(e);
    SiteCollate S(sc, n_blocks, blk_start, pos_off, single_read_thresh, lower_thresh, form, damp_counts);
    const i64 *d_end = sc.in(blk_end, n_blocks);
    const i64 *d_off = sc.in(rec_off, n_blocks + 1);
    const uint4 *d_rec = sc.in((const uint4 *)records, n_recs);
    i32 *d_bad = sc.status();
    if (sc.rc) return sc.rc;
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    if (!S.zero_counters() && n_recs > 0)
        k_site_rec<<<grid_for(n_recs), 256, 0, sc.stream>>>(S.a, d_rec, d_off, n_recs, d_end, d_bad);
    S.finish();
    tm.stop();
    const int n_bad = sc.sync(d_bad);
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    if (sc.rc) return sc.rc;
    if (n_bad) return set_err(TBA_E_ARG, "record position outside its block");
    return S.read_back(out_frac, out_pos, out_cov, out_valid_cov, out_damp_frac, out_counts, out_n_stats);
}

// ---- estimate_alt_model (k_kde.h): levels gathered by k-mer, kernel densities ----------------
namespace {
// n items partitioned by one of n_keys keys, in chunks: a row of per-key counters per chunk (at most 1024
// chunks and at most 2^24 counters; a chunk is a multiple of 64 items and at least 4096).  src: the items' keys
// and where a placed item is stored (k_key_partition, k_scan.h).  count() runs the counting pass over zeroed
// rows and leaves the per-key counts and their offsets on the device; fill() then places the items.
struct KeyPartition {
    Scratch &sc;
    i64 n, n_keys, chunk, n_chunks;
    int key_bits = 0;   // bits that tell the keys apart
    u32 *rows;
    i64 *counts, *off;
    KeyPartition(Scratch &sc_, i64 n_, i64 n_keys_) : sc(sc_), n(n_), n_keys(n_keys_)
    {
        while (((i64)1 << key_bits) < n_keys) key_bits++;
        const i64 max_chunks = std::max<i64>(1, std::min<i64>(1024, ((i64)1 << 24) / n_keys));
        chunk = std::max<i64>(4096, ((n + max_chunks - 1) / max_chunks + 63) / 64 * 64);
        n_chunks = (n + chunk - 1) / chunk;
        rows = sc.out<u32>(n_chunks * n_keys);
        counts = sc.out<i64>(n_keys);
        off = sc.out<i64>(n_keys + 1);
    }
    template <class Src> void count(const Src &src)
    {
        if (sc.zero(rows, n_chunks * n_keys * sizeof(u32))) return;
        k_key_partition<false><<<(unsigned)n_chunks, 64, 0, sc.stream>>>(src, n, chunk, n_keys, key_bits, rows, nullptr);
        k_kmer_colscan<<<grid_for(n_keys), 256, 0, sc.stream>>>(n_keys, n_chunks, rows, counts);
        k_exclusive_prefix<<<1, 256, 0, sc.stream>>>(n_keys, counts, off, off + n_keys);
    }
    template <class Src> void fill(const Src &src)
    {
        k_key_partition<true><<<(unsigned)n_chunks, 64, 0, sc.stream>>>(src, n, chunk, n_keys, key_bits, rows, off);
    }
};

// a call without items: every key's count and offset is zero
static int empty_partition(i64 n_keys, int64_t *out_counts, int64_t *out_off)
{
    std::fill_n(out_counts, n_keys, 0);
    if (out_off) std::fill_n(out_off, n_keys + 1, 0);
    return TBA_OK;
}

// the levels and base codes of a read batch, CSR by read_off; total: its bases
static int check_read_batch(const int64_t *read_off, i64 n_reads, const double *means, const uint8_t *codes, i64 &total)
{
    if (const int rc = check_csr_off(read_off, n_reads)) return rc;
    total = n_reads > 0 ? read_off[n_reads] : 0;
    if (total >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "more than 2^31 - 1 bases in one batch");
    if (total > 0 && (!means || !codes)) return set_err(TBA_E_ARG, "bad arguments");
    return TBA_OK;
}

// values in n_seg > 0 CSR segments, each of fewer than 2^31 values (too_long: the entry's message for a longer one)
static int check_segments(const double *values, const int64_t *off, i64 n_seg, const char *too_long)
{
    if (const int rc = check_csr_off(off, n_seg)) return rc;
    for (i64 s = 0; s < n_seg; s++)
        if (off[s + 1] - off[s] >= ((i64)1 << 31)) return set_err(TBA_E_ARG, too_long);
    if (off[n_seg] > 0 && !values) return set_err(TBA_E_ARG, "bad arguments");
    return TBA_OK;
}
} // namespace

extern "C" int tba_kmer_levels(tba_engine *e, const double *means, const uint8_t *codes,
    const int64_t *read_off, int64_t n_reads, int64_t kmer_width, int64_t central_pos,
    const uint8_t *completed, int64_t *out_counts, int64_t *out_lv_off, double *out_levels,
    int64_t levels_cap)
{
    if (!e || !read_off || !completed || !out_counts || n_reads < 0 || kmer_width < 1 || kmer_width > 10 ||
        central_pos < 0 || central_pos >= kmer_width || (out_levels && (!out_lv_off || levels_cap < 0)))
        return set_err(TBA_E_ARG, "bad arguments");
    const i64 n_kmers = (i64)1 << (2 * kmer_width);
    i64 total;
    if (const int rc = check_read_batch(read_off, n_reads, means, codes, total)) return rc;
    if (total == 0) return empty_partition(n_kmers, out_counts, out_lv_off);
    Scratch sc(e);
    KeyPartition part(sc, total, n_kmers);
    KmerSrc a{};
    a.n_reads = n_reads; a.K = (int)kmer_width; a.cp = (int)central_pos;
    a.read_off = sc.in(read_off, n_reads + 1);
    a.codes = sc.in(codes, total);
    a.completed = sc.in(completed, n_kmers);
    a.means = sc.in(means, total);
    part.count(a);
    if (sc.sync()) return sc.rc;
    if (sc.get(out_counts, part.counts, n_kmers)) return sc.rc;
    if (out_lv_off && sc.get(out_lv_off, part.off, n_kmers + 1)) return sc.rc;
    if (!out_levels) return TBA_OK;
    const i64 n_lv = out_lv_off[n_kmers];
    if (n_lv > levels_cap) return set_err(TBA_E_ARG, "levels_cap is smaller than the number of gathered levels");
    if (n_lv == 0) return TBA_OK;
    a.levels = sc.out<double>(n_lv);
    if (sc.rc) return sc.rc;
    part.fill(a);
    if (sc.sync()) return sc.rc;
    return sc.get(out_levels, a.levels, n_lv);
}

namespace {
// the segments of d_lv (n_seg, CSR by d_off) with more than one level and no NaN sorted ascending in place (shared by
// tba_kde_eval, tba_region_key_levels and tba_segment_medians) -> has_nan per segment; *cov_out: the sizes
static i32 *sort_segments(Scratch &sc, i64 n_seg, const i64 *d_off, double *d_lv, i32 **cov_out = nullptr)
{
    i32 *cov = sc.out<i32>(n_seg), *has_nan = sc.out<i32>(n_seg);
    if (cov_out) *cov_out = cov;
    i64 *lists = sc.out<i64>(3 * n_seg);
    u32 *cls = sc.out<u32>(3);
    if (sc.zero(cls, 3 * sizeof(u32))) return nullptr;
    k_kde_classify<<<grid_for(64 * n_seg), 256, 0, sc.stream>>>(n_seg, d_off, d_lv, cov, has_nan, lists, cls);
    launch_sort_classes(sc.stream, lists, n_seg, cls, cov, d_off, d_lv);
    return has_nan;
}
} // namespace

extern "C" int tba_kde_eval(tba_engine *e, const double *levels, const int64_t *lv_off, int64_t n_seg,
    const double *x, int64_t n_x, double bandwidth, double *out_dens)
{
    if (!e || !lv_off || n_seg < 0 || n_x < 0 || !(bandwidth > 0) || !(bandwidth < INFINITY) ||
        n_x > (int64_t)65535 * 256 || (n_x > 0 && !x) || (n_seg > 0 && n_x > 0 && !out_dens))
        return set_err(TBA_E_ARG, "bad arguments");
    if (n_seg == 0 || n_x == 0) return TBA_OK;
    if (const int rc = check_segments(levels, lv_off, n_seg, "segment of more than 2^31 - 1 levels")) return rc;
    const i64 n_lv = lv_off[n_seg];
    Scratch sc(e);
    double *d_lv = sc.in(levels, n_lv);
    const i64 *d_off = sc.in(lv_off, n_seg + 1);
    const double *d_x = sc.in(x, n_x);
    double *d_dens = sc.out<double>(n_seg * n_x);
    i32 *cov = nullptr;
    const i32 *has_nan = sort_segments(sc, n_seg, d_off, d_lv, &cov);
    if (sc.rc) return sc.rc;
    k_kde_eval<<<dim3((unsigned)std::min<i64>(n_seg, 65535), (unsigned)((n_x + 255) / 256)), 256, 0, e->stream>>>(
        n_seg, cov, has_nan, d_off, d_lv, d_x, n_x, bandwidth, d_dens);
    if (sc.sync()) return sc.rc;
    return sc.get(out_dens, d_dens, n_seg * n_x);
}

// ---- k-mer level distributions (k_kmer_dist.h): plot_kmer_dist, _plot_commands.py:451-559 ----
#define KD_TABLE_MAX ((i64)1 << 27)   // 4^K * n_reads, the dense per-read table; also the most chunk counters
extern "C" int tba_kmer_dist(tba_engine *e, const double *means, const uint8_t *codes, const int64_t *read_off,
    int64_t n_reads, int64_t kmer_width, int64_t central_pos, int64_t kmer_thresh, int64_t num_reads,
    int read_mean, int64_t *out_read_label, int64_t *out_n_sel, int64_t *out_n_examined, int64_t *out_counts,
    int64_t *out_off, double *out_values, int64_t *out_value_label, int64_t values_cap, double *out_kmer_mean,
    double *out_kernel_ms)
{
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (!e || !read_off || !out_read_label || !out_n_sel || !out_n_examined || !out_counts || !out_off || n_reads < 0 ||
        kmer_width < 1 || kmer_width > 9 || central_pos < 0 || central_pos >= kmer_width ||
        (out_values && (!out_value_label || !out_kmer_mean || values_cap < 0)))
        return set_err(TBA_E_ARG, "bad arguments");
    const i64 n_kmers = (i64)1 << (2 * kmer_width);
    i64 total;
    if (const int rc = check_read_batch(read_off, n_reads, means, codes, total)) return rc;
    if (n_reads > KD_TABLE_MAX / n_kmers) return set_err(TBA_E_ARG, "4^kmer_width * n_reads above 2^27");
    *out_n_sel = *out_n_examined = 0;
    if (n_reads == 0) {
        if (out_values) std::fill_n(out_kmer_mean, n_kmers, NAN);
        return empty_partition(n_kmers, out_counts, out_off);
    }
    // chunks that never cross a read: the shortest multiple-of-64 length from 4096 on that keeps the chunk
    // counters within KD_TABLE_MAX (a read has at least one chunk, n_reads of them always fit)
    i64 chunk = 4096, max_len = 0;
    for (i64 r = 0; r < n_reads; r++) max_len = std::max<i64>(max_len, read_off[r + 1] - read_off[r]);
    auto count_chunks = [&](i64 c) { i64 n = 0; for (i64 r = 0; r < n_reads; r++) n += (read_off[r + 1] - read_off[r] + c - 1) / c; return n; };
    while (chunk < max_len && count_chunks(chunk) > KD_TABLE_MAX / n_kmers) chunk *= 2;
    std::vector<KdChunk> chunks;
    std::vector<i64> read_chunk0(n_reads + 1);
    for (i64 r = 0; r < n_reads; r++) {
        read_chunk0[r] = (i64)chunks.size();
        for (i64 p = read_off[r]; p < read_off[r + 1]; p += chunk) chunks.push_back(KdChunk{r, p, std::min<i64>(p + chunk, read_off[r + 1])});
    }
    read_chunk0[n_reads] = (i64)chunks.size();
    const i64 n_chunks = (i64)chunks.size();

    Scratch sc(e);
    KdArgs a{};
    a.n_reads = n_reads; a.n_chunks = n_chunks; a.n_kmers = n_kmers; a.K = (int)kmer_width; a.cp = (int)central_pos;
    a.read_mean = read_mean != 0;
    a.read_off = sc.in(read_off, n_reads + 1);
    a.chunks = sc.in(chunks.data(), n_chunks);
    a.codes = sc.in(codes, total);
    a.means = sc.in(means, total);
    const i64 *d_chunk0 = sc.in(read_chunk0.data(), n_reads + 1);
    u32 *rows = sc.out<u32>(n_chunks * n_kmers), *tab = sc.out<u32>(n_reads * n_kmers);
    u32 *distinct = sc.out<u32>(n_reads), *min_cnt = sc.out<u32>(n_reads);
    i64 *d_label = sc.out<i64>(n_reads), *d_nsel = sc.out<i64>(2);
    i64 *lvl_tot = sc.out<i64>(n_kmers), *ent_tot = sc.out<i64>(n_kmers);
    i64 *lv_off = sc.out<i64>(n_kmers + 1), *ent_off = sc.out<i64>(n_kmers + 1);
    if (sc.rc) return sc.rc;
    double ms = 0.0;
    const unsigned scan_x = (unsigned)std::min<i64>((n_kmers + 255) / 256, 64);
    {
        KernelTimer t(sc, out_kernel_ms != nullptr);
        sc.zero(rows, n_chunks * n_kmers * sizeof(u32));
        sc.zero(distinct, n_reads * sizeof(u32));
        sc.hip(hipMemsetAsync(min_cnt, 0xff, n_reads * sizeof(u32), sc.stream), "hipMemsetAsync");
        if (sc.rc) return sc.rc;
        if (n_chunks > 0) k_kd_gather<false><<<(unsigned)n_chunks, 64, 0, sc.stream>>>(a, rows, nullptr, nullptr, nullptr, nullptr);
        for (i64 r0 = 0; r0 < n_reads; r0 += 65535)   // (blockIdx.y holds 65535 reads)
            k_kd_read_scan<<<dim3(scan_x, (unsigned)std::min<i64>(n_reads - r0, 65535)), 256, 0, sc.stream>>>(
                n_kmers, d_chunk0 + r0, rows, tab + r0 * n_kmers, distinct + r0, min_cnt + r0);
        k_kd_select<<<1, 64, 0, sc.stream>>>(n_reads, n_kmers, kmer_thresh, num_reads, distinct, min_cnt, d_label, d_nsel);
        t.stop();
        ms += t.ms();
    }
    i64 sel_out[2];
    if (sc.sync() || sc.get(out_read_label, d_label, n_reads) || sc.get(sel_out, d_nsel, 2)) return sc.rc;
    const i64 n_sel = *out_n_sel = sel_out[0];
    *out_n_examined = sel_out[1];
    std::vector<i64> sel(n_sel);   // the taken reads in label order: a copy, no arithmetic
    for (i64 r = 0; r < n_reads; r++) if (out_read_label[r] > 0) sel[out_read_label[r] - 1] = r;
    const i64 *d_sel = sc.in(sel.data(), n_sel);
    if (sc.rc) return sc.rc;
    {
        KernelTimer t(sc, out_kernel_ms != nullptr);
        k_kd_kmer_totals<<<grid_for(n_kmers), 256, 0, sc.stream>>>(n_kmers, n_sel, d_sel, tab, lvl_tot, ent_tot);
        k_exclusive_prefix<<<1, 256, 0, sc.stream>>>(n_kmers, lvl_tot, lv_off, lv_off + n_kmers);
        k_exclusive_prefix<<<1, 256, 0, sc.stream>>>(n_kmers, ent_tot, ent_off, ent_off + n_kmers);
        t.stop();
        ms += t.ms();
    }
    const i64 *d_counts = read_mean ? ent_tot : lvl_tot, *d_off = read_mean ? ent_off : lv_off;
    i64 n_lv = 0;
    if (sc.sync() || sc.get(out_counts, d_counts, n_kmers) || sc.get(out_off, d_off, n_kmers + 1) ||
        sc.get(&n_lv, lv_off + n_kmers, 1))
        return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = ms;
    if (!out_values) return TBA_OK;
    const i64 n_val = out_off[n_kmers];
    if (n_val > values_cap) return set_err(TBA_E_ARG, "values_cap is smaller than the number of values");
    double *d_lv = sc.out<double>(n_lv), *d_val = read_mean ? sc.out<double>(n_val) : d_lv;
    i64 *d_vlabel = sc.out<i64>(n_val);
    u32 *seg_start = read_mean ? sc.out<u32>(n_val) : nullptr, *seg_len = read_mean ? sc.out<u32>(n_val) : nullptr;
    double *d_kmean = sc.out<double>(n_kmers);
    if (sc.rc) return sc.rc;
    a.n_lv = n_lv;
    {
        KernelTimer t(sc, out_kernel_ms != nullptr);
        k_kd_seg_bases<<<grid_for(n_kmers), 256, 0, sc.stream>>>(n_kmers, n_sel, d_sel, tab, lv_off, ent_off, seg_start, seg_len, d_vlabel);
        if (n_chunks > 0 && n_lv > 0)
            k_kd_gather<true><<<(unsigned)n_chunks, 64, 0, sc.stream>>>(a, rows, d_label, tab, d_lv, read_mean ? nullptr : d_vlabel);
        if (read_mean && n_val > 0)
            k_kd_seg_means<<<(unsigned)std::min<i64>((n_val + 63) / 64, 65536), 64, 0, sc.stream>>>(n_val, seg_start, seg_len, d_lv, d_val);
        k_kd_kmer_means<<<(unsigned)std::min<i64>(n_kmers, 65536), 64, 0, sc.stream>>>(n_kmers, d_off, d_val, d_kmean);
        t.stop();
        ms += t.ms();
    }
    if (sc.sync() || sc.get(out_values, d_val, n_val) || sc.get(out_value_label, d_vlabel, n_val) ||
        sc.get(out_kmer_mean, d_kmean, n_kmers))
        return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = ms;
    return TBA_OK;
}

// ---- genome tracks (k_tracks.h): pileup sums and coverages, compaction, difference, top N --------
namespace {
static unsigned scan_chunks(i64 n) { return (unsigned)((n + SCAN_CHUNK - 1) / SCAN_CHUNK); }

// flag / scan / scatter of the n words x under `mode` (sel: the search state of the top-N modes); the kept
// indices to d_pos (n + 1 words), the kept words of src to d_val (n words); d_total: how many were kept
static void launch_compact(Scratch &sc, i64 n, int mode, const u64 *x, const TrkSel *sel, const u64 *src,
                           i64 *d_pos, u64 *d_val, i64 *d_total)
{
    const unsigned nb = scan_chunks(n);
    const TrkKeep keep{mode, x, sel};
    i64 *d_cnt = sc.out<i64>(nb);
    if (sc.rc) return;
    k_chunk_total<<<nb, 256, 0, sc.stream>>>(n, keep, d_cnt);
    k_exclusive_prefix<<<1, 256, 0, sc.stream>>>((i64)nb, d_cnt, d_cnt, d_total);
    k_trk_scatter<<<nb, 256, 0, sc.stream>>>(n, keep, src, d_cnt, d_total, d_pos, d_val);
}
} // namespace

extern "C" int tba_tracks_begin(tba_engine *e, int64_t win_start, int64_t win_end, int n_slots)
{
    if (!e || win_start < 0 || win_end <= win_start || win_end - win_start >= ((i64)1 << 31) ||
        n_slots < 1 || n_slots > TRK_MAX_SLOTS)
        return set_err(TBA_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(e->device));
    const i64 W = win_end - win_start;
    e->trk_slots = 0;
    if (e->d_trk_sum.ensure((size_t)n_slots * W * 8) || e->d_trk_cov.ensure((size_t)n_slots * W * 8) ||
        e->d_trk_rcov.ensure((size_t)W * 8))
        return TBA_E_NOMEM;
    // all bits zero: +0.0 sums, zero coverages
    HIP_TRY(hipMemsetAsync(e->d_trk_sum.p, 0, (size_t)n_slots * W * 8, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_trk_cov.p, 0, (size_t)n_slots * W * 8, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_trk_rcov.p, 0, (size_t)W * 8, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->trk_start = win_start; e->trk_W = W; e->trk_slots = n_slots; e->trk_kernel_ms = 0;
    return TBA_OK;
}

extern "C" int tba_tracks_add(tba_engine *e, int64_t n_reads, const int64_t *read_start, const int64_t *read_end,
    const uint8_t *read_flags, const int64_t *read_off, const double *const *slots, int64_t n_tiles,
    const int64_t *tile_read_off, const int32_t *tile_reads)
{
    if (!e || !e->trk_slots) return set_err(TBA_E_ARG, "no track set is open (tba_tracks_begin)");
    const i64 W = e->trk_W;
    const int ns = e->trk_slots;
    if (n_reads < 0 || n_reads >= ((i64)1 << 31) || n_tiles != (W + TRK_TILE - 1) / TRK_TILE || !tile_read_off || !slots ||
        (n_reads > 0 && (!read_start || !read_end || !read_flags || !read_off)))
        return set_err(TBA_E_ARG, "bad arguments");
    if (const int rc = check_csr_off(tile_read_off, n_tiles)) return rc;
    const i64 n_listed = tile_read_off[n_tiles];
    if (n_listed > 0 && !tile_reads) return set_err(TBA_E_ARG, "bad arguments");
    for (i64 i = 0; i < n_listed; i++)
        if (tile_reads[i] < 0 || tile_reads[i] >= n_reads) return set_err(TBA_E_ARG, "tile list names a read outside the batch");
    if (n_reads == 0 || n_listed == 0) return TBA_OK;
    if (const int rc = check_csr_off(read_off, n_reads)) return rc;
    const i64 total = read_off[n_reads];
    for (i64 q = 0; q < n_reads; q++) {
        if (read_end[q] < read_start[q] || read_start[q] < 0) return set_err(TBA_E_ARG, "read with end < start or start < 0");
        if (read_flags[q] >> (1 + ns)) return set_err(TBA_E_ARG, "read flags name a slot the track set does not have");
    }
    for (int s = 0; s < ns; s++) if (total > 0 && !slots[s]) return set_err(TBA_E_ARG, "bad arguments");
    Scratch sc(e);
    TrkAdd a{};
    a.win_start = e->trk_start; a.W = W;
    a.read_start = sc.in(read_start, n_reads);
    a.read_end = sc.in(read_end, n_reads);
    a.read_off = sc.in(read_off, n_reads + 1);
    a.read_flags = sc.in(read_flags, n_reads);
    for (int s = 0; s < ns; s++) a.slot[s] = sc.in(slots[s], total);
    a.tile_off = sc.in(tile_read_off, n_tiles + 1);
    a.tile_reads = sc.in(tile_reads, n_listed);
    a.sum = e->d_trk_sum.as<double>(); a.cov = e->d_trk_cov.as<i64>(); a.rcov = e->d_trk_rcov.as<i64>();
    if (sc.rc) return sc.rc;
    KernelTimer tm(sc);
    (ns == 1 ? k_trk_add<1> : ns == 2 ? k_trk_add<2> : k_trk_add<3>)<<<(unsigned)n_tiles, TRK_TILE, 0, e->stream>>>(a);
    tm.stop();
    const int rc = sc.sync();
    e->trk_kernel_ms += tm.ms();
    return rc;
}

extern "C" int tba_tracks_finish(tba_engine *e, double *means_out, double *sums_out, int64_t *slot_cov_out,
    int64_t *read_cov_out)
{
    if (!e || !e->trk_slots) return set_err(TBA_E_ARG, "no track set is open (tba_tracks_begin)");
    const i64 W = e->trk_W, n = W * e->trk_slots;
    Scratch sc(e);
    if (means_out) {
        double *d_mean = sc.out<double>(n);
        if (sc.rc) return sc.rc;
        KernelTimer tm(sc);
        k_trk_finish<<<grid_for(n), 256, 0, e->stream>>>(n, e->d_trk_sum.as<double>(), e->d_trk_cov.as<i64>(), d_mean);
        tm.stop();
        e->trk_kernel_ms += tm.ms();
        if (sc.sync() || sc.get(means_out, d_mean, n)) return sc.rc;
    } else if (sc.sync()) return sc.rc;
    if (sums_out && sc.get(sums_out, e->d_trk_sum.as<double>(), n)) return sc.rc;
    if (slot_cov_out && sc.get(slot_cov_out, e->d_trk_cov.as<i64>(), n)) return sc.rc;
    if (read_cov_out && sc.get(read_cov_out, e->d_trk_rcov.as<i64>(), W)) return sc.rc;
    return TBA_OK;
}

extern "C" int tba_tracks_kernel_ms(tba_engine *e, double *ms)
{
    if (!e || !ms) return set_err(TBA_E_ARG, "bad arguments");
    *ms = e->trk_kernel_ms;
    return TBA_OK;
}

extern "C" int tba_tracks_compact(tba_engine *e, int mode, const void *values, int64_t n, int64_t *out_pos,
    void *out_val, int64_t *out_count)
{
    if (!e || (mode != TRK_KEEP_NOT_NAN && mode != TRK_KEEP_RUN_START) || n < 0 || n >= ((i64)1 << 31) || !out_count ||
        (n > 0 && (!values || !out_pos || !out_val)))
        return set_err(TBA_E_ARG, "bad arguments");
    *out_count = 0;
    if (n == 0) return TBA_OK;
    Scratch sc(e);
    const u64 *d_x = sc.in((const u64 *)values, n);
    i64 *d_pos = sc.out<i64>(n + 1), *d_total = sc.out<i64>(1);
    u64 *d_val = sc.out<u64>(n);
    launch_compact(sc, n, mode, d_x, nullptr, d_x, d_pos, d_val, d_total);
    if (sc.sync() || sc.get(out_count, d_total, 1)) return sc.rc;
    const i64 k = *out_count;
    if (sc.get(out_pos, d_pos, k + (mode == TRK_KEEP_RUN_START))) return sc.rc;
    return sc.get((u64 *)out_val, d_val, k);
}

extern "C" int tba_tracks_diff(tba_engine *e, const double *a, const double *b, int64_t n, double *out)
{
    if (!e || n < 0 || (n > 0 && (!a || !b || !out))) return set_err(TBA_E_ARG, "bad arguments");
    if (n == 0) return TBA_OK;
    Scratch sc(e);
    const double *d_a = sc.in(a, n), *d_b = sc.in(b, n);
    double *d_out = sc.out<double>(n);
    if (sc.rc) return sc.rc;
    k_trk_diff<false><<<grid_for(n), 256, 0, e->stream>>>(n, d_a, d_b, d_out, nullptr);
    if (sc.sync()) return sc.rc;
    return sc.get(out, d_out, n);
}

extern "C" int tba_tracks_topn(tba_engine *e, const double *a, const double *b, int64_t n, int64_t n_top,
    int64_t *out_pos, double *out_val, int64_t *out_count)
{
    if (!e || n < 0 || n >= ((i64)1 << 31) || n_top < 0 || !out_count || (n > 0 && (!a || !b)) ||
        (n > 0 && n_top > 0 && (!out_pos || !out_val)))
        return set_err(TBA_E_ARG, "bad arguments");
    const i64 N = std::min<i64>(n_top, n);
    *out_count = 0;
    if (N == 0) return TBA_OK;
    Scratch sc(e);
    const double *d_a = sc.in(a, n), *d_b = sc.in(b, n);
    double *d_diff = sc.out<double>(n);
    u64 *d_key = sc.out<u64>(n);
    TrkSel hs{};
    hs.remaining = N;
    TrkSel *d_sel = sc.in(&hs, 1);
    i64 *d_pos = sc.out<i64>(n + 1), *d_total = sc.out<i64>(2);
    u64 *d_val = sc.out<u64>(n);
    if (sc.rc) return sc.rc;
    k_trk_diff<true><<<grid_for(n), 256, 0, e->stream>>>(n, d_a, d_b, d_diff, d_key);
    for (int shift = 56; shift >= 0; shift -= 8) {
        k_trk_hist<<<grid_for(n), 256, 0, e->stream>>>(n, d_key, shift, d_sel);
        k_trk_pick<<<1, 256, 0, e->stream>>>(shift, d_sel);
    }
    if (sc.sync() || sc.get(&hs, d_sel, 1)) return sc.rc;
    // what is above the N-th largest value, in position order, then the highest positions that equal it
    launch_compact(sc, n, TRK_KEEP_ABOVE, d_key, d_sel, (const u64 *)d_diff, d_pos, d_val, d_total);
    launch_compact(sc, n, TRK_KEEP_EQUAL, d_key, d_sel, (const u64 *)d_diff, d_pos + hs.n_above, d_val + hs.n_above,
                   d_total + 1);
    if (sc.sync()) return sc.rc;
    *out_count = N;
    if (sc.get(out_pos, d_pos, N)) return sc.rc;
    return sc.get((u64 *)out_val, d_val, N);
}

// ---- estimate_kmer_model / estimate_motif_alt_model (k_kmer_est.h) ------------------------------
namespace {
// The reads of a batch of regions as tba_region_key_levels and tba_region_level_piles take them (the pointers
// that must not be NULL whatever the sizes are the entry's own first check).  Checked on the host in two steps,
// between which an entry may place checks of its own, then uploaded.
struct RegionReadsIn {
    i64 n_reads; const int64_t *read_start; const uint8_t *read_minus; const int64_t *read_off; const double *means;
    i64 n_regions; const int64_t *reg_read_off, *reg_reads;
    i64 total = 0, n_rr = 0;   // after check_offsets: all levels, all (region, read) pairs

    int check_offsets()
    {
        if (const int rc = check_csr_off(read_off, n_reads)) return rc;
        if (const int rc = check_csr_off(reg_read_off, n_regions)) return rc;
        total = n_reads > 0 ? read_off[n_reads] : 0;
        n_rr = n_regions > 0 ? reg_read_off[n_regions] : 0;
        return TBA_OK;
    }
    int check_reads() const
    {
        if ((total > 0 && !means) || (n_rr > 0 && !reg_reads)) return set_err(TBA_E_ARG, "bad arguments");
        for (i64 q = 0; q < n_rr; q++)
            if (reg_reads[q] < 0 || reg_reads[q] >= n_reads) return set_err(TBA_E_ARG, "a region names a read outside the batch");
        return TBA_OK;
    }
    RegionReads upload(Scratch &sc) const
    {
        return RegionReads{sc.in(reg_read_off, n_regions + 1), sc.in(reg_reads, n_rr), sc.in(read_start, n_reads),
                           sc.in(read_off, n_reads + 1), sc.in(read_minus, n_reads), sc.in(means, total)};
    }
};
} // namespace

extern "C" int tba_region_key_levels(tba_engine *e, int est_mean, int64_t n_reads, const int64_t *read_start,
    const uint8_t *read_minus, const int64_t *read_off, const double *means, int64_t n_regions,
    const int64_t *reg_read_off, const int64_t *reg_reads, int64_t n_pos, const int64_t *pos_reg,
    const int64_t *pos_g, int64_t n_ent, const int64_t *ent_pos, const int64_t *ent_key, int64_t n_keys,
    int64_t *out_counts, int64_t *out_off, double *out_levels, double *out_sds)
{
    if (!e || n_reads < 0 || n_reads >= ((i64)1 << 31) || n_regions < 0 || n_pos < 0 || n_ent < 0 ||
        n_ent >= ((i64)1 << 31) || n_keys < 1 || n_keys > ((i64)1 << 24) || !read_off || !reg_read_off ||
        !out_counts || !out_off || (n_reads > 0 && (!read_start || !read_minus)) ||
        (n_pos > 0 && (!pos_reg || !pos_g)) || (n_ent > 0 && (!ent_pos || !ent_key || !out_levels || !out_sds)))
        return set_err(TBA_E_ARG, "bad arguments");
    RegionReadsIn in{n_reads, read_start, read_minus, read_off, means, n_regions, reg_read_off, reg_reads};
    if (const int rc = in.check_offsets()) return rc;
    if (const int rc = in.check_reads()) return rc;
    for (i64 p = 0; p < n_pos; p++)
        if (pos_reg[p] < 0 || pos_reg[p] >= n_regions) return set_err(TBA_E_ARG, "a position names a region outside the batch");
    for (i64 i = 0; i < n_ent; i++)
        if (ent_pos[i] < 0 || ent_pos[i] >= n_pos || ent_key[i] < 0 || ent_key[i] >= n_keys)
            return set_err(TBA_E_ARG, "an entry names a position or a key outside the batch");
    if (n_ent == 0) return empty_partition(n_keys, out_counts, out_off);
    Scratch sc(e);
    const ListedPos pos{sc.in(pos_reg, n_pos), sc.in(pos_g, n_pos)};
    const RegionReads a = in.upload(sc);
    i32 *cov = sc.out<i32>(n_pos);
    i64 *lv_off = sc.out<i64>(n_pos + 1);
    double *d_level = sc.out<double>(n_pos), *d_sd = sc.out<double>(n_pos);
    if (sc.rc) return sc.rc;
    k_region_pileup<false><<<grid_for(n_pos), 256, 0, e->stream>>>(a, pos, n_pos, cov, nullptr, nullptr);
    k_exclusive_prefix<<<1, 256, 0, e->stream>>>(n_pos, cov, lv_off, lv_off + n_pos);
    i64 n_lv = 0;
    if (sc.sync() || sc.get(&n_lv, lv_off + n_pos, 1)) return sc.rc;
    double *d_lv = sc.out<double>(n_lv);
    if (sc.rc) return sc.rc;
    k_region_pileup<true><<<grid_for(n_pos), 256, 0, e->stream>>>(a, pos, n_pos, nullptr, lv_off, d_lv);
    k_kest_moments<<<grid_for(n_pos), 256, 0, e->stream>>>(n_pos, est_mean, lv_off, d_lv, d_level, d_sd);
    if (!est_mean) {
        const i32 *has_nan = sort_segments(sc, n_pos, lv_off, d_lv);
        if (sc.rc) return sc.rc;
        k_kest_median<<<grid_for(n_pos), 256, 0, e->stream>>>(n_pos, has_nan, lv_off, d_lv, d_level);
    }
    // the entries by key
    const i64 *d_ep = sc.in(ent_pos, n_ent), *d_ek = sc.in(ent_key, n_ent);
    KeyPartition part(sc, n_ent, n_keys);
    double *d_ol = sc.out<double>(n_ent), *d_os = sc.out<double>(n_ent);
    const EntSrc ent{d_ep, d_ek, d_level, d_sd, d_ol, d_os};
    part.count(ent);
    if (sc.rc) return sc.rc;
    part.fill(ent);
    if (sc.sync()) return sc.rc;
    if (sc.get(out_counts, part.counts, n_keys) || sc.get(out_off, part.off, n_keys + 1) ||
        sc.get(out_levels, d_ol, n_ent))
        return sc.rc;
    return sc.get(out_sds, d_os, n_ent);
}

extern "C" int tba_segment_medians(tba_engine *e, const double *values, const int64_t *off, int64_t n_seg,
    double *out_medians)
{
    if (!e || !off || n_seg < 0 || (n_seg > 0 && !out_medians)) return set_err(TBA_E_ARG, "bad arguments");
    if (n_seg == 0) return TBA_OK;
    if (const int rc = check_segments(values, off, n_seg, "segment of more than 2^31 - 1 values")) return rc;
    const i64 n = off[n_seg];
    Scratch sc(e);
    double *d_v = sc.in(values, n);
    const i64 *d_off = sc.in(off, n_seg + 1);
    double *d_out = sc.out<double>(n_seg);
    const i32 *has_nan = sort_segments(sc, n_seg, d_off, d_v);
    if (sc.rc) return sc.rc;
    k_kest_median<<<grid_for(n_seg), 256, 0, e->stream>>>(n_seg, has_nan, d_off, d_v, d_out);
    if (sc.sync()) return sc.rc;
    return sc.get(out_medians, d_out, n_seg);
}

// ---- centring a k-mer model on a batch of reads (k_center.h): center_model_to_median_norm, tombo_stats.py:1599-1705 ----
// The centring step list over the uploaded batch, in two halves (the caller draws the Theil-Sen subsamples between
// them); the normalised signal stays in d_norm from the first to the second.
//   prepare  the whole raw signal normalised -- DNA: launch_normalize alone (no cumulative sum, scores or peaks);
//            RNA (get_event_scale_values, :1603-1622): run_prelude's stall detection over the reversed samples, then
//            step_scores and step_peaks, i.e. t-test scores, peaks, k_remove_stalls, event means, k_rna_event_scale
//            and the normalisation with those scale values --, k_ref_levels over the read's own bases,
//            k_center_place.  (The levels come before the placement: a read with an invalid base AND misplaced
//            events fails as an invalid sequence, the check the per-read form of the host layer makes first.)
//   fit      k_theil_sen (base means over norm + read_start + segs, as in the resquiggle pass), k_center_pick
// d_cout: factors[n][2], medians[2] (float64), n_used (int64), status[n] (int32).
struct CenterOut {
    double *factors, *medians; i64 *n_used; i32 *status;
    static size_t bytes(size_t N) { return (2 * N + 3) * 8 + N * 4; }
    CenterOut(void *p, size_t N) : factors((double *)p), medians(factors + 2 * N), n_used((i64 *)(medians + 2)), status((i32 *)(n_used + 1)) {}
};

extern "C" int tba_center_prepare(tba_engine *e, const tba_params *p, const tba_opts *o, int64_t n_reads,
    const void *raw, int raw_dtype, const int64_t *raw_off, const uint8_t *seq, const int64_t *seq_off,
    const int64_t *starts, const int64_t *start_off, const int64_t *read_start_rel_to_raw,
    const int64_t *num_events, int32_t *status, double *kernel_ms)
{
    if (!e || !p || !o || n_reads <= 0 || !starts || !start_off || !read_start_rel_to_raw || !status)
        return set_err(TBA_E_ARG, "bad centring arguments");
    const bool rna = p->use_t_test_seg != 0;
    if (rna && !num_events) return set_err(TBA_E_ARG, "RNA centring needs num_events");
    if (o->has_const_scale || o->device_subsample || o->skip_seq_scaling)
        return set_err(TBA_E_ARG, "const_scale, device_subsample and skip_seq_scaling do not apply to centring");
    if (!e->have_model) return set_err(TBA_E_STATE, "tba_set_model has not been called");
    if (e->hp.central_pos < 0 || e->hp.kmer_width - e->hp.central_pos - 1 < 1)
        return set_err(TBA_E_ARG, "centring needs a model with at least one downstream base");
    if (start_off[0] != 0) return set_err(TBA_E_ARG, "offset arrays must start at 0");
    for (i64 i = 0; i < n_reads; i++)
        if (start_off[i + 1] < start_off[i]) return set_err(TBA_E_ARG, "offset arrays must be non-decreasing");
    // DNA: the change points are not looked for (two is the least plan_batch takes); RNA: compute_num_events per read
    std::vector<i64> ne((size_t)n_reads, 2);
    if (rna) ne.assign(num_events, num_events + n_reads);
    if (int rc = tba_set_num_events(e, ne.data(), n_reads)) return rc;
    if (int rc = tba_batch_upload_async(e, p, o, n_reads, raw, raw_dtype, raw_off, seq, seq_off, nullptr, nullptr,
                                        nullptr, nullptr, nullptr)) return rc;
    const size_t N = (size_t)n_reads, n_st = (size_t)start_off[n_reads];
    if (e->d_cstart.ensure((n_st + 2 * N + 1) * 8) || e->d_cout.ensure(CenterOut::bytes(N))) return TBA_E_NOMEM;
    i64 *d_starts = e->d_cstart.as<i64>(), *d_soff = d_starts + n_st, *d_rsr = d_soff + N + 1;
    const CenterOut out(e->d_cout.p, N);
    const hipStream_t s = e->stream;
    if (n_st > 0) HIP_TRY(hipMemcpyAsync(d_starts, starts, n_st * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_soff, start_off, (N + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_rsr, read_start_rel_to_raw, N * 8, hipMemcpyHostToDevice, s));
    Run c{e};
    HIP_TRY(hipEventRecord(e->ev[0], s));
    if (int rc = run_prelude(c, TBA_STAGE_SEGMENT, TBA_STAGE_SEGMENT)) return rc;
    if (c.rna) {
        if (int rc = step_scores(c)) return rc;
        if (int rc = step_peaks(c)) return rc;
    } else launch_normalize(c, 0, 1);
    k_ref_levels<<<dim3(c.gB, c.nb), 256, 0, s>>>(c.rs, c.dp, c.seq, c.kmeans, c.ksds, c.refm, c.refs);
    e->refs_put = false;
    k_center_place<<<c.nb, 256, 0, s>>>(c.rs, c.dp, d_starts, d_soff, d_rsr, c.segs, out.status);
    HIP_TRY(hipEventRecord(e->ev[N_STEP], s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(status, out.status, N * 4, hipMemcpyDeviceToHost));
    if (kernel_ms) { float t = 0; (void)hipEventElapsedTime(&t, e->ev[0], e->ev[N_STEP]); *kernel_ms = t; }
    e->ran = e->center_ready = true;
    return 0;
}

extern "C" int tba_center_fit(tba_engine *e, const int64_t *samp_ind, const double *prior, int64_t n_prior,
    int64_t max_reads, int32_t *status, double *factors, double *medians, int64_t *n_used, double *kernel_ms)
{
    if (!e || !status || !factors || !medians || !n_used || n_prior < 0 || (n_prior > 0 && !prior) || max_reads < 1)
        return set_err(TBA_E_ARG, "bad centring arguments");
    if (!e->have_batch || !e->center_ready) return set_err(TBA_E_STATE, "tba_center_prepare has not left a batch to fit");
    e->center_ready = false; // (k_theil_sen moves the reads' scale values on: one fit per prepared batch)
    HIP_TRY(hipSetDevice(e->device));
    const size_t N = (size_t)e->n_reads, NP = (size_t)n_prior;
    if (e->d_csel.ensure((2 * (NP + N) + 2 * NP + 2) * 8)) return TBA_E_NOMEM;
    double *d_sel = e->d_csel.as<double>(), *d_prior = d_sel + 2 * (NP + N);
    const CenterOut out(e->d_cout.p, N);
    const hipStream_t s = e->stream;
    e->have_samp = samp_ind != nullptr;
    if (samp_ind) HIP_TRY(hipMemcpyAsync(e->d_samp.p, samp_ind, N * MAX_TS_POINTS * 8, hipMemcpyHostToDevice, s));
    if (NP > 0) HIP_TRY(hipMemcpyAsync(d_prior, prior, NP * 16, hipMemcpyHostToDevice, s));
    Run c{e};
    HIP_TRY(hipEventRecord(e->ev[0], s));
    if (int rc = step_theil_sen(c)) return rc;
    k_center_pick<<<1, SEL_NT, 0, s>>>(c.rs, c.n, d_prior, n_prior, max_reads, out.factors, out.status, d_sel, out.medians, out.n_used);
    HIP_TRY(hipEventRecord(e->ev[N_STEP], s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<char> h(CenterOut::bytes(N));
    HIP_TRY(hipMemcpy(h.data(), e->d_cout.p, h.size(), hipMemcpyDeviceToHost));
    const CenterOut ho(h.data(), N);
    memcpy(factors, ho.factors, N * 16);
    memcpy(status, ho.status, N * 4);
    *n_used = *ho.n_used;
    if (*ho.n_used > 0) { medians[0] = ho.medians[0]; medians[1] = ho.medians[1]; }
    if (kernel_ms) { float t = 0; (void)hipEventElapsedTime(&t, e->ev[0], e->ev[N_STEP]); *kernel_ms = t; }
    return 0;
}

// ---- region plot data (k_plot.h): the numbers of the box, quantile, density and raw-signal frames ----
namespace {
static int check_fractions(const double *q, i64 n)
{
    for (i64 i = 0; i < n; i++)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return set_err(TBA_E_ARG, "a quantile fraction outside [0, 1]");
    return TBA_OK;
}
static bool plot_coord_ok(i64 v) { return v > -((i64)1 << 62) && v < ((i64)1 << 62); }

// the two percentile forms of every segment of d_v (sorted in place here) enqueued; a failure stays in sc.rc
static void launch_percentiles(Scratch &sc, i64 n_seg, const i64 *d_off, double *d_v, i64 n_ql, const double *q_linear,
                               i64 n_qn, const double *q_nearest, double *d_lin, double *d_near)
{
    const double *d_ql = sc.in(q_linear, n_ql), *d_qn = sc.in(q_nearest, n_qn);
    const i32 *has_nan = sort_segments(sc, n_seg, d_off, d_v);
    if (sc.rc) return;
    k_plot_percentiles<<<grid_for(n_seg * (n_ql + n_qn)), 256, 0, sc.stream>>>(n_seg, has_nan, d_off, d_v, n_ql, d_ql,
        n_qn, d_qn, d_lin, d_near);
}
} // namespace

extern "C" int tba_region_level_piles(tba_engine *e, int64_t n_reads, const int64_t *read_start,
    const uint8_t *read_minus, const int64_t *read_off, const double *means, int64_t n_regions,
    const int64_t *reg_read_off, const int64_t *reg_reads, const int64_t *reg_start, const int64_t *reg_end,
    int64_t n_ql, const double *q_linear, int64_t n_qn, const double *q_nearest, int64_t *out_off,
    double *out_levels, int64_t levels_cap, double *out_lin, double *out_near, double *out_kernel_ms)
{
    if (!e || n_reads < 0 || n_reads >= ((i64)1 << 31) || n_regions < 0 || n_ql < 0 || n_qn < 0 || levels_cap < 0 ||
        !read_off || !reg_read_off || !out_off || (n_reads > 0 && (!read_start || !read_minus)) ||
        (n_regions > 0 && (!reg_start || !reg_end)) || (n_ql > 0 && !q_linear) || (n_qn > 0 && !q_nearest))
        return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    RegionReadsIn in{n_reads, read_start, read_minus, read_off, means, n_regions, reg_read_off, reg_reads};
    if (const int rc = in.check_offsets()) return rc;
    if (const int rc = check_fractions(q_linear, n_ql)) return rc;
    if (const int rc = check_fractions(q_nearest, n_qn)) return rc;
    if (const int rc = in.check_reads()) return rc;
    for (i64 q = 0; q < n_reads; q++)
        if (!plot_coord_ok(read_start[q])) return set_err(TBA_E_ARG, "a read start outside (-2^62, 2^62)");
    std::vector<i64> pos_off((size_t)n_regions + 1, 0);
    for (i64 r = 0; r < n_regions; r++) {
        if (!plot_coord_ok(reg_start[r]) || !plot_coord_ok(reg_end[r]) || reg_end[r] <= reg_start[r])
            return set_err(TBA_E_ARG, "a region must have start < end, both inside (-2^62, 2^62)");
        if (reg_read_off[r + 1] - reg_read_off[r] >= ((i64)1 << 31))
            return set_err(TBA_E_ARG, "a pile of 2^31 levels or more");
        pos_off[r + 1] = pos_off[r] + (reg_end[r] - reg_start[r]);
        if (pos_off[r + 1] >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "2^31 positions or more in one call");
    }
    const i64 n_pos = pos_off[n_regions], nq = n_ql + n_qn;
    out_off[0] = 0;
    if (n_pos == 0) return TBA_OK;
    if ((n_ql > 0 && !out_lin) || (n_qn > 0 && !out_near)) return set_err(TBA_E_ARG, "bad arguments");
    Scratch sc(e);
    const DensePos pos{n_regions, sc.in(pos_off.data(), n_regions + 1), sc.in(reg_start, n_regions)};
    const RegionReads a = in.upload(sc);
    i32 *cov = sc.out<i32>(n_pos);
    i64 *lv_off = sc.out<i64>(n_pos + 1);
    if (sc.rc) return sc.rc;
    KernelTimer tm_count(sc, out_kernel_ms != nullptr);
    k_region_pileup<false><<<grid_for(n_pos), 256, 0, sc.stream>>>(a, pos, n_pos, cov, nullptr, nullptr);
    k_exclusive_prefix<<<1, 256, 0, sc.stream>>>(n_pos, cov, lv_off, lv_off + n_pos);
    tm_count.stop();
    i64 n_lv = 0;
    if (sc.sync() || sc.get(&n_lv, lv_off + n_pos, 1) || sc.get(out_off, lv_off, n_pos + 1)) return sc.rc;
    if (out_levels && n_lv > levels_cap) return set_err(TBA_E_ARG, "levels_cap is smaller than the levels of the call");
    double *d_lv = sc.out<double>(n_lv), *d_sorted = d_lv;
    double *d_lin = sc.out<double>(n_pos * n_ql), *d_near = sc.out<double>(n_pos * n_qn);
    if (out_levels && nq > 0) d_sorted = sc.out<double>(n_lv);   // the frames want read order and the sorters work in place
    if (sc.rc) return sc.rc;
    KernelTimer tm_fill(sc, out_kernel_ms != nullptr);
    if (n_lv > 0) k_region_pileup<true><<<grid_for(n_pos), 256, 0, sc.stream>>>(a, pos, n_pos, nullptr, lv_off, d_lv);
    if (nq > 0) {
        if (d_sorted != d_lv && n_lv > 0)
            sc.hip(hipMemcpyAsync(d_sorted, d_lv, (size_t)n_lv * sizeof(double), hipMemcpyDeviceToDevice, sc.stream), "hipMemcpyAsync");
        launch_percentiles(sc, n_pos, lv_off, d_sorted, n_ql, q_linear, n_qn, q_nearest, d_lin, d_near);
    }
    tm_fill.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = tm_count.ms() + tm_fill.ms();
    if (out_levels && n_lv > 0 && sc.get(out_levels, d_lv, n_lv)) return sc.rc;
    if (n_ql > 0 && sc.get(out_lin, d_lin, n_pos * n_ql)) return sc.rc;
    return n_qn > 0 ? sc.get(out_near, d_near, n_pos * n_qn) : TBA_OK;
}

extern "C" int tba_segment_percentiles(tba_engine *e, const double *values, const int64_t *off, int64_t n_seg,
    int64_t n_ql, const double *q_linear, int64_t n_qn, const double *q_nearest, double *out_lin, double *out_near,
    double *out_kernel_ms)
{
    if (!e || !off || n_seg < 0 || n_ql < 0 || n_qn < 0 || (n_ql > 0 && !q_linear) || (n_qn > 0 && !q_nearest) ||
        (n_seg > 0 && ((n_ql > 0 && !out_lin) || (n_qn > 0 && !out_near))))
        return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (const int rc = check_fractions(q_linear, n_ql)) return rc;
    if (const int rc = check_fractions(q_nearest, n_qn)) return rc;
    if (n_seg == 0 || n_ql + n_qn == 0) return TBA_OK;
    if (n_seg >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "2^31 segments or more in one call");
    if (const int rc = check_segments(values, off, n_seg, "a pile of 2^31 levels or more")) return rc;
    const i64 n = off[n_seg];
    Scratch sc(e);
    double *d_v = sc.in(values, n);
    const i64 *d_off = sc.in(off, n_seg + 1);
    double *d_lin = sc.out<double>(n_seg * n_ql), *d_near = sc.out<double>(n_seg * n_qn);
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    launch_percentiles(sc, n_seg, d_off, d_v, n_ql, q_linear, n_qn, q_nearest, d_lin, d_near);
    tm.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    if (n_ql > 0 && sc.get(out_lin, d_lin, n_seg * n_ql)) return sc.rc;
    return n_qn > 0 ? sc.get(out_near, d_near, n_seg * n_qn) : TBA_OK;
}

// ---- read filters (k_filter.h): dwell percentiles of every read and the "stuck" flag ----
namespace {
static int check_dwell_pairs(int64_t n_pairs, const double *q, const double *thresh)
{
    if (n_pairs < 1 || !q || !thresh) return set_err(TBA_E_ARG, "bad arguments");
    if (const int rc = check_fractions(q, n_pairs)) return rc;
    for (i64 j = 0; j < n_pairs; j++)
        if (thresh[j] != thresh[j]) return set_err(TBA_E_ARG, "a NaN threshold");
    return TBA_OK;
}
static unsigned dwell_grid(i64 n_reads) { return (unsigned)std::min<i64>(n_reads, 1024); }
} // namespace

extern "C" int tba_dwell_pctl_flags(tba_engine *e, int64_t n_reads, const int64_t *segs, const int64_t *seg_off,
    int64_t n_pairs, const double *q, const double *thresh, double *out_vals, uint8_t *out_flags, double *out_kernel_ms)
{
    if (!e || n_reads < 0 || !seg_off || (n_reads > 0 && !out_flags)) return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (const int rc = check_dwell_pairs(n_pairs, q, thresh)) return rc;
    if (const int rc = check_csr_off(seg_off, n_reads)) return rc;
    const i64 total = n_reads > 0 ? seg_off[n_reads] : 0;
    if (total > 0 && !segs) return set_err(TBA_E_ARG, "bad arguments");
    for (i64 r = 0; r < n_reads; r++) {
        if (seg_off[r + 1] - seg_off[r] >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "a read of 2^31 boundaries or more");
        for (i64 i = seg_off[r]; i + 1 < seg_off[r + 1]; i++) {
            if (segs[i + 1] < segs[i]) return set_err(TBA_E_ARG, "a decreasing boundary inside a read");
            if ((u64)segs[i + 1] - (u64)segs[i] >= ((u64)1 << 31)) return set_err(TBA_E_ARG, "a length of 2^31 or more");
        }
    }
    if (n_reads == 0) return TBA_OK;
    Scratch sc(e);
    DwellArgs a{};
    a.n_reads = n_reads; a.n_pairs = n_pairs;
    a.segs = sc.in(segs, total);
    a.seg_off = sc.in(seg_off, n_reads + 1);
    a.q = sc.in(q, n_pairs);
    a.thresh = sc.in(thresh, n_pairs);
    a.vals = out_vals ? sc.out<double>(n_reads * n_pairs) : nullptr;
    a.flags = sc.out<uint8_t>(n_reads);
    if (sc.rc) return sc.rc;
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    k_dwell_pctl<false><<<dwell_grid(n_reads), DW_NT, 0, sc.stream>>>(a);
    tm.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    if (out_vals && sc.get(out_vals, a.vals, n_reads * n_pairs)) return sc.rc;
    return sc.get(out_flags, a.flags, n_reads);
}

extern "C" int tba_batch_dwell_pctl_flags(tba_engine *e, int64_t n_pairs, const double *q, const double *thresh,
    double *out_vals, uint8_t *out_flags, double *out_kernel_ms)
{
    if (!e || !e->ran) return set_err(TBA_E_STATE, "no batch has been run");
    if (!out_flags) return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (const int rc = check_dwell_pairs(n_pairs, q, thresh)) return rc;
    const i64 n_reads = e->n_reads;
    if (n_reads == 0) return TBA_OK;
    Scratch sc(e);
    sc.hip(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    DwellArgs a{};
    a.n_reads = n_reads; a.n_pairs = n_pairs;
    a.segs = e->d_segs.as<i64>();
    a.rs = e->d_rs.as<ReadState>();
    a.q = sc.in(q, n_pairs);
    a.thresh = sc.in(thresh, n_pairs);
    a.vals = out_vals ? sc.out<double>(n_reads * n_pairs) : nullptr;
    a.flags = sc.out<uint8_t>(n_reads);
    if (sc.rc) return sc.rc;
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    k_dwell_pctl<true><<<dwell_grid(n_reads), DW_NT, 0, sc.stream>>>(a);
    tm.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    if (out_vals && sc.get(out_vals, a.vals, n_reads * n_pairs)) return sc.rc;
    return sc.get(out_flags, a.flags, n_reads);
}

extern "C" int tba_region_raw_signal(tba_engine *e, int64_t n_reads, const void *raw, int raw_bytes,
    const int64_t *raw_off, const int64_t *segs, const int64_t *segs_off, const int64_t *read_start,
    const int64_t *rsrtr, const uint8_t *minus, const uint8_t *rna, const double *shift, const double *scale,
    const double *lower_lim, const double *upper_lim, int64_t n_pair, const int64_t *pair_read,
    const int64_t *pair_start, const int64_t *pair_end, int genome_centric, int64_t *out_sig_off,
    double *out_position, double *out_signal, int64_t *out_base_i, int64_t samples_cap, double *out_kernel_ms)
{
    if (!e || n_reads < 0 || n_reads >= ((i64)1 << 31) || n_pair < 0 || n_pair >= ((i64)1 << 31) || samples_cap < 0 ||
        (raw_bytes != 2 && raw_bytes != 4) || !raw_off || !segs_off || !out_sig_off ||
        (n_reads > 0 && (!read_start || !rsrtr || !minus || !rna || !shift || !scale || !lower_lim || !upper_lim)) ||
        (n_pair > 0 && (!pair_read || !pair_start || !pair_end)))
        return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (const int rc = check_csr_off(raw_off, n_reads)) return rc;
    if (const int rc = check_csr_off(segs_off, n_reads)) return rc;
    const i64 n_raw = n_reads > 0 ? raw_off[n_reads] : 0, n_segs = n_reads > 0 ? segs_off[n_reads] : 0;
    if ((n_raw > 0 && !raw) || (n_segs > 0 && !segs)) return set_err(TBA_E_ARG, "bad arguments");
    // every read's window lies inside its signal, whichever bases a pair takes: segments non-decreasing from
    // 0 or above, read_start_rel_to_raw >= 0, the last segment end inside the signal
    for (i64 q = 0; q < n_reads; q++) {
        const i64 *S = segs + segs_off[q];
        const i64 nb = segs_off[q + 1] - segs_off[q] - 1, len = raw_off[q + 1] - raw_off[q];
        if (nb < 1) return set_err(TBA_E_ARG, "a read needs at least one base (two segment entries)");
        if (!plot_coord_ok(read_start[q])) return set_err(TBA_E_ARG, "a read start outside (-2^62, 2^62)");
        if (S[0] < 0 || rsrtr[q] < 0 || rsrtr[q] > len || S[nb] > len - rsrtr[q] || S[nb] - S[0] >= ((i64)1 << 31))
            return set_err(TBA_E_ARG, "a read's segments do not fit its raw signal");
        for (i64 k = 0; k < nb; k++)
            if (S[k + 1] < S[k]) return set_err(TBA_E_ARG, "a read's segments must be non-decreasing");
    }
    for (i64 p = 0; p < n_pair; p++) {
        const i64 q = pair_read[p];
        if (q < 0 || q >= n_reads) return set_err(TBA_E_ARG, "a pair names a read outside the batch");
        if (!plot_coord_ok(pair_start[p]) || !plot_coord_ok(pair_end[p]) || pair_end[p] <= pair_start[p])
            return set_err(TBA_E_ARG, "a pair's region must have start < end, both inside (-2^62, 2^62)");
        const i64 nb = segs_off[q + 1] - segs_off[q] - 1;
        if (pair_start[p] >= read_start[q] + nb || pair_end[p] <= read_start[q])
            return set_err(TBA_E_ARG, "a pair's read does not overlap its region");
    }
    out_sig_off[0] = 0;
    if (n_pair == 0) return TBA_OK;
    Scratch sc(e);
    PlotSigArgs a{};
    a.n_pair = n_pair; a.genome_centric = genome_centric != 0; a.raw_i32 = raw_bytes == 4;
    a.raw = sc.in((const char *)raw, (size_t)n_raw * raw_bytes);
    a.raw_off = sc.in(raw_off, n_reads + 1);
    a.segs = sc.in(segs, n_segs);
    a.segs_off = sc.in(segs_off, n_reads + 1);
    a.read_start = sc.in(read_start, n_reads);
    a.rsrtr = sc.in(rsrtr, n_reads);
    a.minus = sc.in(minus, n_reads);
    a.rna = sc.in(rna, n_reads);
    a.shift = sc.in(shift, n_reads);
    a.scale = sc.in(scale, n_reads);
    a.lower = sc.in(lower_lim, n_reads);
    a.upper = sc.in(upper_lim, n_reads);
    a.pair_read = sc.in(pair_read, n_pair);
    a.pair_start = sc.in(pair_start, n_pair);
    a.pair_end = sc.in(pair_end, n_pair);
    PlotSigGeom *geom = sc.out<PlotSigGeom>(n_pair);
    i32 *cov = sc.out<i32>(n_pair), *d_st = sc.status();
    i64 *sig_off = sc.out<i64>(n_pair + 1);
    if (sc.rc) return sc.rc;
    KernelTimer tm_sizes(sc, out_kernel_ms != nullptr);
    k_plot_sig_sizes<<<grid_for(n_pair), 256, 0, sc.stream>>>(a, geom, cov, d_st);
    k_exclusive_prefix<<<1, 256, 0, sc.stream>>>(n_pair, cov, sig_off, sig_off + n_pair);
    tm_sizes.stop();
    if (const int st = sc.sync(d_st)) return sc.rc ? sc.rc : set_err(st, "a pair failed the device's checks");
    if (sc.get(out_sig_off, sig_off, n_pair + 1)) return sc.rc;
    const i64 total = out_sig_off[n_pair];
    if (out_kernel_ms) *out_kernel_ms = tm_sizes.ms();
    if (total == 0) return TBA_OK;
    if (total > samples_cap || !out_position || !out_signal || !out_base_i)
        return set_err(TBA_E_ARG, "samples_cap is smaller than the samples of the call");
    double *d_pos = sc.out<double>(total), *d_sig = sc.out<double>(total);
    i64 *d_base = sc.out<i64>(total);
    if (sc.rc) return sc.rc;
    KernelTimer tm_fill(sc, out_kernel_ms != nullptr);
    k_plot_sig_fill<<<grid_for(total), 256, 0, sc.stream>>>(a, geom, sig_off, total, d_pos, d_sig, d_base);
    tm_fill.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) *out_kernel_ms += tm_fill.ms();
    if (sc.get(out_position, d_pos, total) || sc.get(out_signal, d_sig, total)) return sc.rc;
    return sc.get(out_base_i, d_base, total);
}

// testable slice of every read -> CSR offsets into a packed copy of (means, levels); one thread
// per read writes its (start, count), the host scans (a handful of values per read)
__global__ void k_denovo_pack(const ReadState *rs, i64 n_reads, const DevParams *dp,
    const double *bm, const double *refm, const double *refs, const i64 *pk_off, double *pm,
    double *pr, double *ps)
{
    const ReadState &r = rs[blockIdx.y];
    const i64 cp = dp->central_pos, dn = dp->kmer_width - dp->central_pos - 1;
    const i64 cnt = pk_off[blockIdx.y + 1] - pk_off[blockIdx.y];
    (void)n_reads;
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < cnt; k += (i64)gridDim.x * 256) {
        const i64 src = r.ref_off + cp + k, dst = pk_off[blockIdx.y] + k;
        pm[dst] = bm[src]; pr[dst] = refm[src]; ps[dst] = refs[src];
    }
    (void)dn;
}
__global__ void k_denovo_unpack(const ReadState *rs, const DevParams *dp, const i64 *pk_off,
    const double *pp, double *out)
{
    const ReadState &r = rs[blockIdx.y];
    const i64 cp = dp->central_pos;
    const i64 cnt = pk_off[blockIdx.y + 1] - pk_off[blockIdx.y];
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < r.B; k += (i64)gridDim.x * 256) {
        const i64 q = k - cp;
        out[r.ref_off + k] = (q >= 0 && q < cnt) ? pp[pk_off[blockIdx.y] + q] : NAN;
    }
}

extern "C" int tba_batch_de_novo_stats(tba_engine *e, int64_t fm_offset, double smallest_pval,
                                       double *pvals, int64_t n_values)
{
    if (!e || !e->have_batch || !e->finished) return set_err(TBA_E_STATE, "no finished batch");
    if (!pvals || n_values < e->z.B_tot || fm_offset < 0 || fm_offset > 64) return set_err(TBA_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->z.B_tot == 0) return 0;
    const size_t N = (size_t)e->n_reads;
    const i64 K = e->hp.kmer_width, cp = e->hp.central_pos, dn = K - cp - 1;
    // per-base means of the final signal (the Events table's norm_mean), on the device
    if (int rc = launch_base_stats(e)) return rc;
    const double *d_m = e->d_stat.as<double>();
    const unsigned gB = base_blocks(e);
    // testable positions of every successful read, packed
    std::vector<ReadState> rs(N);
    HIP_TRY(hipMemcpy(rs.data(), e->d_rs.p, N * sizeof(ReadState), hipMemcpyDeviceToHost));
    std::vector<i64> pk(N + 1, 0);
    for (size_t i = 0; i < N; i++) {
        i64 cnt = rs[i].status == TBA_OK ? rs[i].B - cp - dn : 0;
        // a read shorter than one Fisher window: "P-values vector too short" in the reference
        if (cnt < 2 * fm_offset + 1 || cnt < 1) cnt = 0;
        pk[i + 1] = pk[i] + cnt;
    }
    const i64 total = pk[N];
    Scratch sc(e);
    const i64 *d_pk = sc.in(pk.data(), N + 1);
    double *d_pm = sc.out<double>(total);
    double *d_pr = sc.out<double>(total);
    double *d_ps = sc.out<double>(total);
    double *d_pp = sc.out<double>(total);
    double *d_out = sc.out<double>(e->z.B_tot);
    if (sc.rc) return sc.rc;
    if (total > 0) {
        k_denovo_pack<<<dim3(gB, (unsigned)N), 256, 0, e->stream>>>(e->d_rs.as<ReadState>(), e->n_reads,
            e->d_dp.as<DevParams>(), d_m, e->d_refm.as<double>(), e->d_refs.as<double>(), d_pk, d_pm, d_pr, d_ps);
        k_read_pvals<<<grid_for(total), 256, 0, e->stream>>>(d_pm, d_pr, d_ps, d_pk, (i64)N, total, fm_offset, 1,
            smallest_pval, d_pp);
    }
    k_denovo_unpack<<<dim3(gB, (unsigned)N), 256, 0, e->stream>>>(e->d_rs.as<ReadState>(),
        e->d_dp.as<DevParams>(), d_pk, d_pp, d_out);
    if (sc.sync()) return sc.rc;
    return sc.get(pvals, d_out, e->z.B_tot);
}

// the two division self-tests: out[i] from (a[i], b[i])
static int c_div_selftest(tba_engine *e, void (*kernel)(const double *, const double *, i64, double *),
                          const double *a, const double *b, int64_t n, double *out)
{
    if (!e || !a || !b || !out || n < 1) return set_err(TBA_E_ARG, "bad arguments");
    Scratch sc(e);
    const double *d_a = sc.in(a, n);
    const double *d_b = sc.in(b, n);
    double *d_o = sc.out<double>(n);
    if (sc.rc) return sc.rc;
    kernel<<<grid_for(n), 256, 0, e->stream>>>(d_a, d_b, n, d_o);
    if (sc.sync()) return sc.rc;
    return sc.get(out, d_o, n);
}

extern "C" int tba_selftest_division(tba_engine *e, const double *a, const double *b, int64_t n,
                                     double *out)
{
    return c_div_selftest(e, k_c_div_check, a, b, n, out);
}

extern "C" int tba_selftest_approx_quotient(tba_engine *e, const double *a, const double *b,
                                            int64_t n, double *out)
{
    return c_div_selftest(e, k_c_rcp_check, a, b, n, out);
}

extern "C" int tba_selftest_const_division(tba_engine *e, const double *a, const double *b, int64_t n,
                                           double z_shift, double zcap, double *out)
{
    if (!e || !a || !b || !out || n < 1) return set_err(TBA_E_ARG, "bad arguments");
    Scratch sc(e);
    const double *d_a = sc.in(a, n);
    const double *d_b = sc.in(b, n);
    double *d_o = sc.out<double>(3 * n);
    if (sc.rc) return sc.rc;
    k_c_div_const_check<<<grid_for(n), 256, 0, e->stream>>>(d_a, d_b, n, z_shift, zcap, d_o);
    if (sc.sync()) return sc.rc;
    return sc.get(out, d_o, 3 * n);
}

// ---- ts.identify_stalls (tombo_stats.py:269-368), one read, host buffers --------------------
extern "C" int tba_identify_stalls(tba_engine *e, const void *raw, int raw_dtype, int64_t n,
    int64_t window_size, int64_t n_windows, int64_t mini_window_size, double threshold,
    int64_t min_consecutive_obs, int64_t edge_buffer, int64_t *ints, int64_t cap, int64_t *n_ints)
{
    if (!e || !raw || n < 1 || !n_ints || (cap > 0 && !ints)) return set_err(TBA_E_ARG, "bad arguments");
    if (raw_dtype < TBA_RAW_F64 || raw_dtype > TBA_RAW_I16) return set_err(TBA_E_ARG, "unknown raw dtype");
    if (n_windows < 2 || n_windows > 16 || mini_window_size < 1 ||
        window_size != n_windows * mini_window_size || min_consecutive_obs < 0)
        return set_err(TBA_E_ARG, "bad stall detection parameters");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *n_ints = 0;
    if (n < window_size) return TBA_OK; // tombo_stats.py:305-308
    ReadState r;
    memset(&r, 0, sizeof(r));
    r.n_raw = n;
    r.status = TBA_OK;
    DevParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.o.detect_stalls = 1;
    hp.o.stall_window_size = window_size; hp.o.stall_n_windows = n_windows;
    hp.o.stall_mini_window_size = mini_window_size; hp.o.stall_threshold = threshold;
    hp.o.stall_min_consecutive_obs = min_consecutive_obs; hp.o.stall_edge_buffer = edge_buffer;
    const i64 dev_cap = n / (min_consecutive_obs + 1) + 2;
    Scratch sc(e);
    ReadState *rs = sc.in(&r, 1);
    const DevParams *dp = sc.in(&hp, 1);
    char *d_raw = sc.in((const char *)raw, (size_t)n * raw_elem_bytes(raw_dtype));
    double *d_csum = sc.out<double>(n + 2);
    u64 *d_bits = sc.out<u64>(n / 64 + 2);
    i64 *d_ints = sc.out<i64>(dev_cap * 2);
    if (sc.rc) return sc.rc;
    hipStream_t s = e->stream;
    if (raw_dtype == TBA_RAW_I16 && window_size <= SI_MAXW) {
        const unsigned gq = (unsigned)std::min<i64>(std::max<i64>((n + SI_T - 1) / SI_T, 1), 1024);
        if (n_windows == 7) k_stall_metric_i16<7><<<dim3(gq, 1), 256, 0, s>>>(rs, dp, (int16_t *)d_raw, d_bits);
        else k_stall_metric_i16<0><<<dim3(gq, 1), 256, 0, s>>>(rs, dp, (int16_t *)d_raw, d_bits);
    } else {
        RAW_DISPATCH(raw_dtype, (k_cumsum_scores<32, RT, 1><<<1, 256, 0, s>>>(rs, 1, dp, (RT *)d_raw, d_csum)));
        const unsigned gq2 = (unsigned)std::min<i64>(std::max<i64>((n + SM_T - 1) / SM_T, 1), 1024);
        if (n_windows == 7) k_stall_metric<7><<<dim3(gq2, 1), 256, 0, s>>>(rs, dp, d_csum, d_bits);
        else k_stall_metric<0><<<dim3(gq2, 1), 256, 0, s>>>(rs, dp, d_csum, d_bits);
    }
    k_stall_runs<<<dim3(grid_for(n / 64 + 1), 1), 256, 0, s>>>(rs, dp, d_bits, d_ints);
    k_stall_merge<<<1, 64, 0, s>>>(rs, 1, dp, d_ints);
    if (sc.sync() || sc.get(&r, rs, 1)) return sc.rc;
    if (r.status != TBA_OK) return r.status;
    *n_ints = r.n_stall;
    if (r.n_stall > cap) return set_err(TBA_E_ARG, "interval buffer too small (n_ints holds the count)");
    if (r.n_stall > 0) return sc.get(ints, d_ints, r.n_stall * 2);
    return TBA_OK;
}

// ---- the documented per-read functions of tombo_stats (k_norm_api.h), batches in host buffers ----
extern "C" int tba_normalize_raw_batch(tba_engine *e, int64_t n_reads, const void *raw, int raw_dtype,
    const int64_t *raw_off, const int64_t *start, const int64_t *len, int norm_type,
    const double *sv_in, const int32_t *sv_flags, const double *channel, int has_outlier_thresh,
    double outlier_thresh, double const_scale, double *sv_out, int32_t *has_lims, double *norm,
    int32_t *status, double *out_kernel_ms)
{
    if (!e || n_reads < 0) return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (n_reads == 0) return TBA_OK;
    if (!raw || !raw_off || !start || !len || !sv_out || !has_lims || !norm || !status || (sv_flags && !sv_in))
        return set_err(TBA_E_ARG, "bad arguments");
    if (raw_dtype != TBA_RAW_F64 && raw_dtype != TBA_RAW_I16) return set_err(TBA_E_ARG, "raw dtype must be int16 or float64");
    if (norm_type < TBA_NORMTYPE_NONE || norm_type > TBA_NORMTYPE_ROBUST_MEDIAN) return set_err(TBA_E_ARG, "unknown norm type");
    if (const int rc = check_csr_off(raw_off, n_reads)) return rc;
    std::vector<i64> out_off(n_reads + 1, 0);
    bool all_given = sv_flags != nullptr;
    for (i64 r = 0; r < n_reads; r++) {
        if (start[r] < 0 || len[r] < 1 || len[r] >= ((i64)1 << 31) || start[r] > raw_off[r + 1] - raw_off[r] - len[r])
            return set_err(TBA_E_ARG, "a window is empty or does not lie inside its read");
        out_off[r + 1] = out_off[r] + len[r];
        all_given = all_given && (sv_flags[r] & 1);
    }
    if (norm_type == TBA_NORMTYPE_PA_RAW && !channel && !all_given) return set_err(TBA_E_ARG, "pA_raw needs the channel values");
    const i64 total = out_off[n_reads];
    Scratch sc(e);
    NormApiArgs a;
    memset(&a, 0, sizeof(a));
    a.n_reads = n_reads;
    const char *d_raw = sc.in((const char *)raw, (size_t)raw_off[n_reads] * raw_elem_bytes(raw_dtype));
    a.raw_off = sc.in(raw_off, n_reads + 1);
    a.start = sc.in(start, n_reads);
    a.len = sc.in(len, n_reads);
    a.out_off = sc.in(out_off.data(), n_reads + 1);
    a.sv_in = sv_in ? sc.in(sv_in, 4 * n_reads) : nullptr;
    a.sv_flags = sv_flags ? sc.in(sv_flags, n_reads) : nullptr;
    a.chan = channel ? sc.in(channel, 3 * n_reads) : nullptr;
    a.norm_type = norm_type; a.has_thresh = has_outlier_thresh != 0;
    a.outlier_thresh = outlier_thresh; a.const_scale = const_scale;
    a.sv_out = sc.out<double>(4 * n_reads);
    a.has_lims = sc.out<i32>(n_reads);
    a.status = sc.out<i32>(n_reads);
    double *d_norm = sc.out<double>(total);
    sc.zero(a.sv_out, 4 * n_reads * sizeof(double));
    sc.zero(a.has_lims, n_reads * sizeof(i32));
    if (sc.rc) return sc.rc;
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    if (raw_dtype == TBA_RAW_I16) {
        k_norm_scale<int16_t><<<dim3((unsigned)n_reads), SEL_NT, 0, e->stream>>>(a, (const int16_t *)d_raw);
        k_norm_apply<int16_t><<<grid_for(total), 256, 0, e->stream>>>(a, (const int16_t *)d_raw, d_norm);
    } else {
        k_norm_scale<double><<<dim3((unsigned)n_reads), SEL_NT, 0, e->stream>>>(a, (const double *)d_raw);
        k_norm_apply<double><<<grid_for(total), 256, 0, e->stream>>>(a, (const double *)d_raw, d_norm);
    }
    tm.stop();
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    if (sc.sync() || sc.get(sv_out, a.sv_out, 4 * n_reads) || sc.get(has_lims, a.has_lims, n_reads) ||
        sc.get(status, a.status, n_reads)) return sc.rc;
    return sc.get(norm, d_norm, total);
}

static int check_point_arrays(tba_engine *e, int64_t n_reads, const int64_t *off, std::initializer_list<const void *> arrays,
                              const void *out)
{
    if (!e || n_reads < 0 || (n_reads > 0 && (!off || !out))) return set_err(TBA_E_ARG, "bad arguments");
    if (n_reads == 0) return TBA_OK;
    if (const int rc = check_csr_off(off, n_reads)) return rc;
    for (const void *p : arrays)
        if (off[n_reads] > 0 && !p) return set_err(TBA_E_ARG, "bad arguments");
    return TBA_OK;
}

extern "C" int tba_mom_sums(tba_engine *e, int64_t n_reads, const int64_t *off, const double *event_means,
    const double *model_means, const double *model_inv_vars, double *sums)
{
    if (const int rc = check_point_arrays(e, n_reads, off, {event_means, model_means, model_inv_vars}, sums)) return rc;
    if (n_reads == 0) return TBA_OK;
    const i64 n = off[n_reads];
    Scratch sc(e);
    const i64 *d_off = sc.in(off, n_reads + 1);
    const double *d_e = sc.in(event_means, n), *d_m = sc.in(model_means, n), *d_iv = sc.in(model_inv_vars, n);
    double *d_tmp = sc.out<double>(n), *d_sums = sc.out<double>(5 * n_reads);
    if (sc.rc) return sc.rc;
    k_mom_sums<<<dim3((unsigned)n_reads), 64, 0, e->stream>>>(n_reads, d_off, d_e, d_m, d_iv, d_tmp, d_sums);
    if (sc.sync()) return sc.rc;
    return sc.get(sums, d_sums, 5 * n_reads);
}

extern "C" int tba_seg_scores(tba_engine *e, int64_t n_reads, const int64_t *off, const double *means,
    const double *ref_means, const double *ref_sds, double *scores)
{
    if (const int rc = check_point_arrays(e, n_reads, off, {means, ref_means, ref_sds}, scores)) return rc;
    if (n_reads == 0) return TBA_OK;
    const i64 n = off[n_reads];
    Scratch sc(e);
    const i64 *d_off = sc.in(off, n_reads + 1);
    const double *d_m = sc.in(means, n), *d_rm = sc.in(ref_means, n), *d_rs = sc.in(ref_sds, n);
    double *d_tmp = sc.out<double>(n), *d_scores = sc.out<double>(n_reads);
    if (sc.rc) return sc.rc;
    k_seg_scores<<<dim3((unsigned)n_reads), 64, 0, e->stream>>>(n_reads, d_off, d_m, d_rm, d_rs, d_tmp, d_scores);
    if (sc.sync()) return sc.rc;
    return sc.get(scores, d_scores, n_reads);
}

// ---- ts.trim_rna / ts.estimate_global_scale (k_trim_rna.h) ----
// One device pass of tba_trim_rna_batch over reads [g0, g1): the prefixes (n_raw[i] samples of read i) go up as one
// CSR, the kernels c_valid_cpts launches for one read run over the ReadStates of all of them (shift 0, scale 1: the
// loaders' normalised copy of a signal is the signal), then the segment SDs and the window stage.
// (int16 or float64 samples: the two types these entries take)
#define TRIM_RAW(dt_, call_)                                                                   \
    do {                                                                                       \
        if ((dt_) == TBA_RAW_I16) { typedef int16_t RT; call_; }                               \
        else { typedef double RT; call_; }                                                     \
    } while (0)
struct TrimArgs {
    i64 min_obs_per_base, width, mean_obs_per_event, mw, mr;
    double thresh_scale;
};
static int trim_rna_pass(tba_engine *e, i64 g0, i64 g1, const char *raw, int raw_dtype, const int64_t *raw_off,
                         const i64 *n_raw, const TrimArgs &a, int64_t *adapter_end, int32_t *status, int32_t *ed_form,
                         double *kernel_ms)
{
    const i64 n = g1 - g0;
    const size_t eb = raw_elem_bytes(raw_dtype);
    std::vector<ReadState> hrs(n);
    std::vector<i64> sd_off(n + 1, 0);
    memset(hrs.data(), 0, sizeof(ReadState) * n);
    i64 S = 0, E = 0, max_sds = 0;
    bool whole = true, any_long = false;
    for (i64 i = 0; i < n; i++) {
        ReadState &r = hrs[i];
        r.raw_off = S; r.n_raw = n_raw[g0 + i];
        r.ev_off = E; r.num_events = r.n_raw / a.mean_obs_per_event;
        r.shift = 0.0; r.scale = 1.0;
        // (a prefix without a score or an event: the kernels leave the read out)
        r.status = r.n_raw + 1 - 2 * a.width <= 0 || r.num_events < 1 ? TBA_INTERNAL : TBA_OK;
        whole = whole && r.n_raw == raw_off[g0 + i + 1] - raw_off[g0 + i];
        any_long = any_long || r.n_raw > TBA_LONG_RAW;
        const i64 n_sd = std::max<i64>(r.num_events - 1, 0);
        sd_off[i + 1] = sd_off[i] + n_sd;
        max_sds = std::max(max_sds, n_sd);
        S += r.n_raw; E += r.num_events;
    }
    // the prefixes as one run of samples: the reads as they lie when every prefix is its whole read
    std::vector<char> packed;
    const char *src = raw + (size_t)raw_off[g0] * eb;
    if (!whole) {
        packed.resize((size_t)S * eb);
        for (i64 i = 0; i < n; i++)
            memcpy(packed.data() + (size_t)hrs[i].raw_off * eb, raw + (size_t)raw_off[g0 + i] * eb, (size_t)hrs[i].n_raw * eb);
        src = packed.data();
    }
    // the score-free kernels (k_detect.h) as the batch pipeline takes them: past the latency form's batch size, at the
    // parameters they are compiled for (k_detect leaves reads above TBA_LONG_RAW to kernels this entry does not run)
    const bool detect = n > e->small_batch && 2 * a.width <= DT_W2MAX && a.min_obs_per_base == 3 && !any_long;
    const bool fused_scores = 2 * a.width <= 64, in_lds = max_sds <= TRIM_LDS_SDS;
    const bool widen = !fused_scores && raw_dtype != TBA_RAW_F64;
    DevParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.p.running_stat_width = a.width; dp.p.min_obs_per_base = a.min_obs_per_base;
    Scratch sc(e);
    const char *d_raw = sc.in(src, (size_t)S * eb, 64);
    double *d_norm = detect ? sc.out<double>(S + 2 + 8) : widen ? sc.out<double>(S + 8) : nullptr;
    double *d_csum = sc.out<double>(S + n + 8);
    double *d_score = sc.out<double>(S + 8);
    unsigned char *d_state = sc.out<unsigned char>(S + 64);
    i64 *d_cpts = sc.out<i64>(E);
    ReadState *d_rs = sc.in(hrs.data(), n);
    const DevParams *d_dp = sc.in(&dp, 1);
    const i64 *d_sd_off = sc.in(sd_off.data(), n + 1);
    double *d_sds = sc.out<double>(sd_off[n]);
    double *d_means = in_lds ? nullptr : sc.out<double>(sd_off[n]);
    i64 *d_end = sc.out<i64>(n);
    i32 *d_status = sc.out<i32>(n);
    if (sc.rc) return sc.rc;
    hipStream_t s = e->stream;
    const unsigned nb = (unsigned)n;
    KernelTimer tm(sc, kernel_ms != nullptr);
    if (detect) {
        TRIM_RAW(raw_dtype, (k_detect<2, RT><<<(unsigned)((n + DT_READS - 1) / DT_READS), 256, 0, s>>>(d_rs, n, d_dp, (const RT *)d_raw, d_norm, d_csum, d_score, S)));
        k_pick<<<nb, SEL_NT, 0, s>>>(d_rs, d_dp, d_csum, d_score, d_cpts, 0);
    }
    const int only_flagged = detect ? 1 : 0;
    if (fused_scores) { // (from the samples themselves: what k_detect wrote as their normalised copy is not read)
        if (cs_reads_for(n) == 20) TRIM_RAW(raw_dtype, (k_cumsum_scores<20, RT><<<(unsigned)((n + 19) / 20), 256, 0, s>>>(d_rs, n, d_dp, (const RT *)d_raw, d_score, only_flagged)));
        else TRIM_RAW(raw_dtype, (k_cumsum_scores<32, RT><<<(unsigned)((n + 31) / 32), 256, 0, s>>>(d_rs, n, d_dp, (const RT *)d_raw, d_score, only_flagged)));
    } else {
        const double *d_sig = (const double *)d_raw;
        if (widen) {
            k_trim_widen<int16_t><<<grid_for(S), 256, 0, s>>>((const int16_t *)d_raw, S, d_norm);
            d_sig = d_norm;
        }
        i64 max_raw = 1;
        for (i64 i = 0; i < n; i++) max_raw = std::max(max_raw, hrs[i].n_raw);
        k_cumsum<<<(unsigned)((n + 63) / 64), 64, 0, s>>>(d_rs, n, d_sig, d_csum);
        k_scores_dna<<<dim3(std::min(grid_for(max_raw), 128u), nb), 256, 0, s>>>(d_rs, d_dp, d_csum, d_score);
    }
    launch_peaks(a.min_obs_per_base, nb, s, d_rs, d_dp, d_score, d_state, d_csum, d_cpts, 0, only_flagged, TBA_ED_FORM_SCORES_PEAKS);
    if (sd_off[n] > 0)
        TRIM_RAW(raw_dtype, (k_trim_seg_sds<RT><<<grid_for(sd_off[n]), 256, 0, s>>>(d_rs, n, (const RT *)d_raw, d_cpts, d_sd_off, d_sds)));
    if (in_lds) k_trim_pick<true><<<nb, TRIM_NT, 0, s>>>(d_rs, d_cpts, d_sd_off, d_sds, d_means, a.mw, a.mr, a.thresh_scale, d_end, d_status);
    else k_trim_pick<false><<<nb, TRIM_NT, 0, s>>>(d_rs, d_cpts, d_sd_off, d_sds, d_means, a.mw, a.mr, a.thresh_scale, d_end, d_status);
    tm.stop();
    if (kernel_ms) *kernel_ms += tm.ms();
    if (sc.sync() || sc.get(adapter_end + g0, d_end, n) || sc.get(status + g0, d_status, n)) return sc.rc;
    if (ed_form) {
        if (sc.get(hrs.data(), d_rs, n)) return sc.rc;
        for (i64 i = 0; i < n; i++) ed_form[g0 + i] = hrs[i].ed_form;
    }
    return TBA_OK;
}

extern "C" int tba_trim_rna_batch(tba_engine *e, int64_t n_reads, const void *raw, int raw_dtype, const int64_t *raw_off,
    int64_t min_obs_per_base, int64_t running_stat_width, int64_t mean_obs_per_event, int64_t moving_window_size,
    int64_t min_running_values, double thresh_scale, int64_t max_raw_obs, int64_t *adapter_end, int32_t *status,
    int32_t *ed_form, double *out_kernel_ms)
{
    if (!e || n_reads < 0) return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (n_reads == 0) return TBA_OK;
    if (!raw_off || !adapter_end || !status) return set_err(TBA_E_ARG, "bad arguments");
    if (raw_dtype != TBA_RAW_F64 && raw_dtype != TBA_RAW_I16) return set_err(TBA_E_ARG, "raw dtype must be int16 or float64");
    if (const int rc = check_csr_off(raw_off, n_reads)) return rc;
    if (!raw && raw_off[n_reads] > 0) return set_err(TBA_E_ARG, "bad arguments");
    if (min_obs_per_base < 1 || running_stat_width < 1 || mean_obs_per_event < 1 || moving_window_size < 1 ||
        min_running_values < 1 || max_raw_obs < 1 || thresh_scale != thresh_scale)
        return set_err(TBA_E_ARG, "the segmentation and trimming parameters must be 1 or more, thresh_scale a number");
    if (moving_window_size > TRIM_MAX_WINDOW) return set_err(TBA_E_ARG, "moving_window_size above 8192");
    std::vector<i64> n_raw(n_reads);
    for (i64 i = 0; i < n_reads; i++) {
        n_raw[i] = std::min<i64>(raw_off[i + 1] - raw_off[i], max_raw_obs);
        if (n_raw[i] >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "a prefix of 2^31 samples or more");
    }
    const TrimArgs a = {min_obs_per_base, running_stat_width, mean_obs_per_event, moving_window_size, min_running_values,
                        thresh_scale};
    // passes of at most trim_budget prefix samples and TBA_MAX_BATCH_READS reads (one read at least)
    for (i64 g0 = 0; g0 < n_reads;) {
        i64 g1 = g0, tot = 0;
        while (g1 < n_reads && g1 - g0 < TBA_MAX_BATCH_READS && (g1 == g0 || tot + n_raw[g1] <= e->trim_budget)) tot += n_raw[g1++];
        if (const int rc = trim_rna_pass(e, g0, g1, (const char *)raw, raw_dtype, raw_off, n_raw.data(), a, adapter_end,
                                         status, ed_form, out_kernel_ms))
            return rc;
        g0 = g1;
    }
    return TBA_OK;
}

extern "C" int tba_engine_set_trim_budget(tba_engine *e, int64_t samples)
{
    if (!e) return set_err(TBA_E_ARG, "engine is NULL");
    e->trim_budget = samples < 1 ? TBA_TRIM_BUDGET_DEFAULT : samples;
    return 0;
}

extern "C" int tba_raw_med_mad(tba_engine *e, int64_t n_reads, const void *raw, int raw_dtype, const int64_t *raw_off,
    double *med, double *mad, double *out_kernel_ms)
{
    if (!e || n_reads < 0) return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (n_reads == 0) return TBA_OK;
    if (!raw || !raw_off || !med || !mad) return set_err(TBA_E_ARG, "bad arguments");
    if (raw_dtype != TBA_RAW_F64 && raw_dtype != TBA_RAW_I16) return set_err(TBA_E_ARG, "raw dtype must be int16 or float64");
    if (const int rc = check_csr_off(raw_off, n_reads)) return rc;
    for (i64 i = 0; i < n_reads; i++)
        if (raw_off[i + 1] - raw_off[i] < 1 || raw_off[i + 1] - raw_off[i] >= ((i64)1 << 31))
            return set_err(TBA_E_ARG, "every read needs one sample or more, and fewer than 2^31");
    Scratch sc(e);
    const char *d_raw = sc.in((const char *)raw, (size_t)raw_off[n_reads] * raw_elem_bytes(raw_dtype), 64);
    const i64 *d_off = sc.in(raw_off, n_reads + 1);
    double *d_med = sc.out<double>(n_reads), *d_mad = sc.out<double>(n_reads);
    if (sc.rc) return sc.rc;
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    TRIM_RAW(raw_dtype, (k_raw_med_mad<RT><<<dim3((unsigned)n_reads), SEL_NT, 0, e->stream>>>(d_off, (const RT *)d_raw, d_med, d_mad)));
    tm.stop();
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    if (sc.sync() || sc.get(med, d_med, n_reads)) return sc.rc;
    return sc.get(mad, d_mad, n_reads);
}

// self-test of the device-side subsample: out[t] = image of t under the keyed permutation of
// [0, n) that read `read_index` of a batch would use under `seed` (t < count <= n)
__global__ void k_c_perm_check(i64 n, u64 seed, i64 read_index, i64 count, i64 *out)
{
    const u64 key = subsample_key(seed, read_index);
    for (i64 t = (i64)blockIdx.x * 256 + threadIdx.x; t < count; t += (i64)gridDim.x * 256)
        out[t] = keyed_perm(t, n, key);
}
extern "C" int tba_selftest_subsample(tba_engine *e, int64_t n, uint64_t seed, int64_t read_index,
                                      int64_t count, int64_t *out)
{
    if (!e || !out || n < 1 || count < 1 || count > n) return set_err(TBA_E_ARG, "bad arguments");
    Scratch sc(e);
    i64 *d_o = sc.out<i64>(count);
    if (sc.rc) return sc.rc;
    k_c_perm_check<<<grid_for(count), 256, 0, e->stream>>>(n, seed, read_index, count, d_o);
    if (sc.sync()) return sc.rc;
    return sc.get(out, d_o, count);
}

// ---- host-side packer: per-read arrays -> the CSR buffers of tba_batch_upload_async ----------
// (the reader side of the reference's worker pool, resquiggle.py:1385-1486: one Python thread
// cannot copy 100 k reads/s into a batch; this does it with n_threads native threads, GIL released)
#include <thread>
extern "C" int tba_pack_reads(int64_t n_reads, const void *const *raw_ptrs, int raw_dtype,
    int reverse, const int64_t *raw_off, void *raw_out, const char *const *seq_ptrs,
    const int64_t *seq_off, uint8_t *seq_out, int n_threads)
{
    if (n_reads < 0 || !raw_off || !seq_off || (n_reads > 0 && (!raw_ptrs || !seq_ptrs || !raw_out || !seq_out)))
        return set_err(TBA_E_ARG, "bad arguments");
    if (raw_dtype < TBA_RAW_F64 || raw_dtype > TBA_RAW_I16) return set_err(TBA_E_ARG, "unknown raw dtype");
    const size_t eb = raw_elem_bytes(raw_dtype);
    // ACGT -> 0..3, anything else 255 (the engine reports TBA_INVALID_SEQ).  A function-local static
    // with an initialiser is built once under the C++11 guard: callers pack from several threads
    // (ctypes releases the GIL; ReadFeeder.prefetch runs on a helper thread).
    struct CodeTable {
        unsigned char c[256];
        CodeTable() { for (int i = 0; i < 256; i++) c[i] = 255; c[(int)'A'] = 0; c[(int)'C'] = 1; c[(int)'G'] = 2; c[(int)'T'] = 3; }
    };
    static const CodeTable table;
    const unsigned char *code = table.c;
    auto work = [&](i64 a, i64 b) {
        for (i64 i = a; i < b; i++) {
            const i64 n = raw_off[i + 1] - raw_off[i], m = seq_off[i + 1] - seq_off[i];
            char *dst = (char *)raw_out + (size_t)raw_off[i] * eb;
            const char *src = (const char *)raw_ptrs[i];
            if (!reverse) memcpy(dst, src, (size_t)n * eb);
            else if (eb == 2) { const int16_t *q = (const int16_t *)src; int16_t *d = (int16_t *)dst; for (i64 k = 0; k < n; k++) d[k] = q[n - 1 - k]; }
            else if (eb == 4) { const float *q = (const float *)src; float *d = (float *)dst; for (i64 k = 0; k < n; k++) d[k] = q[n - 1 - k]; }
            else { const double *q = (const double *)src; double *d = (double *)dst; for (i64 k = 0; k < n; k++) d[k] = q[n - 1 - k]; }
            const unsigned char *sq = (const unsigned char *)seq_ptrs[i];
            uint8_t *so = seq_out + seq_off[i];
            for (i64 k = 0; k < m; k++) so[k] = code[sq[k]];
        }
    };
    int nt = std::max(1, std::min<int>(n_threads, (int)std::min<i64>(n_reads, 256)));
    if (nt == 1) { work(0, n_reads); return 0; }
    // cut by bytes, not by reads: the reads of a sorted batch differ in length
    std::vector<std::thread> th;
    const i64 tot = raw_off[n_reads] * (i64)eb + seq_off[n_reads];
    i64 a = 0;
    for (int t = 0; t < nt; t++) {
        i64 b = a;
        const i64 goal = tot / nt * (t + 1);
        while (b < n_reads && (t == nt - 1 || raw_off[b + 1] * (i64)eb + seq_off[b + 1] <= goal)) b++;
        if (t == nt - 1) b = n_reads;
        if (b > a) th.emplace_back(work, a, b);
        a = b;
    }
    for (auto &x : th) x.join();
    return 0;
}

// sizeof of the ABI structs, so that a binding can check its mirrors without a C compiler
// ---- synthetic reads on the device (k_synth.h) --------------------------------------------------
struct tba_synth {
    int device = 0;
    hipStream_t stream = nullptr;
    i64 kmer_width = 0;
    i64 n_reads = 0, S_tot = 0, seq_tot = 0;
    int raw_dtype = TBA_RAW_I16;
    DevBuf d_kmeans, d_sp, d_seq_off, d_base_off, d_raw_off, d_seq, d_starts, d_nraw, d_raw;
    PinBuf h_sp, h_off, h_nraw;
};

extern "C" int tba_synth_create(int device, const double *kmer_means, int64_t kmer_width, tba_synth **out)
{
    if (!out || !kmer_means || kmer_width < 1 || kmer_width > 12) return set_err(TBA_E_ARG, "bad arguments");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return set_err(TBA_E_HIP, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    tba_synth *g = new tba_synth();
    g->device = device;
    g->kmer_width = kmer_width;
    const size_t n = (size_t)1 << (2 * kmer_width);
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess || g->d_kmeans.ensure(n * 8) ||
        hipMemcpy(g->d_kmeans.p, kmer_means, n * 8, hipMemcpyHostToDevice) != hipSuccess) {
        g->d_kmeans.release();
        if (g->stream) (void)hipStreamDestroy(g->stream);
        delete g;
        return set_err(TBA_E_HIP, "tba_synth_create: stream / model upload failed");
    }
    *out = g;
    return 0;
}

extern "C" void tba_synth_destroy(tba_synth *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->stream);
    for (DevBuf *b : {&g->d_kmeans, &g->d_sp, &g->d_seq_off, &g->d_base_off, &g->d_raw_off, &g->d_seq,
                      &g->d_starts, &g->d_nraw, &g->d_raw})
        b->release();
    g->h_sp.release(); g->h_off.release(); g->h_nraw.release();
    (void)hipStreamDestroy(g->stream);
    delete g;
}

// the dwell thresholds and the noise constant of k_synth.h (plain IEEE operations only: the numpy
// restatement builds the same values)
static void synth_fill(SynthParams &sp, const tba_synth_params *p, i64 kmer_width)
{
    memset(&sp, 0, sizeof(sp));
    sp.mean_dwell = p->mean_dwell; sp.min_dwell = p->min_dwell; sp.n_lead = p->n_lead; sp.n_trail = p->n_trail;
    sp.scale = p->scale; sp.offset = p->offset; sp.noise_sd = p->noise_sd;
    sp.dac_per_pa = p->dac_per_pa; sp.dac_offset = p->dac_offset;
    sp.noise_norm = 1.0 / std::sqrt((65536.0 * 65536.0 - 1.0) / 3.0);
    sp.reverse = p->reverse; sp.kmer_width = (i32)kmer_width;
    const double q = 1.0 - 1.0 / (double)p->mean_dwell;
    double t = 1.0;
    for (int k = 0; k < SYNTH_DWELL_MAX; k++) {
        t = t * q;                                   // q^(k+1) = P(dwell > k + 1)
        const double v = std::floor(4294967296.0 * (1.0 - t));
        sp.thr[k] = v >= 4294967295.0 ? 0xffffffffu : (u32)v;
    }
}

extern "C" int tba_synth_dwell_thresholds(const tba_synth_params *p, uint32_t *thr, int64_t n, double *noise_norm)
{
    if (!p || !thr || n < 0 || p->mean_dwell < 1) return set_err(TBA_E_ARG, "bad arguments");
    SynthParams sp;
    synth_fill(sp, p, 1);
    for (i64 k = 0; k < n && k < SYNTH_DWELL_MAX; k++) thr[k] = sp.thr[k];
    if (noise_norm) *noise_norm = sp.noise_norm;
    return 0;
}

extern "C" int tba_synth_generate(tba_synth *g, const tba_synth_params *p, uint64_t seed, int64_t first_read,
                                  int64_t n_reads, const int64_t *n_bases, int raw_dtype,
                                  int64_t *raw_off, int64_t *seq_off, const void **d_raw, const uint8_t **d_seq)
{
    if (!g || !p || n_reads <= 0 || !n_bases || !raw_off || !seq_off || !d_raw || !d_seq)
        return set_err(TBA_E_ARG, "bad arguments");
    if (raw_dtype != TBA_RAW_I16 && raw_dtype != TBA_RAW_F64) return set_err(TBA_E_ARG, "raw dtype must be TBA_RAW_I16 or TBA_RAW_F64");
    if (p->mean_dwell < 1 || p->min_dwell < 1 || p->min_dwell > SYNTH_DWELL_MAX || p->n_lead < 0 || p->n_trail < 0)
        return set_err(TBA_E_ARG, "bad synthesis parameters");
    HIP_TRY(hipSetDevice(g->device));
    const i64 n = n_reads, K = g->kmer_width;
    hipStream_t s = g->stream;
    HIP_TRY(hipStreamSynchronize(s));
    const size_t N = (size_t)n;
    if (g->h_sp.ensure(sizeof(SynthParams)) || g->h_off.ensure(3 * (N + 1) * 8) || g->h_nraw.ensure(N * 8)) return TBA_E_NOMEM;
    synth_fill(*g->h_sp.as<SynthParams>(), p, K);
    i64 *h_seq_off = g->h_off.as<i64>(), *h_base_off = h_seq_off + (n + 1), *h_raw_off = h_base_off + (n + 1);
    h_seq_off[0] = h_base_off[0] = 0;
    for (i64 i = 0; i < n; i++) {
        if (n_bases[i] < 1 || n_bases[i] * SYNTH_DWELL_MAX > 0x7fff0000ll) return set_err(TBA_E_ARG, "bad read length");
        h_seq_off[i + 1] = h_seq_off[i] + n_bases[i] + K - 1;
        h_base_off[i + 1] = h_base_off[i] + n_bases[i];
    }
    const i64 B_tot = h_base_off[n];
    if (g->d_sp.ensure(sizeof(SynthParams)) || g->d_seq_off.ensure((N + 1) * 8) || g->d_base_off.ensure((N + 1) * 8) ||
        g->d_raw_off.ensure((N + 1) * 8) || g->d_seq.ensure((size_t)h_seq_off[n]) ||
        g->d_starts.ensure((size_t)(B_tot + n) * 4) || g->d_nraw.ensure(N * 8))
        return TBA_E_NOMEM;
    HIP_TRY(hipMemcpyAsync(g->d_sp.p, g->h_sp.p, sizeof(SynthParams), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(g->d_seq_off.p, h_seq_off, (N + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(g->d_base_off.p, h_base_off, (N + 1) * 8, hipMemcpyHostToDevice, s));
    k_synth_plan<<<(unsigned)n, SYNTH_NT, 0, s>>>(g->d_sp.as<SynthParams>(), seed, first_read, g->d_seq_off.as<i64>(),
        g->d_base_off.as<i64>(), g->d_seq.as<uint8_t>(), g->d_starts.as<i32>(), g->d_nraw.as<i64>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(g->h_nraw.p, g->d_nraw.p, N * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const i64 *nr = g->h_nraw.as<i64>();
    h_raw_off[0] = 0;
    i64 max_b = 0;
    for (i64 i = 0; i < n; i++) { h_raw_off[i + 1] = h_raw_off[i] + nr[i]; max_b = std::max(max_b, n_bases[i]); }
    const i64 S_tot = h_raw_off[n];
    if (g->d_raw.ensure((size_t)S_tot * raw_elem_bytes(raw_dtype) + 64)) return TBA_E_NOMEM;
    HIP_TRY(hipMemcpyAsync(g->d_raw_off.p, h_raw_off, (N + 1) * 8, hipMemcpyHostToDevice, s));
    const unsigned gx = (unsigned)std::min<i64>(std::max<i64>((max_b + 4 * SYNTH_NT - 1) / (4 * SYNTH_NT), 1), 64);
    if (raw_dtype == TBA_RAW_I16)
        k_synth_raw<int16_t><<<dim3(gx, (unsigned)n), SYNTH_NT, 0, s>>>(g->d_sp.as<SynthParams>(), seed, first_read,
            g->d_seq_off.as<i64>(), g->d_base_off.as<i64>(), g->d_raw_off.as<i64>(), g->d_seq.as<uint8_t>(),
            g->d_starts.as<i32>(), g->d_kmeans.as<double>(), g->d_raw.as<int16_t>());
    else
        k_synth_raw<double><<<dim3(gx, (unsigned)n), SYNTH_NT, 0, s>>>(g->d_sp.as<SynthParams>(), seed, first_read,
            g->d_seq_off.as<i64>(), g->d_base_off.as<i64>(), g->d_raw_off.as<i64>(), g->d_seq.as<uint8_t>(),
            g->d_starts.as<i32>(), g->d_kmeans.as<double>(), g->d_raw.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(raw_off, h_raw_off, (N + 1) * 8);
    memcpy(seq_off, h_seq_off, (N + 1) * 8);
    g->n_reads = n; g->S_tot = S_tot; g->seq_tot = h_seq_off[n]; g->raw_dtype = raw_dtype;
    *d_raw = g->d_raw.p;
    *d_seq = g->d_seq.as<uint8_t>();
    return 0;
}

extern "C" int tba_synth_download(tba_synth *g, void *raw, uint8_t *seq)
{
    if (!g || g->n_reads <= 0) return set_err(TBA_E_STATE, "nothing generated");
    HIP_TRY(hipSetDevice(g->device));
    if (raw) HIP_TRY(hipMemcpy(raw, g->d_raw.p, (size_t)g->S_tot * raw_elem_bytes(g->raw_dtype), hipMemcpyDeviceToHost));
    if (seq) HIP_TRY(hipMemcpy(seq, g->d_seq.p, (size_t)g->seq_tot, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tba_abi_sizes(int64_t *out, int64_t n)
{
    if (!out || n < 3) return set_err(TBA_E_ARG, "bad arguments");
    out[0] = (int64_t)sizeof(tba_params); out[1] = (int64_t)sizeof(tba_opts);
    out[2] = (int64_t)sizeof(tba_read_result);
    if (n >= 4) out[3] = TBA_ABI_VERSION;
    return 0;
}

// the other direction: slices of one flat result array -> one destination array per read
extern "C" int tba_unpack_reads(int64_t n_reads, const void *src, int64_t elem_bytes,
    const int64_t *src_off, const int64_t *count, void *const *dst_ptrs, int n_threads)
{
    if (n_reads < 0 || elem_bytes < 1 || (n_reads > 0 && (!src || !src_off || !count || !dst_ptrs)))
        return set_err(TBA_E_ARG, "bad arguments");
    auto work = [&](i64 a, i64 b) {
        for (i64 i = a; i < b; i++)
            if (count[i] > 0 && dst_ptrs[i])
                memcpy(dst_ptrs[i], (const char *)src + (size_t)src_off[i] * (size_t)elem_bytes,
                       (size_t)count[i] * (size_t)elem_bytes);
    };
    const int nt = std::max(1, std::min<int>(n_threads, (int)std::min<i64>(n_reads, 256)));
    if (nt == 1) { work(0, n_reads); return 0; }
    std::vector<i64> acc((size_t)n_reads + 1, 0);
    for (i64 i = 0; i < n_reads; i++) acc[(size_t)i + 1] = acc[(size_t)i] + std::max<i64>(count[i], 0) + 64;
    std::vector<std::thread> th;
    i64 a = 0;
    for (int t = 0; t < nt; t++) {
        const i64 goal = acc[(size_t)n_reads] / nt * (t + 1);
        i64 b = t == nt - 1 ? n_reads : (i64)(std::upper_bound(acc.begin(), acc.end(), goal) - acc.begin()) - 1;
        b = std::max(a, std::min(b, n_reads));
        if (b > a) th.emplace_back(work, a, b);
        a = b;
    }
    for (auto &x : th) x.join();
    return 0;
}

extern "C" int tba_engine_set_dispatch(tba_engine *e, int64_t small_batch_reads, int64_t tb_wave_below)
{
    if (!e) return set_err(TBA_E_ARG, "engine is NULL");
    if (small_batch_reads >= 0) e->small_batch = small_batch_reads;
    if (tb_wave_below >= 0) e->tb_wave_below = tb_wave_below;
    return 0;
}
extern "C" int tba_engine_get_dispatch(tba_engine *e, int64_t *small_batch_reads, int64_t *tb_wave_below)
{
    if (!e) return set_err(TBA_E_ARG, "engine is NULL");
    if (small_batch_reads) *small_batch_reads = e->small_batch;
    if (tb_wave_below) *tb_wave_below = e->tb_wave_below;
    return 0;
}

extern "C" int tba_engine_set_side_stream(tba_engine *e, int mode)
{
    if (!e || mode < -1 || mode > 1) return set_err(TBA_E_ARG, "bad arguments");
    e->side_mode = mode;
    return 0;
}
extern "C" int tba_engine_last_side_stream(tba_engine *e)
{
    return e ? (e->last_side ? 1 : 0) : 0;
}

extern "C" int tba_engine_last_dp_lowreg(tba_engine *e)
{
    return e ? (e->last_dp.lowreg ? 1 : 0) : 0;
}

extern "C" int tba_engine_last_dp_const_division(tba_engine *e)
{
    return e ? (e->last_dp.cdiv_main ? 1 : 0) | (e->last_dp.cdiv_start ? 2 : 0) : 0;
}
extern "C" int tba_engine_set_dp_const_division(tba_engine *e, int mode)
{
    if (!e || mode < 0 || mode > 1) return set_err(TBA_E_ARG, "bad arguments");
    e->cdiv_auto = mode == 1;
    return 0;
}
extern "C" int tba_engine_model_const_division(tba_engine *e)
{
    return e && e->have_model && e->model_cdiv ? 1 : 0;
}

extern "C" int tba_engine_set_sharing(tba_engine *e, int n_engines)
{
    if (!e || n_engines < 1) return set_err(TBA_E_ARG, "bad arguments");
    e->n_sharing = n_engines;
    return 0;
}

// device bytes this engine's grow-only buffers hold right now (a planner budgets against the
// free memory PLUS this: a batch that fitted before still fits)
extern "C" int tba_engine_held_bytes(tba_engine *e, int64_t *bytes)
{
    if (!e || !bytes) return set_err(TBA_E_ARG, "bad arguments");
    size_t tot = 0;
    e->for_each_devbuf([&](DevBuf &b) { tot += b.cap; });
    *bytes = (int64_t)tot;
    return 0;
}

// ---- ROC / precision-recall (k_roc.h): labels of stored statistics, sorted cumulative counts ------
namespace {
static int check_roc_recs(int64_t n_blocks, const int64_t *rec_off, const int64_t *rec_pos, const double *rec_stat)
{
    if (n_blocks < 0 || !rec_off) return set_err(TBA_E_ARG, "bad arguments");
    if (const int rc = check_csr_off(rec_off, n_blocks)) return rc;
    const i64 n_rec = n_blocks > 0 ? rec_off[n_blocks] : 0;
    if (n_rec >= ((i64)1 << 31)) return set_err(TBA_E_ARG, "2^31 records or more in one call");
    if (n_rec > 0 && (!rec_pos || !rec_stat)) return set_err(TBA_E_ARG, "bad arguments");
    return TBA_OK;
}

// count / scan / scatter of the kept (record, motif) pairs under f; everything after the uploads.  f's own arrays
// are on the device already.  out_counts[n_motifs]; the pairs of all motifs back to back in the outputs.
template <class F>
static int roc_compact(Scratch &sc, F f, RocRecs R, i64 n_motifs, double *out_stats,
    uint8_t *out_has_mod, int64_t *out_index, int64_t *out_counts, double *out_kernel_ms)
{
    const unsigned nb = scan_chunks(R.n_rec);
    const i64 m = (i64)nb * n_motifs;
    i64 *d_cnt = sc.out<i64>(m + 1);
    double *d_stat = sc.out<double>(R.n_rec * n_motifs);
    uint8_t *d_lab = sc.out<uint8_t>(R.n_rec * n_motifs);
    i64 *d_idx = out_index ? sc.out<i64>(R.n_rec * n_motifs) : nullptr;
    if (sc.rc) return sc.rc;
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    if (!sc.rc) {
        const dim3 grid(nb, (unsigned)n_motifs);
        k_chunk_total<<<grid, 256, 0, sc.stream>>>(R.n_rec, RocKept<F>{f, R}, d_cnt);
        k_exclusive_prefix<<<1, 256, 0, sc.stream>>>(m, d_cnt, d_cnt, d_cnt + m);
        k_roc_scatter<<<grid, 256, 0, sc.stream>>>(f, R, d_cnt, d_stat, d_lab, d_idx);
    }
    tm.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    std::vector<i64> base(m + 1);
    if (sc.get(base.data(), d_cnt, m + 1)) return sc.rc;
    for (i64 k = 0; k < n_motifs; k++) out_counts[k] = base[(k + 1) * nb] - base[k * nb];
    const i64 total = base[m];
    if (total == 0) return TBA_OK;
    if (sc.get(out_stats, d_stat, total) || sc.get(out_has_mod, d_lab, total)) return sc.rc;
    if (out_index) return sc.get(out_index, d_idx, total);
    return TBA_OK;
}
} // namespace

extern "C" int tba_roc_motif_labels(tba_engine *e, int64_t n_blocks, const uint8_t *blk_minus,
    const int64_t *blk_seq_start, const int64_t *seq_off, const uint8_t *seq, const int64_t *rec_off,
    const int64_t *rec_pos, const double *rec_stat, int64_t n_motifs, const int32_t *motifs,
    const uint8_t *motif_sets, int mode, int label, double *out_stats, uint8_t *out_has_mod,
    int64_t *out_index, int64_t *out_counts, double *out_kernel_ms)
{
    if (!e || !blk_minus || !blk_seq_start || !seq_off || n_motifs < 1 || n_motifs > ROC_MAX_MOTIFS || !motifs ||
        !motif_sets || (mode != 0 && mode != 1) || !out_stats || !out_has_mod || !out_counts)
        return set_err(TBA_E_ARG, "bad arguments");
    if (const int rc = check_roc_recs(n_blocks, rec_off, rec_pos, rec_stat)) return rc;
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    for (i64 k = 0; k < n_motifs; k++) out_counts[k] = 0;
    const i64 n_rec = n_blocks > 0 ? rec_off[n_blocks] : 0;
    if (const int rc = check_csr_off(seq_off, n_blocks)) return rc;
    const i64 n_seq = seq_off[n_blocks];
    if (n_seq > 0 && !seq) return set_err(TBA_E_ARG, "bad arguments");
    // the motif table of the device: length, mod_pos, mod_base, first set
    std::vector<i32> mot(4 * n_motifs);
    i64 n_sets = 0;
    for (i64 k = 0; k < n_motifs; k++) {
        const i32 len = motifs[3 * k], mp = motifs[3 * k + 1];
        if (len < 1 || len > 1024 || mp < 1 || mp > len) return set_err(TBA_E_ARG, "bad motif");
        mot[4 * k] = len; mot[4 * k + 1] = mp; mot[4 * k + 2] = motifs[3 * k + 2]; mot[4 * k + 3] = (i32)n_sets;
        n_sets += len;
    }
    if (n_rec == 0) return TBA_OK;
    Scratch sc(e);
    RocMotifLabel f{};
    f.blk_minus = sc.in(blk_minus, n_blocks);
    f.blk_seq_start = sc.in(blk_seq_start, n_blocks);
    f.seq_off = sc.in(seq_off, n_blocks + 1);
    f.seq = sc.in(seq, n_seq);
    f.mot = sc.in(mot.data(), mot.size());
    f.sets = sc.in(motif_sets, n_sets);
    f.mode = mode; f.label = label ? 1 : 0;
    RocRecs R{n_blocks, n_rec, sc.in(rec_off, n_blocks + 1), sc.in(rec_pos, n_rec), sc.in(rec_stat, n_rec)};
    return roc_compact(sc, f, R, n_motifs, out_stats, out_has_mod, out_index, out_counts, out_kernel_ms);
}

extern "C" int tba_roc_loc_labels(tba_engine *e, int64_t n_blocks, const int64_t *blk_loc, const int64_t *mod_locs,
    int64_t n_mod, const int64_t *unmod_locs, int64_t n_unmod, const int64_t *rec_off, const int64_t *rec_pos,
    const double *rec_stat, double *out_stats, uint8_t *out_has_mod, int64_t *out_index, int64_t *out_count,
    double *out_kernel_ms)
{
    if (!e || !blk_loc || n_mod < 0 || n_unmod < 0 || (n_mod > 0 && !mod_locs) || (n_unmod > 0 && !unmod_locs) ||
        !out_stats || !out_has_mod || !out_count)
        return set_err(TBA_E_ARG, "bad arguments");
    if (const int rc = check_roc_recs(n_blocks, rec_off, rec_pos, rec_stat)) return rc;
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    *out_count = 0;
    const i64 n_rec = n_blocks > 0 ? rec_off[n_blocks] : 0;
    for (i64 b = 0; b < n_blocks; b++) {
        const i64 *s = blk_loc + 4 * b;
        if (s[0] < 0 || s[1] < s[0] || s[1] > n_mod || s[2] < 0 || s[3] < s[2] || s[3] > n_unmod)
            return set_err(TBA_E_ARG, "location slice outside its list");
    }
    if (n_rec == 0) return TBA_OK;
    Scratch sc(e);
    RocLocLabel f{};
    f.blk_loc = sc.in(blk_loc, 4 * n_blocks);
    f.mod = sc.in(mod_locs, n_mod);
    f.unmod = sc.in(unmod_locs, n_unmod);
    RocRecs R{n_blocks, n_rec, sc.in(rec_off, n_blocks + 1), sc.in(rec_pos, n_rec), sc.in(rec_stat, n_rec)};
    return roc_compact(sc, f, R, 1, out_stats, out_has_mod, out_index, out_count, out_kernel_ms);
}

extern "C" int64_t tba_roc_sort_tile(void) { return ROC_SORT_TILE; }

extern "C" int tba_roc_rank_counts(tba_engine *e, int64_t n, const double *stats, const uint8_t *has_mod,
    int64_t n_ranks, const int64_t *ranks, int64_t *out_tp_at, int64_t *out_tp_total, int64_t *out_n_nan,
    double *out_kernel_ms)
{
    if (!e || n < 0 || n >= ((i64)1 << 31) || n_ranks < 0 || (n > 0 && (!stats || !has_mod)) ||
        (n_ranks > 0 && (!ranks || !out_tp_at)) || !out_tp_total || !out_n_nan)
        return set_err(TBA_E_ARG, "bad arguments");
    for (i64 j = 0; j < n_ranks; j++)
        if (ranks[j] < 0 || ranks[j] >= n || (j > 0 && ranks[j] < ranks[j - 1]))
            return set_err(TBA_E_ARG, "ranks must be non-decreasing and inside [0, n)");
    if (out_kernel_ms) out_kernel_ms[0] = out_kernel_ms[1] = 0.0;
    *out_tp_total = 0; *out_n_nan = 0;
    if (n == 0) return TBA_OK;
    Scratch sc(e);
    const double *d_stat = sc.in(stats, n);
    uint8_t *lab[2] = {sc.in(has_mod, n), sc.out<uint8_t>(n)};
    u64 *key[2] = {sc.out<u64>(n), sc.out<u64>(n)};
    const i64 *d_ranks = n_ranks > 0 ? sc.in(ranks, n_ranks) : nullptr;
    i64 *d_tp = sc.out<i64>(n_ranks);
    unsigned long long *d_hist = sc.out<unsigned long long>(ROC_HIST_BINS + 1);
    const unsigned n_tiles = (unsigned)((n + ROC_SORT_TILE - 1) / ROC_SORT_TILE);
    u32 *d_table = sc.out<u32>((i64)ROC_MAX_DIGITS * n_tiles);
    const unsigned n_tab_chunks = scan_chunks((i64)ROC_MAX_DIGITS * n_tiles), n_lab_chunks = scan_chunks(n);
    i64 *d_tab_cnt = sc.out<i64>(n_tab_chunks + 1), *d_lab_cnt = sc.out<i64>(n_lab_chunks + 1);
    i32 *d_bad = sc.status();
    if (sc.zero(d_hist, (ROC_HIST_BINS + 1) * 8)) return sc.rc;
    // keys first: the sort's passes are chosen from their histogram, on the host
    const bool timed = out_kernel_ms != nullptr;
    std::vector<unsigned long long> hist(ROC_HIST_BINS + 1);
    KernelTimer tm_keys(sc, timed);
    if (!sc.rc) k_roc_keys<<<grid_for(n), 256, 0, e->stream>>>(n, d_stat, lab[0], key[0], d_hist);
    tm_keys.stop();
    if (sc.sync() || sc.get(hist.data(), d_hist, hist.size())) return sc.rc;
    *out_n_nan = (int64_t)hist[ROC_HIST_BINS];
    KernelTimer tm_sort(sc, timed);
    int cur = 0;
    for (int pass = 0; pass < 8 && !sc.rc; pass++) {
        const int nd = pass == 0 ? 512 : 256;
        bool one_digit = false;   // a digit that holds every entry: the pass would change nothing
        for (int d = 0; d < nd; d++) one_digit |= hist[roc_hist_base(pass) + d] == (unsigned long long)n;
        if (one_digit) continue;
        const i64 m = (i64)nd * n_tiles;
        const unsigned nc = scan_chunks(m);
        k_roc_hist<<<n_tiles, 256, 0, e->stream>>>(n, pass, nd, key[cur], lab[cur], d_table);
        k_chunk_total<<<nc, 256, 0, e->stream>>>(m, ArrayCount<u32>{d_table}, d_tab_cnt);
        k_exclusive_prefix<<<1, 256, 0, e->stream>>>((i64)nc, d_tab_cnt, d_tab_cnt, d_tab_cnt + n_tab_chunks);
        k_roc_tab_apply<<<nc, 256, 0, e->stream>>>(m, d_table, d_tab_cnt);
        k_roc_scatter_pass<<<n_tiles, 256, 0, e->stream>>>(n, pass, nd, key[cur], lab[cur], d_table, key[cur ^ 1],
            lab[cur ^ 1]);
        cur ^= 1;
    }
    tm_sort.stop();
    KernelTimer tm_rank(sc, timed);
    if (!sc.rc) {
        k_chunk_total<<<n_lab_chunks, 256, 0, e->stream>>>(n, ArrayCount<uint8_t>{lab[cur]}, d_lab_cnt);
        k_exclusive_prefix<<<1, 256, 0, e->stream>>>((i64)n_lab_chunks, d_lab_cnt, d_lab_cnt, d_lab_cnt + n_lab_chunks);
        if (n_ranks > 0)
            k_roc_gather<<<grid_for(n_ranks), 256, 0, e->stream>>>(n, n_ranks, d_ranks, lab[cur], d_lab_cnt, d_tp, d_bad);
    }
    tm_rank.stop();
    const int bad = sc.sync(d_bad);
    if (sc.rc) return sc.rc;
    if (timed) { out_kernel_ms[0] = tm_keys.ms() + tm_sort.ms(); out_kernel_ms[1] = tm_rank.ms(); }
    if (bad) return set_err(TBA_E_ARG, "rank outside [0, n)");
    if (sc.get(out_tp_total, d_lab_cnt + n_lab_chunks, 1)) return sc.rc;
    return n_ranks > 0 ? sc.get(out_tp_at, d_tp, n_ranks) : TBA_OK;
}

// ---- pairwise distances between rows (k_pdist.h): get_pairwise_dists, order_reads' pdist -----------
namespace {
static int check_pdist(tba_engine *e, int64_t n_rows, int64_t row_len, const double *rows)
{
    if (!e || !rows || n_rows < 1 || row_len < 1) return set_err(TBA_E_ARG, "bad arguments");
    if (n_rows > PDIST_MAX_ROWS) return set_err(TBA_E_ARG, "more than 16384 rows in one call");
    if (row_len > PDIST_MAX_ELEMS / n_rows) return set_err(TBA_E_ARG, "more than 2^28 values in one call");
    return TBA_OK;
}
// the launch shape both modes share: one workgroup per tile of the triangle, the two row sets in LDS when they fit
struct PdistLaunch {
    unsigned blocks;
    int use_lds;
    size_t lds_bytes;
    PdistLaunch(i64 n_rows, i64 row_len)
    {
        const i64 nt = (n_rows + PDIST_TILE - 1) / PDIST_TILE;
        blocks = (unsigned)(nt * (nt + 1) / 2);
        use_lds = row_len <= PDIST_LDS_ROW_MAX;
        lds_bytes = use_lds ? (size_t)2 * PDIST_TILE * (row_len | 1) * sizeof(double) : 0;
    }
};
} // namespace

extern "C" int64_t tba_pdist_tile(void) { return PDIST_TILE; }
extern "C" int64_t tba_pdist_lds_row_max(void) { return PDIST_LDS_ROW_MAX; }

extern "C" int tba_pairwise_window_dists(tba_engine *e, int64_t n_rows, int64_t row_len, int64_t slide_span,
    const double *rows, double *out, double *out_kernel_ms)
{
    if (!out) return set_err(TBA_E_ARG, "bad arguments");
    if (const int rc = check_pdist(e, n_rows, row_len, rows)) return rc;
    if (slide_span < 0 || slide_span > row_len || row_len - 2 * slide_span < 1)
        return set_err(TBA_E_ARG, "slide_span must be >= 0 and leave a window of at least one value");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    Scratch sc(e);
    const double *d_rows = sc.in(rows, (size_t)(n_rows * row_len));
    double *d_out = sc.out<double>((size_t)(n_rows * n_rows));
    if (sc.rc) return sc.rc;
    const PdistLaunch L(n_rows, row_len);
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    if (!sc.rc)
        k_pdist_window<<<L.blocks, PDIST_TILE * PDIST_TILE, L.lds_bytes, sc.stream>>>(n_rows, row_len, slide_span,
            L.use_lds, d_rows, d_out);
    tm.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    return sc.get(out, d_out, (size_t)(n_rows * n_rows));
}

extern "C" int tba_pairwise_nanmean_dists(tba_engine *e, int64_t n_rows, int64_t row_len, const double *rows,
    double *out_condensed, double *out_kernel_ms)
{
    if (const int rc = check_pdist(e, n_rows, row_len, rows)) return rc;
    if (n_rows > 1 && !out_condensed) return set_err(TBA_E_ARG, "bad arguments");
    if (out_kernel_ms) *out_kernel_ms = 0.0;
    if (n_rows == 1) return TBA_OK;
    const size_t n_pairs = (size_t)(n_rows * (n_rows - 1) / 2);
    Scratch sc(e);
    const double *d_rows = sc.in(rows, (size_t)(n_rows * row_len));
    double *d_out = sc.out<double>(n_pairs);
    if (sc.rc) return sc.rc;
    const PdistLaunch L(n_rows, row_len);
    KernelTimer tm(sc, out_kernel_ms != nullptr);
    if (!sc.rc)
        k_pdist_nanmean<<<L.blocks, PDIST_TILE * PDIST_TILE, L.lds_bytes, sc.stream>>>(n_rows, row_len, L.use_lds,
            d_rows, d_out);
    tm.stop();
    if (sc.sync()) return sc.rc;
    if (out_kernel_ms) *out_kernel_ms = tm.ms();
    return sc.get(out_condensed, d_out, n_pairs);
}

// k_trim_rna.h -- the last two raw-signal functions of tombo_stats on the device, for a batch of reads:
//   trim_rna                 tombo_stats.py:235-267   event detection over the reads' prefixes (the batch kernels of
//                                                     k_segment.h / k_detect.h), k_trim_seg_sds, k_trim_pick
//   estimate_global_scale    tombo_stats.py:452-480   k_raw_med_mad (np.mean of the MADs stays on the host)
//
// trim_rna.  The DNA adapter at the head of a direct-RNA read is a stretch of events with little spread: the
// reference cuts the first max_raw_obs samples into num_events = n // mean_obs_per_event events with the plain
// change-point detector (th.valid_cpts_w_cap, sorted), takes the SD of every event (c_new_mean_stds), the mean of
// every moving_window_size consecutive SDs, thresh = mean of those means * thresh_scale, the minimum of every
// min_running_values consecutive means, and answers the change point at the first minimum strictly above thresh
// (0 when there is none).
//
// Order rules (the answer is a comparison of sums, so every sum keeps numpy's association):
//   SD of a segment      c_new_mean_stds (_c_helper.pyx:38-57): two left-to-right loops, sqrt(v / len)
//   mean of a row        .mean(-1) of the as_strided rows: np.add.reduce of a contiguous row / moving_window_size --
//                        eight accumulators up to 128 values, halves on 8-aligned splits beyond (np_pairwise_leaf
//                        under a plan of the tree, below); rows of more than TRIM_MAX_WINDOW values are refused
//                        by the entry (TBA_E_ARG) rather than summed in an order nobody checked
//   mean of the means    .mean() of a contiguous vector: the same pairwise tree over blocks of 8192 values, the
//                        blocks added left to right (wave_np_sum, k_scan.h)
//   minimum              np.minimum.reduce: a NaN stays a NaN (and then compares false against thresh)
// Sizes: s SDs (num_events - 1) give s - moving_window_size + 1 means and n_runs = that - min_running_values + 1
// minima.  n_runs < 0: numpy's 'negative dimensions are not allowed' (TBA_TRIM_TOO_FEW_EVENTS); n_runs == 0: the
// generator over the minima is empty, the answer is 0.
// What bounds k_trim_pick: a read's SDs and means live in LDS (TRIM_LDS_SDS doubles each: the 2 665 SDs of 40 000
// samples at 15 per event fit) -- k_trim_pick<true>; a batch in which any read has more takes k_trim_pick<false>,
// the same code over the SDs in global memory and a global row for the means.  No atomics: the same call gives the
// same bytes.
#pragma once
#include "tba_common.h"
#include "k_select.h"
#include "k_scan.h"
#include "k_norm_api.h"   // na_block_range

#define TRIM_LDS_SDS 2688   // SDs (and means) of a read that k_trim_pick<true> holds in LDS: 2 x 21 KB
#define TRIM_NT 256
#define TRIM_MAX_WINDOW 8192  // the widest row (moving_window_size) of k_trim_pick: one block of numpy's pairwise sum

// float64 copy of the samples (the detector's kernels for 2 * running_stat_width > 64 read float64 only)
template <class RT>
__global__ __launch_bounds__(256) void k_trim_widen(const RT *raw, i64 n, double *out)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) out[i] = (double)raw[i];
}

// The SDs of all reads' segments in one launch: segment j of read r lies between its change points j and j + 1
// (cpts at ev_off, num_events of them, ascending); sd_off: CSR of the reads' num_events - 1 segments.  A thread per
// segment, c_new_mean_stds' two loops.  Reads that failed event detection are left out.
template <class RT>
__global__ __launch_bounds__(256) void k_trim_seg_sds(const ReadState *rs, i64 n_reads, const RT *raw, const i64 *cpts,
                                                      const i64 *sd_off, double *sds)
{
    const i64 total = sd_off[n_reads];
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const i64 ri = dev_csr_row(sd_off, n_reads, i);
        const ReadState &r = rs[ri];
        if (r.status != TBA_OK) continue;
        const i64 j = i - sd_off[ri];
        const i64 a = cpts[r.ev_off + j], b = cpts[r.ev_off + j + 1];
        const RawSamples<RT> x{raw + r.raw_off};
        const double len = (double)(b - a);
        double acc = 0;
        for (i64 k = a; k < b; k++) acc += x[k];
        const double m = acc / len;
        double v = 0;
        for (i64 k = a; k < b; k++) { const double d = x[k] - m; v += d * d; }
        sds[i] = sqrt(v / len);
    }
}

// One workgroup per read: the window stage of trim_rna over the read's SDs.  means_g: a global row per read at
// sd_off (IN_LDS == false only).  Writes adapter_end[r] and status[r]: the read's event-detection status where that
// failed, TBA_TRIM_TOO_FEW_EVENTS, or TBA_OK.
template <bool IN_LDS>
__global__ __launch_bounds__(TRIM_NT) void k_trim_pick(const ReadState *rs, const i64 *cpts, const i64 *sd_off,
    const double *sds_g, double *means_g, i64 mw, i64 mr, double thresh_scale, i64 *adapter_end, i32 *status)
{
    __shared__ double s_sd[IN_LDS ? TRIM_LDS_SDS : 1], s_mean[IN_LDS ? TRIM_LDS_SDS : 1];
    __shared__ WaveSumLds wsl;
    __shared__ int s_adds[128];
    __shared__ double s_stack[8][TRIM_NT];
    __shared__ double s_thresh;
    __shared__ i64 s_first[TRIM_NT / 64];
    const i64 ri = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReadState &r = rs[ri];
    const i64 s = r.num_events - 1, n_means = s - mw + 1, n_runs = n_means - mr + 1;
    if (r.status != TBA_OK || n_runs <= 0) {
        if (tid == 0) {
            adapter_end[ri] = 0;
            status[ri] = r.status != TBA_OK ? r.status : n_runs < 0 ? TBA_TRIM_TOO_FEW_EVENTS : TBA_OK;
        }
        return;
    }
    const double *sd;
    double *mean;
    if constexpr (IN_LDS) {
        for (i64 i = tid; i < s; i += TRIM_NT) s_sd[i] = sds_g[sd_off[ri] + i];
        sd = s_sd; mean = s_mean;
        __syncthreads();
    } else {
        sd = sds_g + sd_off[ri]; mean = means_g + sd_off[ri];
    }
    // The pairwise tree of a row has one shape for all rows: thread 0 walks it once and leaves a plan -- the leaves
    // in visiting order, and after each the number of (left + right) additions that close finished nodes -- which
    // every thread then follows for its rows with a stack of partial sums in LDS (depth <= 7 for 8192 values).
    if (tid == 0) {
        int sp = 0, nl = 0;
        wsl.st_a[0] = 0; wsl.st_n[0] = (int)mw; wsl.st_st[0] = 0;
        while (sp >= 0) {
            const int a0 = wsl.st_a[sp], len = wsl.st_n[sp];
            if (len <= 128) { wsl.l_start[nl] = a0; wsl.l_len[nl] = len; s_adds[nl] = 0; nl++; sp--; continue; }
            int n2 = len / 2;
            n2 -= n2 % 8;
            if (wsl.st_st[sp] == 0) { wsl.st_st[sp] = 1; wsl.st_a[sp + 1] = a0; wsl.st_n[sp + 1] = n2; wsl.st_st[sp + 1] = 0; sp++; }
            else if (wsl.st_st[sp] == 1) { wsl.st_st[sp] = 2; wsl.st_a[sp + 1] = a0 + n2; wsl.st_n[sp + 1] = len - n2; wsl.st_st[sp + 1] = 0; sp++; }
            else { s_adds[nl - 1]++; sp--; }
        }
        wsl.n_leaf = nl;
    }
    __syncthreads();
    const double dmw = (double)mw;
    const int n_leaf = wsl.n_leaf;
    for (i64 i = tid; i < n_means; i += TRIM_NT) {
        int sp = 0;
        for (int l = 0; l < n_leaf; l++) {
            s_stack[sp++][tid] = np_pairwise_leaf(sd + i + wsl.l_start[l], wsl.l_len[l]);
            for (int k = s_adds[l]; k > 0; k--) { sp--; s_stack[sp - 1][tid] = s_stack[sp - 1][tid] + s_stack[sp][tid]; }
        }
        mean[i] = s_stack[0][tid] / dmw;
    }
    __syncthreads();
    // (thread 0 lists the leaves and adds them up; every thread takes leaves -- wave_np_sum strides by 64, so a
    // leaf beyond the 64th is summed by two threads, to the same value)
    const double tot = wave_np_sum(mean, n_means, wsl, tid);
    if (tid == 0) s_thresh = (tot / (double)n_means) * thresh_scale;
    __syncthreads();
    const double thresh = s_thresh;
    // the minima in index order, TRIM_NT at a time: the first one strictly above thresh ends the search
    for (i64 i0 = 0; i0 < n_runs; i0 += TRIM_NT) {
        const i64 i = i0 + tid;
        bool above = false;
        if (i < n_runs) {
            double mn = mean[i];
            for (i64 k = 1; k < mr; k++) { const double v = mean[i + k]; mn = (v < mn || v != v) ? v : mn; }
            above = mn > thresh;
        }
        const u64 b = __ballot(above);
        if (lane == 0) s_first[wave] = b ? i0 + 64 * wave + (__ffsll((unsigned long long)b) - 1) : -1;
        __syncthreads();
        i64 first = -1;
        for (int w = TRIM_NT / 64 - 1; w >= 0; w--) first = s_first[w] >= 0 ? s_first[w] : first;
        __syncthreads();
        if (first >= 0) {
            if (tid == 0) { adapter_end[ri] = cpts[r.ev_off + first]; status[ri] = TBA_OK; }
            return;
        }
    }
    if (tid == 0) { adapter_end[ri] = 0; status[ri] = TBA_OK; }
}

// np.median(raw) and np.median(np.abs(raw - median)) of every read (CSR by off, one sample or more each): the two
// exact selections of k_norm_scale's 'median' type and nothing else -- no normalised signal is written.
template <class RT>
__global__ __launch_bounds__(SEL_NT, 4) void k_raw_med_mad(const i64 *off, const RT *raw, double *med, double *mad)
{
    __shared__ BucketSmem sm;
    const i64 ri = blockIdx.x;
    const i64 n = off[ri + 1] - off[ri];
    const RawSamples<RT> x{raw + off[ri]};
    double mn = 0, mx = 0;
    na_block_range([&](i64 i) { return x[i]; }, n, &sm, mn, mx);
    const double m = block_median_fast([&](i64 i) { return x[i]; }, n, mn, mx, &sm);
    __syncthreads();
    const double e0 = fabs(mn - m), e1 = fabs(mx - m);
    const double d = block_median_fast([&](i64 i) { return fabs(x[i] - m); }, n, 0.0, e0 > e1 ? e0 : e1, &sm);
    if (threadIdx.x == 0) { med[ri] = m; mad[ri] = d; }
}

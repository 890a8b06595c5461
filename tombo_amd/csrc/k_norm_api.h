// k_norm_api.h -- the documented per-read functions of tombo_stats on the device, for a batch of reads:
//   normalize_raw_signal            tombo_stats.py:482-573   k_norm_scale, k_norm_apply
//   calc_kmer_fitted_shift_scale    :426-437 ('mom')         k_mom_sums (the 2x2 solve stays on the host)
//   get_read_seg_score              :2327-2338               k_seg_scores
//
// k_norm_scale.  One workgroup per read over the window [start, start + len) of its raw samples (int16 DAC values
// or float64).  Shift and scale by norm type, the reference's float operations in the reference's order:
//   given values                    as they are
//   'none'                          0, 1
//   'pA_raw'                        -offset, digitisation / range
//   'median'                        np.median(x), np.median(|x - shift|)
//   'median_const_scale'            np.median(x), const_scale
//   'robust_median'                 np.mean(np.percentile(x, (46.5, 53.5))), np.median(|x - shift|)
// ('pA' is 'pA_raw' followed by the moments fit, which needs the host's solve: the host hands its result in as given
// values.)  With an outlier threshold the limits are median -/+ MAD * threshold of the normalised window.
// Every median is np.median: the middle order statistic, or (lower middle + upper middle) / 2.  All of them go
// through block_median_fast (k_select.h), the bucket select with an exact range: it counts and compares only, takes
// any length from 1 up (up to 192 values are ranked directly, a flat window falls through to the radix select) and
// any value -> value map, which the deviations from a shift and the normalised window need.  The one-pass forms of
// k_normalize (block_int_medians, block_hist_medians, block_median_window) need 4096 samples or more and a scratch
// list per read; this entry serves single reads of any length and leaves them to the pipeline.
// np.percentile (linear): vi = (n - 1) q, a = x_(floor vi), b = x_(floor vi + 1), numpy's _lerp on them (k_plot.h
// states it); both order statistics from block_kth, the upper one for free when it shares the lower one's bucket.
// int16 input: numpy subtracts the two order statistics in int16 before it multiplies by the float64 weight.
// A scale of exactly 0 (a flat window, or given): status 1, nothing else is written for the read.
//
// k_norm_apply.  (x - shift) / scale, clipped as c_apply_outlier_thresh clips (_c_helper.pyx:73-87) where the read
// has limits; a grid over the samples of all reads, the read of a sample by binary search in the output offsets.
//
// Sums.  np.add.reduce of a contiguous float64 array: wave_np_sum (k_scan.h), one wavefront per read.  The
// terms are products and quotients of the inputs, so the wavefront writes them to a scratch row first (numpy
// makes the same temporaries) and sums that.
#pragma once
#include "tba_common.h"
#include "k_select.h"
#include "k_segment.h"    // raw_is_int
#include "k_scan.h"

struct NormApiArgs {
    i64 n_reads;
    const i64 *raw_off;             // CSR of the reads' raw samples
    const i64 *start, *len;         // the window of every read inside its samples, len >= 1
    const i64 *out_off;             // CSR of the windows (the normalised signal)
    const double *sv_in;            // [n][4] shift, scale, lower, upper, or NULL
    const i32 *sv_flags;            // bit 0: shift and scale given, bit 1: limits given; or NULL
    const double *chan;             // [n][3] offset, range, digitisation ('pA_raw'), or NULL
    int norm_type, has_thresh;      // TBA_NORMTYPE_*
    double outlier_thresh, const_scale;
    double *sv_out;                 // [n][4]
    i32 *has_lims, *status;         // [n]
};

// min and max of val(0 .. n - 1) over the workgroup; all threads call, all get both
template <class F>
__device__ void na_block_range(F val, i64 n, BucketSmem *sm, double &mn, double &mx)
{
    const int tid = threadIdx.x;
    mn = INFINITY; mx = -INFINITY;
    for (i64 i = tid; i < n; i += SEL_NT) { const double v = val(i); mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    for (int mm = 32; mm >= 1; mm >>= 1) {
        const double a = shfl_xor_f64(mn, mm), b = shfl_xor_f64(mx, mm);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    if ((tid & 63) == 0) { sm->redd[2 * (tid >> 6)] = mn; sm->redd[2 * (tid >> 6) + 1] = mx; }
    __syncthreads();
    mn = sm->redd[0]; mx = sm->redd[1];
    for (int w = 1; w < SEL_NT / 64; w++) {
        mn = sm->redd[2 * w] < mn ? sm->redd[2 * w] : mn;
        mx = sm->redd[2 * w + 1] > mx ? sm->redd[2 * w + 1] : mx;
    }
    __syncthreads();
}

// np.percentile(x, 100 q) of the window, linear interpolation
template <class RT, class F>
__device__ double na_percentile(F val, i64 n, double q, double mn, double mx, BucketSmem *sm)
{
    const double vi = (double)(n - 1) * q, fl = floor(vi);
    const i64 k = (i64)fl;
    const double a = block_kth(val, n, k, mn, mx, sm);
    const int found = sm->found;
    const double nxt = sm->next;
    __syncthreads();
    double b = a;
    if (k + 1 < n) b = (found & 2) ? nxt : block_kth(val, n, k + 1, mn, mx, sm);
    __syncthreads();
    const double t = vi - fl;
    double d = b - a;
    if constexpr (raw_is_int<RT>::value) d = (double)(int16_t)((int)b - (int)a);
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

template <class RT>
__global__ __launch_bounds__(SEL_NT, 4) void k_norm_scale(NormApiArgs a, const RT *raw)
{
    __shared__ BucketSmem sm;
    const i64 r = blockIdx.x;
    const int tid = threadIdx.x;
    const i64 n = a.len[r];
    const RawSamples<RT> x{raw + a.raw_off[r] + a.start[r]};
    const int flags = a.sv_flags ? a.sv_flags[r] : 0;
    double shift = 0.0, scale = 1.0, lo = 0, hi = 0;
    bool have_lims = false;
    double mn = 0, mx = 0;
    const bool given = flags & 1;
    const bool medians = !given && a.norm_type >= TBA_NORMTYPE_MEDIAN;
    if (medians || a.has_thresh) na_block_range([&](i64 i) { return x[i]; }, n, &sm, mn, mx);
    if (given) {
        shift = a.sv_in[4 * r + 0];
        scale = a.sv_in[4 * r + 1];
    } else if (a.norm_type == TBA_NORMTYPE_PA_RAW) {
        shift = -1.0 * a.chan[3 * r + 0];
        scale = a.chan[3 * r + 2] / a.chan[3 * r + 1];
    } else if (a.norm_type == TBA_NORMTYPE_ROBUST_MEDIAN) {
        auto val = [&](i64 i) { return x[i]; };
        const double p0 = na_percentile<RT>(val, n, 46.5 / 100.0, mn, mx, &sm);
        const double p1 = na_percentile<RT>(val, n, 53.5 / 100.0, mn, mx, &sm);
        shift = (p0 + p1) / 2.0;
    }
    // Up to three medians over the window, one call site (as in k_normalize):
    //   what 0: np.median(x) -> shift;   what 1: np.median(|x - shift|) -> scale;
    //   what 2, 3: np.median(norm), np.median(|norm - that|) -> the limits
    double med = 0, mad = 0;
#pragma nounroll
    for (int what = 0; what < 4; what++) {
        if (what == 0 && !(medians && a.norm_type != TBA_NORMTYPE_ROBUST_MEDIAN)) continue;
        if (what == 1) {
            if (!medians) continue;
            if (a.norm_type == TBA_NORMTYPE_MEDIAN_CONST_SCALE) { scale = a.const_scale; continue; }
        }
        if (what >= 2 && (!a.has_thresh || scale == 0.0)) break;
        auto of = [&](double xv) {
            return what == 0 ? xv : what == 1 ? fabs(xv - shift) : what == 2 ? (xv - shift) / scale
                                                                             : fabs((xv - shift) / scale - med);
        };
        auto val = [&](i64 i) { return of(x[i]); };
        // bucket range: anything works, a good guess saves refinement levels
        double rlo = 0.0, rhi;
        if (what == 0) { rlo = mn; rhi = mx; }
        else if (what == 2) { const double e0 = of(mn), e1 = of(mx); rlo = e0 < e1 ? e0 : e1; rhi = e0 > e1 ? e0 : e1; }
        else { const double e0 = of(mn), e1 = of(mx); rhi = e0 > e1 ? e0 : e1; }
        const double res = block_median_fast(val, n, rlo, rhi, &sm);
        __syncthreads();
        if (what == 0) shift = res;
        else if (what == 1) scale = res;
        else if (what == 2) med = res;
        else mad = res;
    }
    if (scale == 0.0) {
        if (tid == 0) a.status[r] = 1;
        return;
    }
    if (a.has_thresh) {
        lo = med - (mad * a.outlier_thresh);
        hi = med + (mad * a.outlier_thresh);
        have_lims = true;
    } else if (flags & 2) {
        lo = a.sv_in[4 * r + 2]; hi = a.sv_in[4 * r + 3];
        have_lims = true;
    }
    if (tid < 4) a.sv_out[4 * r + tid] = tid == 0 ? shift : tid == 1 ? scale : tid == 2 ? lo : hi;
    if (tid == 0) { a.has_lims[r] = have_lims ? 1 : 0; a.status[r] = 0; }
}

template <class RT>
__global__ __launch_bounds__(256) void k_norm_apply(NormApiArgs a, const RT *raw, double *out)
{
    const i64 total = a.out_off[a.n_reads];
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (i64)gridDim.x * blockDim.x) {
        const i64 r = dev_csr_row(a.out_off, a.n_reads, i);
        if (a.status[r] != 0) continue;
        const double shift = a.sv_out[4 * r], scale = a.sv_out[4 * r + 1];
        const double xv = (double)raw[a.raw_off[r] + a.start[r] + (i - a.out_off[r])];
        double v = (xv - shift) / scale;
        if (a.has_lims[r]) {
            const double lo = a.sv_out[4 * r + 2], hi = a.sv_out[4 * r + 3];
            v = v > hi ? hi : (v < lo ? lo : v);
        }
        out[i] = v;
    }
}

// sums[r][0 .. 4] = iv.sum(), (m * iv).sum(), (m * iv * m).sum(), (e * iv).sum(), (e * iv * m).sum() over read r's
// points (CSR by off; e event means, m model means, iv inverse variances).  One wavefront per read; tmp: one value
// per point.
__global__ __launch_bounds__(64) void k_mom_sums(i64 n_reads, const i64 *off, const double *e, const double *m,
                                                 const double *iv, double *tmp, double *sums)
{
    __shared__ WaveSumLds w;
    const i64 r = blockIdx.x;
    if (r >= n_reads) return;
    const int lane = threadIdx.x;
    const i64 o = off[r], n = off[r + 1] - o;
    double *t = tmp + o;
    for (int j = 0; j < 5; j++) {
        const double *src = iv + o;
        if (j > 0) {
            for (i64 i = lane; i < n; i += 64) {
                const double first = (j <= 2 ? m[o + i] : e[o + i]) * iv[o + i];
                t[i] = (j == 2 || j == 4) ? first * m[o + i] : first;
            }
            src = t;
        }
        __syncthreads();   // (one wavefront: orders the row's stores before the loads of the sum)
        const double s = wave_np_sum(src, n, w, lane);
        if (lane == 0) sums[5 * r + j] = s;
        __syncthreads();
    }
}

// scores[r] = np.mean(np.abs((means - ref_means) / ref_sds)) over read r's bases (CSR by off)
__global__ __launch_bounds__(64) void k_seg_scores(i64 n_reads, const i64 *off, const double *means,
                                                   const double *ref_means, const double *ref_sds, double *tmp,
                                                   double *scores)
{
    __shared__ WaveSumLds w;
    const i64 r = blockIdx.x;
    if (r >= n_reads) return;
    const int lane = threadIdx.x;
    const i64 o = off[r], n = off[r + 1] - o;
    double *t = tmp + o;
    for (i64 i = lane; i < n; i += 64) t[i] = fabs((means[o + i] - ref_means[o + i]) / ref_sds[o + i]);
    __syncthreads();
    const double s = wave_np_sum(t, n, w, lane);
    if (lane == 0) scores[r] = s / (double)n;
}

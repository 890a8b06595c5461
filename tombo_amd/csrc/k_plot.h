// k_plot.h -- the device half of the region plot data (tombo/_plot_commands.py:784-984): the numbers of
// the box, quantile, density and raw-signal frames of a batch of plot regions.
//
// Level piles (get_r_boxplot_data / get_r_quant_data / get_r_event_data over intervalData.get_base_levels,
// tombo_helper.py:1976-2032).  Region r covers [reg_start[r], reg_end[r]); its positions are numbered
// reg_pos_off[r] + i over the batch.  Steps of region_level_piles:
//   k_region_pileup<false>  (k_kmer_est.h, over DensePos) levels per position: one thread per position, the
//                         region's reads in order; a read that does not cover the position and a NaN level
//                         count nothing (the frames drop NaN; the k-mer estimation's pile-up keeps it)
//   k_exclusive_prefix    the positions' level offsets (k_scan.h)
//   k_region_pileup<true> the levels in read order; a minus-strand read is reversed to genome order
//   k_kde_classify, k_grp_sort_*   a copy of the piles sorted ascending (k_kde.h, k_group.h)
//   k_plot_percentiles    one thread per (position, quantile): np.percentile, linear and 'nearest'
// segment_percentiles is the last two steps on caller-given segments.
//
// np.percentile on a sorted pile v of n values, q the fraction numpy divides out on the host:
//   nearest  v[around((n - 1) q)]                        (round half to even: rint)
//   linear   vi = (n - 1) q, a = v[floor(vi)], b = v[min(floor(vi) + 1, n - 1)], t = vi - floor(vi):
//            a + (b - a) t, and b - (b - a) (1 - t) where t >= 0.5      (numpy's _lerp: np_pctl_ranks and
//            np_pctl_lerp of tba_common.h, shared with k_filter.h)
// Products and sums stay apart (-ffp-contract=off, tba_common.h), so the bits are numpy's.
//
// Raw signal (get_r_raw_signal_data over th.get_raw_signal, tombo_helper.py:2090-2137, and
// normalize_raw_signal with the read's stored scale values).  A pair is (read, region):
//   k_plot_sig_sizes   one thread per pair: the overlap slice of the read's segments, the start offset, the
//                      first raw sample and the sample count
//   k_exclusive_prefix the pairs' sample offsets
//   k_plot_sig_fill    one thread per output sample: its base by binary search in the pair's slice, the raw
//                      sample (whole signal reversed for RNA, window reversed for '-'), (raw - shift) / scale,
//                      the clip of c_apply_outlier_thresh, Position = (start + base + offset) + i * (1.0 / n)
// Neighbouring threads read neighbouring raw samples and write neighbouring outputs.
// No floating-point atomics, every output at a fixed place: two runs give the same bits.
#pragma once
#include "tba_common.h"
#include "k_scan.h"
#include "k_kmer_est.h"  // k_region_pileup

// the positions of k_region_pileup for plot regions: every position of every region, numbered over the batch
struct DensePos {
    static constexpr bool keep_nan = false;
    i64 n_regions;
    const i64 *reg_pos_off, *reg_start;      // per region: its first position of the batch, its genomic start
    __device__ void locate(i64 p, i64 &r, i64 &g) const
    {
        r = dev_csr_row(reg_pos_off, n_regions, p);
        g = reg_start[r] + (p - reg_pos_off[r]);
    }
};

// One thread per (segment, quantile): the n_ql linear quantiles, then the n_qn nearest ones.  v: the
// segments sorted ascending unless has_nan; an empty segment and one with a NaN give NaN.
__global__ void k_plot_percentiles(i64 n_seg, const i32 *has_nan, const i64 *off, const double *v, i64 n_ql,
    const double *ql, i64 n_qn, const double *qn, double *lin, double *near)
{
    const i64 nq = n_ql + n_qn, total = n_seg * nq;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (i64)gridDim.x * blockDim.x) {
        const i64 s = i / nq, j = i - s * nq;
        const double *x = v + off[s];
        const i64 n = off[s + 1] - off[s];
        const bool none = n == 0 || has_nan[s];
        if (j < n_ql) {
            double res = NAN;
            if (!none) {
                i64 lo, hi;
                double t;
                np_pctl_ranks(n, ql[j], lo, hi, t);
                res = np_pctl_lerp(x[lo], x[hi], t);
            }
            lin[s * n_ql + j] = res;
        } else {
            const i64 k = j - n_ql;
            near[s * n_qn + k] = none ? NAN : x[(i64)rint((double)(n - 1) * qn[k])];
        }
    }
}

struct PlotSigArgs {
    i64 n_pair;
    int genome_centric, raw_i32;             // raw_i32: the raw samples are int32_t (else int16_t)
    const void *raw;                         // the stored DAC values of the reads, CSR by raw_off
    const i64 *raw_off, *segs, *segs_off;    // segs: per read its base starts and the end, CSR by segs_off
    const i64 *read_start, *rsrtr;           // genomic start; read_start_rel_to_raw
    const uint8_t *minus, *rna;
    const double *shift, *scale, *lower, *upper;
    const i64 *pair_read, *pair_start, *pair_end;
};

// what k_plot_sig_sizes leaves per pair for k_plot_sig_fill
struct PlotSigGeom {
    i64 lo, n_ov;        // the overlap slice segs[lo : lo + n_ov] of the read's strand-oriented segments
    i64 start_offset;    // bases of the region in front of the slice (after the read-centric flip)
    i64 raw0;            // index of the window's first sample in the (RNA: reversed) signal
};

// entry k of the read's segments as get_raw_signal orients them: segs[-1] - segs[::-1] for '-'
__device__ __forceinline__ i64 plot_seg_at(const i64 *S, i64 nb, bool minus, i64 k)
{
    return minus ? S[nb] - S[nb - k] : S[k];
}

// entry k of the pair's overlap slice; flip: _plot_commands.py:948-949, ov[-1] - ov[::-1]
__device__ __forceinline__ i64 plot_ov_at(const i64 *S, i64 nb, bool minus, bool flip, const PlotSigGeom &g, i64 k)
{
    if (!flip) return plot_seg_at(S, nb, minus, g.lo + k);
    return plot_seg_at(S, nb, minus, g.lo + g.n_ov - 1) - plot_seg_at(S, nb, minus, g.lo + g.n_ov - 1 - k);
}

// One thread per pair.  cov: its sample count.  A pair the host checks should have refused (no overlap,
// a window outside the signal) gets no samples and sets *status.
__global__ void k_plot_sig_sizes(PlotSigArgs a, PlotSigGeom *geom, i32 *cov, i32 *status)
{
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < a.n_pair; p += (i64)gridDim.x * blockDim.x) {
        const i64 rd = a.pair_read[p], is = a.pair_start[p], ie = a.pair_end[p];
        const i64 *S = a.segs + a.segs_off[rd];
        const i64 nb = a.segs_off[rd + 1] - a.segs_off[rd] - 1, rs = a.read_start[rd];
        const bool minus = a.minus[rd];
        PlotSigGeom g{};
        cov[p] = 0;
        if (nb < 1 || is >= rs + nb || ie <= rs) { geom[p] = g; *status = TBA_INTERNAL; continue; }
        g.start_offset = is < rs ? rs - is : 0;
        g.lo = is < rs ? 0 : is - rs;
        const i64 hi = ie - rs + 1 < nb + 1 ? ie - rs + 1 : nb + 1;     // the slice's stop
        g.n_ov = hi - g.lo;
        const i64 first = plot_seg_at(S, nb, minus, g.lo), last = plot_seg_at(S, nb, minus, hi - 1);
        const i64 n_obs = last - first;
        g.raw0 = a.rsrtr[rd] + (minus ? plot_seg_at(S, nb, true, nb) - last : first);
        if (!a.genome_centric && minus && g.n_ov < ie - is) g.start_offset = ie - is - g.n_ov - g.start_offset;
        geom[p] = g;
        if (n_obs < 0 || n_obs >= ((i64)1 << 31) || g.raw0 < 0 || g.raw0 + n_obs > a.raw_off[rd + 1] - a.raw_off[rd]) {
            *status = TBA_INTERNAL;
            continue;
        }
        cov[p] = (i32)n_obs;
    }
}

// One thread per output sample.  sig_off: n_pair + 1 offsets.
__global__ void k_plot_sig_fill(PlotSigArgs a, const PlotSigGeom *geom, const i64 *sig_off, i64 total,
    double *position, double *signal, i64 *base_i)
{
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (i64)gridDim.x * blockDim.x) {
        const i64 p = dev_csr_row(sig_off, a.n_pair, i);
        const i64 t = i - sig_off[p], n_obs = sig_off[p + 1] - sig_off[p];
        const PlotSigGeom g = geom[p];
        const i64 rd = a.pair_read[p];
        const i64 *S = a.segs + a.segs_off[rd];
        const i64 nb = a.segs_off[rd + 1] - a.segs_off[rd] - 1;
        const bool minus = a.minus[rd], flip = !a.genome_centric && minus;
        // the base of sample t: the last k in [0, n_ov - 2] with ov[k] - ov[0] <= t (bases of no sample are passed over)
        const i64 ov0 = plot_ov_at(S, nb, minus, flip, g, 0);
        i64 lo = 0, hi = g.n_ov - 2;
        while (lo < hi) {
            const i64 mid = (lo + hi + 1) >> 1;
            if (plot_ov_at(S, nb, minus, flip, g, mid) - ov0 <= t) lo = mid; else hi = mid - 1;
        }
        const i64 b0 = plot_ov_at(S, nb, minus, flip, g, lo) - ov0, b1 = plot_ov_at(S, nb, minus, flip, g, lo + 1) - ov0;
        // np.linspace(0, 1, n, endpoint=False): the step once, times the index; the integer part is added last
        const double step = 1.0 / (double)(b1 - b0);
        position[i] = (double)(a.pair_start[p] + lo + g.start_offset) + (double)(t - b0) * step;
        base_i[i] = lo;
        const i64 u = flip ? n_obs - 1 - t : t;                        // index into get_raw_signal's r_sig
        const i64 j = g.raw0 + (minus ? n_obs - 1 - u : u);            // ... into the (RNA: reversed) signal
        const i64 n_raw = a.raw_off[rd + 1] - a.raw_off[rd];
        const i64 k = a.raw_off[rd] + (a.rna[rd] ? n_raw - 1 - j : j);
        const double raw = a.raw_i32 ? (double)((const int32_t *)a.raw)[k] : (double)((const int16_t *)a.raw)[k];
        const double v = (raw - a.shift[rd]) / a.scale[rd];
        const double lower = a.lower[rd], upper = a.upper[rd];
        signal[i] = lower != lower || upper != upper ? v : v > upper ? upper : v < lower ? lower : v;
    }
}

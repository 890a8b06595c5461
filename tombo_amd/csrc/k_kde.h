// k_kde.h -- the device half of estimate_alt_model (tombo_stats.py:1747-2098): the base levels of a
// batch of reads gathered by k-mer (_parse_base_levels_worker, :1747-1776) and the Gaussian kernel
// density of each k-mer's levels on a grid (est_kernel_density, :1914-1939).
//
// Gather.  The reads are concatenated in read order (CSR by read_off: levels and base codes share
// the offsets), so "read order, then position order" is ascending flat position p: the gather is a
// stable partition of the window starts p by k-mer (k_scan.h), KmerSrc its source of keys:
//   k_key_partition<false>  per chunk of positions a row of 4^K counters
//   k_kmer_colscan          per k-mer the exclusive prefix of its counters over the chunks, its total
//   k_exclusive_prefix      the k-mers' level offsets
//   k_key_partition<true>   the levels: lv_off[kmer] + the chunk's prefix + the rank inside the step
// The windows of a homopolymer run cost what any other 64 windows cost.
//
// Density.  dens[s][g] = sum_i exp(-0.5 ((x_g - l_i) / h)^2) / (n h sqrt(2 pi)) over the levels of
// segment s, which is gaussian_kde(l, bw_method=h / l.std(ddof=1)).evaluate(x).
//   k_kde_classify   per segment: its size, whether it holds a NaN, its sorter class of k_group.h
//   k_grp_sort_*     the segment sorted ascending in place (k_group.h)
//   k_kde_eval       one thread per (segment, grid point)
// Grid points lie across the lanes and every lane walks the sorted levels itself: float64 exp is a
// software routine of some forty VALU instructions, whichever way the work is split the number of
// exp calls is the same, and this split needs no cross-lane reduction and no LDS.  The sum runs in
// ascending level order in four interleaved partial sums (level index mod 4), combined as
// (s0 + s1) + (s2 + s3): a fixed order, and four independent dependency chains.
// Cut-off: exp(-a) rounds to zero in float64 once a > 1075 ln 2 = 745.14, i.e. for
// |x_g - l_i| / h > sqrt(2 * 745.14) = 38.604.  A lane walks the levels within KDE_CUT = 38.7
// bandwidths of its grid point (two binary searches), widened to multiples of four levels; every
// level left out contributes exactly zero.
#pragma once
#include "tba_common.h"
#include "k_scan.h"
#include "k_group.h"    // GRP_WAVE_MAX, GRP_LDS_MAX: the sorters' classes

#define KDE_CUT 38.7

// the window starts of a read batch as the items of k_key_partition: the key of flat position p is the k-mer
// of the window that starts there; -1: the window leaves its read, holds a base outside ACGT or its k-mer is
// completed.  The level of the window's central base is what is gathered.
struct KmerSrc {
    i64 n_reads;
    int K, cp;
    const i64 *read_off;
    const uint8_t *codes, *completed;
    const double *means;
    double *levels;

    __device__ i64 key(i64 p) const
    {
        const i64 r = dev_csr_row(read_off, n_reads, p);
        if (p + K > read_off[r + 1]) return -1;
        const i64 k = window_kmer(codes + p, K);
        return k >= 0 && !completed[k] ? k : -1;
    }
    __device__ void store(i64 p, i64 o) const { levels[o] = means[p + cp]; }
};

// rows[chunk][key] of a partition: the counts become each chunk's starting rank, counts[key] the key's total
__global__ void k_kmer_colscan(i64 n_kmers, i64 n_chunks, u32 *rows, i64 *counts)
{
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < n_kmers; q += (i64)gridDim.x * blockDim.x) {
        i64 run = 0;
        for (i64 c = 0; c < n_chunks; c++) {
            const u32 t = rows[c * n_kmers + q];
            rows[c * n_kmers + q] = (u32)run;
            run += t;
        }
        counts[q] = run;
    }
}

// One wavefront per segment.  cov[s]: its size; has_nan[s]; lists: [0, S) wave, [S, 2S) workgroup,
// [2S, 3S) global sorter class of the segments with more than one level and no NaN; counts[3].
__global__ void k_kde_classify(i64 n_seg, const i64 *lv_off, const double *levels, i32 *cov, i32 *has_nan,
                               i64 *lists, u32 *counts)
{
    const int lane = threadIdx.x & 63;
    const i64 wave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const i64 n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 s = wave; s < n_seg; s += n_waves) {
        const i64 n = lv_off[s + 1] - lv_off[s];
        const double *seg = levels + lv_off[s];
        bool bad = false;
        for (i64 i = lane; i < n; i += 64) { const double v = seg[i]; bad = bad || v != v; }
        const bool any = __ballot(bad) != 0;
        if (lane == 0) {
            cov[s] = (i32)n;
            has_nan[s] = any;
            if (!any && n > 1) {
                const int c = n <= GRP_WAVE_MAX ? 0 : n <= GRP_LDS_MAX ? 1 : 2;
                lists[(i64)c * n_seg + atomicAdd(&counts[c], 1u)] = s;
            }
        }
    }
}

// blockIdx.y: 256 grid points; blockIdx.x strides over the segments.  levels: sorted per segment.
// n < 2 or a NaN level: a row of NaN (scipy raises for n < 2; NaN levels make its covariance NaN).
__global__ void __launch_bounds__(256) k_kde_eval(i64 n_seg, const i32 *cov, const i32 *has_nan, const i64 *lv_off,
    const double *levels, const double *x, i64 G, double h, double *dens)
{
    const i64 g = (i64)blockIdx.y * 256 + threadIdx.x;
    if (g >= G) return;
    const double xg = x[g], reach = KDE_CUT * h;
    for (i64 s = blockIdx.x; s < n_seg; s += gridDim.x) {
        const i64 n = cov[s];
        if (n < 2 || has_nan[s]) { dens[s * G + g] = NAN; continue; }
        const double *seg = levels + lv_off[s];
        // [lo, hi): the levels within reach of xg
        i64 lo = 0, hi, b = n;
        while (lo < b) { const i64 m = (lo + b) >> 1; if (seg[m] < xg - reach) lo = m + 1; else b = m; }
        hi = lo; b = n;
        while (hi < b) { const i64 m = (hi + b) >> 1; if (seg[m] <= xg + reach) hi = m + 1; else b = m; }
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        i64 i = lo & ~(i64)3;
        for (; i + 4 <= n && i < hi; i += 4) {
            const double t0 = (xg - seg[i]) / h, t1 = (xg - seg[i + 1]) / h;
            const double t2 = (xg - seg[i + 2]) / h, t3 = (xg - seg[i + 3]) / h;
            s0 += exp(-0.5 * (t0 * t0));
            s1 += exp(-0.5 * (t1 * t1));
            s2 += exp(-0.5 * (t2 * t2));
            s3 += exp(-0.5 * (t3 * t3));
        }
        if (i < hi) {   // the last one to three levels of the segment
            const double t0 = (xg - seg[i]) / h;
            s0 += exp(-0.5 * (t0 * t0));
            if (i + 1 < n) { const double t1 = (xg - seg[i + 1]) / h; s1 += exp(-0.5 * (t1 * t1)); }
            if (i + 2 < n) { const double t2 = (xg - seg[i + 2]) / h; s2 += exp(-0.5 * (t2 * t2)); }
        }
        dens[s * G + g] = ((s0 + s1) + (s2 + s3)) / ((double)n * h * 2.50662827463100050242);
    }
}

// k_group.h -- level pileups across many reads per genomic position: the group (two-sample)
// tests of level_sample_compare (compute_group_reg_stats, tombo_stats.py:4236-4398) and the
// control-sample reference levels of model_sample_compare (get_reads_ref, :3627-3673).
//
// One launch sequence serves a batch of regions.  Region r covers the extended interval
// [start - fm, end + fm) (its length L_r); its positions are numbered gp = pos_off[r] + i over
// the batch.  Per position there are two segments (k = 2 gp + group, group 1 = control) in one
// level buffer: the valid (non-NaN) levels of the region's reads in READ ORDER (a per-thread
// cursor over the reads in input order, no atomics), sorted in place afterwards where a test
// needs them sorted.  Steps:
//   k_grp_pileup<false>  coverage per segment (one thread per position, reads in input order)
//   k_grp_scan           one wavefront per region: level offsets, coverage runs, compact index
//   k_grp_pileup<true>   the levels themselves
//   k_grp_classify       segments to sort -> wave (n <= 64) / workgroup-LDS (n <= 4096) / global
//   k_grp_sort_*         ascending sort (bitonic; the LDS and global classes share one network)
//   k_grp_test           KS / U / t per position, one merge walk over the two sorted segments
//   k_grp_window         Fisher's method / window mean over each run, compacted output
//   k_ref_moments, k_ref_finish   get_reads_ref: mean / np.std in read order, median, prior blend
#pragma once
#include "tba_common.h"
#include "k_scan.h"

#define GRP_WAVE_MAX 64
#define GRP_LDS_MAX 4096   // 32 KB of doubles per workgroup (four workgroups per CU by LDS)

struct GrpArgs {
    i64 n_regions, n_pos, fm;
    const i64 *reg_start, *reg_end, *reg_read_off, *pos_off, *lvl_base;
    const int8_t *reg_strand;    // 0 '+', 1 '-', 2 none (no strand filter)
    const i64 *read_start, *read_off;
    const int8_t *read_strand, *read_ctrl;
    const double *means;     // read-centric, CSR by read_off
};

__device__ __forceinline__ i64 grp_region_of(const i64 *pos_off, i64 n_regions, i64 gp)
{
    i64 lo = 0, hi = n_regions - 1;
    while (lo < hi) { const i64 mid = (lo + hi + 1) >> 1; if (pos_off[mid] <= gp) lo = mid; else hi = mid - 1; }
    return lo;
}

// Pileup, one thread per position.  The reads of the region are visited in input order; a read
// of the other strand is skipped (tombo_helper.py:2022), a minus-strand read is reversed to
// genome order (get_single_slot_genome_centric), NaN levels are no coverage.
template <bool FILL>
__global__ void k_grp_pileup(GrpArgs a, i32 *cov, const i64 *lv_off, double *levels)
{
    for (i64 gp = (i64)blockIdx.x * blockDim.x + threadIdx.x; gp < a.n_pos; gp += (i64)gridDim.x * blockDim.x) {
        const i64 r = grp_region_of(a.pos_off, a.n_regions, gp);
        const i64 g = a.reg_start[r] - a.fm + (gp - a.pos_off[r]);   // genomic position
        const int rs = a.reg_strand[r];
        i64 cur[2] = {0, 0};
        if (FILL) { cur[0] = lv_off[2 * gp]; cur[1] = lv_off[2 * gp + 1]; }
        i32 n[2] = {0, 0};
        for (i64 q = a.reg_read_off[r]; q < a.reg_read_off[r + 1]; q++) {
            if (rs != 2 && a.read_strand[q] != rs) continue;
            const i64 len = a.read_off[q + 1] - a.read_off[q], s = a.read_start[q];
            if (g < s || g >= s + len) continue;
            const i64 k = a.read_strand[q] == 1 ? len - 1 - (g - s) : g - s;
            const double v = a.means[a.read_off[q] + k];
            if (v != v) continue;
            const int grp = a.read_ctrl[q] ? 1 : 0;
            if (FILL) levels[cur[grp]++] = v;
            else n[grp]++;
        }
        if (!FILL) { cov[2 * gp] = n[0]; cov[2 * gp + 1] = n[1]; }
    }
}

// One wavefront (block of 64) per region.  A position is covered when every tested group has
// >= min_reads levels (two_groups: both, else the sample coverage alone).  Runs of covered
// positions shorter than min_run are dropped (:4350).  Outputs per position: level offsets of its
// two segments (lvl_base[r] + prefix of the coverage), the run [run_a, run_b) it lies in (local
// indices) and its index in the compacted output (-1: not kept); out_counts[r] = kept positions.
__global__ void k_grp_scan(GrpArgs a, const i32 *cov, i64 min_reads, int two_groups, i64 min_run,
    i64 *lv_off, i32 *run_a, i32 *run_b, i64 *out_idx, i64 *out_counts)
{
    const i64 r = blockIdx.x;
    const int lane = threadIdx.x;
    const i64 p0 = a.pos_off[r], L = a.pos_off[r + 1] - p0;
    auto covered = [&](i64 i) {
        if (i >= L) return false;
        const i64 gp = p0 + i;
        return cov[2 * gp] >= min_reads && (!two_groups || cov[2 * gp + 1] >= min_reads);
    };
    // forward: level offsets, run starts
    i64 lv_carry = a.lvl_base[r];
    i32 start_carry = -1;
    for (i64 c = 0; c < L; c += 64) {
        const i64 i = c + lane;
        const i64 gp = p0 + i;
        const i64 tot = i < L ? (i64)cov[2 * gp] + cov[2 * gp + 1] : 0;
        const i64 inc = wave_scan_add(tot);
        const bool cv = covered(i), prev = i == 0 ? false : covered(i - 1);
        i32 st = wave_scan_max(cv && !prev ? (i32)i : -1);
        st = st > start_carry ? st : start_carry;
        if (i < L) {
            lv_off[2 * gp] = lv_carry + inc - tot;
            lv_off[2 * gp + 1] = lv_carry + inc - tot + cov[2 * gp];
            run_a[gp] = cv ? st : -1;
        }
        lv_carry += __shfl(inc, 63);
        start_carry = __shfl(st, 63);
    }
    // backward: run ends
    i32 end_carry = 0x7fffffff;
    for (i64 c = ((L + 63) / 64 - 1) * 64; c >= 0; c -= 64) {
        const i64 i = c + lane;
        const bool cv = covered(i), next = covered(i + 1);
        i32 en = wave_rscan_min(cv && !next ? (i32)(i + 1) : 0x7fffffff);
        en = en < end_carry ? en : end_carry;
        if (i < L) run_b[p0 + i] = cv ? en : -1;
        end_carry = __shfl(en, 0);
    }
    __syncthreads();   // (one wavefront: orders its own run_a / run_b stores before the reads below)
    // forward: compact index of the kept positions
    i64 k_carry = 0;
    for (i64 c = 0; c < L; c += 64) {
        const i64 i = c + lane;
        const i64 gp = p0 + i;
        const bool keep = i < L && run_a[gp] >= 0 && run_b[gp] - run_a[gp] >= min_run;
        const i64 inc = wave_scan_add(keep ? 1 : 0);
        if (i < L) out_idx[gp] = keep ? p0 + k_carry + inc - 1 : -1;
        k_carry += __shfl(inc, 63);
    }
    if (lane == 0) out_counts[r] = k_carry;
}

// Segments of the kept positions with more than one level, by size class.  lists: [0, 2P) wave,
// [2P, 4P) workgroup, [4P, 6P) global (2P = number of segments); counts[3].
__global__ void k_grp_classify(i64 n_pos, const i32 *cov, const i64 *out_idx, i64 *lists, u32 *counts)
{
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < 2 * n_pos; k += (i64)gridDim.x * blockDim.x) {
        if (out_idx[k >> 1] < 0 || cov[k] <= 1) continue;
        const int c = cov[k] <= GRP_WAVE_MAX ? 0 : cov[k] <= GRP_LDS_MAX ? 1 : 2;
        lists[(i64)c * 2 * n_pos + atomicAdd(&counts[c], 1u)] = k;
    }
}

// Class 1: one wavefront per segment, one level per lane (+inf past the end), a bitonic network
// over lanes (shuffles).
__global__ void k_grp_sort_wave(const i64 *list, const u32 *count, const i32 *cov, const i64 *lv_off,
                                double *levels)
{
    const int lane = threadIdx.x & 63;
    const i64 wave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const i64 n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 w = wave; w < (i64)*count; w += n_waves) {
        const i64 k = list[w];
        const int n = cov[k];
        double *seg = levels + lv_off[k];
        double v = lane < n ? seg[lane] : INFINITY;
        for (int size = 2; size <= 64; size <<= 1) {
            for (int st = size >> 1; st > 0; st >>= 1) {
                const int m = st == (size >> 1) ? size - 1 : st;   // flip step, then half-cleaners
                const double o = __shfl_xor(v, m);
                // the lower lane of a pair keeps the minimum
                v = (lane & st) == 0 ? (o < v ? o : v) : (o > v ? o : v);
            }
        }
        if (lane < n) seg[lane] = v;
    }
}

// one compare-exchange pass of the ascending bitonic network over a[0, n) (virtual +inf beyond:
// pairs that reach past n never swap); block size `size`, distance `st` (st == size/2: flip step)
template <class T>
__device__ __forceinline__ void grp_bitonic_pass(T *a, i64 n, i64 npow, i64 size, i64 st)
{
    for (i64 t = threadIdx.x; t < npow / 2; t += blockDim.x) {
        i64 i, j;
        if (st == size / 2) { const i64 b = t / st, o = t % st; i = b * size + o; j = b * size + size - 1 - o; }
        else { i = (t / st) * 2 * st + t % st; j = i + st; }
        if (j < n) {
            const double x = a[i], y = a[j];
            if (x > y) { a[i] = y; a[j] = x; }
        }
    }
}

template <class T>
__device__ void grp_bitonic(T *a, i64 n)
{
    i64 npow = 1;
    while (npow < n) npow <<= 1;
    for (i64 size = 2; size <= npow; size <<= 1)
        for (i64 st = size / 2; st > 0; st >>= 1) {
            grp_bitonic_pass(a, n, npow, size, st);
            __syncthreads();
        }
}

// Classes 2 and 3: one workgroup per segment; class 2 sorts a copy in LDS, class 3 (more than
// GRP_LDS_MAX levels: rare, tens of thousands of reads at a position) sorts in place in global
// memory (the workgroup's barriers order its own global stores).
__global__ void __launch_bounds__(256) k_grp_sort_wg(const i64 *list, const u32 *count, const i32 *cov,
                                                     const i64 *lv_off, double *levels, int global_class)
{
    __shared__ double sh[GRP_LDS_MAX];
    for (i64 w = blockIdx.x; w < (i64)*count; w += gridDim.x) {
        const i64 k = list[w];
        const i64 n = cov[k];
        double *seg = levels + lv_off[k];
        if (global_class) { grp_bitonic(seg, n); continue; }
        for (i64 t = threadIdx.x; t < n; t += blockDim.x) sh[t] = seg[t];
        __syncthreads();
        grp_bitonic(sh, n);
        for (i64 t = threadIdx.x; t < n; t += blockDim.x) seg[t] = sh[t];
        __syncthreads();
    }
}

// ---- special functions ------------------------------------------------------------------------
// kstwobign.sf = scipy.special.kolmogorov (complement of the Kolmogorov CDF): Jacobi-theta form
// up to x = 0.82, the alternating series 2 sum (-1)^(k-1) exp(-2 k^2 x^2) beyond; both unrolled
// as in scipy's kolmogorov.c (cephes).
__device__ double grp_kolmogorov(double x)
{
    if (x != x) return x;
    if (x <= 0) return 1.0;
    if (x <= 0.040611972203751713) return 1.0;   // pi / sqrt(-MIN_EXPABLE * 8)
    double sf;
    if (x <= 0.82) {
        const double w = 2.50662827463100050242 / x;   // sqrt(2 pi) / x
        const double logu8 = -M_PI * M_PI / (x * x);
        const double u = exp(logu8 / 8);
        double cdf;
        if (u == 0) cdf = exp(logu8 / 8 + log(w));
        else {
            const double u8 = exp(logu8), u8cub = pow(u8, 3);
            double P = 1.0;
            P = 1 + u8cub * P;
            P = 1 + u8 * u8 * P;
            P = 1 + u8 * P;
            cdf = w * u * P;
        }
        cdf = cdf < 0 ? 0 : cdf > 1 ? 1 : cdf;
        sf = 1 - cdf;
    } else {
        const double v = exp(-2 * x * x), vsq = v * v, v3 = pow(v, 3);
        double P = 1.0;
        P = 1 - v3 * v3 * v * P;
        P = 1 - v3 * vsq * P;
        P = 1 - v3 * P;
        sf = 2 * v * P;
    }
    return sf < 0 ? 0 : sf > 1 ? 1 : sf;
}

// norm.cdf(z) (cephes ndtr: erf near 0, erfc in the tails)
__device__ double grp_ndtr(double z)
{
    const double x = z * 0.70710678118654752440, y = fabs(x);
    if (y < 0.70710678118654752440) return 0.5 + 0.5 * erf(x);
    const double r = 0.5 * erfc(y);
    return x > 0 ? 1 - r : r;
}

// regularized incomplete beta I_x(a, b) by its continued fraction (modified Lentz), the side of
// the mean chosen for convergence
__device__ double grp_betacf(double a, double b, double x)
{
    const double FPMIN = 1e-300, qab = a + b, qap = a + 1, qam = a - 1;
    double c = 1.0, d = 1 - qab * x / qap;
    if (fabs(d) < FPMIN) d = FPMIN;
    d = 1 / d;
    double h = d;
    for (int m = 1; m < 300; m++) {
        const int m2 = 2 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1 + aa * d; if (fabs(d) < FPMIN) d = FPMIN;
        c = 1 + aa / c; if (fabs(c) < FPMIN) c = FPMIN;
        d = 1 / d; h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1 + aa * d; if (fabs(d) < FPMIN) d = FPMIN;
        c = 1 + aa / c; if (fabs(c) < FPMIN) c = FPMIN;
        d = 1 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1) < 1e-16) break;
    }
    return h;
}
__device__ double grp_ibeta(double a, double b, double x)
{
    if (x <= 0) return 0.0;
    if (x >= 1) return 1.0;
    const double lbt = lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log1p(-x);
    if (x < (a + 1) / (a + b + 2)) return exp(lbt) * grp_betacf(a, b, x) / a;
    return 1 - exp(lbt) * grp_betacf(b, a, 1 - x) / b;
}

// Student t CDF with k degrees of freedom (cephes stdtr: the finite series for |t| <= 2, the
// incomplete beta in the tail t < -2)
__device__ double grp_stdtr(i64 k, double t)
{
    if (k <= 0 || t != t) return NAN;
    if (t == 0) return 0.5;
    const double MACHEP = 1.11022302462515654042e-16;
    const double rk = (double)k;
    if (t < -2.0) return 0.5 * grp_ibeta(0.5 * rk, 0.5, rk / (rk + t * t));
    const double x = t < 0 ? -t : t, z = 1.0 + (x * x) / rk;
    double p;
    if (k & 1) {
        const double xsqk = x / sqrt(rk);
        p = atan(xsqk);
        if (k > 1) {
            double f = 1.0, tz = 1.0;
            for (i64 j = 3; j <= k - 2 && tz / f > MACHEP; j += 2) { tz *= (double)(j - 1) / (z * (double)j); f += tz; }
            p += f * xsqk / z;
        }
        p *= 2.0 / M_PI;
    } else {
        double f = 1.0, tz = 1.0;
        for (i64 j = 2; j <= k - 2 && tz / f > MACHEP; j += 2) { tz *= (double)(j - 1) / (z * (double)j); f += tz; }
        p = f * x / sqrt(z * rk);
    }
    if (t < 0) p = -p;
    return 0.5 + 0.5 * p;
}

// ---- per-position tests -----------------------------------------------------------------------
// kind 0 KS, 1 U, 2 t; return_p: p-value, else the statistic.  s / c: the sorted sample and
// control levels.  U: equal values rank sample first (the reference's unstable argsort leaves
// cross-group ties in an unstated order).
__device__ double grp_test(int kind, int return_p, const double *s, i64 ns, const double *c, i64 nc)
{
    if (kind == 0) {
        double d = 0.0;
        i64 i = 0, j = 0;
        while (i < ns || j < nc) {
            const double vs = i < ns ? s[i] : INFINITY, vc = j < nc ? c[j] : INFINITY;
            const double v = vs < vc ? vs : vc;
            while (i < ns && s[i] == v) i++;
            while (j < nc && c[j] == v) j++;
            const double df = fabs((double)i / (double)ns - (double)j / (double)nc);
            d = df > d ? df : d;
            if (v == INFINITY) break;
        }
        if (!return_p) return 1 - d;
        const double en = sqrt((double)(ns * nc) / (double)(ns + nc));
        return grp_kolmogorov((en + 0.12 + 0.11 / en) * d);
    }
    if (kind == 1) {
        i64 i = 0, j = 0, rk = 1, rsum = 0;
        while (i < ns || j < nc) {
            if (j >= nc || (i < ns && s[i] <= c[j])) { rsum += rk; i++; }
            else j++;
            rk++;
        }
        const i64 tot = ns * nc;
        const double u1 = (double)rsum - (double)(ns * (ns + 1)) / 2.0;
        const double u2 = (double)tot - u1;
        const double u = u2 < u1 ? u2 : u1;
        const double mu = (double)tot / 2.0;
        if (!return_p) return (u - mu) / mu;
        const double rhou = sqrt((double)(tot * (tot + 1)) / 12.0);
        return grp_ndtr((u - mu) / rhou) * 2.0;
    }
    // c_mean_std (_c_helper.pyx:22-36): sequential sum, sequential squared deviations
    auto mean_std = [](const double *v, i64 n, double &m, double &sd) {
        double acc = 0;
        for (i64 i = 0; i < n; i++) acc += v[i];
        m = acc / (double)n;
        double var = 0;
        for (i64 i = 0; i < n; i++) { const double d = v[i] - m; var += d * d; }
        sd = sqrt(var / (double)n);
    };
    double sm, ssd, cm, csd;
    mean_std(s, ns, sm, ssd);
    mean_std(c, nc, cm, csd);
    if (!return_p) return -fabs(sm - cm) / sqrt(((ssd * ssd) + (csd * csd)) / 2);
    const double sp = sqrt((((double)(ns - 1) * (ssd * ssd)) + (double)(nc - 1) * (csd * csd)) /
                           (double)(ns + nc - 2));
    const double t = -fabs(sm - cm) / (sp * sqrt((1.0 / (double)ns) + (1.0 / (double)nc)));
    return grp_stdtr(ns + nc - 2, t) * 2.0;
}

__global__ void k_grp_test(i64 n_pos, int kind, int return_p, const i32 *cov, const i64 *lv_off,
                           const i64 *out_idx, const double *levels, double *raw)
{
    for (i64 gp = (i64)blockIdx.x * blockDim.x + threadIdx.x; gp < n_pos; gp += (i64)gridDim.x * blockDim.x) {
        if (out_idx[gp] < 0) continue;
        raw[gp] = grp_test(kind, return_p, levels + lv_off[2 * gp], cov[2 * gp], levels + lv_off[2 * gp + 1],
                           cov[2 * gp + 1]);
    }
}

// Windows over each run (fm > 0): Fisher's method for p-values (calc_window_fishers_method,
// :2252-2271; chi2.sf for even degrees of freedom by chi2_sf_even, tba_common.h, as k_read_pvals),
// the window mean for statistics (calc_window_means, :2273-2287); sums in numpy's order
// (np_sum_by); the first and last fm positions of a run are NaN.  Writes the compacted outputs.
__global__ void k_grp_window(GrpArgs a, int return_p, double smallest, const i32 *cov,
    const i32 *run_a, const i32 *run_b, const i64 *out_idx, const double *raw, double *out_stats,
    i64 *out_poss, i64 *out_cov, i64 *out_ctrl_cov)
{
    const i64 fm = a.fm;
    for (i64 gp = (i64)blockIdx.x * blockDim.x + threadIdx.x; gp < a.n_pos; gp += (i64)gridDim.x * blockDim.x) {
        const i64 o = out_idx[gp];
        if (o < 0) continue;
        const i64 r = grp_region_of(a.pos_off, a.n_regions, gp);
        const i64 i = gp - a.pos_off[r];
        double res;
        if (fm <= 0) res = raw[gp];
        else if (i - run_a[gp] < fm || run_b[gp] - 1 - i < fm) res = NAN;
        else {
            const i64 w = 2 * fm + 1, b = gp - fm;
            if (return_p) {
                const double ls = np_sum_by([&](i64 k) {
                    double p = raw[b + k];
                    p = p < smallest ? smallest : p;   // np.maximum: NaN stays NaN
                    return log(p);
                }, w);
                res = chi2_sf_even(-ls, w);
            } else {
                res = np_sum_by([&](i64 k) { return raw[b + k]; }, w) / (double)w;
            }
        }
        out_stats[o] = res;
        out_poss[o] = a.reg_start[r] - fm + i;
        out_cov[o] = cov[2 * gp];
        out_ctrl_cov[o] = cov[2 * gp + 1];
    }
}

// get_reads_ref, first half (levels still in read order): np.mean / np.std of the valid levels
__global__ void k_ref_moments(i64 n_pos, const i32 *cov, const i64 *lv_off, const i64 *out_idx,
                              const double *levels, double *mean, double *sd)
{
    for (i64 gp = (i64)blockIdx.x * blockDim.x + threadIdx.x; gp < n_pos; gp += (i64)gridDim.x * blockDim.x) {
        if (out_idx[gp] < 0) continue;
        const double *v = levels + lv_off[2 * gp];
        const i64 n = cov[2 * gp];
        const double m = np_sum_by([&](i64 k) { return v[k]; }, n) / (double)n;
        mean[gp] = m;
        sd[gp] = sqrt(np_sum_by([&](i64 k) { const double d = v[k] - m; return d * d; }, n) / (double)n);
    }
}

// second half (levels sorted): the median unless est_mean, the prior blend
// (compute_posterior_samp_dists, :3572-3624) where prior levels are given, zero sd -> NaN
__global__ void k_ref_finish(i64 n_pos, int est_mean, const i32 *cov, const i64 *lv_off,
    const i64 *out_idx, const double *levels, const double *mean, const double *sd,
    const double *prior_means, const double *prior_sds, double w_mean, double w_sd,
    double *out_means, double *out_sds, i64 *out_cov)
{
    for (i64 gp = (i64)blockIdx.x * blockDim.x + threadIdx.x; gp < n_pos; gp += (i64)gridDim.x * blockDim.x) {
        const i64 n = cov[2 * gp];
        double m = NAN, s = NAN;
        if (out_idx[gp] >= 0) {
            const double *v = levels + lv_off[2 * gp];
            m = est_mean ? mean[gp] : (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
            s = sd[gp];
        }
        if (prior_means) {
            m = ((w_mean * prior_means[gp]) + ((double)n * m)) / (w_mean + (double)n);
            s = ((w_sd * prior_sds[gp]) + ((double)n * s)) / (w_sd + (double)n);
        }
        if (s == 0) { m = NAN; s = NAN; }
        out_means[gp] = m;
        out_sds[gp] = s;
        out_cov[gp] = n;
    }
}

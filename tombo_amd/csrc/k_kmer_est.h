// k_kmer_est.h -- the device half of estimate_kmer_model / estimate_motif_alt_model
// (get_region_kmer_levels, tombo_stats.py:1242-1359; tabulate_kmer_levels, :1454-1501;
// tabulate_mod_kmer_levels, :2108-2158).
//
// The host does what the reference does with strings (region sequence, motif search, k-mer codes)
// and the coverage intervals; it hands over, for a batch of regions,
//   reads      start, strand, levels (CSR by read_off), uploaded once however many regions use them
//   regions    the indices of their reads, in the region's read order (CSR by reg_read_off)
//   positions  the wanted positions: (region, genomic position), each computed once
//   entries    (position index, key) in output order: region, position, entry
// Steps of region_key_levels:
//   k_region_pileup<false>  reads per position (one thread per position, the region's reads in order)
//   k_exclusive_prefix      level offsets of the positions (k_scan.h)
//   k_region_pileup<true>   the levels in read order; a minus-strand read is reversed to genome order;
//                           NaN levels are kept (they count towards the coverage, get_reads_events)
//   k_kest_moments          per position np.std (np_sum_by order) in read order, or with est_mean the
//                           pair of c_mean_std (_c_helper.pyx:22-36: left-to-right sums)
//   k_kde_classify, k_grp_sort_*   without est_mean: the positions' levels sorted (k_kde.h, k_group.h)
//   k_kest_median           np.median of each sorted segment
//   k_key_partition         the entries stably partitioned by key into the two output columns (k_scan.h,
//                           EntSrc its source of keys)
// No floating-point atomics anywhere, every sum in a fixed order: two runs give the same bits.
// segment_medians is k_kde_classify, the sorters and k_kest_median on a copy of the values.
// k_region_pileup also piles the levels of the plot regions (k_plot.h), whose positions are dense.
#pragma once
#include "tba_common.h"
#include "k_scan.h"

// the reads of a batch of regions
struct RegionReads {
    const i64 *reg_read_off, *reg_reads;     // per region: its reads, in its read order
    const i64 *read_start, *read_off;
    const uint8_t *read_minus;               // 1: minus strand (levels reversed to genome order)
    const double *means;                     // read-centric, CSR by read_off
};

// the positions of a pile-up: locate(p, r, g) gives position p's region and genomic position; keep_nan: a NaN
// level counts and is stored like any other.  ListedPos: the wanted positions, each listed by the host.
struct ListedPos {
    static constexpr bool keep_nan = true;
    const i64 *pos_reg, *pos_g;
    __device__ void locate(i64 p, i64 &r, i64 &g) const { r = pos_reg[p]; g = pos_g[p]; }
};

// One thread per position.  lv_off: n_pos + 1 offsets (FILL); cov: the levels per position.
template <bool FILL, class Pos>
__global__ void k_region_pileup(RegionReads a, Pos pos, i64 n_pos, i32 *cov, const i64 *lv_off, double *levels)
{
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < n_pos; p += (i64)gridDim.x * blockDim.x) {
        i64 r, g;
        pos.locate(p, r, g);
        i64 cur = FILL ? lv_off[p] : 0;
        i32 n = 0;
        for (i64 q = a.reg_read_off[r]; q < a.reg_read_off[r + 1]; q++) {
            const i64 rd = a.reg_reads[q];
            const i64 len = a.read_off[rd + 1] - a.read_off[rd], s = a.read_start[rd];
            if (g < s || g >= s + len) continue;
            double v = 0.0;
            if (FILL || !Pos::keep_nan) v = a.means[a.read_off[rd] + (a.read_minus[rd] ? len - 1 - (g - s) : g - s)];
            if (!Pos::keep_nan && v != v) continue;
            if (FILL) levels[cur++] = v;
            else n++;
        }
        if (!FILL) cov[p] = n;
    }
}

// One thread per position, levels in read order.  est_mean: level = the sequential mean, sd =
// sqrt of the sequential sum of squared deviations over n (c_mean_std); else the level is left
// to k_kest_median and sd = np.std.  A position without a read: NaN.
__global__ void k_kest_moments(i64 n_pos, int est_mean, const i64 *lv_off, const double *levels,
                               double *level, double *sd)
{
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < n_pos; p += (i64)gridDim.x * blockDim.x) {
        const double *v = levels + lv_off[p];
        const i64 n = lv_off[p + 1] - lv_off[p];
        if (n == 0) { level[p] = NAN; sd[p] = NAN; continue; }
        if (est_mean) {
            double acc = 0;
            for (i64 i = 0; i < n; i++) acc += v[i];
            const double m = acc / (double)n;
            double var = 0;
            for (i64 i = 0; i < n; i++) { const double d = v[i] - m; var += d * d; }
            level[p] = m;
            sd[p] = sqrt(var / (double)n);
        } else {
            const double m = np_sum_by([&](i64 k) { return v[k]; }, n) / (double)n;
            sd[p] = sqrt(np_sum_by([&](i64 k) { const double d = v[k] - m; return d * d; }, n) / (double)n);
        }
    }
}

// np.median of every segment (sorted by the k_grp sorters unless it holds a NaN or fewer than two
// values): NaN for an empty segment or one with a NaN, the mean of the two middle values for an
// even count.
__global__ void k_kest_median(i64 n_seg, const i32 *has_nan, const i64 *lv_off, const double *levels, double *out)
{
    for (i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x; s < n_seg; s += (i64)gridDim.x * blockDim.x) {
        const double *v = levels + lv_off[s];
        const i64 n = lv_off[s + 1] - lv_off[s];
        out[s] = n == 0 || has_nan[s] ? NAN : (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
    }
}

// the entries as the items of k_key_partition: entry e has the key ent_key[e] and takes the level and the sd
// of its position
struct EntSrc {
    const i64 *ent_pos, *ent_key;
    const double *level, *sd;
    double *out_levels, *out_sds;

    __device__ i64 key(i64 e) const { return ent_key[e]; }
    __device__ void store(i64 e, i64 o) const
    {
        const i64 p = ent_pos[e];
        out_levels[o] = level[p];
        out_sds[o] = sd[p];
    }
};

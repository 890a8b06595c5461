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
//   k_kest_pileup<false>  reads per position (one thread per position, the region's reads in order)
//   k_kest_offsets        one workgroup: level offsets of the positions (exclusive prefix)
//   k_kest_pileup<true>   the levels in read order; a minus-strand read is reversed to genome order;
//                         NaN levels are kept (they count towards the coverage, get_reads_events)
//   k_kest_moments        per position np.std (np_sum_by order) in read order, or with est_mean the
//                         pair of c_mean_std (_c_helper.pyx:22-36: left-to-right sums)
//   k_kde_classify, k_grp_sort_*   without est_mean: the positions' levels sorted (k_kde.h, k_group.h)
//   k_kest_median         np.median of each sorted segment
//   k_kest_partition      the entries stably partitioned by key into the two output columns
// The partition is k_kmer_gather's scheme (k_kde.h) with the key read from the entry: entries are
// cut into chunks, one wavefront per chunk, 64 entries a step; the lanes of a step that hold the
// same key find each other with one ballot per key bit.  Work is split by entry and never by key.
// No floating-point atomics anywhere, every sum in a fixed order: two runs give the same bits.
// segment_medians is k_kde_classify, the sorters and k_kest_median on a copy of the values.
#pragma once
#include "tba_common.h"
#include "k_group.h"
#include "k_kde.h"

struct KestArgs {
    i64 n_pos;
    const i64 *pos_reg, *pos_g;              // per wanted position: its region, its genomic position
    const i64 *reg_read_off, *reg_reads;     // per region: its reads, in its read order
    const i64 *read_start, *read_off;
    const uint8_t *read_minus;               // 1: minus strand (levels reversed to genome order)
    const double *means;                     // read-centric, CSR by read_off
};

// One thread per wanted position.  lv_off: n_pos + 1 offsets (FILL); cov: the reads per position.
template <bool FILL>
__global__ void k_kest_pileup(KestArgs a, i32 *cov, const i64 *lv_off, double *levels)
{
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < a.n_pos; p += (i64)gridDim.x * blockDim.x) {
        const i64 r = a.pos_reg[p], g = a.pos_g[p];
        i64 cur = FILL ? lv_off[p] : 0;
        i32 n = 0;
        for (i64 q = a.reg_read_off[r]; q < a.reg_read_off[r + 1]; q++) {
            const i64 rd = a.reg_reads[q];
            const i64 len = a.read_off[rd + 1] - a.read_off[rd], s = a.read_start[rd];
            if (g < s || g >= s + len) continue;
            if (FILL) levels[cur++] = a.means[a.read_off[rd] + (a.read_minus[rd] ? len - 1 - (g - s) : g - s)];
            else n++;
        }
        if (!FILL) cov[p] = n;
    }
}

// One workgroup of 256: off[n + 1], the exclusive prefix of cov.  Every thread owns one run of
// consecutive positions; the runs' totals are scanned in LDS.
__global__ void __launch_bounds__(256) k_kest_offsets(i64 n, const i32 *cov, i64 *off)
{
    __shared__ i64 part[256];
    const i64 run = (n + 255) / 256;
    const i64 a = (i64)threadIdx.x * run < n ? (i64)threadIdx.x * run : n;
    const i64 b = a + run < n ? a + run : n;
    i64 tot = 0;
    for (i64 i = a; i < b; i++) tot += cov[i];
    part[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 acc = 0;
        for (int t = 0; t < 256; t++) { const i64 v = part[t]; part[t] = acc; acc += v; }
        off[n] = acc;
    }
    __syncthreads();
    i64 acc = part[threadIdx.x];
    for (i64 i = a; i < b; i++) { off[i] = acc; acc += cov[i]; }
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

// One wavefront (block of 64) per chunk of `chunk` consecutive entries (a multiple of 64).
// rows[chunk][key]: counted here (FILL false, zeroed before), or the chunk's starting rank inside
// the key's segment (FILL true, from k_kmer_colscan).  key_bits: bits that tell the keys apart.
template <bool FILL>
__global__ void __launch_bounds__(64) k_kest_partition(i64 n_ent, i64 chunk, i64 n_keys, int key_bits,
    const i64 *ent_pos, const i64 *ent_key, u32 *rows, const i64 *key_off, const double *level,
    const double *sd, double *out_levels, double *out_sds)
{
    const int lane = threadIdx.x;
    u32 *row = rows + (i64)blockIdx.x * n_keys;
    const i64 e0 = (i64)blockIdx.x * chunk;
    const i64 e1 = e0 + chunk < n_ent ? e0 + chunk : n_ent;
    for (i64 c = e0; c < e1; c += 64) {
        const i64 e = c + lane;
        const i64 key = e < e1 ? ent_key[e] : -1;
        u64 peers = __ballot(key >= 0);
        for (int b = 0; b < key_bits; b++) {
            const bool bit = (key >> b) & 1;
            const u64 m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        if (key >= 0) {
            const u32 rank = __popcll(peers & (((u64)1 << lane) - 1)), cnt = __popcll(peers);
            const u32 cur = row[key];
            if (FILL) {
                const i64 o = key_off[key] + cur + rank, p = ent_pos[e];
                out_levels[o] = level[p];
                out_sds[o] = sd[p];
            }
            if (rank == cnt - 1) row[key] = cur + cnt;
        }
        __syncthreads();   // (one wavefront: orders this step's counter stores before the next step's loads)
    }
}

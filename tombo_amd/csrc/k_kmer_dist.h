// k_kmer_dist.h -- the numbers of `tombo plot kmer` (plot_kmer_dist, _plot_commands.py:451-559): the levels of a
// batch of reads grouped by (k-mer, read), the reads the plot takes, and np.mean of every group and k-mer.
//
// Grouping.  The reads are concatenated in read order (CSR by read_off) as in k_kde.h, and the flat positions are cut
// into chunks that never cross a read (the host lists them: KdChunk; a read's chunks are consecutive and every
// chunk but a read's last is `chunk` positions long, a multiple of 64).  One wavefront per chunk, 64 windows a step,
// each a step of the partition by key of k_scan.h:
//   k_kd_gather<false>  per chunk a row of 4^K counters
//   k_kd_read_scan      per (read, k-mer): the exclusive prefix of the counters over the read's chunks and the
//                       read's count tab[read][kmer]; per read the number of distinct k-mers and the smallest count
//   k_kd_select         one wavefront, an ordered scan over the reads: which are valid, which are examined before
//                       num_reads were added, their labels 1, 2, ... (0: not taken)
//   k_kd_kmer_totals    per k-mer over the taken reads: its levels and the reads that show it
//   k_exclusive_prefix  (k_scan.h) the exclusive prefixes of both
//   k_kd_seg_bases      tab[read][kmer] becomes the first level of segment (kmer, read): k-mer major, taken reads in
//                       label order; the read_mean form lists the non-empty segments per k-mer, compacted
//   k_kd_gather<true>   the levels: tab[read][kmer] + the chunk's prefix + the rank inside the step
// so a k-mer's levels stand in read order, then position order, and every run writes the same bytes.  The only
// atomics are the integer add / min of k_kd_read_scan, whose results do not depend on their order.
//
// Means.  np.mean of a Python list is np.add.reduce over a contiguous copy, divided by n; np.add.reduce adds
// 8192-value blocks left to right, each summed pairwise (np_pairwise_sum, tba_common.h).
//   k_kd_seg_means      the read_mean form: one value per listed segment
//   k_kd_kmer_means     per k-mer, over its output run (the levels, or the compacted per-read means)
// A lane sums a segment of at most 128 levels itself (one leaf of the pairwise tree: a serial loop is numpy's own
// order); longer ones -- a homopolymer read makes one of thousands -- are summed by the whole wavefront
// (wave_np_sum, k_scan.h: the scheme of k_final_score, k_tail.h).
#pragma once
#include "tba_common.h"
#include "k_scan.h"

struct KdChunk { i64 read, p0, p1; };   // flat positions [p0, p1) of one read

struct KdArgs {
    i64 n_reads, n_chunks, n_kmers, n_lv;
    int K, cp, read_mean, pad;
    const i64 *read_off;
    const KdChunk *chunks;
    const uint8_t *codes;
    const double *means;
};

// One wavefront (block of 64) per chunk.  rows[chunk][kmer]: counted here (FILL false, zeroed before), or the chunk's
// starting rank inside its read's segment of the k-mer (FILL true, from k_kd_read_scan).  FILL: tab[read][kmer] is
// the segment's first level; a read that is not taken is left out; labels_out (raw form, else NULL): the read's
// label beside every level.
template <bool FILL>
__global__ void __launch_bounds__(64) k_kd_gather(KdArgs a, u32 *rows, const i64 *label, const u32 *tab,
                                                  double *levels, i64 *labels_out)
{
    const int lane = threadIdx.x;
    const KdChunk ch = a.chunks[blockIdx.x];
    const i64 lab = FILL ? label[ch.read] : 0;
    if (FILL && lab == 0) return;
    u32 *row = rows + (i64)blockIdx.x * a.n_kmers;
    const u32 *base = FILL ? tab + ch.read * a.n_kmers : nullptr;
    const i64 read_end = a.read_off[ch.read + 1];
    for (i64 c = ch.p0; c < ch.p1; c += 64) {
        const i64 p = c + lane;
        // the k-mer of the window that starts at p; -1: no window, or a base outside ACGT
        const i64 key = p < ch.p1 && p + a.K <= read_end ? window_kmer(a.codes + p, a.K) : -1;
        const u64 peers = wave_key_peers(key, 2 * a.K, key >= 0);
        if (key >= 0) {
            const i64 at = (i64)partition_step(peers, row, key) + (FILL ? base[key] : 0);
            if (FILL && at < a.n_lv) {   // (always: the offsets come from the same counts)
                levels[at] = a.means[p + a.cp];
                if (labels_out) labels_out[at] = lab;
            }
        }
        __syncthreads();   // between two steps: see partition_step
    }
}

// blockIdx.y: the read; the threads stride over the k-mers.  read_chunk0[n_reads + 1]: the reads' first chunks.
// distinct / min_cnt [n_reads]: zeroed / set to all ones before.
__global__ void __launch_bounds__(256) k_kd_read_scan(i64 n_kmers, const i64 *read_chunk0, u32 *rows, u32 *tab,
                                                      u32 *distinct, u32 *min_cnt)
{
    const i64 r = blockIdx.y;
    const i64 c0 = read_chunk0[r], c1 = read_chunk0[r + 1];
    u32 n_seen = 0, least = 0xffffffffu;
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < n_kmers; q += (i64)gridDim.x * blockDim.x) {
        u32 run = 0;
        for (i64 c = c0; c < c1; c++) {
            const u32 t = rows[c * n_kmers + q];
            rows[c * n_kmers + q] = run;
            run += t;
        }
        tab[r * n_kmers + q] = run;
        if (run) { n_seen++; least = run < least ? run : least; }
    }
    if (n_seen) { atomicAdd(&distinct[r], n_seen); atomicMin(&min_cnt[r], least); }
}

// One wavefront.  Rule of plot_kmer_dist: a read is valid under kmer_thresh == 0, or if it shows all k-mers and
// (kmer_thresh == 1 or its rarest k-mer occurs MORE than kmer_thresh times); read i is examined if fewer than
// num_reads valid reads stand before it (the first read always is); an examined valid read is taken.
// out[0]: reads taken, out[1]: reads examined.
__global__ void __launch_bounds__(64) k_kd_select(i64 n_reads, i64 n_kmers, i64 kmer_thresh, i64 num_reads,
                                                  const u32 *distinct, const u32 *min_cnt, i64 *label, i64 *out)
{
    const int lane = threadIdx.x;
    i64 carry = 0, n_exam = 0, n_sel = 0;
    for (i64 c = 0; c < n_reads; c += 64) {
        const i64 i = c + lane;
        i64 valid = 0;
        if (i < n_reads)
            valid = kmer_thresh == 0 ||
                ((i64)distinct[i] == n_kmers && (kmer_thresh == 1 || (i64)min_cnt[i] > kmer_thresh));
        const i64 inc = carry + wave_scan_add(valid);
        const bool examined = i < n_reads && (i == 0 || inc - valid < num_reads);
        const bool taken = examined && valid;
        if (i < n_reads) label[i] = taken ? inc : 0;
        n_exam += __popcll(__ballot(examined));
        n_sel += __popcll(__ballot(taken));
        carry = shfl_i64(inc, 63);
        if (carry >= num_reads) {   // nothing behind this step is examined
            for (i64 j = c + 64 + lane; j < n_reads; j += 64) label[j] = 0;
            break;
        }
    }
    if (lane == 0) { out[0] = n_sel; out[1] = n_exam; }
}

// sel[n_sel]: the taken reads in label order.  lvl_tot / ent_tot [n_kmers]: the k-mer's levels / the reads with any.
__global__ void k_kd_kmer_totals(i64 n_kmers, i64 n_sel, const i64 *sel, const u32 *tab, i64 *lvl_tot, i64 *ent_tot)
{
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < n_kmers; q += (i64)gridDim.x * blockDim.x) {
        i64 lv = 0, en = 0;
        for (i64 j = 0; j < n_sel; j++) { const u32 c = tab[sel[j] * n_kmers + q]; lv += c; en += c != 0; }
        lvl_tot[q] = lv;
        ent_tot[q] = en;
    }
}

// tab[read][kmer]: count -> first level of the segment.  seg_start != NULL (the read_mean form): the non-empty
// segments of k-mer q listed from ent_off[q] on in label order.
__global__ void k_kd_seg_bases(i64 n_kmers, i64 n_sel, const i64 *sel, u32 *tab, const i64 *lv_off, const i64 *ent_off,
                               u32 *seg_start, u32 *seg_len, i64 *seg_label)
{
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < n_kmers; q += (i64)gridDim.x * blockDim.x) {
        i64 run = lv_off[q], e = seg_start ? ent_off[q] : 0;
        for (i64 j = 0; j < n_sel; j++) {
            u32 *t = tab + sel[j] * n_kmers + q;
            const u32 c = *t;
            *t = (u32)run;
            if (seg_start && c) { seg_start[e] = (u32)run; seg_len[e] = c; seg_label[e] = j + 1; e++; }
            run += c;
        }
    }
}

// The read_mean form: values[e] = np.mean of listed segment e.  One wavefront (block of 64) per 64 segments: a lane
// sums its own segment if that is a single leaf, the wavefront then takes the longer ones one after the other.
__global__ void __launch_bounds__(64) k_kd_seg_means(i64 n_ent, const u32 *seg_start, const u32 *seg_len,
                                                     const double *levels, double *values)
{
    __shared__ WaveSumLds w;
    const int lane = threadIdx.x;
    for (i64 c = (i64)blockIdx.x * 64; c < n_ent; c += (i64)gridDim.x * 64) {
        const i64 e = c + lane;
        const i64 n = e < n_ent ? seg_len[e] : 0;
        const double *seg = levels + (e < n_ent ? seg_start[e] : 0);
        if (n > 0 && n <= 128) values[e] = np_pairwise_leaf(seg, n) / (double)n;
        u64 big = __ballot(n > 128);
        while (big) {   // (the same for every lane)
            const int src = __ffsll((long long)big) - 1;
            big &= big - 1;
            const i64 e2 = c + src;
            const i64 n2 = seg_len[e2];
            const double s = wave_np_sum(levels + seg_start[e2], n2, w, lane);
            if (lane == 0) values[e2] = s / (double)n2;
        }
    }
}

// kmer_mean[q] = np.mean of values[off[q] .. off[q + 1]), NaN for a k-mer without entries.  A wavefront per k-mer.
__global__ void __launch_bounds__(64) k_kd_kmer_means(i64 n_kmers, const i64 *off, const double *values, double *kmer_mean)
{
    __shared__ WaveSumLds w;
    const int lane = threadIdx.x;
    for (i64 q = blockIdx.x; q < n_kmers; q += gridDim.x) {
        const i64 n = off[q + 1] - off[q];
        if (n == 0) { if (lane == 0) kmer_mean[q] = NAN; continue; }
        const double s = wave_np_sum(values + off[q], n, w, lane);
        if (lane == 0) kmer_mean[q] = s / (double)n;
    }
}

// k_roc.h -- scoring stored statistics against a ground truth: the labels of compute_motif_stats /
// compute_ctrl_motif_stats / compute_ground_truth_stats (tombo_stats.py:2406-2535) and the sorted
// cumulative counts behind prep_accuracy_rates (_plot_commands.py:60-82, tombo_stats.py:2384-2404).
//
// Labels.  Records (position, statistic) are CSR by block.  A motif block carries the sequence the
// host fetched for it (codes 0-3 = A, C, G, T, 4 = anything else) and the genome coordinate of
// that sequence's first base; a minus-strand block reads the complement backwards.  One thread
// evaluates one (record, motif) pair:
//   base     the base under the record, in strand orientation, is the motif's mod_base (A/C/G/T)
//   match    every motif position lies inside the fetched sequence and its base is in the
//            position's set, the modified position on the record
//   motif form (mode 0):   keep = base, label = match
//   control form (mode 1): keep = match, label = the call's constant
// A location block carries [lo, hi) slices of two sorted position lists: keep = in either list,
// label = in the modified one (binary searches).
// Every read of the sequence and of the lists is bounds-checked against the block's own slice
// before its address is formed.  The kept pairs are compacted per motif in record order: flags ->
// per-chunk counts (k_chunk_total over RocKept) -> scan (k_exclusive_prefix) -> write (k_roc_scatter),
// chunks of SCAN_CHUNK records (k_scan.h), grid.y = motif, all motifs back to back in one output.
//
// Rank counts.  tp_at[j] = number of True labels among the ranks[j] + 1 first entries in
// (statistic, label) order.  The statistic becomes the order-preserving key of k_select.h (f64_key,
// -0.0 first made 0.0); a stable least-significant-digit radix sort then orders (key, label) with
// the label as the least significant digit: pass 0 sorts by the 9-bit digit (low key byte, label),
// passes 1-7 by the remaining key bytes.  k_roc_keys also counts NaNs and the values of every digit
// over the whole input, so the host skips a pass in which one digit value holds all entries.
// One pass = three kernels, each finished before the next starts (no workgroup ever waits for
// another):
//   k_roc_hist     digit counts of every tile of ROC_SORT_TILE entries -> table[digit][tile]
//   scan           exclusive prefix of the table in that (digit-major) order: k_chunk_total over
//                  ArrayCount<u32>, k_exclusive_prefix, k_roc_tab_apply
//   k_roc_scatter_pass   each wavefront owns ROC_SORT_TILE / 4 consecutive entries of the tile; the
//                  wavefronts' digit counts (LDS) give each its first output index per digit, then
//                  a wavefront walks its entries 64 at a time in element order and ranks equal
//                  digits among their peers (wave_key_peers), which keeps the order of equal digits.
// All counters are integers (LDS and global integer atomics in the histograms only), so the result
// does not depend on the order of those adds.  After the last pass the labels are scanned in
// chunks of SCAN_CHUNK (k_chunk_total over ArrayCount<uint8_t>) and k_roc_gather reads the inclusive
// count at every rank.
#pragma once
#include "tba_common.h"
#include "k_scan.h"

#define ROC_SORT_TILE 4096          // entries per workgroup per pass: 4 wavefronts x 16 steps x 64
#define ROC_WAVE_SPAN (ROC_SORT_TILE / 4)
#define ROC_MAX_DIGITS 512          // pass 0: (low key byte << 1) | label
#define ROC_MAX_MOTIFS 64
#define ROC_HIST_BINS (512 + 7 * 256)

struct RocRecs {
    i64 n_blocks, n_rec;
    const i64 *rec_off, *rec_pos;   // [n_blocks + 1], [n_rec]
    const double *rec_stat;
};

// the block of record r: the last b with rec_off[b] <= r (empty blocks share their offset with the next)
__device__ __forceinline__ i64 roc_block_of(const RocRecs &R, i64 r)
{
    i64 lo = 0, hi = R.n_blocks;
    while (hi - lo > 1) {
        const i64 mid = lo + (hi - lo) / 2;
        if (R.rec_off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// bit 0: keep, bit 1: label
struct RocMotifLabel {
    const uint8_t *blk_minus;           // [n_blocks] 1: minus strand
    const i64 *blk_seq_start, *seq_off; // [n_blocks], [n_blocks + 1]
    const uint8_t *seq;                 // base codes, all blocks
    const i32 *mot;                     // [n_motifs][4]: length, mod_pos (1-based), mod_base code, first set
    const uint8_t *sets;                // one 4-bit base set per motif position
    int mode, label;

    __device__ int operator()(const RocRecs &R, i64 r, int m) const
    {
        const i64 b = roc_block_of(R, r);
        const i64 s0 = seq_off[b], L = seq_off[b + 1] - s0;
        const bool minus = blk_minus[b] != 0;
        const i64 idx = R.rec_pos[r] - blk_seq_start[b];
        const i32 len = mot[4 * m], mp = mot[4 * m + 1], mb = mot[4 * m + 2], set0 = mot[4 * m + 3];
        bool base = false;
        if (idx >= 0 && idx < L) {
            const int c = seq[s0 + idx];
            base = c < 4 && (minus ? 3 - c : c) == mb;
        }
        if (mode == 0 && !base) return 0;
        bool match = true;
        for (i32 j = 0; j < len && match; j++) {
            const i64 o = j - (mp - 1), g = minus ? idx - o : idx + o;
            if (g < 0 || g >= L) { match = false; break; }
            const int c = seq[s0 + g];
            match = c < 4 && ((sets[set0 + j] >> (minus ? 3 - c : c)) & 1);
        }
        if (mode == 0) return 1 | (match ? 2 : 0);
        return match ? (1 | (label ? 2 : 0)) : 0;
    }
};

struct RocLocLabel {
    const i64 *blk_loc;                 // [n_blocks][4]: mod lo, hi, unmod lo, hi
    const i64 *mod, *unmod;             // sorted inside every block's slice

    __device__ int operator()(const RocRecs &R, i64 r, int) const
    {
        const i64 b = roc_block_of(R, r), x = R.rec_pos[r];
        const i64 *s = blk_loc + 4 * b;
        if (find(mod, s[0], s[1], x)) return 3;
        return find(unmod, s[2], s[3], x) ? 1 : 0;
    }
    __device__ static bool find(const i64 *v, i64 lo, i64 hi, i64 x)
    {
        const i64 end = hi;
        while (lo < hi) {
            const i64 mid = lo + (hi - lo) / 2;
            if (v[mid] < x) lo = mid + 1; else hi = mid;
        }
        return lo < end && v[lo] == x;
    }
};

// the count functors of k_chunk_total: whether (record i, motif m) is kept under the label functor f ...
template <class F>
struct RocKept {
    F f;
    RocRecs R;
    __device__ int operator()(i64 i, int m) const { return f(R, i, m) & 1; }
};
// ... and the words of an array themselves
template <class T>
struct ArrayCount {
    const T *v;
    __device__ T operator()(i64 i, int) const { return v[i]; }
};

// the kept pairs in (motif, record) order from block_base on; out_index (may be NULL): the record
template <class F>
__global__ void __launch_bounds__(256) k_roc_scatter(F f, RocRecs R, const i64 *block_base, double *out_stat,
    uint8_t *out_label, i64 *out_index)
{
    __shared__ i64 lds[4];
    const i64 i0 = (i64)blockIdx.x * SCAN_CHUNK + threadIdx.x * 4;
    int fl[4];
    i64 keep[4], t;
    const auto flag = [&](i64 i, int m) { return (fl[i - i0] = f(R, i, m)) & 1; };
    i64 at = block_base[(i64)blockIdx.y * gridDim.x + blockIdx.x] + chunk_scan(R.n_rec, flag, lds, keep, t);
    for (int j = 0; j < 4; j++)
        if (keep[j]) {
            out_stat[at] = R.rec_stat[i0 + j];
            out_label[at] = (uint8_t)(fl[j] >> 1);
            if (out_index) out_index[at] = i0 + j;
            at++;
        }
}

// ---- rank counts -------------------------------------------------------------------------------
__device__ __forceinline__ u32 roc_digit(u64 key, u32 label, int pass)
{
    return pass == 0 ? (u32)((key & 255) << 1) | label : (u32)((key >> (8 * pass)) & 255);
}
__host__ __device__ __forceinline__ int roc_hist_base(int pass) { return pass == 0 ? 0 : 256 + 256 * pass; }

// keys, labels made 0 / 1 in place, the NaN count (hist[ROC_HIST_BINS]) and the digit counts of all eight
// passes over the whole input
__global__ void __launch_bounds__(256) k_roc_keys(i64 n, const double *stat, uint8_t *label, u64 *key,
    unsigned long long *hist)
{
    __shared__ u32 h[ROC_HIST_BINS + 1];
    for (int k = threadIdx.x; k <= ROC_HIST_BINS; k += 256) h[k] = 0;
    __syncthreads();
    // (a loop the whole workgroup walks together, so that the ballots below see every lane)
    for (i64 base = (i64)blockIdx.x * 256; base < n; base += (i64)gridDim.x * 256) {
        const i64 i = base + threadIdx.x;
        const bool live = i < n;
        const double x = live ? stat[i] : 0.0;
        const u64 k = f64_key(x == 0.0 ? 0.0 : x);
        const u32 lab = live && label[i] ? 1 : 0;
        if (live) { key[i] = k; label[i] = (uint8_t)lab; }
        if (live && x != x) atomicAdd(&h[ROC_HIST_BINS], 1u);
        const u64 live_mask = __ballot(live);
        for (int p = 0; p < 8; p++) {
            // a digit shared by the whole wavefront (the constant low bytes of statistics on a coarse grid) is
            // one add of the count, not 64 adds to one address
            const u32 d = roc_digit(k, lab, p);
            const u32 d0 = (u32)__builtin_amdgcn_readfirstlane((int)d);   // lane 0 is live whenever any lane is
            if (__ballot(live && d == d0) == live_mask) {
                if ((threadIdx.x & 63) == 0 && live) atomicAdd(&h[roc_hist_base(p) + d0], (u32)__popcll(live_mask));
            } else if (live)
                atomicAdd(&h[roc_hist_base(p) + d], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k <= ROC_HIST_BINS; k += 256)
        if (h[k]) atomicAdd(&hist[k], (unsigned long long)h[k]);
}

// table[digit * gridDim.x + tile]: the tile's entries with that digit
__global__ void __launch_bounds__(256) k_roc_hist(i64 n, int pass, int n_digits, const u64 *key, const uint8_t *label,
    u32 *table)
{
    __shared__ u32 h[ROC_MAX_DIGITS];
    for (int k = threadIdx.x; k < n_digits; k += 256) h[k] = 0;
    __syncthreads();
    const i64 t0 = (i64)blockIdx.x * ROC_SORT_TILE;
    for (int k = threadIdx.x; k < ROC_SORT_TILE; k += 256) {
        const i64 i = t0 + k;
        if (i < n) atomicAdd(&h[roc_digit(key[i], label[i], pass)], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_digits; k += 256) table[(i64)k * gridDim.x + blockIdx.x] = h[k];
}

// scan of the table (m words, every prefix below 2^31): after the chunk sums and their prefix (block_base),
// the exclusive prefix in place
__global__ void __launch_bounds__(256) k_roc_tab_apply(i64 m, u32 *table, const i64 *block_base)
{
    __shared__ i64 lds[4];
    const i64 i0 = (i64)blockIdx.x * SCAN_CHUNK + threadIdx.x * 4;
    i64 v[4], t;
    i64 at = block_base[blockIdx.x] + chunk_scan(m, ArrayCount<u32>{table}, lds, v, t);
    for (int j = 0; j < 4; j++)
        if (i0 + j < m) { table[i0 + j] = (u32)at; at += v[j]; }
}

// stable scatter of one tile; table: the scanned table (first output index of every (digit, tile))
__global__ void __launch_bounds__(256) k_roc_scatter_pass(i64 n, int pass, int n_digits, const u64 *key,
    const uint8_t *label, const u32 *table, u64 *out_key, uint8_t *out_label)
{
    __shared__ u32 cnt[4][ROC_MAX_DIGITS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < 4 * ROC_MAX_DIGITS; k += 256) cnt[k / ROC_MAX_DIGITS][k % ROC_MAX_DIGITS] = 0;
    __syncthreads();
    const i64 w0 = (i64)blockIdx.x * ROC_SORT_TILE + (i64)w * ROC_WAVE_SPAN;
    for (int s = 0; s < ROC_WAVE_SPAN; s += 64) {
        const i64 i = w0 + s + lane;
        if (i < n) atomicAdd(&cnt[w][roc_digit(key[i], label[i], pass)], 1u);
    }
    __syncthreads();
    // per digit: the wavefronts' counts -> each wavefront's first output index
    for (int d = threadIdx.x; d < n_digits; d += 256) {
        u32 at = table[(i64)d * gridDim.x + blockIdx.x];
        for (int k = 0; k < 4; k++) { const u32 c = cnt[k][d]; cnt[k][d] = at; at += c; }
    }
    __syncthreads();
    for (int s = 0; s < ROC_WAVE_SPAN; s += 64) {
        const i64 i = w0 + s + lane;
        const bool live = i < n;
        const u64 k = live ? key[i] : 0;
        const u32 lab = live ? label[i] : 0;
        const u32 d = roc_digit(k, lab, pass);
        const u64 peers = wave_key_peers(d, 9, live);
        if (live) {
            const u32 rank = __popcll(peers & (((u64)1 << lane) - 1)), c = __popcll(peers);
            const u32 cur = cnt[w][d];
            const i64 o = (i64)cur + rank;
            if (o < n) { out_key[o] = k; out_label[o] = (uint8_t)lab; }
            if (rank == c - 1) cnt[w][d] = cur + c;
        }
        // cnt[w] belongs to this wavefront alone: only its own stores have to be ordered before its next loads.  The
        // workgroup barrier does that (every wavefront runs the same 16 steps) and is more than is needed.
        __syncthreads();
    }
}

// tp_at[j]: True labels among the ranks[j] + 1 first sorted entries; a rank outside [0, n) sets *bad
__global__ void k_roc_gather(i64 n, i64 n_ranks, const i64 *ranks, const uint8_t *label, const i64 *block_base,
    i64 *tp_at, i32 *bad)
{
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n_ranks; j += (i64)gridDim.x * blockDim.x) {
        const i64 r = ranks[j];
        if (r < 0 || r >= n) { *bad = 1; tp_at[j] = 0; continue; }
        const i64 c = r / SCAN_CHUNK;
        i64 sum = block_base[c];
        for (i64 i = c * SCAN_CHUNK; i <= r; i++) sum += label[i];
        tp_at[j] = sum;
    }
}

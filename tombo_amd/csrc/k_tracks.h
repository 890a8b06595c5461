// k_tracks.h -- genome tracks: the pileup of per-base values over every read at every genomic
// position (get_mean_slot_genome_centric, tombo_helper.py:1661-1676; TomboReads._compute_coverage,
// :1394-1404), its ordered compactions (filter_cs_nans, _text_output_commands.py:230-233;
// iter_coverage_regions, tombo_helper.py:1430-1453) and the sample - control difference with its
// N largest positions (get_signal_differences / get_largest_signal_differences, :1714-1742).
//
// Pileup.  The reference adds the reads to a float64 array one after the other, so the sum of a
// position is the left-to-right sum of its values in READ ORDER and depends on that order.  A
// floating-point atomic, or any split of one position's reads over several threads, reorders the
// adds.  Here the positions of a window are cut into tiles of TRK_TILE, one workgroup per tile, one
// thread per position; the host hands every tile the reads that overlap it, in input order (CSR:
// tile_read_off, tile_reads), and a thread walks that list from front to back.  Work is
// O(positions x reads that touch their tile), each position is written by its own thread only, and
// the sums stay in device memory between calls: a further call continues every position's chain
// where the last one stopped, which is what one call over all the reads would have done.
// A workgroup stages the records of up to TRK_TILE listed reads in LDS (one read per thread), then
// every thread takes them TRK_U at a time: the value loads of TRK_U reads are issued first, the
// adds follow in list order (memory-level parallelism: the note at the top of k_select.h).
//
// Ordered compaction: flag, scan, scatter over chunks of SCAN_CHUNK consecutive elements, order kept
// (k_chunk_total and k_exclusive_prefix of k_scan.h, then k_trk_scatter).  The flag is one of
// TRK_KEEP_* (TrkKeep); the same three kernels serve the NaN filter, the run-length form of a coverage
// track and the two selections of the top-N search.
//
// Top N.  |a - b| after nan_to_num is non-negative, so its bit pattern orders like the value.  Eight
// passes of a 256-bin histogram over the whole grid (integer atomics: counts do not depend on
// their order) fix the key of the N-th largest value one byte at a time, most significant first
// (k_trk_hist, k_trk_pick); what is larger than it is compacted, then as many of the positions that
// equal it as are still missing, the HIGHEST positions first.
#pragma once
#include "tba_common.h"
#include "k_scan.h"

#define TRK_TILE 256        // positions per tile = threads per workgroup of k_trk_add
#define TRK_MAX_SLOTS 3
#define TRK_U 4             // reads whose loads are in flight together

// read_flags: bit 0 minus strand (the slot arrays are read-centric: reversed to genome order);
// bit 1 + s: the read has slot s
struct TrkAdd {
    i64 win_start, W;       // the window [win_start, win_start + W) of the chromosome
    const i64 *read_start, *read_end, *read_off;
    const uint8_t *read_flags;
    const double *slot[TRK_MAX_SLOTS];
    const i64 *tile_off;
    const i32 *tile_reads;
    double *sum;            // [NS][W]
    i64 *cov, *rcov;        // [NS][W] values added; [W] reads whose [start, end) holds the position
};

template <int NS>
__global__ void __launch_bounds__(TRK_TILE) k_trk_add(TrkAdd a)
{
    __shared__ i64 s_start[TRK_TILE], s_end[TRK_TILE], s_off[TRK_TILE], s_len[TRK_TILE];
    __shared__ u32 s_fl[TRK_TILE];
    const int tid = threadIdx.x;
    const i64 p = (i64)blockIdx.x * TRK_TILE + tid;   // inside the window
    const i64 g = a.win_start + p;                    // on the chromosome
    const bool live = p < a.W;
    double sum[NS];
    i64 cov[NS], rc = 0;
#pragma unroll
    for (int s = 0; s < NS; s++) { sum[s] = live ? a.sum[s * a.W + p] : 0.0; cov[s] = live ? a.cov[s * a.W + p] : 0; }
    if (live) rc = a.rcov[p];
    const i64 q0 = a.tile_off[blockIdx.x], q1 = a.tile_off[blockIdx.x + 1];
    for (i64 c = q0; c < q1; c += TRK_TILE) {
        const int m = (int)(q1 - c < TRK_TILE ? q1 - c : TRK_TILE);
        __syncthreads();
        if (tid < m) {
            const i64 q = a.tile_reads[c + tid];
            s_start[tid] = a.read_start[q];
            s_end[tid] = a.read_end[q];
            s_off[tid] = a.read_off[q];
            s_len[tid] = a.read_off[q + 1] - a.read_off[q];
            s_fl[tid] = a.read_flags[q];
        }
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < m; j += TRK_U) {
            double v[TRK_U][NS];
            bool has[TRK_U][NS], in_read[TRK_U];
#pragma unroll
            for (int u = 0; u < TRK_U; u++) {
                const int jj = j + u < m ? j + u : m - 1;
                const bool listed = j + u < m;
                const i64 k = g - s_start[jj], len = s_len[jj];
                const u32 fl = s_fl[jj];
                const bool in_slot = listed && k >= 0 && k < len;
                in_read[u] = listed && k >= 0 && g < s_end[jj];
                const i64 idx = s_off[jj] + ((fl & 1) ? len - 1 - k : k);
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    has[u][s] = in_slot && ((fl >> (1 + s)) & 1);
                    v[u][s] = has[u][s] ? a.slot[s][idx] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < TRK_U; u++) {
#pragma unroll
                for (int s = 0; s < NS; s++)
                    if (has[u][s]) { sum[s] += v[u][s]; cov[s]++; }
                rc += in_read[u];
            }
        }
    }
    if (live) {
#pragma unroll
        for (int s = 0; s < NS; s++) { a.sum[s * a.W + p] = sum[s]; a.cov[s * a.W + p] = cov[s]; }
        a.rcov[p] = rc;
    }
}

// mean = sum / cov; 0 / 0 = NaN where nothing was added
__global__ void k_trk_finish(i64 n, const double *sum, const i64 *cov, double *mean)
{
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x)
        mean[i] = sum[i] / (double)cov[i];
}

// np.nan_to_num(a - b) or np.nan_to_num(np.abs(a - b)); key (ABS only, may be NULL): the value's bits
template <bool ABS>
__global__ void k_trk_diff(i64 n, const double *a, const double *b, double *out, u64 *key)
{
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        double d = a[i] - b[i];
        if (ABS) d = fabs(d);
        if (d != d) d = 0.0;
        else if (d == INFINITY) d = 1.7976931348623157e308;
        else if (d == -INFINITY) d = -1.7976931348623157e308;
        out[i] = d;
        if (ABS && key) key[i] = (u64)__double_as_longlong(d);
    }
}

// ---- ordered compaction ------------------------------------------------------------------------
enum { TRK_KEEP_NOT_NAN = 0,   // x: float64 bits; keeps what is not NaN
       TRK_KEEP_RUN_START,     // x: int64; keeps i == 0 and every i with x[i] != x[i - 1]
       TRK_KEEP_ABOVE,         // x: keys; keeps x[i] > sel->key
       TRK_KEEP_EQUAL };       // x: keys; keeps x[i] == sel->key

// the state of the top-N search, in device memory
struct TrkSel {
    u64 key;                 // the bytes fixed so far of the N-th largest key
    i64 remaining;           // how many of the values that share those bytes are still wanted
    i64 n_above, n_equal;    // after the last pass: keys > key, keys == key
    unsigned long long hist[256];
};

// whether element i of x is kept under `mode` (sel: the search state of the two key modes, else NULL)
struct TrkKeep {
    int mode;
    const u64 *x;
    const TrkSel *sel;

    __device__ bool operator()(i64 i, int) const
    {
        const u64 v = x[i];
        switch (mode) {
        case TRK_KEEP_NOT_NAN: return (v & 0x7fffffffffffffffull) <= 0x7ff0000000000000ull;
        case TRK_KEEP_RUN_START: return i == 0 || v != x[i - 1];
        case TRK_KEEP_ABOVE: return v > sel->key;
        default: return v == sel->key;
        }
    }
};

// the kept elements' indices and src words, in order, from output index -skip on (what falls before
// index 0 is dropped: skip = the kept elements to leave out at the front; sel: skip = n_equal -
// remaining).  TRK_KEEP_RUN_START also writes n behind the last index (iter_coverage_regions' end).
__global__ void __launch_bounds__(256) k_trk_scatter(i64 n, TrkKeep f, const u64 *src, const i64 *block_base,
    const i64 *total, i64 *out_pos, u64 *out_val)
{
    __shared__ i64 lds[4];
    const int mode = f.mode;
    const i64 skip = mode == TRK_KEEP_EQUAL ? f.sel->n_equal - f.sel->remaining : 0;
    const i64 i0 = (i64)blockIdx.x * SCAN_CHUNK + threadIdx.x * 4;
    i64 keep[4], t;
    i64 at = block_base[blockIdx.x] + chunk_scan(n, f, lds, keep, t) - skip;
    for (int j = 0; j < 4; j++)
        if (keep[j]) {
            if (at >= 0) { out_pos[at] = i0 + j; out_val[at] = src[i0 + j]; }
            at++;
        }
    if (mode == TRK_KEEP_RUN_START)
        for (int j = 0; j < 4; j++) if (i0 + j == n - 1) out_pos[*total] = n;
}

// ---- the key of the N-th largest value -----------------------------------------------------------
// one pass: the histogram of byte `shift / 8` over the keys that share the bytes above it with sel->key
__global__ void __launch_bounds__(256) k_trk_hist(i64 n, const u64 *key, int shift, TrkSel *sel)
{
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const u64 want = sel->key;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const u64 k = key[i];
        if (shift == 56 || (k >> (shift + 8)) == (want >> (shift + 8))) atomicAdd(&h[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&sel->hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// one workgroup of 256: the byte in which the count from the top reaches `remaining`
__global__ void __launch_bounds__(256) k_trk_pick(int shift, TrkSel *sel)
{
    __shared__ i64 h[256];
    h[threadIdx.x] = (i64)sel->hist[threadIdx.x];
    __syncthreads();
    sel->hist[threadIdx.x] = 0;
    if (threadIdx.x != 0) return;
    i64 above = 0;
    int b = 255;
    while (b > 0 && above + h[b] < sel->remaining) above += h[b--];
    sel->key |= (u64)b << shift;
    sel->remaining -= above;
    sel->n_above += above;
    sel->n_equal = h[b];
}

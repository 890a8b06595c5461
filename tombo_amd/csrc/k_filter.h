// k_filter.h -- the device half of the "stuck read" filter (tombo/_filter_reads.py:58-96 and the worker loop's
// --obs-per-base-filter, resquiggle.py:1449-1456): per read, np.percentile(base_lens, pctl) for a few
// (pctl, thresh) pairs and whether any of them lies above its threshold.
//
// The lengths of a read are the successive differences of its base boundaries (int64, CSR), small integers
// with a rare very long one.  A percentile needs two order statistics, so nothing is sorted and no float64 copy
// of the lengths is made.  One workgroup per read:
//   pass 1   one stream over the boundaries: hist[min(len, DW_NB - 1)]++ in LDS (integer atomics) and the
//            read's longest length; an inclusive scan turns the counts into ranks in place
//   ranks    per pair the two ranks np.percentile reads (np_pctl_ranks) are looked up in the scanned
//            histogram by bisection: a rank that lands below the last bin IS its bin index
//   overflow a rank inside the last bin (a length of DW_NB - 1 or more) is the longest length when it is the
//            last rank; otherwise an exact radix select over the lengths of that bin (four passes of 8 bits on
//            the 32-bit length, dwell_select_long) finds it.  Reads without such ranks never run it.
//   result   np_pctl_lerp of the two lengths as float64 (exact below 2^53), compared strictly with thresh
// Counting and comparisons only, no floating-point atomics: two runs give the same bits.
// LDS: 16 KB of histogram + 1 KB for the select + a few words: nine workgroups fit a CU's 160 KB, more than
// the 32 wavefronts of 8 workgroups of 256 it can hold.
// Every LDS index is clamped, whatever the boundaries hold: a decreasing boundary (the host entries refuse it)
// counts as a length of the last bin.
#pragma once
#include "tba_common.h"
#include "k_select.h"    // block_stream

#define DW_NT 256        // threads per workgroup: one per bin of the select's histogram
#define DW_NB 4096       // bins of pass 1: the lengths 0 .. DW_NB - 2 exactly, the last bin everything longer

struct DwellSmem {
    u32 hist[DW_NB];     // counts, then inclusive prefix counts
    u32 sel[DW_NT];      // the select's digit histogram
    u32 wsum[DW_NT / 64];
    u32 mx;              // the read's longest length
    u32 s_prefix, s_k;   // the select's state
};

struct DwellArgs {
    i64 n_reads;
    const i64 *segs;         // base starts and the end of every read
    const i64 *seg_off;      // caller-given reads: n_reads + 1 offsets into segs
    const ReadState *rs;     // resident batch: seg_off, B and status of every read
    i64 n_pairs;
    const double *q, *thresh;
    double *vals;            // [n_reads][n_pairs], or NULL
    uint8_t *flags;          // [n_reads]
};

__device__ __forceinline__ u32 dwell_key(i64 d) { return (u64)d > 0xffffffffull ? 0xffffffffu : (u32)d; }

// sm->hist: counts -> inclusive prefix counts (all threads call, after the barrier that ends the counting)
__device__ __forceinline__ void dwell_scan(DwellSmem *sm)
{
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr int per = DW_NB / DW_NT;
    u32 loc[per], c = 0;
#pragma unroll
    for (int k = 0; k < per; k++) { c += sm->hist[tid * per + k]; loc[k] = c; }
    u32 inc = c;
    for (int d = 1; d < 64; d <<= 1) {
        const u32 t = (u32)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) sm->wsum[tid >> 6] = inc;
    __syncthreads();
    u32 exc = inc - c;
    for (int w = 0; w < (tid >> 6); w++) exc += sm->wsum[w];
#pragma unroll
    for (int k = 0; k < per; k++) sm->hist[tid * per + k] = exc + loc[k];
    __syncthreads();
}

// the bin of rank k in the scanned histogram: the first b with hist[b] > k (the last bin when there is none)
__device__ __forceinline__ int dwell_find(const DwellSmem *sm, u32 k)
{
    int lo = 0, hi = DW_NB - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sm->hist[mid] > k) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the k-th smallest (0-based) of the lengths of the last bin, S[i + 1] - S[i] >= DW_NB - 1 over i < n: radix
// select, 8 bits a pass from the top.  All threads call and all get the value; sm->hist is left alone.
__device__ i64 dwell_select_long(const i64 *S, i64 n, u32 k, DwellSmem *sm)
{
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) { sm->s_prefix = 0; sm->s_k = k; }
    for (int pass = 3; pass >= 0; pass--) {
        sm->sel[tid] = 0;
        __syncthreads();
        const int sh = 8 * pass;
        const u32 prefix = sm->s_prefix, himask = pass == 3 ? 0u : ~0u << (sh + 8);
        block_stream<4>(n, [&](i64 i) { return S[i + 1] - S[i]; }, [&](i64, i64 d) {
            const u32 key = dwell_key(d);
            if ((u64)d >= DW_NB - 1 && (key & himask) == prefix) atomicAdd(&sm->sel[(key >> sh) & 255], 1u);
        });
        __syncthreads();
        // thread b holds digit b: the digit whose ranks hold s_k
        const u32 c = sm->sel[tid], kk = sm->s_k;
        u32 inc = c;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 t = (u32)__shfl_up((int)inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) sm->wsum[tid >> 6] = inc;
        __syncthreads();
        u32 exc = inc - c;
        for (int w = 0; w < (tid >> 6); w++) exc += sm->wsum[w];
        if (exc <= kk && kk < exc + c) { sm->s_prefix = prefix | ((u32)tid << sh); sm->s_k = kk - exc; }
        __syncthreads();
    }
    const i64 res = sm->s_prefix;
    __syncthreads();                                // (the next call resets the state)
    return res;
}

// One workgroup per read.  RESIDENT: the reads of the engine's batch (a read whose status is not 0: NaN, flag 0);
// else caller-given reads by seg_off.  A read without lengths: NaN, flag 1.
template <bool RESIDENT>
__global__ __launch_bounds__(DW_NT) void k_dwell_pctl(DwellArgs a)
{
    __shared__ DwellSmem sm;
    const int tid = threadIdx.x;
    for (i64 r = blockIdx.x; r < a.n_reads; r += gridDim.x) {
        i64 off, n;
        bool live = true;
        if (RESIDENT) {
            const ReadState &s = a.rs[r];
            off = s.seg_off; n = s.B; live = s.status == TBA_OK;
        } else {
            off = a.seg_off[r]; n = a.seg_off[r + 1] - off - 1;
        }
        if (!live || n < 1) {
            if (a.vals)
                for (i64 j = tid; j < a.n_pairs; j += DW_NT) a.vals[r * a.n_pairs + j] = NAN;
            if (tid == 0) a.flags[r] = live ? 1 : 0;
            continue;
        }
        const i64 *S = a.segs + off;
        for (int b = tid; b < DW_NB; b += DW_NT) sm.hist[b] = 0;
        if (tid == 0) sm.mx = 0;
        __syncthreads();
        u32 mx = 0;
        block_stream<4>(n, [&](i64 i) { return S[i + 1] - S[i]; }, [&](i64, i64 d) {
            atomicAdd(&sm.hist[(u64)d < DW_NB - 1 ? (int)d : DW_NB - 1], 1u);
            const u32 key = dwell_key(d);
            mx = key > mx ? key : mx;
        });
        for (int m = 32; m >= 1; m >>= 1) {
            const u32 o = (u32)__shfl_xor((int)mx, m, 64);
            mx = o > mx ? o : mx;
        }
        if ((tid & 63) == 0) atomicMax(&sm.mx, mx);
        __syncthreads();
        dwell_scan(&sm);
        const i64 longest = sm.mx;
        const u32 n_short = sm.hist[DW_NB - 2];     // lengths below the last bin
        bool stuck = false;
        for (i64 j = 0; j < a.n_pairs; j++) {       // (the same for every thread: the select is collective)
            i64 rk[2], v[2];
            double t;
            np_pctl_ranks(n, a.q[j], rk[0], rk[1], t);
            for (int w = 0; w < 2; w++) {
                if (w && rk[1] == rk[0]) { v[1] = v[0]; break; }
                const int b = dwell_find(&sm, (u32)rk[w]);
                v[w] = b < DW_NB - 1 ? b : rk[w] == n - 1 ? longest : dwell_select_long(S, n, (u32)rk[w] - n_short, &sm);
            }
            const double val = np_pctl_lerp((double)v[0], (double)v[1], t);
            stuck |= val > a.thresh[j];
            if (tid == 0 && a.vals) a.vals[r * a.n_pairs + j] = val;
        }
        if (tid == 0) a.flags[r] = stuck ? 1 : 0;
        __syncthreads();                            // (the next read clears the histogram)
    }
}

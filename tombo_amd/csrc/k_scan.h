// k_scan.h -- the parallel building blocks of the statistics kernels, one copy of each: scans over a
// wavefront, a workgroup and a whole array, the row of a flat index in CSR offsets, numpy's sum by one
// wavefront, and the stable partition of items by key.  Every result here is an integer, or a double
// summed in a fixed order, so a kernel built from these writes the same bytes on every run.
//
// Scans.  wave_scan_* over the 64 lanes; block_scan_256 over a workgroup of 256; k_exclusive_prefix
// over an array by one workgroup; and for arrays too long for one workgroup the two-level form over
// chunks of SCAN_CHUNK items: k_chunk_total (each chunk's sum), k_exclusive_prefix over those, then
// the caller's own kernel, which takes every item's place from chunk_scan.  What an item counts is a
// functor f(i, y), y = blockIdx.y: a 2-D grid scans gridDim.y sequences of n items back to back.
//
// Partition by key.  Items are cut into chunks of consecutive items, one wavefront per chunk, 64
// items a step, and every chunk has a row of per-key counters that its own wavefront alone touches
// (no atomics).  Inside a step the lanes that hold the same key find each other with one ballot per
// key bit (wave_key_peers); an item's rank is the number of such lanes below it and the highest of
// them advances the chunk's counter (partition_step).  A counting pass over zeroed rows, the
// exclusive prefix of every key's counters over the chunks (k_kmer_colscan, k_kde.h) and of the
// keys' totals (k_exclusive_prefix), then the same walk again place every item: its key's offset +
// its chunk's prefix + its rank.  Work is split by item and never by key, so a key that holds most
// of the items costs what any other does.  k_key_partition is that walk for chunks of equal length.
#pragma once
#include "tba_common.h"

// ---- wavefront inclusive scans (64 lanes) ----------------------------------------------------------
__device__ __forceinline__ i64 wave_scan_add(i64 v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const i64 o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}
__device__ __forceinline__ i32 wave_scan_max(i32 v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const i32 o = __shfl_up(v, d); if (lane >= d) v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ i32 wave_rscan_min(i32 v)   // suffix min
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const i32 o = __shfl_down(v, d); if (lane + d < 64) v = o < v ? o : v; }
    return v;
}

// exclusive prefix of v over the 256 threads of the workgroup; total: their sum.  lds: 4 words.
__device__ __forceinline__ i64 block_scan_256(i64 v, i64 *lds, i64 &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const i64 inc = wave_scan_add(v);
    __syncthreads();
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    i64 base = 0;
    total = 0;
    for (int k = 0; k < 4; k++) { if (k < w) base += lds[k]; total += lds[k]; }
    return base + inc - v;
}

// One workgroup of 256: off[i] = cnt[0] + ... + cnt[i - 1] for i < n, *total = the sum of all n.
// Every thread owns one run of consecutive counts: it sums the run, the runs' sums are scanned over
// the workgroup, and it walks the run again.  No barrier per 256 counts, so a long array costs two
// streaming passes.  A thread reads a count before it writes that offset and touches its own run
// alone, so off may be cnt itself (T = i64).
template <class T>
__global__ void __launch_bounds__(256) k_exclusive_prefix(i64 n, const T *cnt, i64 *off, i64 *total)
{
    __shared__ i64 lds[4];
    const i64 run = (n + 255) / 256;
    const i64 a = (i64)threadIdx.x * run < n ? (i64)threadIdx.x * run : n;
    const i64 b = a + run < n ? a + run : n;
    i64 sum = 0, all;
    for (i64 i = a; i < b; i++) sum += (i64)cnt[i];
    i64 acc = block_scan_256(sum, lds, all);
    for (i64 i = a; i < b; i++) { const i64 v = (i64)cnt[i]; off[i] = acc; acc += v; }
    if (threadIdx.x == 0) *total = all;
}

// ---- chunks of SCAN_CHUNK items: 256 threads x 4 consecutive items ---------------------------------
#define SCAN_CHUNK 1024

// cnt[j] = f(i0 + j, blockIdx.y) for the thread's four items i0 + j < n (0 behind n); returns the sum of
// the chunk's items in front of i0, total: the chunk's sum.  lds: 4 words.
template <class F>
__device__ __forceinline__ i64 chunk_scan(i64 n, F f, i64 *lds, i64 (&cnt)[4], i64 &total)
{
    const i64 i0 = (i64)blockIdx.x * SCAN_CHUNK + threadIdx.x * 4;
    i64 c = 0;
    for (int j = 0; j < 4; j++) { cnt[j] = i0 + j < n ? (i64)f(i0 + j, (int)blockIdx.y) : 0; c += cnt[j]; }
    return block_scan_256(c, lds, total);
}

// chunk_cnt[y * gridDim.x + chunk]: the chunk's sum
template <class F>
__global__ void __launch_bounds__(256) k_chunk_total(i64 n, F f, i64 *chunk_cnt)
{
    __shared__ i64 lds[4];
    i64 cnt[4], total;
    chunk_scan(n, f, lds, cnt, total);
    if (threadIdx.x == 0) chunk_cnt[(i64)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// ---- CSR ---------------------------------------------------------------------------------------------
// row of flat index i in the CSR offsets off[n_rows + 1] (binary search)
__device__ __forceinline__ i64 dev_csr_row(const i64 *off, i64 n_rows, i64 i)
{
    i64 lo = 0, hi = n_rows - 1;
    while (lo < hi) { const i64 mid = (lo + hi + 1) >> 1; if (off[mid] <= i) lo = mid; else hi = mid - 1; }
    return lo;
}

// ---- numpy's sum by one wavefront ----------------------------------------------------------------------
// np.add.reduce of a[0 .. n) by one wavefront (all lanes call it with the same a, n; the result is valid in lane
// 0): per block of 8192 values lane 0 lists the leaves of the pairwise tree (pre-order, left first: at most
// 127), the lanes sum a leaf each, lane 0 adds the leaf sums in the recursion's order.
struct WaveSumLds {
    int l_start[128], l_len[128], n_leaf;
    double l_sum[128];
    int st_a[16], st_n[16], st_st[16];
    double st_v[16];
};
__device__ inline double wave_np_sum(const double *a, i64 n, WaveSumLds &w, int lane)
{
    double acc = 0.0;
    for (i64 c0 = 0; c0 < n; c0 += 8192) {
        const int m = (int)(n - c0 < 8192 ? n - c0 : 8192);
        if (lane == 0) {
            int sp = 0, nl = 0;
            w.st_a[0] = 0; w.st_n[0] = m;
            while (sp >= 0) {
                const int s0 = w.st_a[sp], len = w.st_n[sp];
                sp--;
                if (len <= 128) { w.l_start[nl] = s0; w.l_len[nl] = len; nl++; continue; }
                int n2 = len / 2;
                n2 -= n2 % 8;
                w.st_a[sp + 1] = s0 + n2; w.st_n[sp + 1] = len - n2; // right, visited after ...
                w.st_a[sp + 2] = s0; w.st_n[sp + 2] = n2;            // ... the left half
                sp += 2;
            }
            w.n_leaf = nl;
        }
        __syncthreads();
        for (int k = lane; k < w.n_leaf; k += 64) w.l_sum[k] = np_pairwise_leaf(a + c0 + w.l_start[k], w.l_len[k]);
        __syncthreads();
        if (lane == 0) { // the recursion again, leaf values from l_sum in visiting order
            int sp = 0, next = 0;
            double ret = 0;
            w.st_n[0] = m; w.st_st[0] = 0;
            while (sp >= 0) {
                const int len = w.st_n[sp];
                if (len <= 128) { ret = w.l_sum[next++]; sp--; continue; }
                int n2 = len / 2;
                n2 -= n2 % 8;
                if (w.st_st[sp] == 0) { w.st_st[sp] = 1; w.st_n[sp + 1] = n2; w.st_st[sp + 1] = 0; sp++; }
                else if (w.st_st[sp] == 1) { w.st_v[sp] = ret; w.st_st[sp] = 2; w.st_n[sp + 1] = len - n2; w.st_st[sp + 1] = 0; sp++; }
                else { ret = w.st_v[sp] + ret; sp--; }
            }
            acc += ret;
        }
        __syncthreads();
    }
    return acc;
}

// ---- stable partition by key ---------------------------------------------------------------------------
// the live lanes of the wavefront that hold this lane's key (key_bits: the bits that tell the keys apart);
// every lane of the wavefront calls it
__device__ __forceinline__ u64 wave_key_peers(i64 key, int key_bits, bool live)
{
    u64 peers = __ballot(live);
    for (int b = 0; b < key_bits; b++) {
        const bool bit = (key >> b) & 1;
        const u64 m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// One step of a live lane: its item's place among the chunk's items of its key, counter[key] + the peers
// below this lane; the highest peer moves the counter past them all.  The counters may be in global memory
// and the next step's lanes read what other lanes stored here, so the caller puts a __syncthreads()
// between two steps (it orders a wavefront's own stores before its next loads).
__device__ __forceinline__ u32 partition_step(u64 peers, u32 *counter, i64 key)
{
    const int lane = threadIdx.x & 63;
    const u32 rank = __popcll(peers & (((u64)1 << lane) - 1)), cnt = __popcll(peers);
    const u32 cur = counter[key];
    if (rank == cnt - 1) counter[key] = cur + cnt;
    return cur + rank;
}

// the k-mer of the K base codes from c on, first base most significant; -1: a code outside ACGT (0-3)
__device__ __forceinline__ i64 window_kmer(const uint8_t *c, int K)
{
    i64 k = 0;
    bool acgt = true;
    for (int j = 0; j < K; j++) { const unsigned b = c[j]; acgt = acgt && b < 4; k = k * 4 + (b & 3); }
    return acgt ? k : -1;
}

// One wavefront (block of 64) per chunk of `chunk` consecutive items (a multiple of 64).  src.key(i): the
// key of item i in [0, n_keys), -1: the item is left out; src.store(i, o) (FILL): item i goes to output
// index o.  rows[chunk][key]: counted here (FILL false, zeroed before), or the chunk's starting rank inside
// the key's segment (FILL true, from k_kmer_colscan); key_off (FILL): the keys' segment offsets.
template <bool FILL, class Src>
__global__ void __launch_bounds__(64) k_key_partition(Src src, i64 n, i64 chunk, i64 n_keys, int key_bits, u32 *rows,
                                                      const i64 *key_off)
{
    const int lane = threadIdx.x;
    u32 *row = rows + (i64)blockIdx.x * n_keys;
    const i64 i0 = (i64)blockIdx.x * chunk;
    const i64 i1 = i0 + chunk < n ? i0 + chunk : n;
    for (i64 c = i0; c < i1; c += 64) {
        const i64 i = c + lane;
        const i64 key = i < i1 ? src.key(i) : -1;
        const u64 peers = wave_key_peers(key, key_bits, key >= 0);
        if (key >= 0) {
            const u32 at = partition_step(peers, row, key);
            if (FILL) src.store(i, key_off[key] + at);
        }
        __syncthreads();   // between two steps: see partition_step
    }
}

// k_center.h -- ts.center_model_to_median_norm (tombo_stats.py:1599-1705) for a batch of reads: what the centring
// step list of tba_engine.hip adds to the kernels of the resquiggle pass.
//   k_center_place   the read's own event boundaries, from the `start` column of its Events table, as the
//                    boundaries k_theil_sen takes (get_read_corr_factors, :1642-1656), with every check that keeps a
//                    caller's number from becoming a device address
//   k_center_pick    the first max_reads successes in call order and the np.median of their factors (:1674-1698)
#pragma once
#include "k_select.h"

#define CENTER_COORD_MAX ((i64)1 << 62) // |read_start_rel_to_raw| and |start| stay below: no sum of two overflows

// One workgroup per read.  starts / start_off: the `start` columns of the batch (CSR, as the caller gave them);
// rsr[read]: read_start_rel_to_raw.  With up = central_pos and dn = K - up - 1 the read of n rows gets
//   read_start = rsr + start[up],  segs[j] = start[up + j] - start[up] for j = 0 .. n - K + 1 (= B),  norm_len = segs[B]
// -- the B + 1 entries of its slice of `segs` (B = seq_len - K + 1, ReadState).  A read fails where the per-read form
// of the host layer raises: rows and bases differ in number or there are fewer than K + 1 of them
// (TBA_SEQ_SEG_MISMATCH), boundaries not strictly increasing (TBA_ZERO_LEN), read_start < 0 (TBA_NEG_START),
// read_start + norm_len > n_raw (TBA_PAST_END).  A value outside +-CENTER_COORD_MAX fails like a boundary out of
// order.  Nothing is read outside the read's rows, and a read that passes has 0 <= read_start, segs ascending from
// 0 to norm_len, read_start + norm_len <= n_raw: every sample k_theil_sen sums lies inside the read's signal.
// status_out[read]: the read's status after this kernel (the statuses of the batch in one small download).
__global__ __launch_bounds__(256) void k_center_place(ReadState *rs, const DevParams *dp, const i64 *starts,
    const i64 *start_off, const i64 *rsr, i64 *segs, i32 *status_out)
{
    ReadState &r = rs[blockIdx.x];
    const int tid = threadIdx.x;
    const i32 was = r.status;                   // (read by every thread before thread 0 may write it: barrier below)
    const i64 K = dp->kmer_width, up = dp->central_pos;
    const i64 n_rows = start_off[blockIdx.x + 1] - start_off[blockIdx.x];
    const i64 *st = starts + start_off[blockIdx.x];
    i64 *out = segs + r.seg_off;
    int rc = was;
    if (rc == TBA_OK && (n_rows != r.seq_len || r.seq_len < K + 1 || r.B != r.seq_len - K + 1)) rc = TBA_SEQ_SEG_MISMATCH;
    int bad = 0;
    i64 s0 = 0;
    if (rc == TBA_OK) {
        s0 = st[up];                            // (up <= K - 2 < n_rows)
        const i64 my_rsr = rsr[blockIdx.x];
        if (s0 <= -CENTER_COORD_MAX || s0 >= CENTER_COORD_MAX || my_rsr <= -CENTER_COORD_MAX || my_rsr >= CENTER_COORD_MAX) bad = 1;
        for (i64 j = tid; j <= r.B; j += 256) { // row up + j <= up + B = n_rows - dn < n_rows
            const i64 a = st[up + j];
            if (a <= -CENTER_COORD_MAX || a >= CENTER_COORD_MAX) { bad = 1; continue; }
            if (j > 0) {
                const i64 b = st[up + j - 1];
                if (b <= -CENTER_COORD_MAX || b >= CENTER_COORD_MAX || a - b <= 0) bad = 1;
            }
            out[j] = a - s0;
        }
    }
    bad = __syncthreads_or(bad);
    if (tid != 0) return;
    if (rc == TBA_OK) {
        if (bad) rc = TBA_ZERO_LEN;
        else {
            const i64 read_start = rsr[blockIdx.x] + s0, norm_len = st[up + r.B] - s0;
            if (read_start < 0) rc = TBA_NEG_START;
            else if (read_start > r.n_raw || norm_len > r.n_raw - read_start) rc = TBA_PAST_END;
            else { r.read_start = r.dp_read_start = read_start; r.norm_len = norm_len; }
        }
    }
    if (rc != was) r.status = rc;               // (every failure found here: k_theil_sen must not take the read)
    status_out[blockIdx.x] = rc;
}

// One workgroup.  The reads of the call in order, behind the n_prior successes of the calls before it
// (prior[i][2]: their factors): those with status TBA_OK are the successes, the first max_reads of them count.
// factors[read][2] = (shift_corr_factor, scale_corr_factor) = (-inter / slope, 1 / slope) of k_theil_sen, NaN for a
// read that failed; status_out[read]; medians[2] = np.median of the counted factors (the middle value, or the mean
// of the two middle values: block_median; NaN where one of them is NaN, as numpy has it), untouched without a
// success; *n_used = how many counted.  sel: room for 2 * (n_prior + n_reads) doubles.
__global__ __launch_bounds__(SEL_NT) void k_center_pick(const ReadState *rs, i64 n_reads, const double *prior,
    i64 n_prior, i64 max_reads, double *factors, i32 *status_out, double *sel, double *medians, i64 *n_used)
{
    __shared__ SelectSmem sm;
    __shared__ i64 s_cnt[SEL_NT / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double *sel_a = sel, *sel_b = sel + (n_prior + n_reads);
    i64 taken = n_prior < max_reads ? n_prior : max_reads;
    taken = taken < 0 ? 0 : taken;
    for (i64 i = tid; i < taken; i += SEL_NT) { sel_a[i] = prior[2 * i]; sel_b[i] = prior[2 * i + 1]; }
    for (i64 i0 = 0; i0 < n_reads; i0 += SEL_NT) { // (workgroup-uniform trip count: barriers inside)
        const i64 i = i0 + tid;
        const bool ok = i < n_reads && rs[i].status == TBA_OK;
        const double a = ok ? rs[i].ts[2] : NAN, b = ok ? rs[i].ts[3] : NAN;
        if (i < n_reads) { status_out[i] = rs[i].status; factors[2 * i] = a; factors[2 * i + 1] = b; }
        const u64 m = __ballot(ok);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        i64 before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < SEL_NT / 64; w++) { if (w < wave) before += s_cnt[w]; total += s_cnt[w]; }
        const i64 rank = taken + before;
        if (ok && rank < max_reads) { sel_a[rank] = a; sel_b[rank] = b; }
        taken += total;
        __syncthreads();
    }
    const i64 m = taken < max_reads ? taken : max_reads;
    if (m > 0) {
        __threadfence_block();
        __syncthreads();                         // (the list was written by other threads of this workgroup)
        int nan = 0;
        for (i64 i = tid; i < m; i += SEL_NT) nan |= (sel_a[i] != sel_a[i] ? 1 : 0) | (sel_b[i] != sel_b[i] ? 2 : 0);
        const int nan_a = __syncthreads_or(nan & 1), nan_b = __syncthreads_or(nan & 2);
        double med_a = NAN, med_b = NAN;
        if (!nan_a) med_a = block_median([&](i64 i) { return f64_key(sel_a[i]); }, m, &sm);
        if (!nan_b) med_b = block_median([&](i64 i) { return f64_key(sel_b[i]); }, m, &sm);
        if (tid == 0) { medians[0] = med_a; medians[1] = med_b; }
    }
    if (tid == 0) *n_used = m;
}

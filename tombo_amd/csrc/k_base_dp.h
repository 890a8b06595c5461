// k_base_dp.h -- the pieces of the raw-signal DP of one base (_c_dynamic_programming.pyx:17-182), one copy each, for
// the window forms of the skipped-base stage (k_tail.h) and for the per-kernel C entries (k_cabi.h).
#pragma once
#include "tba_common.h"

// c_base_z_scores (pyx:17-32) of one sample from its quotient q = (x - mean) / sd.  The division is the caller's:
// the IEEE quotient, or div_by_recip (tba_common.h: the same value) where the row's 1 / sd is at hand.
__device__ __forceinline__ double base_z(double q, bool winsor, double mh)
{
    if (q > 0) q = -q;
    if (winsor && q < -mh) q = -mh;
    return q;
}

// c_base_forward_pass (pyx:99-163): forward scores b_fwd and last-diagonal counters b_ld of a base over the positions
// [b_start, b_end) from those of the previous base over [prev_start, prev_end); b_data / prev_data: the two bases'
// z-scores; cum: room for np.cumsum(prev_data).  One serial chain, the previous position carried in registers.
// Negative indices wrap like the Cython buffer accesses, other out-of-range accesses are the reference's IndexError
// (TBA_INTERNAL).  Callers: the C entry tba_c_base_forward_pass, whose arrays and bounds are a caller's and may take
// every one of those paths, and raw_window_dp's general row (k_tail.h).  There both bases span len positions m apart,
// so i0 = m - 1 and `at` = len - m are not negative for len >= m (no wrap) and pos - b_start <= len - m < b_len (that
// return is not reached): on every window the planner makes (len > 2 m) the row is what direct indexing gives.  A
// window shorter than m, which only del_fix_window == max_del_fix_window lets through, gets the reference's
// wrap-around or its IndexError instead of a read in front of the row.
__device__ __forceinline__ int base_forward_row(const double *b_data, i64 b_start, i64 b_end,
    const double *prev_data, i64 prev_start, i64 prev_end, const double *prev_fwd, const i64 *prev_ld, i64 m,
    double *cum, double *b_fwd, i64 *b_ld)
{
    const i64 b_len = b_end - b_start, plen = prev_end - prev_start;
    { double acc = 0; for (i64 k = 0; k < plen; k++) { acc = k == 0 ? prev_data[k] : acc + prev_data[k]; cum[k] = acc; } }
    i64 i0 = b_start - prev_start - 1;
    if (i0 < 0) i0 += plen;
    if (i0 < 0 || i0 >= plen) return TBA_INTERNAL;
    double stay_run = b_data[0] + prev_fwd[i0]; // b_fwd / b_ld of the previous position
    i64 ld_run = 1;
    b_fwd[0] = stay_run;
    b_ld[0] = 1;
    for (i64 pos = b_start + 1; pos < prev_end + 1; pos++) {
        if (pos - b_start >= b_len) return TBA_INTERNAL;
        i64 lag = 1;
        for (;;) {
            i64 idx = pos - prev_start - lag;
            if (idx < 0) idx += plen;
            if (idx < 0 || idx >= plen) return TBA_INTERNAL;
            if (prev_ld[idx] + lag <= m) lag++;
            else break;
        }
        i64 di = pos - prev_start - lag;
        if (di < 0) di += plen;
        double diag = prev_fwd[di];
        if (lag > 1) diag += cum[pos - prev_start - 1] - cum[di];
        double best;
        if (diag > stay_run) { best = diag; ld_run = 1; }
        else { best = stay_run; ld_run += 1; }
        stay_run = b_data[pos - b_start] + best;
        b_fwd[pos - b_start] = stay_run;
        b_ld[pos - b_start] = ld_run;
    }
    if (b_end > prev_end + 1) {
        i64 at = prev_end - b_start;
        if (at < 0) at += b_len;
        if (at < 0 || at >= b_len) return TBA_INTERNAL;
        double fv = b_fwd[at];
        i64 cl = b_ld[at];
        for (i64 k = 0; k < b_end - prev_end - 1; k++) {
            fv += b_data[k + prev_end - b_start + 1];
            cl += 1;
            b_fwd[k + prev_end - b_start + 1] = fv;
            b_ld[k + prev_end - b_start + 1] = cl;
        }
    }
    return TBA_OK;
}

// c_base_traceback (pyx:165-182), the walk: the boundary between the base whose forward scores are `curr` (from
// curr_start) and the one before it (`next`, over [next_start, next_end)), walking down from sig_start.  -1 where the
// reference runs off the loop (returns None).  PY_INDEX: the arrays are a caller's (tba_c_base_traceback) -- negative
// indices wrap, others out of range are the reference's IndexError (-2); raw_window_dp's own rows are indexed inside
// [0, len) by construction (curr_start < sp <= sig_start, sp - 1 < next_end) and its walk does without the checks.
template <bool PY_INDEX>
__device__ __forceinline__ i64 base_traceback(const double *curr, i64 curr_len, i64 curr_start, const double *next,
    i64 next_len, i64 next_start, i64 next_end, i64 sig_start, i64 m)
{
    i64 cnt = 1;
    for (i64 sp = sig_start; sp >= 0; sp--) {
        cnt += 1;
        if (cnt <= m || sp - 1 >= next_end) continue;
        if (sp <= curr_start) return sp;
        i64 ni = sp - next_start - 1, ci = sp - curr_start - 1;
        if (PY_INDEX) {
            if (ni < 0) ni += next_len;
            if (ci < 0) ci += curr_len;
            if (ni < 0 || ni >= next_len || ci < 0 || ci >= curr_len) return -2;
        }
        if (next[ni] > curr[ci]) return sp;
    }
    return -1;
}

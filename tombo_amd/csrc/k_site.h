// k_site.h -- per-site modified fractions of the model-based tests (de_novo, sample_compare,
// model_compare): compute_reg_stats / collate_reg_stats / apply_per_read_thresh
// (tombo_stats.py:4084-4229) and calc_damp_fraction (:2537-2552) for a batch of tracks.
//
// A track is one (region, statistic name); it covers the genomic interval [trk_start, trk_end) and
// its positions are numbered gp = pos_off[t] + (g - trk_start[t]) over the batch (as k_group.h
// numbers the positions of its regions).  Every per-read statistic is computed once, by the device
// functions of k_cabi.h that k_read_pvals / k_c_llh_windows run, and never leaves the device unless
// the per-read output is asked for.  Steps:
//   k_site_z / k_site_win   one thread per statistic: the statistic, then up to three integer
//                           atomic adds on the counters (cov, valid, ge) of its (track, position)
//   k_site_stat             the same scatter from statistics k_read_pvals left on the device
//                           (Fisher's method, fm_offset > 0)
//   k_site_rec              the same scatter from STORED per-read records (a per-read statistics
//                           file: aggregate_per_read_stats), a track being one stored block
//   k_site_finish           one wavefront per track: positions with cov > 0 compacted in ascending
//                           order, fraction / coverage / dampened fraction written out
// The counters are integers, so the sums do not depend on the order the atomics land in.
#pragma once
#include "tba_common.h"
#include "k_cabi.h"
#include "k_scan.h"

struct SiteArgs {
    i64 n_tracks;
    const i64 *trk_start, *pos_off;   // pos_off[n_tracks + 1]
    int valid_mode;                   // 0: stat <= lower || stat >= single; 1: |stat| >= single; 2: all
    double single, lower;
    i32 *cnt;                         // 3 counters per position: cov, valid, ge
};

// NaN statistics are dropped before anything else (collate_reg_stats :4130-4132)
__device__ __forceinline__ void site_accumulate(const SiteArgs &a, i64 t, i64 g, double stat)
{
    if (stat != stat) return;
    i32 *c = a.cnt + 3 * (a.pos_off[t] + (g - a.trk_start[t]));
    const bool ge = stat >= a.single;
    const bool valid = a.valid_mode == 0 ? (stat <= a.lower || ge)
                     : a.valid_mode == 1 ? fabs(stat) >= a.single : true;
    atomicAdd(c, 1);
    if (valid) atomicAdd(c + 1, 1);
    if (valid && ge) atomicAdd(c + 2, 1);
}

// z form (de_novo, sample_compare): the arrays of k_read_pvals plus, per read, its track and the
// genomic position of its first value.  per_read (may be NULL): the statistics in the input layout.
// This fused kernel serves fm_offset == 0 (the z-test alone: dev_read_pval with a constant window of
// 0, so its Fisher branch and the out-of-line call in it are not compiled in).
__global__ void k_site_z(SiteArgs a, const double *means, const double *ref_means,
    const double *ref_sds, const i64 *off, i64 n_reads, i64 total, const i64 *read_track,
    const i64 *read_pos, int floor_out, double smallest, double *per_read)
{
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (i64)gridDim.x * blockDim.x) {
        const i64 r = dev_csr_row(off, n_reads, i);
        const i64 b0 = off[r];
        const double stat = dev_read_pval(means, ref_means, ref_sds, b0, off[r + 1], i, 0, floor_out, smallest);
        if (per_read) per_read[i] = stat;
        site_accumulate(a, read_track[r], read_pos[r] + (i - b0), stat);
    }
}

// fm_offset > 0: Fisher's method sums its window through np_pw_leaf (tba_common.h), an out-of-line
// call whose eight-way unrolled leaf spills (k_read_pvals: 604 bytes of scratch per lane).  Rather
// than carry that into a kernel of this file, the host runs k_read_pvals itself into a device
// buffer and this kernel scatters from it: 16 bytes more traffic per statistic, on the device only.
__global__ void k_site_stat(SiteArgs a, const double *stats, const i64 *off, i64 n_reads, i64 total,
    const i64 *read_track, const i64 *read_pos)
{
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (i64)gridDim.x * blockDim.x) {
        const i64 r = dev_csr_row(off, n_reads, i);
        site_accumulate(a, read_track[r], read_pos[r] + (i - off[r]), stats[i]);
    }
}

// stored-record form (aggregate_per_read_stats, tombo_stats.py:4699-4725): recs are the blocks'
// records in the layout they are stored in, numpy's packed [('pos','u4'),('stat','f8'),
// ('read_id','u4')]: 16 bytes, the float64 at byte offset 4, so a record is read as one uint4 and
// the double rebuilt from its two dwords (x: pos, y / z: low / high half of stat, w: read id, not
// used: the compiler narrows the load to three dwords).  Track t (a block) owns records rec_off[t] .. rec_off[t + 1].  The position comes from
// the file, not from the host's own bookkeeping, so it is tested against [trk_start, trk_end) of
// its block BEFORE any counter address is formed: a record outside counts into n_bad and touches
// nothing else (the entry then fails the call).
__global__ void k_site_rec(SiteArgs a, const uint4 *recs, const i64 *rec_off, i64 n_recs,
    const i64 *trk_end, i32 *n_bad)
{
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_recs; i += (i64)gridDim.x * blockDim.x) {
        const uint4 q = recs[i];
        const i64 t = dev_csr_row(rec_off, a.n_tracks, i);
        const i64 g = q.x;
        if (g < a.trk_start[t] || g >= trk_end[t]) { atomicAdd(n_bad, 1); continue; }
        site_accumulate(a, t, g, __hiloint2double((int)q.z, (int)q.y));
    }
}

// window form (model_compare): the arrays of k_c_llh_windows plus, per window, its track and
// genomic position
__global__ void k_site_win(SiteArgs a, int kind, const double *means, const double *ref_means,
    const double *alt_means, const double *ref_vars, const double *alt_vars, i64 width,
    const i64 *starts, i64 n_windows, double par0, double par1, double par2, const i64 *win_track,
    const i64 *win_pos, double *per_read)
{
    for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < n_windows; w += (i64)gridDim.x * blockDim.x) {
        const double stat = dev_llh_window(kind, means, ref_means, alt_means, ref_vars, alt_vars, width,
                                           starts[w], par0, par1, par2);
        if (per_read) per_read[w] = stat;
        site_accumulate(a, win_track[w], win_pos[w], stat);
    }
}

// One wavefront (block of 64) per track.  Kept positions (cov > 0) of track t are written from
// pos_off[t] on, in ascending order; out_counts[t] of them, out_n_stats[t] = sum of their cov.
// frac = ge / valid (NaN without valid coverage); damp (may be NULL) =
// (rint(frac * valid) + unmod) / (valid + damp_sum), calc_damp_fraction with np.round's
// round-half-even.
__global__ void k_site_finish(SiteArgs a, double unmod, double damp_sum, double *out_frac,
    i64 *out_pos, i64 *out_cov, i64 *out_valid, double *out_damp, i64 *out_counts, i64 *out_n_stats)
{
    const i64 t = blockIdx.x;
    const int lane = threadIdx.x;
    const i64 p0 = a.pos_off[t], L = a.pos_off[t + 1] - p0;
    i64 k_carry = 0, n_carry = 0;
    for (i64 c = 0; c < L; c += 64) {
        const i64 i = c + lane;
        i32 cov = 0, valid = 0, ge = 0;
        if (i < L) { const i32 *q = a.cnt + 3 * (p0 + i); cov = q[0]; valid = q[1]; ge = q[2]; }
        const i64 inc = wave_scan_add(cov > 0 ? 1 : 0);
        const i64 n_inc = wave_scan_add(cov);
        if (cov > 0) {
            const i64 o = p0 + k_carry + inc - 1;
            const double frac = valid > 0 ? (double)ge / (double)valid : NAN;
            out_frac[o] = frac;
            out_pos[o] = a.trk_start[t] + i;
            out_cov[o] = cov;
            out_valid[o] = valid;
            if (out_damp) out_damp[o] = (rint(frac * (double)valid) + unmod) / ((double)valid + damp_sum);
        }
        k_carry += __shfl(inc, 63);
        n_carry += __shfl(n_inc, 63);
    }
    if (lane == 0) { out_counts[t] = k_carry; out_n_stats[t] = n_carry; }
}

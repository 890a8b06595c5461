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
//   k_site_pair_plan /      the z form's inputs made on the device from a reads table (every read uploaded
//   k_site_gather           once) and (region, read) pairs: the region clip, the failure scans and the count
//                           of each pair, then one thread per statistic fills means / ref_means / ref_sds in
//                           the layout k_site_z and k_read_pvals take
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

// ---- the z form's inputs from a reads table (tba_site_fractions_reads) -----------------------------
// Every read is on the device once (read-centric levels and, form 0, base codes, CSR by read_off); a
// pair is one (region, read): pair p tests read pair_read[p] in region pair_reg[p].  What a pair
// contributes is the reference's per-read preparation (compute_de_novo_read_stats :3796-3855,
// compute_sample_compare_read_stats :3700-3750) as index arithmetic.  Read [s, e), region [a, b),
// fm = fm_offset, K / cp of the model, dn = K - cp - 1:
//   form 0 (de_novo)         (lag_b, lag_e) = (cp, dn) on '+', (dn, cp) on '-';
//                            cs = max(s, a - lag_b - fm), ce = min(e, b + lag_e + fm); statistics at genomic
//                            g in [cs + lag_b, ce - lag_e); fails when ce - cs < K, when a base code of the
//                            clipped part is not 0..3, or (fm > 0) when fewer than 2 fm + 1 statistics
//   form 1 (sample_compare)  cs = max(s, a - fm), ce = min(e, b + fm); statistics at g in [cs, ce); fails when no g
//                            has level, control mean and control sd all non-NaN, or (fm > 0) when fewer than
//                            2 fm + 1 statistics
// At g the read index is i = g - s on '+' and e - 1 - g on '-'; the clipped part is read indices
// [cs - s, ce - s) on '+' and [e - ce, e - cs) on '-'.  The host has checked that every read overlaps
// its region, so cs < ce, and every index below stays inside the read and the region's extended positions.
struct SitePairArgs {
    int form, K, cp;
    i64 fm, n_pairs;
    const i64 *reg_start, *reg_end, *pos_off;            // per region; pos_off: its first extended position
    const i64 *pair_reg, *pair_read;                     // per pair
    const i64 *read_start, *read_off;                    // per read
    const int8_t *read_strand;
    const double *means;                                 // read-centric levels
    const uint8_t *seq;                                  // form 0: read-centric base codes
    const double *pos_means, *pos_sds;                   // form 1: control levels per extended position
    const double *kmeans, *ksds;                         // form 0: the model's level table
};

struct SitePairGeom { i64 s, e, cs, ce, first, count; bool minus; };

__device__ __forceinline__ SitePairGeom site_pair_geom(const SitePairArgs &a, i64 p)
{
    SitePairGeom q;
    const i64 rd = a.pair_read[p], r = a.pair_reg[p];
    q.s = a.read_start[rd];
    q.e = q.s + (a.read_off[rd + 1] - a.read_off[rd]);
    q.minus = a.read_strand[rd] != 0;
    const i64 dn = a.K - a.cp - 1;
    const i64 lag_b = a.form != 0 ? 0 : q.minus ? dn : a.cp;
    const i64 lag_e = a.form != 0 ? 0 : q.minus ? a.cp : dn;
    const i64 lo = a.reg_start[r] - lag_b - a.fm, hi = a.reg_end[r] + lag_e + a.fm;
    q.cs = q.s > lo ? q.s : lo;
    q.ce = q.e < hi ? q.e : hi;
    q.first = q.cs + lag_b;
    q.count = (q.ce - lag_e) - q.first;
    return q;
}

// One wavefront per pair (blocks of 256: four pairs a block, the rest by the stride loop).  pair_ok: the
// pair did not fail; pair_pos: the genomic position of its first statistic; pair_cnt: its statistics (0
// when it failed).
__global__ void __launch_bounds__(256) k_site_pair_plan(SitePairArgs a, i32 *pair_ok, i64 *pair_pos, i64 *pair_cnt)
{
    const int lane = threadIdx.x & 63;
    const i64 wave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 p = wave; p < a.n_pairs; p += n_waves) {
        const SitePairGeom q = site_pair_geom(a, p);
        const i64 rd = a.pair_read[p], base = a.read_off[rd];
        bool ok = a.form != 0 || q.ce - q.cs >= a.K;
        if (a.fm > 0 && q.count < 2 * a.fm + 1) ok = false;
        if (ok && a.form == 0) {   // any base of the clipped part outside ACGT
            const i64 i0 = q.minus ? q.e - q.ce : q.cs - q.s, n = q.ce - q.cs;
            bool bad = false;
            for (i64 k = lane; k < n; k += 64) bad = bad || a.seq[base + i0 + k] > 3;
            ok = !__any(bad);
        } else if (ok) {           // any position with level, control mean and control sd
            const i64 r = a.pair_reg[p];
            const i64 c0 = a.pos_off[r] + (q.cs - (a.reg_start[r] - a.fm));
            bool have = false;
            for (i64 k = lane; k < q.count; k += 64) {
                const i64 g = q.cs + k;
                const double m = a.means[base + (q.minus ? q.e - 1 - g : g - q.s)], cm = a.pos_means[c0 + k], sd = a.pos_sds[c0 + k];
                have = have || (m == m && cm == cm && sd == sd);
            }
            ok = __any(have) != 0;
        }
        if (lane == 0) { pair_ok[p] = ok ? 1 : 0; pair_pos[p] = q.first; pair_cnt[p] = ok ? q.count : 0; }
    }
}

// One thread per statistic: j lies in pair p = the row of j in pair_off (the exclusive scan of pair_cnt),
// k = j - pair_off[p] positions behind the pair's first.  Writes the three arrays of k_read_pvals /
// k_site_z in their layout: off = pair_off, read_track = pair_reg, read_pos = pair_pos.
__global__ void k_site_gather(SitePairArgs a, const i64 *pair_off, const i64 *pair_pos, i64 total,
    double *out_means, double *out_ref_means, double *out_ref_sds)
{
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (i64)gridDim.x * blockDim.x) {
        const i64 p = dev_csr_row(pair_off, a.n_pairs, j);
        const i64 g = pair_pos[p] + (j - pair_off[p]);
        const i64 rd = a.pair_read[p], base = a.read_off[rd], s = a.read_start[rd];
        const i64 e = s + (a.read_off[rd + 1] - base);
        const i64 i = a.read_strand[rd] != 0 ? e - 1 - g : g - s;
        out_means[j] = a.means[base + i];
        if (a.form == 0) {
            const i64 km = window_kmer(a.seq + base + i - a.cp, a.K);   // (>= 0: the plan has scanned these bases)
            out_ref_means[j] = km >= 0 ? a.kmeans[km] : NAN;
            out_ref_sds[j] = km >= 0 ? a.ksds[km] : NAN;
        } else {
            const i64 r = a.pair_reg[p];
            const i64 c = a.pos_off[r] + (g - (a.reg_start[r] - a.fm));
            out_ref_means[j] = a.pos_means[c];
            out_ref_sds[j] = a.pos_sds[c];
        }
    }
}

"""TEST INFRASTRUCTURE: a stand-in for the statistics methods of tombo_amd._native.Engine in numpy /
scipy, so that the HOST layer of tombo_amd.tombo_stats (clips, flips, motif search, track building,
per-read blocks, per-region assembly) runs on a box without a GPU: pass an instance as `engine=`.
The arithmetic is that of tests/stats_reference.py and tests/site_stats_reference.py (both pinned to
the reference's recorded output); `group_level_stats` is not implemented."""
import math

import numpy as np

from tombo_amd._native import SiteFractions
from tombo_amd._default_parameters import SMALLEST_PVAL
import stats_reference as sr
import site_stats_reference as ssr


class _Read(object):
    def __init__(self, start, strand, means):
        self.start, self.end, self.strand, self.means = start, start + means.shape[0], strand, means


def _llh_window(kind, m, r, a, rv, av, par):
    """c_calc_llh_ratio / _const_var / c_calc_scaled_llh_ratio_const_var (_c_helper.pyx:277-358) on
    one window, terms added in index order"""
    if kind == 0:
        ref_z = ref_lv = alt_z = alt_lv = 0.0
        for i in range(len(m)):
            ref_z += ((m[i] - r[i]) * (m[i] - r[i])) / rv[i]
            ref_lv += math.log(rv[i])
            alt_z += ((m[i] - a[i]) * (m[i] - a[i])) / av[i]
            alt_lv += math.log(av[i])
        return alt_z + alt_lv - ref_z - ref_lv
    run = 0.0
    for i in range(len(m)):
        rd, ad = m[i] - r[i], m[i] - a[i]
        if kind == 1:
            run += ((ad * ad) - (rd * rd)) / rv[0]
        elif r[i] != a[i]:
            sd = m[i] - (a[i] + r[i]) / 2
            run += math.exp(-(sd * sd) / (par[0] * rv[0])) * ((ad * ad) - (rd * rd)) / (
                rv[0] * math.pow(abs(a[i] - r[i]), par[2]) * par[1])
    return run


class NumpyStatsEngine(object):
    def read_pvals(self, means, ref_means, ref_sds, off, fm_offset, floor_out, smallest_pval):
        assert smallest_pval == SMALLEST_PVAL
        m, r, s = (np.asarray(x, dtype=np.float64) for x in (means, ref_means, ref_sds))
        out = np.empty(m.shape[0])
        with np.errstate(invalid='ignore', divide='ignore'):
            for a, b in zip(off[:-1], off[1:]):
                if floor_out:
                    out[a:b] = sr.de_novo_pvals(m[a:b], r[a:b], s[a:b], fm_offset)
                else:
                    p = sr.z_pvals(m[a:b], r[a:b], s[a:b])
                    out[a:b] = sr.calc_window_fishers_method(p, fm_offset) if fm_offset > 0 else p
        return out

    def llh_ratio_windows(self, kind, means, ref_means, alt_means, ref_vars, starts, width, alt_vars, par):
        cols = [None if x is None else np.asarray(x, dtype=np.float64).tolist()
                for x in (means, ref_means, alt_means, ref_vars, alt_vars)]
        return np.array([_llh_window(kind, *(None if c is None else c[s:s + width] for c in cols), par)
                         for s in np.asarray(starts).tolist()], dtype=np.float64)

    def reads_ref_levels(self, est_mean, fm_offset, min_test_reads, pileup, prior_means, prior_sds, w_mean, w_sd):
        pl = pileup
        lm, ls = np.empty(int(pl.pos_off[-1])), np.empty(int(pl.pos_off[-1]))
        cov = np.empty(int(pl.pos_off[-1]), dtype=np.int64)
        for r in range(pl.reg_start.shape[0]):
            reads = [_Read(int(pl.read_start[q]), '+-'[pl.read_strand[q]], pl.means[pl.read_off[q]:pl.read_off[q + 1]])
                     for q in range(pl.reg_read_off[r], pl.reg_read_off[r + 1])]
            start, end, strand = int(pl.reg_start[r]), int(pl.reg_end[r]), ('+', '-', None)[pl.reg_strand[r]]
            a, b = int(pl.pos_off[r]), int(pl.pos_off[r + 1])
            pm, ps = (None, None) if prior_means is None else (prior_means[a:b], prior_sds[a:b])
            with np.errstate(invalid='ignore'):
                lm[a:b], ls[a:b], _ = sr.get_reads_ref(reads, start, end, strand, min_test_reads, fm_offset,
                                                       pm, ps, (w_mean, w_sd), bool(est_mean))
            cov[a:b] = (~np.isnan(sr.base_levels(reads, start - fm_offset, end + fm_offset, strand))).sum(axis=1)
        return lm, ls, cov

    @staticmethod
    def _collate(trk_start, trk_end, stats, stat_track, stat_pos, is_alt, single_read_thresh, lower_thresh,
                 damp_counts, return_per_read):
        """collate_reg_stats / apply_per_read_thresh per track, laid out like the engine's outputs"""
        trk_start, trk_end = np.asarray(trk_start, dtype=np.int64), np.asarray(trk_end, dtype=np.int64)
        pos_off = np.concatenate([[0], np.cumsum(trk_end - trk_start)]).astype(np.int64)
        n_trk, n_pos = trk_start.shape[0], int(pos_off[-1])
        frac, damp = np.full(n_pos, np.nan), None if damp_counts is None else np.full(n_pos, np.nan)
        poss, cov, valid = (np.zeros(n_pos, dtype=np.int64) for _ in range(3))
        counts, n_stats = np.zeros(n_trk, dtype=np.int64), np.zeros(n_trk, dtype=np.int64)
        for t in range(n_trk):
            sel = stat_track == t
            assert np.all((stat_pos[sel] >= trk_start[t]) & (stat_pos[sel] < trk_end[t]))
            res = ssr.collate(stats[sel], stat_pos[sel], single_read_thresh, lower_thresh, is_alt)
            if res is None:
                continue
            a, b = int(pos_off[t]), int(pos_off[t]) + res[1].shape[0]
            frac[a:b], poss[a:b], cov[a:b], valid[a:b] = res[0], res[1], res[2], res[4]
            counts[t], n_stats[t] = res[1].shape[0], res[2].sum()
            if damp is not None:
                with np.errstate(invalid='ignore'):
                    damp[a:b] = ssr.damp_fraction({'unmod': damp_counts[0], 'mod': damp_counts[1]}, res[0], res[4])
        return SiteFractions(pos_off, frac, poss, cov, valid, damp, counts, n_stats,
                             stats if return_per_read else None)

    def site_fractions_z(self, trk_start, trk_end, means, ref_means, ref_sds, off, read_track, read_pos,
                         fm_offset, floor_out, smallest_pval, single_read_thresh, lower_thresh=None,
                         damp_counts=None, return_per_read=False):
        stats = self.read_pvals(means, ref_means, ref_sds, off, fm_offset, floor_out, smallest_pval)
        lens = np.diff(off)
        return self._collate(trk_start, trk_end, stats, np.repeat(read_track, lens),
                             np.repeat(read_pos - off[:-1], lens) + np.arange(stats.shape[0]), False,
                             single_read_thresh, lower_thresh, damp_counts, return_per_read)

    def site_fractions_windows(self, trk_start, trk_end, kind, means, ref_means, alt_means, ref_vars, alt_vars,
                               starts, width, win_track, win_pos, par, single_read_thresh, lower_thresh=None,
                               damp_counts=None, return_per_read=False):
        stats = self.llh_ratio_windows(kind, means, ref_means, alt_means, ref_vars, starts, width, alt_vars, par)
        return self._collate(trk_start, trk_end, stats, np.asarray(win_track), np.asarray(win_pos), True,
                             single_read_thresh, lower_thresh, damp_counts, return_per_read)

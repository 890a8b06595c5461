"""TEST INFRASTRUCTURE: the numpy stand-in engine of tests/stats_stub_engine.py with `site_fractions_reads`, a
restatement of the pair geometry of tba_site_fractions_reads (include/tombo_amd.h) pair by pair, feeding the
stand-in's `site_fractions_z`; with the genome tracks `th.iter_cov_regs` needs and a `group_level_stats` from
tests/stats_reference.py, so that `tombo_stats.test_significance` runs on a box without a GPU."""
import numpy as np

from tombo_amd import _native
import stats_reference as sr
from stats_stub_engine import NumpyStatsEngine, _Read
from tracks_stub_engine import NumpyTracksEngine


def pair_geometry(form, K, cp, fm, s, e, minus, a, b):
    """-> (cs, ce, first statistic, number of statistics) of read [s, e) in region [a, b)"""
    dn = K - cp - 1
    lag_b, lag_e = (0, 0) if form == 1 else ((dn, cp) if minus else (cp, dn))
    cs, ce = max(s, a - lag_b - fm), min(e, b + lag_e + fm)
    return cs, ce, cs + lag_b, (ce - lag_e) - (cs + lag_b)


class SiteReadsStubEngine(NumpyStatsEngine, NumpyTracksEngine):
    def __init__(self):
        NumpyTracksEngine.__init__(self)
        self.model = None
        self.kmer_width = self.central_pos = None
        self.reads_calls = []      # the SiteReads of every site_fractions_reads call

    def ensure_model(self, std_ref):
        self.model = (np.asarray(std_ref.level_means, dtype=np.float64), np.asarray(std_ref.level_sds, dtype=np.float64))
        self.kmer_width, self.central_pos = int(std_ref.kmer_width), int(std_ref.central_pos)

    def site_fractions_reads(self, form, reg_start, reg_end, read_start, read_strand, read_off, means, seq,
                             reg_pair_off, pair_read, pos_means, pos_sds, fm_offset, smallest_pval,
                             single_read_thresh, lower_thresh=None, damp_counts=None, return_per_read=False):
        t = _native._check_site_reads_args(form, reg_start, reg_end, read_start, read_strand, read_off, means, seq,
                                           reg_pair_off, pair_read, pos_means, pos_sds, fm_offset)
        if form == 0 and self.model is None:
            raise ValueError('form 0 (de_novo) needs a model (set_model)')
        self.reads_calls.append(t)
        K, cp = (self.kmer_width, self.central_pos) if form == 0 else (1, 0)
        fm, n_pairs = t.fm_offset, t.pair_read.shape[0]
        ok, pos, cnt = np.zeros(n_pairs, np.int32), np.zeros(n_pairs, np.int64), np.zeros(n_pairs, np.int64)
        cols = ([], [], [])
        for r in range(t.reg_start.shape[0]):
            a, b = int(t.reg_start[r]), int(t.reg_end[r])
            for p in range(int(t.reg_pair_off[r]), int(t.reg_pair_off[r + 1])):
                q = int(t.pair_read[p])
                o0, o1 = int(t.read_off[q]), int(t.read_off[q + 1])
                s, minus = int(t.read_start[q]), bool(t.read_strand[q])
                e = s + o1 - o0
                cs, ce, first, n = pair_geometry(form, K, cp, fm, s, e, minus, a, b)
                pos[p] = first
                g = np.arange(first, first + max(n, 0))
                i = (e - 1 - g) if minus else (g - s)
                m = t.means[o0:o1][i]
                if form == 0:
                    part = t.seq[o0:o1][(e - ce) if minus else (cs - s):(e - cs) if minus else (ce - s)]
                    if ce - cs < K or (part > 3).any():
                        continue
                    km = np.zeros(n, dtype=np.int64)
                    for j in range(K):
                        km = km * 4 + t.seq[o0:o1][i - cp + j]
                    rm, rs = self.model[0][km], self.model[1][km]
                else:
                    c0 = int(t.pos_off[r]) + first - (a - fm)
                    rm, rs = t.pos_means[c0:c0 + n], t.pos_sds[c0:c0 + n]
                    if not (~(np.isnan(m) | np.isnan(rm) | np.isnan(rs))).any():
                        continue
                if fm > 0 and n < 2 * fm + 1:
                    continue
                ok[p], cnt[p] = 1, n
                for c, x in zip(cols, (m, rm, rs)):
                    c.append(x)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        cat = [np.concatenate(c) if c else np.zeros(0) for c in cols]
        keep = np.flatnonzero(ok)      # (the stand-in's read_pvals takes no empty read: the failed pairs hold none)
        pair_reg = np.repeat(np.arange(t.reg_start.shape[0]), np.diff(t.reg_pair_off))
        res = self.site_fractions_z(t.reg_start - fm, t.reg_end + fm, *cat,
                                    np.concatenate([[0], np.cumsum(cnt[keep])]).astype(np.int64), pair_reg[keep],
                                    pos[keep], fm, form == 0, smallest_pval, single_read_thresh, lower_thresh,
                                    damp_counts, return_per_read)
        return res, ok, pos, off

    def group_level_stats(self, kind, return_p, fm_offset, min_test_reads, pileup, smallest_pval):
        pl = pileup
        stat_type = ('ks', 'u', 't')[kind] + ('_test' if return_p else '_stat_test')
        n_pos = int(pl.pos_off[-1])
        stats, poss = np.full(n_pos, np.nan), np.zeros(n_pos, dtype=np.int64)
        cov, ccov = np.zeros(n_pos, dtype=np.int64), np.zeros(n_pos, dtype=np.int64)
        counts = np.zeros(pl.reg_start.shape[0], dtype=np.int64)
        for r in range(pl.reg_start.shape[0]):
            groups = ([], [])
            for q in range(pl.reg_read_off[r], pl.reg_read_off[r + 1]):
                groups[pl.read_ctrl[q]].append(_Read(int(pl.read_start[q]), '+-'[pl.read_strand[q]],
                                                     pl.means[pl.read_off[q]:pl.read_off[q + 1]]))
            with np.errstate(all='ignore'):
                res = sr.compute_group_reg_stats(groups[0], groups[1], int(pl.reg_start[r]), int(pl.reg_end[r]),
                                                 ('+', '-', None)[pl.reg_strand[r]], fm_offset, min_test_reads, stat_type)
            if res is not None:
                a, n = int(pl.pos_off[r]), res[0].shape[0]
                stats[a:a + n], poss[a:a + n], cov[a:a + n], ccov[a:a + n] = res
                counts[r] = n
        return stats, poss, cov, ccov, counts

"""TEST INFRASTRUCTURE: the statistics stand-in engine of tests/stats_stub_engine.py plus numpy forms of
`Engine.kmer_levels` and `Engine.kde_eval`, so that the host layer of the alternate-model estimation
(tombo_amd.tombo_stats.parse_base_levels ... estimate_alt_model) runs on a box without a GPU.  The
argument checks are the binding's own (tombo_amd._native._check_*), the arithmetic is the definition in
include/tombo_amd.h written out in numpy."""
import numpy as np

from tombo_amd import _native
from stats_stub_engine import NumpyStatsEngine


def kmer_levels(means, codes, read_off, kmer_width, central_pos, completed):
    K, cp = int(kmer_width), int(central_pos)
    per_kmer = [[] for _ in range(4 ** K)]
    for a, b in zip(read_off[:-1].tolist(), read_off[1:].tolist()):
        for i in range(b - a - K + 1):
            win = codes[a + i:a + i + K]
            if (win > 3).any():
                continue
            k = 0
            for c in win.tolist():
                k = k * 4 + c
            if not completed[k]:
                per_kmer[k].append(means[a + cp + i])
    counts = np.array([len(v) for v in per_kmer], dtype=np.int64)
    lv_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    levels = np.array([x for v in per_kmer for x in v], dtype=np.float64)
    return counts, levels, lv_off


def kde_eval(levels, lv_off, x, bandwidth):
    """sum_i exp(-0.5 ((x - l_i) / h)^2) / (n h sqrt(2 pi)) per segment, over the sorted levels"""
    out = np.full((lv_off.shape[0] - 1, x.shape[0]), np.nan)
    for s, (a, b) in enumerate(zip(lv_off[:-1].tolist(), lv_off[1:].tolist())):
        lv = np.sort(levels[a:b])
        if b - a < 2 or np.isnan(lv).any():
            continue
        acc = np.zeros(x.shape[0])
        with np.errstate(under='ignore', over='ignore', invalid='ignore'):
            for c in range(0, b - a, 2048):
                t = (x[:, None] - lv[None, c:c + 2048]) / bandwidth
                acc += np.exp(-0.5 * (t * t)).sum(axis=1)
        out[s] = acc / ((b - a) * bandwidth * 2.50662827463100050242)
    return out


class AltEstStubEngine(NumpyStatsEngine):
    def __init__(self):
        self.calls = []   # (method name, number of reads or segments) of every call, for the tests

    def kmer_levels(self, means, codes, read_off, kmer_width, central_pos, completed):
        m, c, off, done = _native._check_kmer_levels_args(means, codes, read_off, kmer_width, central_pos, completed)
        self.calls.append(('kmer_levels', off.shape[0] - 1))
        return kmer_levels(m, c, off, kmer_width, central_pos, done)

    def kde_eval(self, levels, lv_off, x, bandwidth):
        lv, off, x = _native._check_kde_eval_args(levels, lv_off, x, bandwidth)
        self.calls.append(('kde_eval', off.shape[0] - 1))
        return kde_eval(lv, off, x, bandwidth)

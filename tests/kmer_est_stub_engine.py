"""TEST INFRASTRUCTURE: numpy forms of `Engine.region_key_levels` and `Engine.segment_medians` on top of the
genome-track stand-in (iter_cov_regs needs the coverage calls), so that the host layer of the k-mer model
estimation runs on a box without a GPU.  The argument checks are the binding's own (tombo_amd._native._check_*),
the arithmetic is the definition in include/tombo_amd.h written out with kmer_est_reference.pair."""
import numpy as np

from tombo_amd import _native
from tracks_stub_engine import NumpyTracksEngine
import kmer_est_reference as kr


def region_key_levels(est_mean, rs, rm, off, m, roff, rr, pr, pg, ep, ek, n_keys):
    pairs = []
    for r, g in zip(pr.tolist(), pg.tolist()):
        vals = []
        for q in rr[roff[r]:roff[r + 1]].tolist():
            n = int(off[q + 1] - off[q])
            if rs[q] <= g < rs[q] + n:
                vals.append(m[off[q] + (n - 1 - (g - rs[q]) if rm[q] else g - rs[q])])
        pairs.append(kr.pair(vals, est_mean) if vals else (np.nan, np.nan))
    order = np.argsort(ek, kind='stable')
    counts = np.bincount(ek, minlength=n_keys).astype(np.int64)
    koff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    lv = np.array([pairs[p][0] for p in ep[order].tolist()], dtype=np.float64)
    sd = np.array([pairs[p][1] for p in ep[order].tolist()], dtype=np.float64)
    return counts, koff, lv, sd


def theil_sen_factors(base_means, ref_means):
    """calc_kmer_fitted_shift_scale(method='theil_sen') after the draw, with c_compute_slopes: the median of the
    slopes of all pairs (1000 where the two base means are equal), the median intercept -> (-inter / slope,
    1 / slope), or None where the slope is 0"""
    i, j = np.triu_indices(base_means.shape[0], 1)
    de, dm = base_means[i] - base_means[j], ref_means[i] - ref_means[j]
    with np.errstate(all='ignore'):
        slope = np.median(np.where(de == 0, 1000.0, dm / np.where(de == 0, 1.0, de)))
        inter = np.median(ref_means - (slope * base_means))
    return None if slope == 0 else (-inter / slope, 1 / slope)


class PipelineSlices(object):
    """the slices of the resident pipeline center_model_to_median_norm drives (ensure_model, upload, put,
    run_stages, get of a batch of one), in numpy"""

    def ensure_model(self, ref):
        self.model = (np.array(ref.level_means), int(ref.kmer_width))

    def set_num_events(self, num_events):
        pass

    def upload(self, params, opts, raws, seqs, samp_ind=None, **kw):
        self.raw, self.codes, self.samp, self.status, self.put_data = np.asarray(raws[0], dtype=np.float64), seqs[0], samp_ind, 0, {}

    def put(self, what, data, per_read=None):
        self.put_data[what] = (np.array(data), per_read)

    def run_stages(self, first, last):
        if first == _native.STAGE_SEGMENT:
            shift = np.median(self.raw)
            self.norm = (self.raw - shift) / np.median(np.abs(self.raw - shift))
        if first <= _native.STAGE_REF_LEVELS <= last:
            means, K = self.model
            idx = np.zeros(self.codes.shape[0] - K + 1, dtype=np.int64)
            for j in range(K):
                idx = idx * 4 + self.codes[j:j + idx.shape[0]]
            self.ref_means = means[idx]
        if last == _native.STAGE_RESCALE:
            norm = self.put_data[_native.PUT_NORM][0]
            segs, (read_start, _) = self.put_data[_native.PUT_DP_SEGS]
            x = norm[read_start:]
            bm = []
            for a, b in zip(segs[:-1].tolist(), segs[1:].tolist()):    # c_new_means: sequential sum, one divide
                acc = 0.0
                for v in x[a:b].tolist():
                    acc += v
                bm.append(acc / (b - a))
            bm, ref = np.array(bm), self.ref_means
            if self.samp is not None:
                bm, ref = bm[self.samp[0]], ref[self.samp[0]]
            self.fit = theil_sen_factors(bm, ref)
            self.status = 19 if self.fit is None else 0

    def get(self, what):
        if what == _native.GET_STATUS:
            return np.array([self.status], dtype=np.int32)
        if what == _native.GET_SEG_NORM:
            return self.norm
        assert what == _native.GET_THEIL_SEN
        return np.array([[np.nan, np.nan, self.fit[0], self.fit[1]]])


class KmerEstStubEngine(NumpyTracksEngine, PipelineSlices):
    def __init__(self):
        NumpyTracksEngine.__init__(self)
        self.calls = []   # (method name, regions or segments, entries or values) of every call, for the tests

    def region_key_levels(self, est_mean, read_start, read_minus, read_off, means, reg_read_off, reg_reads, pos_reg,
                          pos_g, ent_pos, ent_key, n_keys):
        args = _native._check_region_key_levels_args(read_start, read_minus, read_off, means, reg_read_off, reg_reads,
                                                     pos_reg, pos_g, ent_pos, ent_key, n_keys)
        self.calls.append(('region_key_levels', args[4].shape[0] - 1, args[8].shape[0]))
        return region_key_levels(est_mean, *args, n_keys=int(n_keys))

    def segment_medians(self, values, off):
        v, off = _native._check_segment_medians_args(values, off)
        self.calls.append(('segment_medians', off.shape[0] - 1, v.shape[0]))
        return kr.medians(v, off)

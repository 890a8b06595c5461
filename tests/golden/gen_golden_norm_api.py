"""Golden vectors of the documented per-read functions of tombo_stats from the REFERENCE (build container only).

    python tests/golden/gen_golden_norm_api.py   # writes tests/golden/stats_norm_api.npz

(The `stats_` prefix keeps the npz out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference (tools/ref_oracle.py) on the cases of tests/norm_api_cases.py:
  ts.normalize_raw_signal            every case of norm_cases(), and 'pA' over the points of points()
  ts.calc_kmer_fitted_shift_scale    'mom' at POINT_SIZES, 'theil_sen' at THEIL_SIZES (np.random.seed before) and on a
                                     zero slope
  ts.get_read_seg_score              at POINT_SIZES
The inputs are made from seeds by norm_api_cases.py; only their SHA-256 is stored.  Per normalisation case: the five
scale-value fields, the SHA-256 of the normalised signal's bytes, and the signal itself where it has at most 512
samples (all of them in one array, by offsets).  Only data is written."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_oracle  # noqa: E402
import norm_api_cases as nc  # noqa: E402

rq, ts, th = ref_oracle.load()


def digest(a):
    return np.frombuffer(bytes.fromhex(nc.sha(a)), dtype=np.uint8)


class NormRecords(object):
    """what normalize_raw_signal returned, case by case"""

    def __init__(self):
        self.sv, self.failed, self.lims_none, self.is_int, self.sha, self.full, self.full_off = [], [], [], [], [], [], [0]

    def add(self, run):
        try:
            norm, sv = run()
        except FloatingPointError:
            self.sv.append([np.nan] * 4)
            self.failed.append(1)
            self.lims_none.append(True)
            self.is_int.append(False)
            self.sha.append(np.zeros(32, np.uint8))
            self.full_off.append(self.full_off[-1])
            return None
        assert norm.dtype == np.float64 and norm.ndim == 1
        none = sv.lower_lim is None
        assert none == (sv.upper_lim is None)
        self.sv.append([float(sv.shift), float(sv.scale), np.nan if none else float(sv.lower_lim),
                        np.nan if none else float(sv.upper_lim)])
        self.failed.append(0)
        self.lims_none.append(none)
        self.is_int.append(isinstance(sv.shift, int) and isinstance(sv.scale, int))
        self.sha.append(digest(norm))
        if norm.shape[0] <= nc.MAX_FULL:
            self.full.append(norm)
        self.full_off.append(self.full_off[-1] + (norm.shape[0] if norm.shape[0] <= nc.MAX_FULL else 0))
        return sv

    def store(self, store, prefix):
        store[prefix + '/sv'] = np.array(self.sv, dtype=np.float64).reshape(-1, 4)
        store[prefix + '/failed'] = np.array(self.failed, dtype=np.uint8)
        store[prefix + '/lims_none'] = np.array(self.lims_none, dtype=np.bool_)
        store[prefix + '/is_int'] = np.array(self.is_int, dtype=np.bool_)
        store[prefix + '/sha'] = np.array(self.sha, dtype=np.uint8).reshape(-1, 32)
        store[prefix + '/full'] = np.concatenate(self.full) if self.full else np.zeros(0)
        store[prefix + '/full_off'] = np.array(self.full_off, dtype=np.int64)


def main():
    store, inputs = {}, {}
    channel = th.channelInfo(nc.CHANNEL[0], nc.CHANNEL[1], nc.CHANNEL[2], 7, 4000.0)
    cases = nc.norm_cases()
    rec = NormRecords()
    signals = {}
    for c in cases:
        key = (c.kind, c.dtype, c.n_sig, c.seed)
        if key not in signals:
            signals[key] = nc.case_signal(c)
            inputs['/'.join(map(str, key))] = nc.sha(signals[key])
        sig = signals[key]
        sv = None if c.sv is None else th.scaleValues(c.sv[0], c.sv[1], c.sv[2], c.sv[3], None)
        out = rec.add(lambda: ts.normalize_raw_signal(
            sig, c.start, c.n, c.norm_type, c.thresh, channel, sv, const_scale=c.const_scale))
        assert out is None or out.outlier_thresh == c.thresh
    rec.store(store, 'norm')
    print('%d normalisation cases, %d failed, %d stored whole' % (len(cases), sum(rec.failed), len(rec.full)))
    # the reference refuses an unknown type without scale values
    try:
        ts.normalize_raw_signal(np.arange(10.0), norm_type='no_such_type')
        raise AssertionError('accepted')
    except th.TomboError as e:
        invalid_type_msg = str(e)

    prev_shift, prev_scale = -1 * nc.CHANNEL[0], nc.CHANNEL[2] / nc.CHANNEL[1]
    mom_fit, mom_sums, scores = [], [], []
    for n in nc.POINT_SIZES:
        e, m, iv, sds = nc.points(n, 100 + n)
        inputs['points/%d' % n] = nc.sha(np.concatenate([e, m, iv, sds]))
        mom_fit.append(ts.calc_kmer_fitted_shift_scale(prev_shift, prev_scale, e, m, iv, method='mom'))
        mom_sums.append(nc.mom_sums(e, m, iv))      # numpy's own sums: what the recorder's solve was given
        scores.append(ts.get_read_seg_score(e, m, sds))
    store['mom/fit'], store['mom/sums'] = np.array(mom_fit, dtype=np.float64), np.array(mom_sums)
    store['seg_score'] = np.array(scores, dtype=np.float64)

    # 'pA': the moments fit inside normalize_raw_signal
    pa = NormRecords()
    for dtype in ('int16', 'float64'):
        for n_sig, n_pts in ((65, 129), (4096, 8193)):
            sig = nc.make_signal('noise', dtype, n_sig, 6000 + n_sig)
            inputs['pA/%s/%d' % (dtype, n_sig)] = nc.sha(sig)
            e, m, iv, _ = nc.points(n_pts, 100 + n_pts)
            for thresh in (None, 5.0):
                pa.add(lambda: ts.normalize_raw_signal(sig, 3, n_sig - 7, 'pA', thresh, channel, None, e, m, iv))
    pa.store(store, 'pA')

    theil = []
    for n in nc.THEIL_SIZES:
        e, m, _, _ = nc.points(n, 200 + n)
        np.random.seed(300 + n)
        theil.append(ts.calc_kmer_fitted_shift_scale(0.25, 1.5, e, m, method='theil_sen'))
    store['theil_sen/fit'] = np.array(theil, dtype=np.float64)
    e, m, _, _ = nc.points(50, 250)
    try:
        ts.calc_kmer_fitted_shift_scale(0.25, 1.5, e, np.full(50, 0.75), method='theil_sen')
        raise AssertionError('accepted')
    except th.TomboError as err:
        zero_slope_msg = str(err)

    store['meta'] = np.array(json.dumps(dict(
        numpy=np.__version__, n_norm_cases=len(cases), case_names_sha=nc.sha(np.array('\n'.join(c.name for c in cases))),
        inputs=inputs, invalid_type_msg=invalid_type_msg, zero_slope_msg=zero_slope_msg)))
    np.savez_compressed(nc.GOLDEN, **store)
    print('wrote %s (%d bytes)' % (nc.GOLDEN, os.path.getsize(nc.GOLDEN)))


if __name__ == '__main__':
    main()

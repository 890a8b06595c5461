"""TEST INFRASTRUCTURE: a stand-in for the genome-track methods of tombo_amd._native.Engine in numpy, so that the
HOST layer (tile lists, windows, slots, batches, writers, argument checks) runs on a box without a GPU: pass an
instance as `engine=`.  tracks_add does what the kernel does -- it walks every tile's read list in order and adds
only what that list names -- so a wrong tile list shows up here as it would on the device."""
import numpy as np

from tombo_amd import _native
from tombo_amd._native import TRK_TILE, TrackSet


class NumpyTracksEngine(object):
    def __init__(self):
        self._trk = None
        self.windows = []       # every (win_start, win_end, n_slots) opened

    def tracks_begin(self, win_start, win_end, n_slots):
        _native._check_tracks_begin_args(win_start, win_end, n_slots)
        W = int(win_end - win_start)
        self._trk = dict(start=int(win_start), W=W, ns=int(n_slots), sums=np.zeros((n_slots, W)),
                         cov=np.zeros((n_slots, W), dtype=np.int64), rcov=np.zeros(W, dtype=np.int64))
        self.windows.append((int(win_start), int(win_end), int(n_slots)))

    def tracks_add(self, read_start, read_end, read_flags, read_off, slots, tile_read_off, tile_reads):
        if self._trk is None:
            raise ValueError('no track set is open (tracks_begin)')
        t = self._trk
        rs, re_, fl, off, sl, toff, tr = _native._check_tracks_add_args(
            t['W'], t['ns'], read_start, read_end, read_flags, read_off, slots, tile_read_off, tile_reads)
        for tile in range(toff.shape[0] - 1):
            lo, hi = t['start'] + tile * TRK_TILE, t['start'] + min((tile + 1) * TRK_TILE, t['W'])
            for q in tr[toff[tile]:toff[tile + 1]]:
                a, b = max(lo, int(rs[q])), min(hi, int(re_[q]))
                if b > a:
                    t['rcov'][a - t['start']:b - t['start']] += 1
                n = int(off[q + 1] - off[q])
                a, b = max(lo, int(rs[q])), min(hi, int(rs[q]) + n)
                for s in range(t['ns']):
                    if b > a and (fl[q] >> (1 + s)) & 1:
                        v = sl[s][off[q]:off[q + 1]]
                        v = v[::-1] if fl[q] & 1 else v
                        t['sums'][s, a - t['start']:b - t['start']] += v[a - rs[q]:b - rs[q]]
                        t['cov'][s, a - t['start']:b - t['start']] += 1

    def tracks_finish(self, want_sums=False):
        t = self._trk
        with np.errstate(all='ignore'):
            means = t['sums'] / t['cov']
        return TrackSet(means, t['sums'].copy() if want_sums else None, t['cov'].copy(), t['rcov'].copy())

    def tracks_compact(self, values):
        v, mode = _native._check_compact_args(values)
        if mode == 0:
            keep = np.flatnonzero(~np.isnan(v))
            return keep, v[keep]
        starts = np.concatenate([[0], np.flatnonzero(np.diff(v)) + 1, [v.shape[0]]]).astype(np.int64)
        return starts, v[starts[:-1]]

    def tracks_diff(self, a, b):
        a, b = _native._check_track_pair(a, b)
        with np.errstate(all='ignore'):
            return np.nan_to_num(a - b)

    def tracks_topn(self, a, b, n_top):
        a, b = _native._check_track_pair(a, b)
        with np.errstate(all='ignore'):
            d = np.nan_to_num(np.abs(a - b))
        order = np.lexsort((np.arange(d.shape[0]), d))[::-1][:int(n_top)]
        return d[order], order.astype(np.int64)

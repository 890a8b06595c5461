"""TEST INFRASTRUCTURE: a stand-in for the read-filter methods of tombo_amd._native.Engine in numpy (on top of the
genome-track stand-in, which th.compute_coverage needs), so that the HOST layer of tombo_amd.filter_reads and
mapping.filter_and_index_records_batch runs on a box without a GPU: pass an instance as `engine=`.  The argument
checks are the real engine's."""
import numpy as np

from tombo_amd import _native
from tracks_stub_engine import NumpyTracksEngine
import filter_reference as fref


class NumpyFilterEngine(NumpyTracksEngine):
    def __init__(self):
        NumpyTracksEngine.__init__(self)
        self.calls = []         # (reads, boundaries) of every dwell_pctl_flags call
        self.resident = None    # (segs, seg_off, status) of the "resident batch"

    def dwell_pctl_flags(self, segs, seg_off, pairs):
        segs, off, _, _ = _native._check_dwell_pctl_args(segs, seg_off, pairs)
        self.calls.append((off.shape[0] - 1, segs.shape[0]))
        return fref.dwell_pctl_flags(segs, off, pairs)

    @property
    def n(self):
        return self.resident[2].shape[0]

    def batch_dwell_pctl_flags(self, pairs):
        _native._check_dwell_pairs(pairs)
        segs, off, status = self.resident
        vals, flags = fref.dwell_pctl_flags(segs, off, pairs)
        vals[status != 0], flags[status != 0] = np.nan, False
        return vals, flags

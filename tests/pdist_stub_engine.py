"""TEST INFRASTRUCTURE: the pairwise-distance methods of `_native.Engine` over the numpy restatement of
tests/pdist_reference.py, with the engine's own argument checks, on top of the numpy genome-track engine -- so that
the host layer (get_pairwise_dists, order_reads, cluster_most_signif_dists) runs on a box without a GPU: pass an
instance as `engine=`."""
import pdist_reference as ref
from tracks_stub_engine import NumpyTracksEngine
from tombo_amd import _native


class NumpyPdistEngine(NumpyTracksEngine):
    def __init__(self):
        NumpyTracksEngine.__init__(self)
        self.calls = []      # (entry, rows, row length) of every call
        self.last_pdist_kernel_ms = 0.0

    def pairwise_window_dists(self, rows, slide_span=0):
        rows = _native._check_pdist_rows(rows, slide_span)
        self.calls.append(('window', rows.shape[0], rows.shape[1]))
        return ref.window_dists(rows, int(slide_span))

    def pairwise_nanmean_dists(self, rows):
        rows = _native._check_pdist_rows(rows)
        self.calls.append(('nanmean', rows.shape[0], rows.shape[1]))
        return ref.nanmean_dists(rows)

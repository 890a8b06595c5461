"""TEST INFRASTRUCTURE: a numpy form of `Engine.kmer_dist`, so that the host layer of `tombo plot kmer`
(tombo_amd/plot_commands.py) runs on a box without a GPU.  The argument checks are the binding's own
(tombo_amd._native._check_kmer_dist_args), the arithmetic is tests/kmer_dist_reference.py, which
tests/test_kmer_dist_reference.py pins to the live reference's recorded frames."""
from tombo_amd import _native
import kmer_dist_reference as kr


class KmerDistStubEngine(object):
    def __init__(self):
        self.calls = []   # (n_reads, kmer_width) of every call, for the tests
        self.last_kmer_dist_kernel_ms = 0.0

    def kmer_dist(self, means, codes, read_off, kmer_width, central_pos, kmer_thresh, num_reads, read_mean):
        m, c, off = _native._check_kmer_dist_args(means, codes, read_off, kmer_width, central_pos, kmer_thresh, num_reads)
        self.calls.append((off.shape[0] - 1, int(kmer_width)))
        return kr.kmer_dist(m, c, off, int(kmer_width), int(central_pos), int(kmer_thresh), int(num_reads), bool(read_mean))

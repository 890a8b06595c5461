"""tba_kmer_dist (csrc/tba_engine.hip, k_kmer_dist.h) where its host code leaves the first launch regime: more reads
than one slice of k_kd_read_scan (blockIdx.y holds 65 535 reads; the slices get pointer offsets), and a 9-mer read
long enough that the chunk counters would pass KD_TABLE_MAX, so the chunk doubles (k_kd_kmer_means then also
strides: 4^9 k-mers are more than its 65 536 blocks).  Against tests/kmer_dist_reference.py, everything by bits."""
import numpy as np
import pytest

import kmer_dist_reference as kr
import launch_caps as lc
from test_gpu_kmer_dist import assert_same
from tombo_amd import resquiggle as rq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def many_short_reads():
    """65 535 + 65 535 + 7 reads of 1 - 4 bases; the reads on both sides of each slice end and the last read hold
    all four bases (kmer_thresh 1 takes them), most others do not"""
    n_reads = 2 * lc.KD_READ_SLICE + 7
    assert -(-n_reads // lc.KD_READ_SLICE) == 3 and n_reads % lc.KD_READ_SLICE == 7
    rng = np.random.default_rng(51)
    lens = rng.integers(1, 5, n_reads)
    planted = np.array([0, lc.KD_READ_SLICE - 1, lc.KD_READ_SLICE, 2 * lc.KD_READ_SLICE - 1, 2 * lc.KD_READ_SLICE,
                        n_reads - 1])
    lens[planted] = 4
    off = np.zeros(n_reads + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    codes = rng.integers(0, 4, int(off[-1])).astype(np.uint8)
    codes[rng.integers(0, codes.shape[0], 300)] = 4
    means = rng.standard_normal(codes.shape[0]) * 2 + 80
    for k, r in enumerate(planted.tolist()):
        codes[off[r]:off[r] + 4] = np.roll(np.arange(4), k)
        means[off[r]:off[r] + 4] = 1000.0 * (k + 1) + np.arange(4)
    return means, codes, off, planted


@pytest.mark.parametrize('read_mean', [True, False])
def test_k1_three_slices_of_reads(many_short_reads, read_mean):
    means, codes, off, planted = many_short_reads
    args = (means, codes, off, 1, 0, 1, 10 ** 6, read_mean)
    want = kr.kmer_dist(*args)
    label = want[0]
    assert (label[planted] > 0).all() and want[2] == off.shape[0] - 1
    for a in range(0, label.shape[0], lc.KD_READ_SLICE):       # taken and rejected reads in every slice
        part = label[a:a + lc.KD_READ_SLICE]
        assert (part > 0).any() and (part == 0).sum() > part.shape[0] // 2
    assert 1000 < want[1] < 10000
    assert_same(rq.get_engine().kmer_dist(*args), want)


def test_k9_long_read_doubles_the_chunk():
    K = 9
    lens = [40, lc.KD_CHUNK * (lc.KD_TABLE_MAX // 4 ** K - 2) + 1, 9]
    chunk, n_chunks = lc.kmer_dist_geometry(lens, K)
    assert lc.kmer_dist_geometry([v - (v > 100) for v in lens], K)[0] == lc.KD_CHUNK    # one base less: no doubling
    assert chunk == 2 * lc.KD_CHUNK and n_chunks == -(-lens[1] // chunk) + 2
    assert 4 ** K > lc.KD_MEANS_BLOCKS
    rng = np.random.default_rng(52)
    off = np.zeros(4, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    codes = rng.integers(0, 4, int(off[-1])).astype(np.uint8)
    codes[rng.integers(0, codes.shape[0], 50)] = 4
    means = rng.standard_normal(codes.shape[0]) * 2 + 80
    args = (means, codes, off, K, 4, 0, 3, True)
    want = kr.kmer_dist(*args)
    assert want[1] == 3 and np.count_nonzero(want[3]) > 4 ** K - 1000 and want[3].max() >= 2
    assert_same(rq.get_engine().kmer_dist(*args), want)

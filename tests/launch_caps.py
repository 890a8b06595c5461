"""TEST INFRASTRUCTURE: the fixed sizes at which the host code of the statistics entries (csrc/tba_engine.hip)
changes how it launches a kernel, in one place.  The tests that drive an entry across such a size take it from
here and assert with it that their input is in the regime they name; test_launch_caps.py reads the sources and
fails when one of these numbers is no longer the one the engine uses ("Launch caps")."""
import numpy as np

# grid_for(n): one thread per item, at most GRID_BLOCKS blocks of GRID_THREADS; the rest by the stride loop
GRID_BLOCKS, GRID_THREADS = 4096, 256
GRID_PASS = GRID_BLOCKS * GRID_THREADS
WAVE = 64

# k_kde_classify is launched as grid_for(64 * n_seg): one wavefront per segment up to this many segments
CLASSIFY_PASS = GRID_PASS // WAVE

# launch_sort_classes: (blocks, threads) of the wave sorter, the LDS sorter and the global sorter, and the sizes
# that put a segment in a class (n <= 64: one wavefront; n <= 4096: one workgroup in LDS; above: in global memory)
SORT_WAVE_GRID, SORT_LDS_GRID, SORT_GLOBAL_GRID = (1024, 256), (1024, 256), (256, 256)
SORT_WAVE_PASS = SORT_WAVE_GRID[0] * SORT_WAVE_GRID[1] // WAVE    # segments the wave sorter takes at once
SORT_LDS_PASS = SORT_LDS_GRID[0]
SORT_GLOBAL_PASS = SORT_GLOBAL_GRID[0]
SORT_WAVE_MAX, SORT_LDS_MAX = 64, 4096

# k_kde_eval: gridDim.x = min(n_seg, KDE_EVAL_BLOCKS); k_kd_read_scan: slices of KD_READ_SLICE reads;
# k_kd_seg_means / k_kd_kmer_means: at most KD_MEANS_BLOCKS blocks
KDE_EVAL_BLOCKS = 65535
KD_READ_SLICE = 65535
KD_MEANS_BLOCKS = 65536

# k_scan.h: items per block of the chunked scans
SCAN_CHUNK = 1024

# KeyPartition: chunks of PART_CHUNK items until there would be more than min(PART_MAX_CHUNKS, PART_MAX_COUNTERS /
# n_keys) of them
PART_CHUNK, PART_MAX_CHUNKS, PART_MAX_COUNTERS = 4096, 1024, 1 << 24

# tba_kmer_dist: 4^K * n_reads and the chunk counters stay within KD_TABLE_MAX; chunks of KD_CHUNK bases, doubled
KD_TABLE_MAX = 1 << 27
KD_CHUNK = 4096


def partition_geometry(n, n_keys):
    """KeyPartition's rule -> (chunk, n_chunks, key_bits) for n items under n_keys keys"""
    key_bits = 0
    while (1 << key_bits) < n_keys:
        key_bits += 1
    max_chunks = max(1, min(PART_MAX_CHUNKS, PART_MAX_COUNTERS // n_keys))
    chunk = max(PART_CHUNK, (-(-n // max_chunks) + 63) // 64 * 64)
    return chunk, -(-n // chunk), key_bits


def kmer_dist_geometry(read_lens, kmer_width):
    """tba_kmer_dist's rule -> (chunk, n_chunks): chunks never cross a read, the chunk doubles while the chunk
    counters (n_chunks * 4^K) exceed KD_TABLE_MAX and a read is longer than a chunk"""
    lens = [int(v) for v in read_lens]
    n_kmers = 4 ** int(kmer_width)
    count = lambda c: sum(-(-v // c) for v in lens)   # noqa: E731
    chunk = KD_CHUNK
    while chunk < max(lens) and count(chunk) > KD_TABLE_MAX // n_kmers:
        chunk *= 2
    return chunk, count(chunk)


def pass_sample(n, seed, n_random=2000, edge=64, pass_len=GRID_PASS):
    """the items a test with a per-item Python reference compares: the first and last `edge` items of every grid
    pass of `pass_len` over n items and n_random other items drawn from the whole range without replacement
    (at least 1000, at least 2000 items in all), ascending and unique"""
    picks = []
    for a in range(0, n, pass_len):
        b = min(a + pass_len, n)
        picks += [np.arange(a, min(a + edge, b)), np.arange(max(b - edge, a), b)]
    edges = np.unique(np.concatenate(picks))
    drawn = np.random.default_rng(seed).choice(n, n_random + edges.shape[0], replace=False)
    drawn = drawn[~np.isin(drawn, edges)][:n_random]
    sample = np.union1d(edges, drawn)
    assert drawn.shape[0] == n_random >= 1000 and sample.shape[0] == edges.shape[0] + n_random >= 2000
    return sample

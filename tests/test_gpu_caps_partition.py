"""KeyPartition (the host side of k_key_partition, k_kmer_colscan and k_exclusive_prefix; csrc/tba_engine.hip)
beyond its first regime: more than 12 key bits, chunks longer than 4096 items that are no multiple of 4096, a
partial last chunk, both sides of the switch between the two chunk rules, and 2^24 keys (k_kmer_colscan's second
grid pass).  The references are the numpy stubs (alt_est_stub_engine.kmer_levels, kmer_est_stub_engine.
region_key_levels); counts, offsets and the gathered values are compared bit for bit: the partition is stable, so
the order of a key's values is part of the answer.  Every test asserts from launch_caps.partition_geometry that its
input is in the regime it names."""
import numpy as np
import pytest

import alt_est_stub_engine as alt_stub
import kmer_est_stub_engine as est_stub
from kmer_est_cases import bits
from launch_caps import GRID_PASS, PART_CHUNK, partition_geometry
from test_gpu_kmer_est import random_call
from tombo_amd import tombo_stats as ts, resquiggle as rq

pytestmark = pytest.mark.gpu


def second_regime(n, n_keys):
    """the geometry of n items under n_keys keys, required to be past the 4096-item chunks with a partial last one"""
    chunk, n_chunks, key_bits = partition_geometry(n, n_keys)
    assert chunk > PART_CHUNK and chunk % PART_CHUNK != 0 and n % chunk != 0 and key_bits > 12
    return chunk, n_chunks, key_bits


def kmer_batch(seed, K, read_lens, plant_every):
    """reads of the given lengths with random ACGT codes, one code outside ACGT per ~1500 bases, a completed mask
    over a tenth of the k-mers, and a stretch of K + 3 A's from base 100 of every `plant_every` bases (the all-A
    k-mer, key 0, then has levels in every chunk of that length: every chunk prefix of its column is in use)"""
    rng = np.random.default_rng(seed)
    off = ts._csr_offsets(read_lens)
    total = int(off[-1])
    codes = rng.integers(0, 4, total).astype(np.uint8)
    planted = np.arange(100, total - K - 3, plant_every)
    for p in planted.tolist():
        r = int(np.searchsorted(off, p, side='right')) - 1
        assert p + K + 3 <= off[r + 1], 'a planted stretch crosses a read end'
        codes[p:p + K + 3] = 0
    bad = rng.integers(0, total, total // 1500)
    bad = bad[((bad[:, None] < planted[None, :]) | (bad[:, None] >= planted[None, :] + K + 3)).all(axis=1)]
    codes[bad] = rng.integers(4, 7, bad.shape[0])
    means = rng.normal(0, 1, total)
    means[rng.integers(0, total, 20)] = np.nan
    done = (rng.random(4 ** K) < 0.1).astype(np.uint8)
    done[0] = 0
    return means, codes, off, K, K // 2, done


@pytest.mark.parametrize('K,read_lens', [
    (10, [20000, 9, 15000, 3, 30825]),                  # 65 537 + 300 bases: 20 key bits, 16 chunks of 4160
    (9, [100000, 8, 62144, 90000, 10292])])             # 262 144 + 300 bases: 18 key bits, 64 chunks of 4160
def test_kmer_levels_long_kmers_leave_the_4096_chunks(K, read_lens):
    eng = rq.get_engine()
    total = sum(read_lens)
    chunk, n_chunks, key_bits = second_regime(total, 4 ** K)
    assert (chunk, key_bits) == (4160, 2 * K) and n_chunks == (16 if K == 10 else 64)
    assert partition_geometry(total - 301, 4 ** K)[0] == PART_CHUNK        # ... and only just
    args = kmer_batch(40 + K, K, read_lens, chunk)
    want = alt_stub.kmer_levels(*args)
    assert want[0][0] >= 4 * n_chunks and (args[1] > 3).sum() > 20 and (want[0][args[5] != 0] == 0).all()
    assert want[0].max() == want[0][0] and np.count_nonzero(want[0]) > 30000
    for _ in range(2):
        counts, levels, lv_off = eng.kmer_levels(*args)
        assert counts.dtype == np.int64 and np.array_equal(counts, want[0]) and np.array_equal(lv_off, want[2])
        assert np.array_equal(bits(levels), bits(want[1]))


def key_call(seed, n_keys, n_ent, est_mean):
    """random_call of test_gpu_kmer_est (a key most entries share, unused keys, uncovered positions) with the
    highest key in the first and in the last entries and half of the other keys in the upper half of the range"""
    rng = np.random.default_rng(seed)
    args = list(random_call(rng, 300, 9, n_keys, 700, n_ent, est_mean))
    ek = args[10]
    upper = rng.random(n_ent) < 0.2
    ek[upper] = rng.integers(n_keys // 2, n_keys, int(upper.sum()))
    ek[[0, 1, n_ent // 2, n_ent - 2, n_ent - 1]] = n_keys - 1
    return tuple(args)


def check_key_call(args):
    eng = rq.get_engine()
    n_keys = args[-1]
    want = est_stub.region_key_levels(*args[:-1], n_keys=n_keys)
    assert want[0][n_keys - 1] >= 5 and want[0][n_keys // 3] > args[10].shape[0] // 3
    for _ in range(2):
        got = eng.region_key_levels(*args)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(bits(got[2]), bits(want[2])) and np.array_equal(bits(got[3]), bits(want[3]))


def test_region_key_levels_with_2_to_the_24_keys():
    """the most keys the entry takes: one chunk whose length is no multiple of 4096, keys that use bit 23, and
    k_kmer_colscan and the prefix over 2^24 columns (sixteen grid passes)"""
    n_keys, n_ent = 1 << 24, 5001
    chunk, n_chunks, key_bits = partition_geometry(n_ent, n_keys)
    assert (n_chunks, key_bits) == (1, 24) and chunk > PART_CHUNK and chunk % PART_CHUNK != 0 and n_ent % chunk != 0
    assert n_keys > GRID_PASS
    args = key_call(24, n_keys, n_ent, False)
    assert (args[10] >> 23).any() and not (args[10] >> 23).all()
    check_key_call(args)


def test_region_key_levels_with_21_key_bits_and_15_chunks():
    n_keys, n_ent = (1 << 20) + 1, 15 * PART_CHUNK + 777
    chunk, n_chunks, key_bits = second_regime(n_ent, n_keys)
    assert (chunk, n_chunks, key_bits) == (4160, 15, 21) and n_keys > GRID_PASS
    args = key_call(21, n_keys, n_ent, True)
    assert (args[10] == 1 << 20).sum() >= 5          # the one key that needs the twenty-first bit
    check_key_call(args)


@pytest.mark.parametrize('n_ent', [16 * PART_CHUNK, 16 * PART_CHUNK + 1])
def test_region_key_levels_on_both_sides_of_the_chunk_switch(n_ent):
    """2^20 keys allow sixteen chunks: sixteen full chunks of 4096 are the last input of the first rule, one entry
    more gives sixteen chunks of 4160 with a short last one"""
    n_keys = 1 << 20
    chunk, n_chunks, key_bits = partition_geometry(n_ent, n_keys)
    assert (n_chunks, key_bits) == (16, 20)
    assert chunk == (PART_CHUNK if n_ent == 16 * PART_CHUNK else 4160)
    if n_ent > 16 * PART_CHUNK:
        second_regime(n_ent, n_keys)
    check_key_call(key_call(n_ent, n_keys, n_ent, n_ent % 2 == 0))

"""Genome tracks on the device (csrc/k_tracks.h) against the live reference's recorded output
(tests/golden/stats_tracks.npz, written by tests/golden/gen_golden_tracks.py): the cases of tests/tracks_cases.py,
which test_tracks_host_layer.py runs on the numpy stand-in, through the same public functions on the engine.

Tolerances: sums and means bit-equal with matching NaN masks (rtol 0: the kernel adds the same float64 values in
the same order as the reference's loop over the reads); coverages, positions and runs exact; file bytes equal.
The kernels' own edges (compaction blocks, scan chunks, ties at the top-N cut, non-finite differences) are
checked against tests/tracks_stub_engine.py, whose results are numpy's."""
import numpy as np
import pytest

from tombo_amd import tombo_helper as th
from tombo_amd._native import TRK_TILE as T
import tracks_cases as tc
from tracks_stub_engine import NumpyTracksEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def c():
    return tc.Case()


@pytest.fixture(scope='module')
def eng():
    from tombo_amd import resquiggle as rq
    return rq.get_engine()


@pytest.mark.parametrize('check', [tc.check_sizes, tc.check_means, tc.check_accumulation, tc.check_windows,
                                   tc.check_differences, tc.check_coverage], ids=lambda f: f.__name__)
def test_case(c, eng, check):
    check(c, eng)


def test_writers(c, eng, tmp_path):
    tc.check_writers(c, eng, tmp_path)


def test_default_engine_is_the_process_engine(c):
    reads = c.samp[('chrS', '+')]
    tc.same_bits(th.get_mean_slot_genome_centric(reads, c.sizes['chrS'], 'norm_mean'),
                 c.g['mean_0_chrS_+_norm_mean'])


def test_deep_stack_twice_same_bits(c, eng):
    """case 2 run twice: 300 reads over 64 positions across a tile edge, two LDS chunks of reads per tile"""
    index = {('chrD', '+'): c.samp[('chrD', '+')]}
    a, b = tc.all_tracks(c, eng, index, c.samp_slots), tc.all_tracks(c, eng, index, c.samp_slots)
    for x, y in zip(a[('chrD', '+')], b[('chrD', '+')]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, 4097, 262143, 262144, 262145, 300001])
def test_compaction_sizes(eng, n):
    """around one chunk of 1024 elements, several chunks, around the 256 chunks one step of the scan over the chunk
    counts takes (1024 * 256 elements), and more chunks than that"""
    rng, stub = np.random.default_rng(n), NumpyTracksEngine()
    v = rng.normal(size=n)
    v[rng.random(n) < 0.4] = np.nan
    v[-1] = 1.0
    cov = np.repeat(rng.integers(0, 4, n), rng.integers(1, 9, n))[:n].astype(np.int64)
    for x in (v, np.full(n, np.nan), cov, np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64)):
        got, want = eng.tracks_compact(x), stub.tracks_compact(x)
        tc.exact(got[0], want[0])
        tc.same_bits(got[1], want[1])
        assert got[0].dtype == np.int64 and got[1].dtype == x.dtype


def test_difference_of_non_finite_means(eng):
    a = np.array([1.0, np.nan, np.inf, -np.inf, np.inf, 3.0, -0.0, 1e308])
    b = np.array([0.5, 1.0, 1.0, 1.0, np.inf, np.nan, 0.0, -1e308])
    stub = NumpyTracksEngine()
    tc.same_bits(eng.tracks_diff(a, b), stub.tracks_diff(a, b))
    for n in (1, 3, 8, 20):
        got, want = eng.tracks_topn(a, b, n), stub.tracks_topn(a, b, n)
        tc.same_bits(got[0], want[0])
        tc.exact(got[1], want[1])


@pytest.mark.parametrize('n', [777, 5000, 70001])
def test_top_n_with_ties_takes_the_higher_position(eng, n):
    """few distinct values, so every cut falls inside a run of equal differences"""
    rng, stub = np.random.default_rng(n), NumpyTracksEngine()
    a, b = rng.integers(0, 12, n).astype(np.float64), rng.integers(0, 12, n).astype(np.float64)
    a[rng.random(n) < 0.1] = np.nan
    for k in (0, 1, 7, 100, n - 1, n, n + 5):
        got, want = eng.tracks_topn(a, b, k), stub.tracks_topn(a, b, k)
        tc.same_bits(got[0], want[0])
        tc.exact(got[1], want[1])
    a = rng.normal(size=n) * 10.0 ** rng.integers(-300, 300, n)
    got, want = eng.tracks_topn(a, b, 50), stub.tracks_topn(a, b, 50)
    tc.same_bits(got[0], want[0])
    tc.exact(got[1], want[1])


def test_engine_refuses_bad_tile_lists(eng):
    eng.tracks_begin(0, T + 1, 1)
    ok = dict(read_start=np.array([0]), read_end=np.array([4]), read_flags=np.array([2], dtype=np.uint8),
              read_off=np.array([0, 4]), slots=[np.ones(4)], tile_read_off=np.array([0, 1, 1]),
              tile_reads=np.array([0], dtype=np.int32))
    eng.tracks_add(**ok)
    with pytest.raises(ValueError):
        eng.tracks_add(**dict(ok, tile_reads=np.array([1], dtype=np.int32)))
    with pytest.raises(ValueError):
        eng.tracks_add(**dict(ok, tile_read_off=np.array([0, 1])))
    res = eng.tracks_finish(want_sums=True)
    assert res.sums[0][:5].tolist() == [1, 1, 1, 1, 0] and res.read_cov[:5].tolist() == [1, 1, 1, 1, 0]

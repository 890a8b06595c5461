"""The host layer of the genome tracks (tombo_amd.tombo_helper.GenomeTracks and the functions around it,
tombo_amd.text_output) on the numpy stand-in engine of tests/tracks_stub_engine.py: every case of
tests/golden/stats_tracks.npz through the public functions, so tile lists, windows, slots, batches, writers and
argument checks are tested without a GPU.  The same cases run on the device in test_gpu_tracks.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tombo_amd import _native, tombo_helper as th, text_output
from tombo_amd._native import TRK_TILE as T
import tracks_cases as tc
import tracks_reference as tr
from tracks_stub_engine import NumpyTracksEngine

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
ENTRIES = ['tba_tracks_begin', 'tba_tracks_add', 'tba_tracks_finish', 'tba_tracks_compact', 'tba_tracks_diff',
           'tba_tracks_topn']


@pytest.fixture(scope='module')
def c():
    return tc.Case()


@pytest.fixture()
def eng():
    return NumpyTracksEngine()


@pytest.mark.parametrize('check', [tc.check_sizes, tc.check_means, tc.check_accumulation, tc.check_windows,
                                   tc.check_differences, tc.check_coverage], ids=lambda f: f.__name__)
def test_case(c, eng, check):
    check(c, eng)


def test_writers(c, eng, tmp_path):
    tc.check_writers(c, eng, tmp_path)


def test_windows_are_cut_where_asked(c, eng):
    tc.all_tracks(c, eng, {('chrA', '+'): c.samp[('chrA', '+')]}, c.samp_slots, max_window=T + 3)
    size = c.sizes['chrA']
    assert [(a, b) for a, b, _ in eng.windows] == [(s, min(s + T + 3, size)) for s in range(0, size, T + 3)]
    assert all(ns == 3 for _, _, ns in eng.windows)


def test_tile_lists():
    starts = np.array([0, T - 1, T, 10, 3 * T, 5, 2 * T + 1])
    ends = np.array([T, T, T + 1, 10, 3 * T + 7, 2 * T + 1, 2 * T + 2])
    off, reads = th.build_tile_lists(starts, ends, 0, 3 * T + 7, T)
    assert off.dtype == np.int64 and reads.dtype == np.int32
    lists = [reads[a:b].tolist() for a, b in zip(off[:-1], off[1:])]
    assert lists == [[0, 1, 5], [2, 5], [5, 6], [4]]       # input order inside a tile; the empty read 3 nowhere
    # a window inside the chromosome: reads are clipped to it
    off, reads = th.build_tile_lists(starts, ends, T - 1, 2 * T + 1, T)
    assert [reads[a:b].tolist() for a, b in zip(off[:-1], off[1:])] == [[0, 1, 2, 5], [5]]


def test_a_read_without_events_counts_as_read_coverage_only(eng):
    reads = [tr.Read(3, 9, '+', 'a', np.arange(6.0)), tr.Read(5, 12, '-', 'b', None)]
    res = th.GenomeTracks({'c': 12}, engine=eng).add_reads('c', '+', reads).finish()[('c', '+')]
    assert res.read_cov.tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 2, 1, 1, 1]
    assert res.slot_cov[0].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    assert np.isnan(res.means[0][9:]).all() and res.means[0][3:9].tolist() == list(np.arange(6.0))


def test_slots_by_read_id_and_missing_slots(eng):
    reads = [tr.Read(0, 3, '-', 'a', np.array([1.0, 2.0, 3.0]))]
    got = th.get_mean_slot_genome_centric(reads, 4, 'length', {'a': np.array([7, 8, 9], dtype=np.uint32)}, engine=eng)
    assert got[:3].tolist() == [9.0, 8.0, 7.0] and np.isnan(got[3])
    with pytest.raises(ValueError, match='needs `slots`'):
        th.get_mean_slot_genome_centric(reads, 4, 'norm_stdev', engine=eng)
    with pytest.raises(ValueError, match='outside'):
        th.get_mean_slot_genome_centric(reads, 2, 'norm_mean', engine=eng)
    with pytest.raises(ValueError, match='differ in length'):
        th.GenomeTracks({'c': 9}, slots=('norm_mean', 'length'), engine=eng).add_reads(
            'c', '-', reads, {'length': [np.array([1, 2], dtype=np.uint32)]})
    with pytest.raises(ValueError, match='slots'):
        th.GenomeTracks({'c': 9}, slots=('norm_mean', 'base'))


def test_statistics_file_types_are_named(c, eng):
    for t in ('fraction', 'dampened_fraction', 'statistic', 'valid_coverage'):
        with pytest.raises(NotImplementedError, match=t):
            text_output.write_all_browser_files(c.samp, None, 'x', ['coverage', t], engine=eng)


def test_argument_checks():
    ok = dict(read_start=np.array([0, 5]), read_end=np.array([4, 9]), read_flags=np.array([2, 3], dtype=np.uint8),
              read_off=np.array([0, 4, 8]), slots=[np.zeros(8)], tile_read_off=np.array([0, 2, 2]),
              tile_reads=np.array([0, 1], dtype=np.int32))
    _native._check_tracks_add_args(T + 1, 1, **ok)
    bad = [dict(read_off=np.array([0, 5, 4])), dict(read_off=np.array([1, 4, 8])),
           dict(tile_read_off=np.array([0, 2, 1])), dict(tile_read_off=np.array([0, 2])),
           dict(tile_reads=np.array([0, 2], dtype=np.int32)), dict(tile_reads=np.array([-1, 1], dtype=np.int32)),
           dict(tile_reads=np.array([0, 1], dtype=np.int64)), dict(read_flags=np.array([2, 4], dtype=np.uint8)),
           dict(read_end=np.array([4, 3])), dict(slots=[np.zeros(7)]), dict(slots=[np.zeros(8), np.zeros(8)]),
           dict(read_start=np.array([0.0, 5.0]))]
    for change in bad:
        with pytest.raises(ValueError):
            _native._check_tracks_add_args(T + 1, 1, **dict(ok, **change))
    for args in ((0, 10, 0), (0, 10, 4), (5, 5, 1), (-1, 4, 1), (0, 2 ** 31, 1)):
        with pytest.raises(ValueError):
            _native._check_tracks_begin_args(*args)
    with pytest.raises(ValueError):
        _native._check_track_pair(np.zeros(3), np.zeros(4))
    with pytest.raises(ValueError):
        _native._check_compact_args(np.zeros(3, dtype=np.float32))


def test_abi_and_entries():
    assert _native.ABI_VERSION == 13
    hdr = open(os.path.join(ROOT, 'include', 'tombo_amd.h')).read()
    assert int(re.search(r'#define\s+TBA_ABI_VERSION\s+(\d+)', hdr).group(1)) == 13
    assert int(re.search(r'#define\s+TBA_TRK_TILE\s+(\d+)', hdr).group(1)) == _native.TRK_TILE
    src = open(os.path.join(_native.CSRC, 'k_tracks.h')).read()
    assert int(re.search(r'#define\s+TRK_TILE\s+(\d+)', src).group(1)) == _native.TRK_TILE
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    lib = ctypes.CDLL(_native.build())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in ('tracks_begin', 'tracks_add', 'tracks_finish', 'tracks_compact', 'tracks_diff', 'tracks_topn'):
        assert callable(getattr(_native.Engine, name)) and callable(getattr(NumpyTracksEngine, name))

"""The kernel times the statistics entries report (last_site_aggregate_kernel_ms, last_roc_kernel_ms,
last_roc_sort_ms / last_roc_gather_ms, tracks_kernel_ms), on the smallest inputs that launch a kernel.

A kernel time is measured inside its call, so the wall-clock time of the Python call around the entry bounds it
from above with no tolerance; from below it is positive whenever a kernel ran, and exactly 0.0 when the entry
returns before the device."""
import math
import time

import numpy as np
import pytest

from tombo_amd import _native, resquiggle as rq
from tombo_amd._native import TRK_TILE as T

pytestmark = pytest.mark.gpu

I64 = lambda *v: np.array(v, dtype=np.int64)     # noqa: E731


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


def wall_ms(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def check_inside(ms, wall):
    print('kernel %.6f ms, call %.6f ms' % (ms, wall))
    assert math.isfinite(ms) and 0.0 < ms <= wall


def test_site_aggregate(eng):
    rec = np.zeros(3, dtype=_native.PER_READ_DTYPE)
    rec['pos'], rec['stat'], rec['read_id'] = [10, 12, 12], [0.25, -1.0, 2.0], [0, 1, 2]
    wall = wall_ms(lambda: eng.site_aggregate(I64(10), I64(14), I64(0, 3), rec, 0.5))
    check_inside(eng.last_site_aggregate_kernel_ms, wall)
    eng.site_aggregate(I64(), I64(), I64(0), rec[:0], 0.5)
    assert eng.last_site_aggregate_kernel_ms == 0.0


RECS = (I64(0, 3), I64(5, 6, 7), np.array([0.5, -0.5, 1.5]))
NO_RECS = (I64(0, 0), I64(), np.empty(0))


def test_roc_loc_labels(eng):
    wall = wall_ms(lambda: eng.roc_loc_labels(I64(0, 2, 0, 1).reshape(1, 4), I64(5, 7), I64(6), *RECS))
    check_inside(eng.last_roc_kernel_ms, wall)
    eng.roc_loc_labels(I64(0, 2, 0, 1).reshape(1, 4), I64(5, 7), I64(6), *NO_RECS)
    assert eng.last_roc_kernel_ms == 0.0


def test_roc_motif_labels(eng):
    block = (np.zeros(1, dtype=np.uint8), I64(4), I64(0, 6), np.array([0, 1, 2, 3, 0, 1], dtype=np.uint8))
    motifs = [(2, 1, 1, np.array([2, 4], dtype=np.uint8))]      # C then G, the modified base the C
    wall = wall_ms(lambda: eng.roc_motif_labels(*block, *RECS, motifs))
    check_inside(eng.last_roc_kernel_ms, wall)
    eng.roc_motif_labels(*block, *NO_RECS, motifs)
    assert eng.last_roc_kernel_ms == 0.0


def test_roc_rank_counts(eng):
    stats, has_mod = np.array([0.5, -1.0, 2.0, 0.5, 0.0]), np.array([True, False, True, False, True])
    wall = wall_ms(lambda: eng.roc_rank_counts(stats, has_mod, I64(1, 4)))
    print('sort %.6f ms, gather %.6f ms' % (eng.last_roc_sort_ms, eng.last_roc_gather_ms))
    assert eng.last_roc_sort_ms > 0.0 and eng.last_roc_gather_ms > 0.0
    assert eng.last_roc_kernel_ms == eng.last_roc_sort_ms + eng.last_roc_gather_ms
    check_inside(eng.last_roc_kernel_ms, wall)
    eng.roc_rank_counts(stats[:0], has_mod[:0], I64())
    assert eng.last_roc_sort_ms == 0.0 and eng.last_roc_gather_ms == 0.0 and eng.last_roc_kernel_ms == 0.0


def test_tracks(eng):
    """one window of two tiles, one slot, two reads (the second lies across the tile edge)"""
    reads = (I64(3, T - 2), I64(7, T + 2), np.array([2, 2], dtype=np.uint8), I64(0, 4, 8), [np.arange(8.0)],
             I64(0, 2, 3), np.array([0, 1, 1], dtype=np.int32))
    eng.tracks_begin(0, T + 5, 1)
    times = [eng.tracks_kernel_ms()]
    assert times[0] == 0.0
    eng.tracks_add(*reads)
    times.append(eng.tracks_kernel_ms())
    eng.tracks_add(*reads)
    times.append(eng.tracks_kernel_ms())
    res = eng.tracks_finish()
    times.append(eng.tracks_kernel_ms())
    print('tracks_kernel_ms after begin, add, add, finish:', times)
    assert all(math.isfinite(t) for t in times) and times[0] < times[1] < times[2] < times[3]
    assert res.slot_cov[0, 3:7].tolist() == [2] * 4 and res.means[0, T].tolist() == 6.0
    eng.tracks_begin(0, T + 5, 1)
    assert eng.tracks_kernel_ms() == 0.0
    eng.tracks_finish()

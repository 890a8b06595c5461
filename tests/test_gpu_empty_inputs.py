"""Empty arrays among non-empty ones, at every place where a statistics entry uploads an array that its caller
may leave empty: the entry must give what the numpy forms of the other GPU tests give, bit for bit, with the
smallest surroundings that still reach the device."""
import numpy as np
import pytest

from tombo_amd import _native, resquiggle as rq
from tombo_amd._native import TRK_TILE as T
import alt_est_stub_engine as alt_stub
import kmer_est_cases as kc
import kmer_est_reference as kr
import kmer_est_stub_engine as kmer_stub
import roc_reference as ref
import stat_store_cases as sc
import tracks_cases as tc
from stat_store_stub_engine import NumpyStatStoreEngine
from tracks_stub_engine import NumpyTracksEngine

pytestmark = pytest.mark.gpu

I64 = lambda *v: np.array(v, dtype=np.int64)     # noqa: E731
U8 = lambda *v: np.array(v, dtype=np.uint8)      # noqa: E731


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


def test_kde_eval_only_empty_segments(eng):
    args = (np.empty(0), I64(0, 0, 0), np.array([-1.0, 0.0, 2.5]), 0.25)
    got, want = eng.kde_eval(*args), alt_stub.kde_eval(*args)
    assert got.shape == want.shape == (2, 3) and np.isnan(want).all()
    assert np.array_equal(kc.bits(got), kc.bits(want))


def test_segment_medians_only_empty_segments(eng):
    got, want = eng.segment_medians(np.empty(0), I64(0, 0, 0)), kr.medians(np.empty(0), I64(0, 0, 0))
    assert got.shape == want.shape == (2,) and np.isnan(want).all()
    assert np.array_equal(kc.bits(got), kc.bits(want))


def test_tracks_add_a_listed_read_without_levels(eng):
    """the read covers [3, 9) of the window and is listed by its tile, but has no level in the slot"""
    reads = (I64(3), I64(9), U8(2), I64(0, 0), [np.empty(0)], I64(0, 1), np.array([0], dtype=np.int32))
    out = []
    for e in (eng, NumpyTracksEngine()):
        e.tracks_begin(0, T, 1)
        e.tracks_add(*reads)
        out.append(e.tracks_finish(want_sums=True))
    got, want = out
    assert want.read_cov[3:9].tolist() == [1] * 6 and want.read_cov.sum() == 6 and not want.slot_cov.any()
    tc.same_bits(got.means, want.means)
    tc.same_bits(got.sums, want.sums)
    tc.exact(got.slot_cov, want.slot_cov)
    tc.exact(got.read_cov, want.read_cov)


@pytest.mark.parametrize('est_mean', [False, True])
def test_region_key_levels_region_without_reads(eng, est_mean):
    """no read at all: the region's read list, the reads' starts, strands and levels are all empty"""
    args = (est_mean, I64(), U8(), I64(0), np.empty(0), I64(0, 0), I64(), I64(0), I64(17), I64(0), I64(2))
    got, want = eng.region_key_levels(*args, 4), kmer_stub.region_key_levels(*args, n_keys=4)
    assert want[0].tolist() == [0, 0, 1, 0] and want[1].tolist() == [0, 0, 0, 1, 1]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(kc.bits(got[2]), kc.bits(want[2])) and np.array_equal(kc.bits(got[3]), kc.bits(want[3]))


def check_labels(got, want):
    assert len(got) == len(want) == 3
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[1].dtype == np.bool_ and got[2].dtype == np.int64


RECS = (I64(0, 2), I64(5, 6), np.array([0.5, -1.5]))


@pytest.mark.parametrize('ctrl_label', [None, True])
def test_roc_motif_labels_block_without_sequence(eng, ctrl_label):
    """two records in a block whose sequence is empty: no base is known, so nothing matches"""
    block = (U8(0), I64(5), I64(0, 0), U8())
    motifs = [(2, 1, 1, U8(2, 4))]
    got = eng.roc_motif_labels(*block, *RECS, motifs, ctrl_label, return_index=True)
    want = ref.motif_labels(*block, *RECS, motifs, ctrl_label)
    assert len(got) == len(want) == 1 and want[0][0].shape == (0,)
    check_labels(got[0], want[0])


@pytest.mark.parametrize('mod,unmod', [(I64(), I64(5, 9)), (I64(6, 9), I64())], ids=['no_mod', 'no_unmod'])
def test_roc_loc_labels_one_empty_list(eng, mod, unmod):
    loc = I64(0, mod.shape[0], 0, unmod.shape[0]).reshape(1, 4)
    got = eng.roc_loc_labels(loc, mod, unmod, *RECS, return_index=True)
    want = ref.loc_labels(loc, mod, unmod, *RECS)
    assert want[0].shape == (1,)
    check_labels(got, want)


def test_site_aggregate_block_without_records(eng):
    args = (I64(10), I64(14), I64(0, 0), np.zeros(0, dtype=_native.PER_READ_DTYPE), 0.5, None, False, (1.0, 2.0))
    got, want = eng.site_aggregate(*args), NumpyStatStoreEngine().site_aggregate(*args)
    assert want.counts.tolist() == [0] and want.n_stats.tolist() == [0]
    sc.check_equal_results(got, want)

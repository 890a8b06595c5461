"""The launches of the segment sorters and of the kernel densities beyond their fixed grids (csrc/tba_engine.hip):
k_kde_classify past grid_for(64 * n_seg)'s cap (16 384 segments), more segments of each sorter class than
launch_sort_classes' grids take at once (4096 wavefronts, 1024 and 256 workgroups), k_kde_eval past 65 535 blocks,
and the second grid pass of k_kest_median and k_plot_percentiles.  References: kmer_est_reference.medians,
plot_reference.segment_percentiles and alt_est_stub_engine.kde_eval; medians and percentiles bit for bit, densities
under alt_est_cases.assert_density_close, as in the tests of those entries at small sizes.

Where the reference is a Python loop per segment over a million segments, it is run on launch_caps.pass_sample's
segments (both ends of every pass and 2000 drawn ones), and the whole output must equal, bit for bit, the same
entry called on pieces that each stay below the pass."""
import numpy as np
import pytest

import alt_est_cases as ac
import alt_est_stub_engine as alt_stub
import kmer_est_reference as kr
import plot_reference as ref
import launch_caps as lc
from kmer_est_cases import bits
from tombo_amd import tombo_stats as ts, resquiggle as rq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


def small_segments(rng, n_seg, max_len, nan_rate=0.01):
    """n_seg segments of 0 .. max_len values each, a NaN in about nan_rate of them, the values of segment s around s
    (a median or a density that lands in another segment's row shows)"""
    sizes = rng.integers(0, max_len + 1, n_seg)
    off = ts._csr_offsets(sizes)
    values = np.repeat(np.arange(n_seg, dtype=np.float64), sizes) + ref.full_mantissa(rng, int(off[-1]))
    values[rng.random(values.shape[0]) < nan_rate / max(max_len / 2.0, 1.0)] = np.nan
    return values, off


def sub_segments(values, off, segs):
    """the CSR of the listed segments alone"""
    parts = [values[off[s]:off[s + 1]] for s in segs.tolist()]
    return np.concatenate(parts), ts._csr_offsets([p.shape[0] for p in parts])


def pieces(n, piece):
    return [(a, min(a + piece, n)) for a in range(0, n, piece)]


def piece_of(values, off, a, b):
    return values[off[a]:off[b]], off[a:b + 1] - off[a]


# ---- k_kde_classify: one wavefront per segment up to CLASSIFY_PASS segments --------------------------------------
def test_segment_medians_classify_beyond_one_pass(eng):
    n_seg = lc.CLASSIFY_PASS + 1
    assert lc.WAVE * n_seg > lc.GRID_PASS >= lc.WAVE * (n_seg - 1)
    values, off = small_segments(np.random.default_rng(31), n_seg, 6)
    want = kr.medians(values, off)
    assert np.isnan(want).sum() > 1000 and (~np.isnan(want[-70:])).sum() > 30
    got = eng.segment_medians(values, off)
    assert np.array_equal(bits(got), bits(want))


def test_kde_eval_classify_beyond_one_pass(eng):
    n_seg = lc.CLASSIFY_PASS + 1
    assert lc.WAVE * n_seg > lc.GRID_PASS and n_seg < lc.KDE_EVAL_BLOCKS
    rng = np.random.default_rng(32)
    sizes = rng.integers(0, 6, n_seg)
    sizes[[0, lc.CLASSIFY_PASS - 1, lc.CLASSIFY_PASS]] = (3, 4, 5)
    off = ts._csr_offsets(sizes)
    levels = rng.normal(0, 1, int(off[-1]))
    levels[rng.integers(0, levels.shape[0], 40)] = np.nan
    x = np.array([-0.5, 0.125, 0.75])
    want = alt_stub.kde_eval(levels, off, x, 0.3)
    got = eng.kde_eval(levels, off, x, 0.3)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want[[0, -2, -1]]).any()
    ok = ~np.isnan(want[:, 0])
    assert 0.5 * n_seg < ok.sum() < n_seg - 30
    ac.assert_density_close(got[ok], want[ok])


# ---- launch_sort_classes: more segments of a class than its grid ---------------------------------------------------
@pytest.fixture(scope='module')
def class_segments():
    """4200 segments of 2 .. 64 values, 1100 of 65 .. 80 and 257 of 4097, interleaved (a global-class segment every
    21 others, an LDS-class one every fifth), an empty segment or one with a NaN after every 16th"""
    rng = np.random.default_rng(33)
    n_wave, n_lds, n_glob = lc.SORT_WAVE_PASS + 104, lc.SORT_LDS_PASS + 76, lc.SORT_GLOBAL_PASS + 1
    kinds = np.concatenate([np.zeros(n_wave, int), np.ones(n_lds, int), np.full(n_glob, 2)])
    kinds = kinds[rng.permutation(kinds.shape[0])]
    segs = []
    for i, k in enumerate(kinds.tolist()):
        n = (int(rng.integers(2, lc.SORT_WAVE_MAX + 1)), int(rng.integers(lc.SORT_WAVE_MAX + 1, 81)),
             lc.SORT_LDS_MAX + 1)[k]
        segs.append(ref.full_mantissa(rng, n) if i % 2 else rng.integers(-40, 41, n) / 64.0)
        if i % 16 == 3:
            segs.append(np.empty(0))
        if i % 16 == 11:
            segs.append(np.array([0.25, np.nan, 0.5]))
    sizes = np.array([s.shape[0] for s in segs])
    assert ((sizes >= 2) & (sizes <= lc.SORT_WAVE_MAX)).sum() > lc.SORT_WAVE_PASS
    assert ((sizes > lc.SORT_WAVE_MAX) & (sizes <= lc.SORT_LDS_MAX)).sum() > lc.SORT_LDS_PASS
    assert (sizes > lc.SORT_LDS_MAX).sum() > lc.SORT_GLOBAL_PASS
    assert sizes.shape[0] < lc.CLASSIFY_PASS       # the classify launch itself stays in one pass here
    return np.concatenate(segs), ts._csr_offsets(sizes)


def test_segment_medians_more_segments_than_every_sorter_grid(eng, class_segments):
    values, off = class_segments
    before = values.copy()
    want = kr.medians(values, off)
    got = eng.segment_medians(values, off)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(values), bits(before))
    assert 600 < np.isnan(want).sum() < 800


Q_LIN = np.true_divide([0, 1, 25, 50, 75, 99, 100], 100)
Q_NEAR = np.true_divide([0, 1, 10, 49, 50, 51, 99, 100], 100)


def test_segment_percentiles_more_segments_than_every_sorter_grid(eng, class_segments):
    values, off = class_segments
    want = ref.segment_percentiles(values, off, Q_LIN, Q_NEAR)
    got = eng.segment_percentiles(values, off, Q_LIN, Q_NEAR)
    ref.same_bits(got[0], want[0])
    ref.same_bits(got[1], want[1])


# ---- k_kde_eval: blockIdx.x strides over the segments from 65 535 on ----------------------------------------------
def test_kde_eval_more_segments_than_blocks(eng):
    n_seg = lc.KDE_EVAL_BLOCKS + 1 + 3
    assert n_seg > lc.KDE_EVAL_BLOCKS and n_seg == 65536 + 3
    rng = np.random.default_rng(34)
    sizes = rng.integers(0, 5, n_seg)
    sizes[[lc.KDE_EVAL_BLOCKS - 1, lc.KDE_EVAL_BLOCKS, n_seg - 1]] = (2, 3, 4)
    off = ts._csr_offsets(sizes)
    levels = rng.normal(0, 1, int(off[-1]))
    levels[rng.integers(0, levels.shape[0], 100)] = np.nan
    levels[off[lc.KDE_EVAL_BLOCKS]:off[lc.KDE_EVAL_BLOCKS] + 3] = (0.5, -0.25, 0.125)
    levels[off[n_seg - 1]:off[n_seg]] = (0.75, 0.0, -1.0, 0.3)
    x = np.array([-0.4, 0.6])
    got = eng.kde_eval(levels, off, x, 0.25)
    sample = lc.pass_sample(n_seg, 35, pass_len=lc.KDE_EVAL_BLOCKS)
    assert sample.shape[0] >= 2000 and {0, lc.KDE_EVAL_BLOCKS - 1, lc.KDE_EVAL_BLOCKS, n_seg - 1} <= set(sample.tolist())
    want = alt_stub.kde_eval(*sub_segments(levels, off, sample), x, 0.25)
    assert np.array_equal(np.isnan(got[sample]), np.isnan(want))
    ok = ~np.isnan(want[:, 0])
    assert ok[-1] and ok.sum() > 800
    ac.assert_density_close(got[sample][ok], want[ok])
    for a, b in pieces(n_seg, 16000):       # every row: the entry on pieces below the classify and the block caps
        assert b - a < lc.CLASSIFY_PASS
        assert np.array_equal(bits(got[a:b]), bits(eng.kde_eval(*piece_of(levels, off, a, b), x, 0.25))), a


# ---- second grid pass of k_kest_median and k_plot_percentiles ------------------------------------------------------
def test_segment_medians_second_grid_pass(eng):
    n_seg = lc.GRID_PASS + 1
    assert n_seg > lc.GRID_PASS
    rng = np.random.default_rng(36)
    sizes = rng.integers(0, 4, n_seg)
    sizes[[lc.GRID_PASS - 1, lc.GRID_PASS]] = (2, 3)
    off = ts._csr_offsets(sizes)
    values = np.repeat(np.arange(n_seg, dtype=np.float64), sizes) + ref.full_mantissa(rng, int(off[-1]))
    values[rng.random(values.shape[0]) < 0.005] = np.nan
    # planted: the last item of the first pass, the first of the second (the last segment of the call)
    values[off[lc.GRID_PASS - 1]:off[lc.GRID_PASS]] = (3.5, -1.0)
    values[off[lc.GRID_PASS]:] = (7.25, 9.0, 8.0)
    got = eng.segment_medians(values, off)
    assert got[lc.GRID_PASS - 1] == 1.25 and got[lc.GRID_PASS] == 8.0
    sample = lc.pass_sample(n_seg, 37)
    assert sample.shape[0] >= 2000
    want = kr.medians(*sub_segments(values, off, sample))
    assert np.array_equal(bits(got[sample]), bits(want)) and (~np.isnan(want)).sum() > 1000
    for a, b in pieces(n_seg, lc.GRID_PASS // 2 + 1):
        assert b - a < lc.GRID_PASS
        assert np.array_equal(bits(got[a:b]), bits(eng.segment_medians(*piece_of(values, off, a, b)))), a


def test_segment_percentiles_second_grid_pass(eng):
    """one thread per (segment, fraction): 20 000 segments of 53 fractions are 1 060 000 items"""
    n_seg = 20000
    ql, qn = np.linspace(0, 1, 27), np.linspace(0, 1, 26)
    nq = ql.shape[0] + qn.shape[0]
    assert n_seg * nq > lc.GRID_PASS and (n_seg // 2 + 1) * nq < lc.GRID_PASS
    values, off = small_segments(np.random.default_rng(38), n_seg, 9)
    lin, near = eng.segment_percentiles(values, off, ql, qn)
    edge = lc.GRID_PASS // nq        # the segment whose fractions straddle the end of the first pass
    assert edge * nq < lc.GRID_PASS < (edge + 1) * nq
    sample = np.unique(np.concatenate([np.arange(0, 3), np.arange(edge - 3, edge + 4), np.arange(n_seg - 3, n_seg),
                                       np.random.default_rng(39).choice(n_seg, 2000, replace=False)]))
    assert sample.shape[0] >= 2000
    want = ref.segment_percentiles(*sub_segments(values, off, sample), ql, qn)
    ref.same_bits(lin[sample], want[0])
    ref.same_bits(near[sample], want[1])
    assert (~np.isnan(want[0][:, 0])).sum() > 1000
    for a, b in pieces(n_seg, n_seg // 2 + 1):
        part = eng.segment_percentiles(*piece_of(values, off, a, b), ql, qn)
        ref.same_bits(lin[a:b], part[0])
        ref.same_bits(near[a:b], part[1])

"""The second grid pass of the one-thread-per-item statistics kernels: grid_for(n) (csrc/tba_engine.hip) launches at
most 4096 blocks of 256 threads, so from item launch_caps.GRID_PASS on a kernel's stride loop does the work.  Every
test here gives an entry GRID_PASS + 1 items (or as many as its launch needs to cross), asserts that from
launch_caps, and compares with the reference the entry's own tests use, under their tolerance: p-values 1e-12
relative (_close / _rtol of test_gpu_stats_edges), everything else by bits.

Distinct values stand at items GRID_PASS - 1 and GRID_PASS (the last one).  Where the reference is a Python loop per
item (group statistics, piles, medians), it is run on launch_caps.pass_sample's items -- both ends of every pass and
2000 or more drawn ones -- and the whole output must equal, bit for bit, the same entry called on pieces that each stay
below one pass."""
import numpy as np
import pytest

import kmer_est_stub_engine as est_stub
import norm_api_cases as nc
import plot_reference as ref
import stats_reference as sr
import test_gpu_plot_data as plot_tests
import tracks_cases as tc
from kmer_est_cases import bits
from launch_caps import GRID_PASS, pass_sample
from stats_stub_engine import NumpyStatsEngine, _Read
from test_gpu_stats_edges import _close, _rtol
from tracks_stub_engine import NumpyTracksEngine
from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq
from tombo_amd._default_parameters import SMALLEST_PVAL
from tombo_amd._native import TRK_TILE

pytestmark = pytest.mark.gpu
N = GRID_PASS + 1
EDGE = np.array([GRID_PASS - 1, GRID_PASS])        # the last item of the first pass, the one item of the second


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


def halves(n, piece=GRID_PASS // 2 + 1):
    cuts = list(range(0, n, piece)) + [n]
    assert max(b - a for a, b in zip(cuts[:-1], cuts[1:])) < GRID_PASS
    return list(zip(cuts[:-1], cuts[1:]))


# ---- read_pvals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fm', [0, 2])
def test_read_pvals_second_pass(eng, fm):
    rng = np.random.default_rng(60 + fm)
    off = ts._csr_offsets([400000, 300000, N - 700000])
    assert int(off[-1]) == N > GRID_PASS
    ref_m, ref_s = rng.normal(0, 1, N), np.abs(rng.normal(0.3, 0.05, N)) + 0.05
    z = rng.normal(0, 1.5, N)
    z[EDGE - fm] = (0.5, 2.5)
    means = ref_m + z * ref_s
    means[rng.integers(0, N - 10, 50)] = np.nan
    got = eng.read_pvals(means, ref_m, ref_s, off, fm, True, SMALLEST_PVAL)
    want = NumpyStatsEngine().read_pvals(means, ref_m, ref_s, off, fm, True, SMALLEST_PVAL)
    assert not np.isnan(want[EDGE - fm]).any() and len(set(want[EDGE - fm].tolist())) == 2
    _close(got, want, 1e-12)


# ---- llh_ratio_windows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_llh_ratio_windows_second_pass(eng, kind):
    rng = np.random.default_rng(70 + kind)
    width, n_windows = 1, N
    assert n_windows > GRID_PASS
    n = n_windows + width - 1
    m, r = rng.normal(0, 1, n), rng.normal(0, 1, n)
    a = r + rng.choice([-1.0, 0.0, 1.0], n) * rng.uniform(0.2, 2.0, n)
    rv, av = rng.uniform(0.05, 0.5, n), rng.uniform(0.05, 0.5, n)
    m[EDGE] = r[EDGE] + (0.25, -0.5)
    a[EDGE] = r[EDGE] + 1.0
    starts = np.arange(n_windows, dtype=np.int64)
    par = (4.0, 0.33, 0.33)
    call = lambda st: eng.llh_ratio_windows(kind, m, r, a, rv, st, width, av if kind == 0 else None, par)   # noqa: E731
    got = call(starts)
    sample = pass_sample(n_windows, 71)
    assert sample.shape[0] >= 2000
    want = NumpyStatsEngine().llh_ratio_windows(kind, m, r, a, rv, starts[sample], width, av if kind == 0 else None, par)
    assert len(set(want[np.searchsorted(sample, EDGE)].tolist())) == 2
    if kind == 1:
        assert np.array_equal(bits(got[sample]), bits(want))
    else:
        np.testing.assert_allclose(got[sample], want, rtol=1e-12, atol=1e-12 if kind == 0 else 1e-13)
    for lo, hi in halves(n_windows):
        assert np.array_equal(bits(got[lo:hi]), bits(call(starts[lo:hi]))), lo


# ---- group_level_stats / reads_ref_levels -----------------------------------------------------------------------
def group_pileup(n_pos, start=5000, one_group=False):
    """one region of n_pos positions, no strand filter; sample reads over [0, 0.6 n) ('+') and [0.4 n, n) ('-'),
    control reads over [0, 0.75 n) and [0.25 n, n): coverage 0 - 2 per group (blocks of NaN levels make the zeros),
    single NaN levels elsewhere, distinct levels at the last position of the first pass and the first of the next"""
    rng = np.random.default_rng(n_pos)
    spans = [(0, 6 * n_pos // 10, '+', 0), (4 * n_pos // 10, n_pos, '-', 0), (0, 3 * n_pos // 4, '+', 1),
             (n_pos // 4, n_pos, '+', 1)]
    reads = []
    for k, (a, b, strand, ctrl) in enumerate(spans):
        m = rng.normal(0.4 * ctrl, 1, b - a)
        m[rng.random(b - a) < 0.01] = np.nan
        hole = (45 + 10 * ctrl) * n_pos // 100              # both reads of a group are NaN here: coverage 0
        m[max(hole - a, 0):max(hole + n_pos // 200 - a, 0)] = np.nan
        for p in (n_pos - 2, n_pos - 1) + ((GRID_PASS - 1, GRID_PASS) if n_pos > GRID_PASS else ()):
            if a <= p < b:
                m[p - a] = 0.125 * (k + 1) + 1e-3 * (p % 7)
        reads.append((start + a, strand, m[::-1].copy() if strand == '-' else m, ctrl))
    i64, i8 = np.int64, np.int8
    pl = ts.Pileup(np.array([start], i64), np.array([start + n_pos], i64), np.array([2], i8), np.array([0, 4], i64),
                   np.array([r[0] for r in reads], i64), np.array([r[1] == '-' for r in reads], i8),
                   np.array([0 if one_group else r[3] for r in reads], i8), ts._csr_offsets([r[2].shape[0] for r in reads]),
                   np.concatenate([r[2] for r in reads]), np.array([0, n_pos], i64))
    return pl, [_Read(r[0], r[1], r[2]) for r in reads if r[3] == 0], [_Read(r[0], r[1], r[2]) for r in reads if r[3] == 1]


def sub_region(pl, a, b):
    """the same reads under the region [reg_start + a, reg_start + b)"""
    s = int(pl.reg_start[0])
    return pl._replace(reg_start=np.array([s + a], np.int64), reg_end=np.array([s + b], np.int64),
                       pos_off=np.array([0, b - a], np.int64))


GROUP_SIZES = [GRID_PASS // 2 + 1, N]      # k_grp_classify runs over 2 n_pos items: it crosses first


@pytest.mark.parametrize('n_pos', GROUP_SIZES)
@pytest.mark.parametrize('stat_type', ['u_stat_test', 'ks_test'])
def test_group_level_stats_second_pass(eng, n_pos, stat_type):
    assert 2 * n_pos > GRID_PASS
    pl, samp, ctrl = group_pileup(n_pos)
    start = int(pl.reg_start[0])
    kind = ts._GROUP_KINDS[stat_type]
    stats, poss, cov, ccov, counts = eng.group_level_stats(*kind, 0, 1, pl, SMALLEST_PVAL)
    # positions and coverages of every position, from the reference's pileup
    s_cov = (~np.isnan(sr.base_levels(samp, start, start + n_pos, None))).sum(axis=1)
    c_cov = (~np.isnan(sr.base_levels(ctrl, start, start + n_pos, None))).sum(axis=1)
    assert set(s_cov.tolist()) == {0, 1, 2} == set(c_cov.tolist())
    kept = np.flatnonzero((s_cov >= 1) & (c_cov >= 1))
    n = int(counts[0])
    assert n == kept.shape[0] and kept[-1] == n_pos - 1 and n < n_pos - n_pos // 200
    assert np.array_equal(poss[:n], start + kept) and np.array_equal(cov[:n], s_cov[kept]) and np.array_equal(ccov[:n], c_cov[kept])
    # the statistic on the sample, one position per call of the reference
    sample = pass_sample(n_pos, 81, n_random=2500, pass_len=GRID_PASS if n_pos > GRID_PASS else GRID_PASS // 2)
    assert sample.shape[0] >= 2500
    want = np.full(sample.shape[0], np.nan)
    with np.errstate(all='ignore'):
        for i, p in enumerate(sample.tolist()):
            res = sr.compute_group_reg_stats(samp, ctrl, start + p, start + p + 1, None, 0, 1, stat_type)
            assert (res is None) == (s_cov[p] < 1 or c_cov[p] < 1)
            if res is not None:
                want[i] = res[0][0]
    in_out = np.isin(sample, kept)
    assert in_out.sum() >= 2000 and not np.isnan(want[in_out]).any()
    _close(stats[np.searchsorted(kept, sample[in_out])], want[in_out], _rtol(stat_type))
    # every position: the entry on regions that each stay below half a pass
    at = 0
    for a, b in halves(n_pos, GRID_PASS // 2 - 1):
        assert 2 * (b - a) < GRID_PASS
        part = eng.group_level_stats(*kind, 0, 1, sub_region(pl, a, b), SMALLEST_PVAL)
        k = int(part[4][0])
        assert np.array_equal(bits(stats[at:at + k]), bits(part[0][:k])) and np.array_equal(poss[at:at + k], part[1][:k])
        at += k
    assert at == n


@pytest.mark.parametrize('n_pos', GROUP_SIZES)
@pytest.mark.parametrize('est_mean', [False, True])
def test_reads_ref_levels_second_pass(eng, n_pos, est_mean):
    assert 2 * n_pos > GRID_PASS
    pl, samp, ctrl = group_pileup(n_pos, one_group=True)
    reads, start = samp + ctrl, int(pl.reg_start[0])        # (the pileup's read order)
    lm, ls, cov = eng.reads_ref_levels(est_mean, 0, 1, pl, None, None, 0.0, 0.0)
    lv = sr.base_levels(reads, start, start + n_pos, None)
    want_cov = (~np.isnan(lv)).sum(axis=1)
    assert set(want_cov.tolist()) >= {1, 2, 3, 4}
    assert np.array_equal(cov, want_cov)
    sample = pass_sample(n_pos, 82, n_random=2500, pass_len=GRID_PASS if n_pos > GRID_PASS else GRID_PASS // 2)
    want_m, want_s = np.full(sample.shape[0], np.nan), np.full(sample.shape[0], np.nan)
    with np.errstate(all='ignore'):
        for i, p in enumerate(sample.tolist()):
            m, s, _ = sr.get_reads_ref(reads, start + p, start + p + 1, None, 1, 0, est_mean=est_mean)
            want_m[i], want_s[i] = m[0], s[0]
    assert sample.shape[0] >= 2500 and (~np.isnan(want_m)).sum() >= 2000
    _close(lm[sample], want_m, 0)
    _close(ls[sample], want_s, 0)
    for a, b in halves(n_pos, GRID_PASS // 2 - 1):
        part = eng.reads_ref_levels(est_mean, 0, 1, sub_region(pl, a, b), None, None, 0.0, 0.0)
        assert np.array_equal(bits(lm[a:b]), bits(part[0])) and np.array_equal(bits(ls[a:b]), bits(part[1]))
        assert np.array_equal(cov[a:b], part[2])


# ---- region_key_levels: k_region_pileup, k_kest_moments, k_kest_median over n_pos -------------------------------
@pytest.mark.parametrize('est_mean', [False, True])
def test_region_key_levels_positions_second_pass(eng, est_mean):
    """GRID_PASS + 1 listed positions of one region under three reads; the entries name the sampled positions (the
    stub's loop over positions then runs over those alone: an entry's pair depends on its own position only)"""
    n_pos = N
    assert n_pos > GRID_PASS
    rng = np.random.default_rng(90)
    spans = [(95, 7 * n_pos // 10, 0), (100 + n_pos // 3, n_pos - n_pos // 3 + 9, 1), (100 + n_pos // 2, n_pos // 2 + 7, 0)]
    means = [rng.normal(0, 1, n) for _, n, _ in spans]
    means[0][::37] = np.nan
    rs, rm = np.array([s for s, _, _ in spans], np.int64), np.array([m for _, _, m in spans], np.uint8)
    off = ts._csr_offsets([m.shape[0] for m in means])
    pos_g = 100 + np.arange(n_pos, dtype=np.int64)
    sample = pass_sample(n_pos, 91, n_random=5000)      # the entries: both ends of the passes, 5000 positions of the whole range
    assert sample.shape[0] >= 5000
    ent_pos = np.concatenate([sample, sample[::3]])[rng.permutation(sample.shape[0] + sample[::3].shape[0])]
    ent_key = rng.integers(0, 64, ent_pos.shape[0]).astype(np.int64)
    head = (est_mean, rs, rm, off, np.concatenate(means), np.array([0, 3], np.int64), np.arange(3, dtype=np.int64))
    got = eng.region_key_levels(*head, np.zeros(n_pos, np.int64), pos_g, ent_pos, ent_key, 64)
    want = est_stub.region_key_levels(*head, np.zeros(sample.shape[0], np.int64), pos_g[sample],
                                      np.searchsorted(sample, ent_pos), ent_key, n_keys=64)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(bits(got[2]), bits(want[2])) and np.array_equal(bits(got[3]), bits(want[3]))
    assert np.isnan(want[2]).sum() > 3 and (~np.isnan(want[2])).sum() > 5000
    assert {GRID_PASS - 1, GRID_PASS} <= set(ent_pos.tolist())


# ---- region_level_piles ---------------------------------------------------------------------------------------
def pile_region(n_pos, start=100):
    """one region of n_pos positions: a plus read over its first two thirds, a minus read from one third to its last
    position, a tenth of the levels NaN (dropped) -> (the arguments, the [n_pos, 2] levels by position and read)"""
    rng = np.random.default_rng(92)
    a_len, b0, b_len = (2 * n_pos) // 3, start + n_pos // 3, n_pos - n_pos // 3
    m = ref.full_mantissa(rng, a_len + b_len)
    m[rng.random(m.shape[0]) < 0.1] = np.nan
    m[[a_len - 1, a_len]] = (0.625, 0.375)            # the plus read's last level; the minus read's: the last position
    args = (np.array([start, b0], np.int64), np.array([0, 1], np.uint8), np.array([0, a_len, a_len + b_len], np.int64), m,
            np.array([0, 2], np.int64), np.array([0, 1], np.int64), np.array([start], np.int64), np.array([start + n_pos], np.int64))
    value = np.full((n_pos, 2), np.nan)
    value[:a_len, 0] = m[:a_len]
    value[n_pos // 3:, 1] = m[a_len:][::-1]
    return args, value


def test_region_level_piles_second_pass(eng):
    """test_pile_offsets_across_the_steps_of_the_prefix_kernel's construction with one position more than a pass (no
    read reaches its last fifth), and a region whose last position -- the one item of the second pass -- is covered:
    offsets and levels of every position from the levels laid out by position and read"""
    n_pos = N
    assert n_pos > GRID_PASS
    plot_tests.test_pile_offsets_across_the_steps_of_the_prefix_kernel(eng, n_pos)
    args, value = pile_region(n_pos)
    kept = ~np.isnan(value)
    cov = kept.sum(axis=1, dtype=np.int64)
    assert set(cov.tolist()) == {0, 1, 2} and cov[GRID_PASS] == 1 and value[GRID_PASS, 1] == 0.375
    off, levels, lin, near = eng.region_level_piles(*args)
    assert lin is None and near is None
    assert off.dtype == np.int64 and np.array_equal(off, np.concatenate([[0], np.cumsum(cov)]))
    assert np.array_equal(levels, value[kept])


def test_region_level_piles_percentiles_second_pass(eng):
    """the same region with fractions: k_plot_percentiles over n_pos * 3 items, the sorter over n_pos piles"""
    n_pos, start = N, 100
    args, _ = pile_region(n_pos, start)
    ql, qn = np.array([0.25, 0.5]), np.array([0.5])
    off, levels, lin, near = eng.region_level_piles(*args, q_linear=ql, q_nearest=qn)
    assert set(np.diff(off).tolist()) == {0, 1, 2}
    sample = pass_sample(n_pos, 93)
    assert sample.shape[0] >= 2000
    parts = [levels[off[p]:off[p + 1]] for p in sample.tolist()]
    want = ref.segment_percentiles(np.concatenate(parts), ts._csr_offsets([p.shape[0] for p in parts]), ql, qn)
    ref.same_bits(lin[sample], want[0])
    ref.same_bits(near[sample], want[1])
    for a, b in halves(n_pos, GRID_PASS // 3 - 1):
        assert 3 * (b - a) < GRID_PASS
        part = eng.region_level_piles(*(args[:6] + (np.array([start + a], np.int64), np.array([start + b], np.int64))),
                                      q_linear=ql, q_nearest=qn)
        ref.same_bits(part[0], off[a:b + 1] - off[a])
        ref.same_bits(part[1], levels[off[a]:off[b]])
        ref.same_bits(part[2], lin[a:b])
        ref.same_bits(part[3], near[a:b])


# ---- region_raw_signal ----------------------------------------------------------------------------------------
def test_region_raw_signal_second_pass(eng):
    """five reads of 5 500 bases with dwells of 20 - 60 samples, every strand / RNA combination, a pair per read over
    the whole read and two partial ones: more than GRID_PASS output samples for k_plot_sig_fill"""
    rng = np.random.default_rng(94)
    raws, segs = [], []
    for q in range(5):
        s = np.concatenate([[0], np.cumsum(rng.integers(20, 61, 5500))]).astype(np.int64) + q
        raws.append(rng.integers(-300, 2000, 17 + int(s[-1]) + q).astype(np.int16))
        segs.append(s)
    csr = lambda xs: ts._csr_offsets([len(x) for x in xs])   # noqa: E731
    f8 = lambda v: np.array(v, dtype=np.float64)             # noqa: E731
    rs = np.array([1000, 1200, 900, 5000, 40], np.int64)
    args = (np.concatenate(raws), csr(raws), np.concatenate(segs), csr(segs), rs, np.full(5, 17, np.int64),
            np.array([0, 1, 0, 1, 1], np.uint8), np.array([0, 0, 1, 1, 0], np.uint8), f8([400, 410, 395, 405, 402]),
            f8([70, 80, 75, 85, 90]), f8([-2.5, -2.0, np.nan, -2.2, -2.1]), f8([2.5, 2.0, np.nan, 2.2, 2.1]),
            np.array([0, 1, 2, 3, 4, 1, 3], np.int64), np.concatenate([rs, [1190, 6000]]).astype(np.int64),
            np.concatenate([rs + 5500, [3000, 12000]]).astype(np.int64))
    for genome_centric in (True, False):
        got = eng.region_raw_signal(*args, genome_centric=genome_centric)
        assert int(got[0][-1]) > GRID_PASS
        want = ref.raw_signal(*args, genome_centric=genome_centric)
        for g, w in zip(got, want):
            ref.same_bits(g, w)
        assert (want[2] == 2.5).any() and (want[2] == -2.0).any()       # clipped samples


# ---- normalize_raw_batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['int16', 'float64'])
def test_normalize_raw_batch_second_pass(eng, dtype):
    lens = [210001, 209999, 210000, 210003, 209000]
    assert sum(lens) > GRID_PASS > sum(lens[:4])
    raws = [nc.make_signal('noise', dtype, n + 30, 700 + i) for i, n in enumerate(lens)]
    # the samples at items GRID_PASS - 1 and GRID_PASS of the batch's output and the last one
    k = GRID_PASS - sum(lens[:4])
    raws[4][11 + k - 1], raws[4][11 + k], raws[4][11 + lens[4] - 1] = 7000, 513, -1500
    out = ts.normalize_raw_signal_batch(raws, [11] * 5, lens, 'median', 5.0)
    for raw, n, o in zip(raws, lens, out):
        norm, shift, scale, lower, upper = nc.normalize(raw, 11, n, 'median', 5.0, None, None)
        assert o[0].tobytes() == norm.tobytes()
        assert [np.float64(v).tobytes() for v in tuple(o[1])[:4]] == [np.float64(v).tobytes() for v in (shift, scale, lower, upper)]
        assert (norm == upper).any() and (norm == lower).any()
    last = out[4][0]
    assert last[k - 1] == out[4][1].upper_lim and last[-1] == out[4][1].lower_lim and abs(last[k]) < 1


# ---- genome tracks --------------------------------------------------------------------------------------------
def test_tracks_window_second_pass(eng):
    W, win_start = N, 1000
    assert W > GRID_PASS
    rng = np.random.default_rng(95)
    spans = [(0, 400, 0, 3), (3, 900, 1, 1), (GRID_PASS // 2, GRID_PASS // 2 + 5000, 0, 3), (GRID_PASS - 700, GRID_PASS - 100, 1, 3),
             (GRID_PASS - 300, N, 0, 2), (GRID_PASS - 50, N + 40, 1, 3), (-30, 20, 0, 3)]
    rstart = np.array([win_start + a for a, _, _, _ in spans], np.int64)
    rend = np.array([win_start + b for _, b, _, _ in spans], np.int64)
    flags = np.array([minus | (has << 1) for _, _, minus, has in spans], np.uint8)
    off = ts._csr_offsets(rend - rstart)
    slots = [ref.full_mantissa(rng, int(off[-1])) for _ in range(2)]
    toff, treads = th.build_tile_lists(rstart, rend, win_start, win_start + W, TRK_TILE)
    assert (rstart >= 0).all() and toff.shape[0] - 1 == -(-W // TRK_TILE)
    results = []
    for e in (eng, NumpyTracksEngine()):
        e.tracks_begin(win_start, win_start + W, 2)
        e.tracks_add(rstart, rend, flags, off, slots, toff, treads)
        results.append(e.tracks_finish(want_sums=True))
    got, want = results
    tc.same_bits(got.means, want.means)
    tc.same_bits(got.sums, want.sums)
    tc.exact(got.slot_cov, want.slot_cov)
    tc.exact(got.read_cov, want.read_cov)
    assert want.slot_cov[0, [0, GRID_PASS - 1, GRID_PASS]].tolist() == [2, 1, 1] and want.slot_cov[1, GRID_PASS] == 2
    assert want.read_cov[[0, 10, GRID_PASS]].tolist() == [2, 3, 2] and np.isnan(want.means[0, 2000])


def test_tracks_diff_and_topn_second_pass(eng):
    n = N
    assert n > GRID_PASS
    rng, stub = np.random.default_rng(96), NumpyTracksEngine()
    a, b = rng.integers(0, 12, n).astype(np.float64), rng.integers(0, 12, n).astype(np.float64)
    a[rng.random(n) < 0.1] = np.nan
    # winners on both sides of the pass, a tie across it and a tie at the cut of the four largest
    for p, v in ((5, 100.0), (GRID_PASS - 1, 90.0), (GRID_PASS, -90.0), (GRID_PASS - 2, 80.0), (100, -80.0)):
        a[p], b[p] = v, 0.0
    tc.same_bits(eng.tracks_diff(a, b), stub.tracks_diff(a, b))
    for k in (1, 3, 4, 5, 50, 3000):
        got, want = eng.tracks_topn(a, b, k), stub.tracks_topn(a, b, k)
        tc.same_bits(got[0], want[0])
        tc.exact(got[1], want[1])
    assert stub.tracks_topn(a, b, 4)[1].tolist() == [5, GRID_PASS, GRID_PASS - 1, GRID_PASS - 2]


# ---- the per-kernel C entries that launch grid_for(n) -----------------------------------------------------------
def test_c_entries_second_pass(eng):
    import oracle
    from tombo_amd import _c_dynamic_programming as cdp, _c_helper as ch
    n = N
    assert n > GRID_PASS
    rng = np.random.default_rng(97)
    sig = rng.normal(0.3, 1.0, n)
    sig[EDGE] = (0.3 + 0.35 * 9.0, 0.3 - 0.35 * 0.5)      # winsorised, inside
    z = cdp.c_base_z_scores(sig, 0.3, 0.35, True, 2.5)
    np.testing.assert_array_equal(z, oracle.base_z_scores(sig, 0.3, 0.35, True, 2.5))
    assert len(set(z[EDGE].tolist())) == 2
    np.testing.assert_array_equal(ch.c_apply_outlier_thresh(sig, -0.5, 0.75), oracle.apply_outlier_thresh(sig, -0.5, 0.75))
    lens = rng.integers(1, 4, n)
    segs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    long_sig = rng.normal(0, 1, int(segs[-1]) + 3) * np.exp(rng.normal(0, 2, int(segs[-1]) + 3))
    m, s = ch.c_new_mean_stds(long_sig, segs)
    want_m, want_s = oracle.new_mean_stds(long_sig, segs)
    np.testing.assert_array_equal(m, want_m)
    np.testing.assert_array_equal(s, want_s)


# ---- site_fractions_z / site_fractions_windows ------------------------------------------------------------------
def same_site_fractions(got, want, per_read_rtol):
    """the compacted per-site records of every track by bits, the per-read statistics under their tolerance"""
    assert np.array_equal(got.pos_off, want.pos_off) and np.array_equal(got.counts, want.counts)
    assert np.array_equal(got.n_stats, want.n_stats)
    for a, k in zip(got.pos_off[:-1].tolist(), got.counts.tolist()):
        assert k > 1000
        for name in ('frac', 'damp'):
            assert np.array_equal(bits(getattr(got, name)[a:a + k]), bits(getattr(want, name)[a:a + k])), name
        for name in ('poss', 'cov', 'valid'):
            assert np.array_equal(getattr(got, name)[a:a + k], getattr(want, name)[a:a + k]), name
    _close(got.per_read, want.per_read, per_read_rtol)


def test_site_fractions_z_second_pass(eng):
    """four reads whose bases total GRID_PASS + 1 on two tracks (three reads deep on the first): k_site_z and
    k_site_stat run one thread per base"""
    rng = np.random.default_rng(98)
    lens = [GRID_PASS // 4] * 3 + [N - 3 * (GRID_PASS // 4)]
    off = ts._csr_offsets(lens)
    assert int(off[-1]) == N > GRID_PASS
    trk_start, trk_end = np.array([1000, 50], np.int64), np.array([1000 + lens[3] + 20, 50 + lens[2]], np.int64)
    read_track, read_pos = np.array([0, 0, 1, 0], np.int64), np.array([1000, 1010, 50, 1020], np.int64)
    ref_m, ref_s = rng.normal(0, 1, N), np.abs(rng.normal(0.3, 0.05, N)) + 0.05
    z = rng.normal(0, 1.5, N)
    z[GRID_PASS - 3:GRID_PASS - 1], z[GRID_PASS - 1:] = 0.01, 3.5      # (the last base has no window: NaN)
    means = ref_m + z * ref_s
    means[rng.integers(0, N - 10, 50)] = np.nan
    args = (trk_start, trk_end, means, ref_m, ref_s, off, read_track, read_pos, 1, True, SMALLEST_PVAL, 0.4)
    kw = dict(lower_thresh=0.05, damp_counts=(2.0, 1.0), return_per_read=True)
    want = NumpyStatsEngine().site_fractions_z(*args, **kw)
    assert want.per_read[GRID_PASS - 2] > want.per_read[GRID_PASS - 1] > 0 and np.isnan(want.per_read[GRID_PASS])
    same_site_fractions(eng.site_fractions_z(*args, **kw), want, 1e-12)


def test_site_fractions_windows_second_pass(eng):
    """GRID_PASS + 1 windows of width 1 (the constant-variance ratio: no transcendental, bit-equal) on two tracks,
    four windows deep: k_site_win runs one thread per window"""
    rng = np.random.default_rng(99)
    n_windows = N
    assert n_windows > GRID_PASS
    n_site = GRID_PASS // 8
    trk_start, trk_end = np.array([700, 90], np.int64), np.array([700 + n_site + 1, 90 + n_site], np.int64)
    w = np.arange(n_windows, dtype=np.int64)
    win_track = (w % 2).astype(np.int64)
    win_pos = trk_start[win_track] + (w // 2) % n_site
    win_track[-1], win_pos[-1] = 0, 700 + n_site             # the one window of the second pass: a site of its own
    m, r = rng.normal(0, 1, n_windows), rng.normal(0, 1, n_windows)
    a = r + rng.choice([-1.0, 1.0], n_windows) * rng.uniform(0.2, 2.0, n_windows)
    rv = np.full(n_windows, 0.25)
    m[EDGE], a[EDGE] = r[EDGE] + (0.1, 0.9), r[EDGE] + 1.0
    args = (trk_start, trk_end, 1, m, r, a, rv, None, w, 1, win_track, win_pos, (4.0, 0.33, 0.33), 0.5)
    kw = dict(damp_counts=(1.0, 1.0), return_per_read=True)
    want = NumpyStatsEngine().site_fractions_windows(*args, **kw)
    assert want.counts.tolist() == [n_site + 1, n_site] and want.cov[n_site] == 1 and want.valid[n_site] == 1
    assert want.per_read[GRID_PASS - 1] * want.per_read[GRID_PASS] < 0
    same_site_fractions(eng.site_fractions_windows(*args, **kw), want, 0)

"""The region plot kernels of csrc/k_plot.h (Engine.region_level_piles, segment_percentiles, region_raw_signal)
against the live reference's recorded frames (tests/golden/stats_plot_data.npz, every case through
tombo_amd.plot_commands) and, beyond the fixture, against the numpy restatement that tests/test_plot_reference.py
pins to the same fixture.  Floats are compared by bits, without tolerance: the operations are IEEE add / subtract /
multiply / divide in a fixed order.

Shapes: segments of 0, 1, 2, 3 values and around the sorter classes of k_group.h (GRP_WAVE_MAX 64, GRP_LDS_MAX
4096) in one call; piles that cross 64 and one of 4 100 levels; bases of 1 and of 1 000 samples; 1 and 2 049 pairs
(past one block of the offsets scan)."""
import numpy as np
import pytest

import plot_cases as pcs
import plot_reference as ref
from tombo_amd import resquiggle as rq

pytestmark = pytest.mark.gpu

Q_LIN = np.true_divide([0, 1, 25, 50, 75, 99, 100], 100)
Q_NEAR = np.true_divide([0, 1, 10, 49, 50, 51, 99, 100], 100)
SEGMENT_SIZES = [0, 1, 2, 3, 63, 64, 65, 4095, 4096, 4097]


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


def same_outputs(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        ref.same_bits(g, w)


# ---- the fixture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', pcs.CASE_NAMES)
def test_frames_equal_the_reference(eng, case):
    pcs.check_case(eng, case)
    assert eng.last_plot_kernel_ms > 0.0


# ---- segment_percentiles ----------------------------------------------------------------------------------
def mixed_segments(rng):
    """every size class in one call, the large ones not next to each other; ties in every other segment"""
    sizes = [SEGMENT_SIZES[i] for i in (7, 0, 4, 9, 1, 5, 2, 8, 6, 3)]
    parts = [ref.full_mantissa(rng, n) if i % 2 else rng.integers(-40, 41, n) / 64.0 for i, n in enumerate(sizes)]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_segment_percentiles_across_the_sorter_classes(eng):
    values, off = mixed_segments(np.random.default_rng(5))
    before = values.copy()
    got = eng.segment_percentiles(values, off, Q_LIN, Q_NEAR)
    assert eng.last_plot_kernel_ms > 0.0 and np.array_equal(values, before)
    same_outputs(got, ref.segment_percentiles(values, off, Q_LIN, Q_NEAR))
    assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all()          # the empty segment
    same_outputs(eng.segment_percentiles(values, off, Q_LIN, Q_NEAR), got)  # the same bytes again
    for s, n in enumerate(np.diff(off).tolist()):                           # ... and numpy itself on a few of them
        if 0 < n <= 65:
            ref.same_bits(got[0][s], np.percentile(values[off[s]:off[s + 1]], Q_LIN * 100))
            ref.same_bits(got[1][s], np.percentile(values[off[s]:off[s + 1]], Q_NEAR * 100, method='nearest'))


def test_segment_percentiles_nan_segment_and_one_sided_fractions(eng):
    rng = np.random.default_rng(6)
    values = ref.full_mantissa(rng, 200)
    values[70] = np.nan
    off = np.array([0, 50, 130, 200], dtype=np.int64)
    lin, near = eng.segment_percentiles(values, off, Q_LIN, Q_NEAR)
    same_outputs((lin, near), ref.segment_percentiles(values, off, Q_LIN, Q_NEAR))
    assert np.isnan(lin[1]).all() and np.isnan(near[1]).all() and not np.isnan(lin[[0, 2]]).any()
    assert lin[0, 0] == values[:50].min() == near[0, 0] and lin[0, -1] == values[:50].max() == near[0, -1]   # q of 0 and 1
    only_lin = eng.segment_percentiles(values, off, Q_LIN, None)
    only_near = eng.segment_percentiles(values, off, np.empty(0), Q_NEAR)
    ref.same_bits(only_lin[0], lin)
    ref.same_bits(only_near[1], near)
    assert only_lin[1].shape == (3, 0) and only_near[0].shape == (3, 0)


# ---- region_level_piles -----------------------------------------------------------------------------------
def pile_batch(rng, n_regions, n_pos, cov_lo, cov_hi):
    """regions of n_pos positions 100 apart with cov_lo .. cov_hi reads each that hang over either end, lie inside
    or cover the region (every fiftieth region: cov_hi reads that all cover it); both strands; NaN levels; every third
    read is listed by two regions"""
    rs, rm, means, roff, rr, st, en = [], [], [], [0], [], [], []
    for r in range(n_regions):
        start = 1000 + 100 * r
        deep = r % 50 == 7                         # cov_hi reads that all span the region: piles of cov_hi levels
        for _ in range(cov_hi if deep else int(rng.integers(cov_lo, cov_hi + 1))):
            a = start + int(rng.integers(-8, 1 if deep else n_pos - 1))
            n = n_pos + 8 if deep else int(rng.integers(1, n_pos + 12))
            m = ref.full_mantissa(rng, n) if rng.random() < 0.7 else rng.integers(-40, 41, n) / 64.0
            m[rng.random(n) < (0.0 if deep else 0.05)] = np.nan
            if len(rs) % 3 == 0 and r > 0:
                rr.append(len(rs) - 1)               # a read of the region before (it may not reach this one)
            rr.append(len(rs))
            rs.append(a)
            rm.append(rng.random() < 0.5)
            means.append(m)
        roff.append(len(rr))
        st.append(start)
        en.append(start + n_pos)
    off = np.concatenate([[0], np.cumsum([m.shape[0] for m in means])]).astype(np.int64)
    return (np.array(rs, dtype=np.int64), np.array(rm, dtype=np.uint8), off, np.concatenate(means),
            np.array(roff, dtype=np.int64), np.array(rr, dtype=np.int64), np.array(st, dtype=np.int64),
            np.array(en, dtype=np.int64))


def check_piles(eng, args, q_linear=Q_LIN, q_nearest=Q_NEAR):
    pile_off, levels = ref.level_piles(*args)
    lin, near = ref.segment_percentiles(levels, pile_off, q_linear, q_nearest)
    got = eng.region_level_piles(*args, q_linear=q_linear, q_nearest=q_nearest)
    assert eng.last_plot_kernel_ms > 0.0
    same_outputs(got, (pile_off, levels, lin, near))
    return got


def test_one_region_of_one_position(eng):
    args = (np.array([7, 9, 3], dtype=np.int64), np.array([0, 1, 0], dtype=np.uint8), np.array([0, 4, 6, 9], dtype=np.int64),
            np.arange(9, dtype=np.float64) / 7, np.array([0, 3], dtype=np.int64), np.array([2, 0, 1], dtype=np.int64),
            np.array([9], dtype=np.int64), np.array([10], dtype=np.int64))
    off, levels, lin, near = check_piles(eng, args)
    assert off.tolist() == [0, 2] and levels.tolist() == [2 / 7, 5 / 7]      # read order; the minus read reversed


def test_many_regions_with_piles_across_64(eng):
    args = pile_batch(np.random.default_rng(11), 300, 21, 5, 70)
    got = check_piles(eng, args)
    sizes = np.diff(got[0])
    assert sizes.shape == (6300,) and sizes.min() < 5 and sizes.max() > 64
    same_outputs(eng.region_level_piles(*args, q_linear=Q_LIN, q_nearest=Q_NEAR), got)       # the same bytes again
    off2, levels2, lin2, near2 = eng.region_level_piles(*args, q_linear=Q_LIN, want_levels=False)
    assert levels2 is None and near2 is None
    same_outputs((off2, lin2), (got[0], got[2]))
    off3, levels3, lin3, near3 = eng.region_level_piles(*args)               # the piles alone (the density frame)
    assert lin3 is None and near3 is None
    same_outputs((off3, levels3), got[:2])


def test_one_position_with_4100_reads(eng):
    rng = np.random.default_rng(12)
    n = 4100
    args = (np.full(n, 50, dtype=np.int64), (rng.random(n) < 0.5).astype(np.uint8), np.arange(n + 1, dtype=np.int64),
            ref.full_mantissa(rng, n), np.array([0, n], dtype=np.int64), rng.permutation(n).astype(np.int64),
            np.array([50], dtype=np.int64), np.array([51], dtype=np.int64))
    off, levels, lin, near = check_piles(eng, args)
    assert off.tolist() == [0, n] and np.array_equal(levels, args[3][args[5]])


@pytest.mark.parametrize('n_pos', [1, 63, 64, 65, 255, 256, 257, 513, 65537])
def test_pile_offsets_across_the_steps_of_the_prefix_kernel(eng, n_pos):
    """one region whose positions end on either side of a wavefront (64), of one 256-wide step of the exclusive
    prefix, of two steps, and far beyond; a plus read over its first two thirds and a minus read over its middle,
    so a position has 0, 1 or 2 levels, some of them NaN (dropped): the offsets are the running sum of the
    coverage and the levels stand in read order"""
    start = 100
    a0, a_len = start - 3, 3 + (2 * n_pos + 2) // 3                 # read 0, '+': positions [0, (2 n + 2) / 3)
    b0, b_len = start + n_pos // 3, n_pos - n_pos // 3 - n_pos // 5   # read 1, '-': positions [n / 3, n - n / 5)
    a, b = np.arange(a_len, dtype=np.float64), 1e6 + np.arange(b_len, dtype=np.float64)
    a[::7] = np.nan
    b[::5] = np.nan
    args = (np.array([a0, b0], dtype=np.int64), np.array([0, 1], dtype=np.uint8),
            np.array([0, a_len, a_len + b_len], dtype=np.int64), np.concatenate([a, b]), np.array([0, 2], dtype=np.int64),
            np.array([0, 1], dtype=np.int64), np.array([start], dtype=np.int64), np.array([start + n_pos], dtype=np.int64))
    g = start + np.arange(n_pos, dtype=np.int64)
    value = np.full((n_pos, 2), np.nan)
    for k, (r0, genome_order) in enumerate(((a0, a), (b0, b[::-1]))):
        inside = (g >= r0) & (g < r0 + genome_order.shape[0])
        value[inside, k] = genome_order[g[inside] - r0]
    kept = ~np.isnan(value)
    cov = kept.sum(axis=1, dtype=np.int64)
    if n_pos >= 63:
        assert set(cov.tolist()) == {0, 1, 2}
    off, levels, lin, near = eng.region_level_piles(*args)
    assert lin is None and near is None
    assert off.dtype == np.int64 and np.array_equal(off, np.concatenate([[0], np.cumsum(cov)]))
    assert np.array_equal(levels, value[kept])


def test_regions_without_a_covering_read(eng):
    args = list(pile_batch(np.random.default_rng(13), 4, 11, 3, 6))
    args[6] = args[6] + np.array([0, 5000, 0, 5000])        # two regions moved away from their reads
    args[7] = args[7] + np.array([0, 5000, 0, 5000])
    args[4] = np.concatenate([args[4], args[4][-1:]])       # and a region without any read
    args[6], args[7] = np.concatenate([args[6], [20]]), np.concatenate([args[7], [24]])
    off, levels, lin, near = check_piles(eng, tuple(args))
    sizes = np.diff(off)
    assert sizes[11:22].sum() == 0 and sizes[33:].sum() == 0 and sizes[:11].sum() > 0
    assert np.isnan(lin[11:22]).all() and np.isnan(near[44:]).all()


# ---- region_raw_signal ------------------------------------------------------------------------------------
def signal_batch(rng, n_reads, n_pair, raw_dtype, long_base=False):
    """reads of 4 .. 30 bases with dwells of 1 .. 12 samples (long_base: one base of 1 000 samples in every fourth
    read), every strand / RNA combination, every fourth read without limits; pairs whose region starts before, at or
    inside the read and ends inside, at or past it"""
    raws, segs, rs, rsr, mn, rn, sh, sc, lo, hi = [], [], [], [], [], [], [], [], [], []
    for q in range(n_reads):
        nb = int(rng.integers(4, 31))
        dwell = rng.integers(1, 13, nb)
        dwell[rng.random(nb) < 0.3] = 1
        if long_base and q % 4 == 0:
            dwell[int(rng.integers(0, nb))] = 1000
        s = np.concatenate([[0], np.cumsum(dwell)]).astype(np.int64) + int(rng.integers(0, 3))
        rsrtr = int(rng.integers(0, 30))
        raws.append(rng.integers(-300, 2000, rsrtr + int(s[-1]) + int(rng.integers(0, 9))).astype(raw_dtype))
        segs.append(s)
        rs.append(int(rng.integers(0, 500)))
        rsr.append(rsrtr)
        mn.append(q % 2)
        rn.append((q // 2) % 2)
        sh.append(400 + rng.standard_normal() * 9)
        sc.append(70 + rng.random() * 20)
        lo.append(np.nan if q % 4 == 3 else -2.0 - rng.random())
        hi.append(np.nan if q % 4 == 3 else 2.0 + rng.random())
    pr = rng.integers(0, n_reads, n_pair).astype(np.int64)
    pr[:min(n_reads, n_pair)] = np.arange(min(n_reads, n_pair))
    nb = np.array([s.shape[0] - 1 for s in segs])[pr]
    start = np.array(rs)[pr]
    ps = start + rng.integers(-6, nb)                        # before the read .. its last base
    pe = np.maximum(ps, start) + 1 + rng.integers(0, nb + 6)
    ps[::7], pe[1::7] = start[::7], (start + nb)[1::7]       # exactly at the read's start / end
    pe = np.maximum(pe, np.maximum(ps, start) + 1)
    csr = (lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64))
    u8, f8 = (lambda v: np.array(v, dtype=np.uint8)), (lambda v: np.array(v, dtype=np.float64))
    return (np.concatenate(raws), csr(raws), np.concatenate(segs), csr(segs), np.array(rs, dtype=np.int64),
            np.array(rsr, dtype=np.int64), u8(mn), u8(rn), f8(sh), f8(sc), f8(lo), f8(hi), pr, ps.astype(np.int64),
            pe.astype(np.int64))


@pytest.mark.parametrize('raw_dtype,n_reads,n_pair,long_base', [
    (np.int16, 1, 1, False), (np.int32, 1, 1, True), (np.int16, 40, 300, True), (np.int32, 40, 300, False),
    (np.int16, 64, 2049, False)])
def test_raw_signal_pairs(eng, raw_dtype, n_reads, n_pair, long_base):
    args = signal_batch(np.random.default_rng(n_pair + long_base), n_reads, n_pair, raw_dtype, long_base)
    for genome_centric in (True, False):
        got = eng.region_raw_signal(*args, genome_centric=genome_centric)
        assert eng.last_plot_kernel_ms > 0.0
        same_outputs(got, ref.raw_signal(*args, genome_centric=genome_centric))
        same_outputs(eng.region_raw_signal(*args, genome_centric=genome_centric), got)       # the same bytes again
    if n_pair > 1:
        ps, pe, start = args[13], args[14], args[4][args[12]]
        assert (ps > start).any() and (ps < start).any() and (pe < start + 4).any()          # start offsets, early ends


def test_raw_signal_int16_and_int32_agree(eng):
    args = signal_batch(np.random.default_rng(3), 8, 20, np.int16)
    wide = (args[0].astype(np.int32),) + args[1:]
    same_outputs(eng.region_raw_signal(*wide), eng.region_raw_signal(*args))


# ---- empty inputs: arrays of the right dtype and shape, nothing launched ----------------------------------
def test_zero_regions_pairs_and_fractions(eng):
    i8, f8 = np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float64)
    zero = np.zeros(1, dtype=np.int64)
    eng.last_plot_kernel_ms = -1.0
    off, levels, lin, near = eng.region_level_piles(i8, np.empty(0, dtype=np.uint8), zero, f8, zero, i8, i8, i8, Q_LIN, Q_NEAR)
    assert off.tolist() == [0] and off.dtype == np.int64 and levels.shape == (0,) and levels.dtype == np.float64
    assert lin.shape == (0, 7) and near.shape == (0, 8) and lin.dtype == near.dtype == np.float64
    assert eng.last_plot_kernel_ms == 0.0
    lin, near = eng.segment_percentiles(f8, zero, Q_LIN, Q_NEAR)
    assert lin.shape == (0, 7) and near.shape == (0, 8) and eng.last_plot_kernel_ms == 0.0
    lin, near = eng.segment_percentiles(np.arange(3.0), np.array([0, 3], dtype=np.int64), None, None)
    assert lin.shape == (1, 0) and near.shape == (1, 0) and eng.last_plot_kernel_ms == 0.0
    args = signal_batch(np.random.default_rng(4), 3, 2, np.int16)
    sig_off, position, signal, base_i = eng.region_raw_signal(*(args[:12] + (i8, i8, i8)))
    assert sig_off.tolist() == [0] and position.shape == signal.shape == base_i.shape == (0,)
    assert (position.dtype, signal.dtype, base_i.dtype) == (np.float64, np.float64, np.int64)
    assert eng.last_plot_kernel_ms == 0.0
    sig_off, _, _, _ = eng.region_raw_signal(np.empty(0, dtype=np.int16), zero, i8, zero, i8, i8, np.empty(0, dtype=np.uint8),
                                             np.empty(0, dtype=np.uint8), f8, f8, f8, f8, i8, i8, i8)
    assert sig_off.tolist() == [0]
    # a pile call without fractions still gives the piles
    off, levels, lin, near = eng.region_level_piles(*pile_batch(np.random.default_rng(14), 2, 5, 2, 3))
    assert lin is None and near is None and off.shape == (11,) and levels.shape == (off[-1],)


# ---- the C entries check again what the binding checks ----------------------------------------------------
def test_c_entries_refuse_bad_indices_without_a_launch(eng):
    import ctypes as C
    from tombo_amd import _native
    ms = C.c_double(-1.0)

    def piles(**change):
        a = dict(zip(('rs', 'rm', 'off', 'm', 'roff', 'rr', 'st', 'en'), pile_batch(np.random.default_rng(15), 2, 5, 2, 3)))
        a.update(ql=Q_LIN, qn=Q_NEAR)
        a.update(change)
        n_pos = 10
        out_off, lv = np.zeros(n_pos + 1, dtype=np.int64), np.empty(1000)
        lin, near = np.empty((n_pos, a['ql'].shape[0])), np.empty((n_pos, a['qn'].shape[0]))
        eng._call('tba_region_level_piles', a['rs'].shape[0], a['rs'], a['rm'], a['off'], a['m'], a['st'].shape[0], a['roff'],
                  a['rr'], a['st'], a['en'], a['ql'].shape[0], a['ql'], a['qn'].shape[0], a['qn'], out_off, lv, 1000, lin, near,
                  C.byref(ms))

    piles()
    assert ms.value > 0.0
    good = pile_batch(np.random.default_rng(15), 2, 5, 2, 3)
    for change in (dict(rr=np.where(np.arange(good[5].shape[0]) == 1, 99, good[5])), dict(rr=good[5] - 1),
                   dict(en=good[6].copy()), dict(roff=good[4][::-1].copy()), dict(off=good[2] + 1), dict(ql=np.array([1.5])),
                   dict(qn=np.array([np.nan])), dict(st=good[6] - 2 ** 62)):
        with pytest.raises(_native.EngineError, match=r'\(-1\)'):
            piles(**change)
        assert ms.value == 0.0

    def signal(raw_bytes=2, **change):
        names = ('raw', 'roff', 'segs', 'soff', 'rs', 'rsr', 'mn', 'rn', 'sh', 'sc', 'lo', 'hi', 'pr', 'ps', 'pe')
        a = dict(zip(names, signal_batch(np.random.default_rng(16), 3, 4, np.int16)))
        a.update(change)
        sig_off = np.zeros(a['pr'].shape[0] + 1, dtype=np.int64)
        pos, sig, base = np.empty(5000), np.empty(5000), np.empty(5000, dtype=np.int64)
        eng._call('tba_region_raw_signal', a['rs'].shape[0], C.c_void_p(a['raw'].ctypes.data), raw_bytes, a['roff'], a['segs'],
                  a['soff'], a['rs'], a['rsr'], a['mn'], a['rn'], a['sh'], a['sc'], a['lo'], a['hi'], a['pr'].shape[0], a['pr'],
                  a['ps'], a['pe'], 1, sig_off, pos, sig, base, 5000, C.byref(ms))

    signal()
    assert ms.value > 0.0
    good = signal_batch(np.random.default_rng(16), 3, 4, np.int16)
    for change in (dict(pr=good[12] + 3), dict(pr=good[12] - 3), dict(pe=good[13].copy()), dict(ps=good[13] + 10 ** 6, pe=good[14] + 10 ** 6),
                   dict(segs=good[2] + 10 ** 6), dict(segs=good[2][::-1].copy()), dict(rsr=good[5] - 100), dict(raw_bytes=3),
                   dict(soff=np.arange(4, dtype=np.int64))):
        with pytest.raises(_native.EngineError, match=r'\(-1\)'):
            signal(**change)
        assert ms.value == 0.0

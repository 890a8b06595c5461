"""tests/plot_reference.py (the numpy restatement of the region plot arithmetic) against the live reference's
recorded frames (tests/golden/stats_plot_data.npz) and against np.percentile itself, bit for bit.  CPU only.  The
restatement is then the yardstick of the GPU tests beyond the fixture (tests/test_gpu_plot_data.py)."""
import numpy as np
import pytest

import plot_cases as pcs
import plot_reference as ref

BOX_Q = np.true_divide([0, 25, 50, 75, 100], 100)


def packed_levels(regs):
    """engine-layout arrays of the regions' level reads (every read once per region)"""
    rs, rm, means, roff, rr, st, en = [], [], [], [0], [], [], []
    for reg in regs:
        for rd in reg.level_reads():
            rr.append(len(rs))
            rs.append(rd.start)
            rm.append(rd.strand == '-')
            means.append(rd.means)
        roff.append(len(rr))
        st.append(reg.start)
        en.append(reg.end)
    off = np.concatenate([[0], np.cumsum([m.shape[0] for m in means])]).astype(np.int64)
    return (np.array(rs, dtype=np.int64), np.array(rm, dtype=np.uint8), off, np.concatenate(means),
            np.array(roff, dtype=np.int64), np.array(rr, dtype=np.int64), np.array(st, dtype=np.int64),
            np.array(en, dtype=np.int64))


def typed_regions(case, plot_type):
    """the regions of a recorded single-sample case that got plot_type, with their reads"""
    info = pcs.gold()['meta']['cases'][case]
    index = pcs.reads_index(0)
    regs = [r for r in (p.add_reads(index) for p in pcs.intervals(info['regions'])) if len(r.reads) > 0]
    assert len(regs) == len(info['plot_types'])
    return [r for r, t in zip(regs, info['plot_types']) if t == plot_type]


@pytest.mark.parametrize('n', [1, 2, 3, 4, 51, 64, 65, 151, 1000])
def test_percentile_forms_equal_numpy(n):
    rng = np.random.default_rng(n)
    qs = np.true_divide([0, 1, 5, 10, 25, 33, 49, 50, 51, 75, 90, 99, 100], 100)
    for v in (ref.full_mantissa(rng, n), rng.integers(-40, 41, n) / 64.0):
        lin, near = ref.segment_percentiles(v, np.array([0, n], dtype=np.int64), qs, qs)
        ref.same_bits(lin[0], np.percentile(v, qs * 100))
        ref.same_bits(near[0], np.percentile(v, qs * 100, method='nearest'))
    # the fractions the frames pass are what np.percentile divides out
    ref.same_bits(ref.segment_percentiles(v, np.array([0, n], dtype=np.int64), BOX_Q, BOX_Q[:0])[0][0],
                  np.array([np.percentile(v, q) for q in (0, 25, 50, 75, 100)]))


def test_round_half_even_shows_at_51_and_151():
    """(n - 1) * 0.01 is 0.5 and 1.5: 'nearest' takes elements 0 and 2"""
    for n, k in ((51, 0), (151, 2)):
        v = np.arange(n, dtype=np.float64)[::-1].copy()
        assert ref.percentile_nearest(v, np.true_divide(1, 100)) == k == np.percentile(v, 1, method='nearest')


def test_nan_and_empty_segments_give_nan_rows():
    v = np.array([1.0, np.nan, 3.0, 2.0, 5.0])
    lin, near = ref.segment_percentiles(v, np.array([0, 3, 3, 5], dtype=np.int64), BOX_Q, BOX_Q[:2])
    assert np.isnan(lin[:2]).all() and np.isnan(near[:2]).all()
    assert np.isnan(np.percentile(v[:3], 50))
    ref.same_bits(lin[2], np.percentile(v[3:], BOX_Q * 100))


def test_base_levels_equal_the_recorded_matrices():
    g = pcs.gold()
    for key, which, transpose in (('base_levels|all', 2, False), ('base_levels|rows', 1, True)):
        reg = pcs.intervals([which])[0].add_reads(pcs.reads_index(0))
        rs, rm, off, m, roff, rr, st, en = packed_levels([reg])
        got = ref.base_levels(rs, rm, off, m, rr.tolist(), reg.start, reg.end)
        ref.same_bits(got.T if transpose else got, g[key])


def test_box_numbers_equal_the_recorded_frame():
    g = pcs.gold()
    regs = typed_regions('boxplot', 'Boxplot')
    rs, rm, off, m, roff, rr, st, en = packed_levels(regs)
    pile_off, levels = ref.level_piles(rs, rm, off, m, roff, rr, st, en)
    lin, _ = ref.segment_percentiles(levels, pile_off, BOX_Q, BOX_Q[:0])
    rows, first = [], 0
    for reg in regs:
        kept = np.flatnonzero(np.diff(pile_off[first:first + reg.end - reg.start + 1]) > 0) + first
        rows += [kept for strand in '+-' if any(rd.strand == strand for rd in reg.reads)]
        first += reg.end - reg.start
    rows = np.concatenate(rows)
    for j, col in enumerate(('SigMin', 'Sig25', 'SigMed', 'Sig75', 'SigMax')):
        ref.same_bits(lin[rows, j], g['boxplot|Box|%s' % col])


def test_quantile_numbers_equal_the_recorded_frame():
    g = pcs.gold()
    regs = typed_regions('quantile', 'Quantile')
    pile_off, levels = ref.level_piles(*packed_levels(regs))
    qn = np.concatenate([np.true_divide([1, 10, 20, 30, 40, 49], 100), np.true_divide([99, 90, 80, 70, 60, 51], 100)])
    _, near = ref.segment_percentiles(levels, pile_off, qn[:0], qn)
    assert set(np.diff(pile_off).tolist()) >= {51, 151}
    rows, first = [], 0
    for reg in regs:
        kept = np.flatnonzero(np.diff(pile_off[first:first + reg.end - reg.start + 1]) > 0) + first
        rows += [kept for strand in '+-' if any(rd.strand == strand for rd in reg.reads)]
        first += reg.end - reg.start
    rows = np.concatenate(rows)
    ref.same_bits(near[rows, :6].reshape(-1), g['quantile|Quant|Lower'])
    ref.same_bits(near[rows, 6:].reshape(-1), g['quantile|Quant|Upper'])


def test_density_levels_equal_the_recorded_frame():
    g = pcs.gold()
    parts = [reg.copy(include_reads=False).update(reads=[rd for rd in reg.reads if rd.strand == strand])
             for reg in typed_regions('density', 'Density') for strand in '+-'
             if any(rd.strand == strand for rd in reg.reads)]
    pile_off, levels = ref.level_piles(*packed_levels(parts))
    sizes = np.diff(pile_off)
    keep = np.repeat(sizes >= 2, sizes)
    ref.same_bits(levels[keep], g['density|Event|Signal'])


@pytest.mark.parametrize('case', ['signal', 'rna'])
def test_raw_signal_equals_the_recorded_frame(case):
    g = pcs.gold()
    regs = typed_regions(case, 'Signal')
    reads, pairs = [], []
    for reg in regs:
        for rd in reg.reads:
            if rd.raw_signal is not None:
                pairs.append((len(reads), reg.start, reg.end))
                reads.append(rd)
    csr = (lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64))
    f8 = (lambda vs: np.array([np.nan if v is None else v for v in vs], dtype=np.float64))
    sig_off, position, signal, base_i = ref.raw_signal(
        np.concatenate([rd.raw_signal for rd in reads]), csr([rd.raw_signal for rd in reads]),
        np.concatenate([rd.segs for rd in reads]), csr([rd.segs for rd in reads]),
        np.array([rd.start for rd in reads]), np.array([rd.read_start_rel_to_raw for rd in reads]),
        np.array([rd.strand == '-' for rd in reads]), np.array([rd.rna for rd in reads]),
        f8([rd.scale_values.shift for rd in reads]), f8([rd.scale_values.scale for rd in reads]),
        f8([rd.scale_values.lower_lim for rd in reads]), f8([rd.scale_values.upper_lim for rd in reads]),
        np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]), np.array([p[2] for p in pairs]))
    ref.same_bits(position, g['%s|Signal|Position' % case])
    ref.same_bits(signal, g['%s|Signal|Signal' % case])
    assert sig_off[-1] == position.shape[0] == base_i.shape[0]

"""The host layer of the most-significant-sites family (tombo_stats.get_pairwise_dists, transform_and_trim_stats,
order_reads, ModelStats.iter_stat_seqs, cluster_most_signif_dists, tombo_helper.get_unique_intervals,
text_output.write_most_signif) on the numpy stand-in engine of tests/pdist_stub_engine.py, against the live
reference's recorded results (tests/golden/stats_pdist.npz).  No GPU."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

import pdist_cases as pc
import pdist_reference as ref
from pdist_stub_engine import NumpyPdistEngine
from tombo_amd import tombo_stats as ts, tombo_helper as th, _native


@pytest.fixture()
def eng():
    return NumpyPdistEngine()


@pytest.mark.parametrize('name,slide_span', pc.WINDOW_CASES)
def test_get_pairwise_dists(eng, name, slide_span):
    pc.check_window_case(eng, name, slide_span)
    assert eng.calls == [('window',) + pc.gold()['%s_rows' % name].shape]     # one engine call for the matrix


def test_single_pair_forms():
    g = pc.gold()
    rows = g['w27_rows']
    assert ts.euclidian_dist(rows[5], rows[3]) == g['w27_dists_s0'][5, 3]
    assert ts.sliding_window_dist(rows[5], rows[3], 3, 21) == g['w27_dists_s3'][5, 3]


def test_slide_span_none_is_zero(eng):
    rows = pc.gold()['w27_rows']
    with np.errstate(all='ignore'):
        ref.same_bits(ts.get_pairwise_dists(rows, None, engine=eng), pc.gold()['w27_dists_s0'])


def test_unequal_rows_name_the_first_short_row(eng):
    rows = [np.zeros(27), np.zeros(27), np.zeros(20), np.zeros(19)]
    with pytest.raises(th.TomboError, match=r'^Region 2 holds 20 signal differences where the first region holds 27'):
        ts.get_pairwise_dists(rows, 3, engine=eng)
    assert eng.calls == []


def test_no_window_left(eng):
    with pytest.raises(th.TomboError, match=r'^Regions of 6 bases leave no window with a slide span of 3\.$'):
        ts.get_pairwise_dists(np.zeros((3, 6)), 3, engine=eng)
    with pytest.raises(th.TomboError, match='^No regions'):
        ts.get_pairwise_dists([], 0, engine=eng)
    assert eng.calls == []
    with pytest.raises(ValueError, match='slide_span'):
        eng.pairwise_window_dists(np.zeros((3, 6)), 3)
    with pytest.raises(ValueError, match='float64'):
        eng.pairwise_window_dists(np.zeros((3, 6), dtype=np.float32))
    with pytest.raises(ValueError, match='contiguous'):
        eng.pairwise_nanmean_dists(np.zeros((6, 3)).T)
    with pytest.raises(ValueError, match='at least one'):
        eng.pairwise_nanmean_dists(np.zeros((0, 3)))
    with pytest.raises(ValueError, match='at most'):
        eng.pairwise_nanmean_dists(np.zeros((_native.PDIST_MAX_ROWS + 1, 1)))


@pytest.mark.parametrize('name,are_pvals,trim', [('pvals', True, 'pval_trim'), ('llrs', False, 'llr_trim')])
def test_transform_and_trim_stats(name, are_pvals, trim):
    g = pc.gold()
    given = g[name].copy()
    with np.errstate(all='ignore'):
        got = ts.transform_and_trim_stats(given, are_pvals, pc.meta()[trim])
    ref.same_bits(got, g['%s_trimmed' % name])
    ref.same_bits(given, g['%s_after' % name])        # likelihood ratios are trimmed in place, p-values are not
    assert (got is given) == (not are_pvals)


@pytest.mark.parametrize('name', ['pvals', 'llrs'])
def test_order_reads(eng, name):
    pytest.importorskip('scipy')
    pc.check_order_reads(eng, name)


def test_order_reads_of_one_read(eng):
    assert ts.order_reads(pc.gold()['llrs_trimmed'][:1], engine=eng) == [0] == pc.gold()['one_read_leaves'].tolist()
    assert eng.calls == []


def test_order_reads_without_scipy(eng, monkeypatch):
    monkeypatch.setitem(sys.modules, 'scipy.cluster.hierarchy', None)     # (import of it raises ImportError)
    with pytest.raises(th.TomboError, match='needs scipy'):
        ts.order_reads(pc.gold()['llrs_trimmed'], engine=eng)
    assert eng.calls == []


@pytest.mark.parametrize('key', sorted(pc.meta()['iter_stat_seqs']))
def test_iter_stat_seqs(key):
    before, after = (int(v) for v in key.split('_'))
    want = pc.meta()['iter_stat_seqs'][key]
    stats = pc.open_stats()
    got = list(stats.iter_stat_seqs(pc.genome(), before, after))
    assert [[s, c, st, int(a), int(b)] for s, c, st, a, b in got] == want['with_pos']
    assert list(stats.iter_stat_seqs(pc.genome(), before, after, include_pos=False)) == want['seqs']
    if (before, after) != (0, 0):       # windows that leave a chromosome at either end are skipped
        assert len(got) < len(stats.most_signif_stats)


def test_get_unique_intervals():
    u = pc.meta()['unique_intervals']
    stats = pc.open_stats()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        regions = stats.get_most_signif_regions(11, 40)
        overlapping = stats.get_most_signif_regions(11, 40, unique_pos=False)
    rows = lambda regs: [list(r) for r in regs]
    assert rows(regions) == u['regions'] and rows(overlapping) == u['overlapping_regions']
    g = pc.gold()
    covered = dict(((chrm, strand), set(np.flatnonzero(g['covered|%s|%s' % (chrm, strand)]).tolist()))
                   for chrm in pc.meta()['chrm_lens'] for strand in '+-')
    assert rows(th.get_unique_intervals(regions)) == u['plain']
    assert rows(th.get_unique_intervals(regions, covered)) == u['covered']
    assert rows(th.get_unique_intervals(regions, covered, 5)) == u['covered_5']
    assert rows(th.get_unique_intervals(regions, None, 3)) == u['plain_3']
    assert rows(th.get_unique_intervals(overlapping)) == u['overlapping_plain']
    # the boolean tracks cluster_most_signif_dists uses answer `in` as the sets do
    tracks = ts._CoveredByBoth(((cs, ts._CoveredPositions(g['covered|%s|%s' % cs])) for cs in covered))
    assert rows(th.get_unique_intervals(regions, tracks)) == u['covered']
    assert -1 not in tracks[('chrA', '+')] and 10 ** 6 not in tracks[('chrA', '+')] and 5 not in tracks[('chrZ', '+')]


@pytest.mark.parametrize('key', sorted(pc.meta()['most_signif_text']))
def test_write_most_signif(key):
    source, num_regions, num_bases = key.split('_')
    assert pc.most_signif_text(source, int(num_regions), int(num_bases)) == pc.meta()['most_signif_text'][key]


def test_write_most_signif_of_an_empty_file():
    import io
    want = pc.meta()['empty_text']
    from tombo_amd import text_output
    with pytest.raises(th.TomboError) as exc:
        text_output.write_most_signif(pc.open_stats(empty=True), io.StringIO(), 5, 9, genome_index=pc.genome())
    assert str(exc.value) in want and str(exc.value) == 'No locations identified. Most likely an empty statistics file.'
    with pytest.raises(th.TomboError, match='^Must provide either reads or a genome FASTA'):
        text_output.write_most_signif(pc.open_stats(), io.StringIO(), 5, 9)


# ---- cluster_most_signif_dists: the reference's statements over the recorded pieces -----------------------
class LevelRead(pc.Read):
    pass


def level_reads(rng, shift, min_start=0):
    """the recorded reads (those from min_start on) with levels: a function of the position, the sample shifted at
    some positions"""
    index = {}
    for chrm, strand, start, end, seq in pc.meta()['reads']:
        if start < min_start:
            continue
        rd = LevelRead(chrm, strand, start, end, seq)
        pos = np.arange(start, end)
        lv = np.sin(pos * 0.37) + (pos % 7) / 64.0 + shift * ((pos // 9) % 3) + rng.standard_normal(end - start) * 1e-3
        rd.means = lv if strand == '+' else lv[::-1].copy()
        index.setdefault((chrm, strand), []).append(rd)
    return index


@pytest.mark.parametrize('slide_span,with_fasta', [(0, True), (2, False)])
def test_cluster_most_signif_dists(eng, slide_span, with_fasta):
    rng = np.random.default_rng(3)
    # (no control read below 8: a region that starts at 0 cannot be widened by two bases, see the next test)
    samp, ctrl = level_reads(rng, 0.5), level_reads(rng, 0.0, min_start=8)
    del ctrl[('chrB', '+')]                 # significant regions there have no control: covered by one set only
    stats, num_bases, width = pc.open_stats(), 7, 7 + 2 * slide_span
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dists, intervals, names = ts.cluster_most_signif_dists(
            stats, samp, ctrl, 40, num_bases, slide_span, genome_index=pc.genome() if with_fasta else None,
            with_seqs=True, engine=eng)
        regions = stats.get_most_signif_regions(width, 40)
    # the reference's statements (_plot_commands.py:2133-2173) over sets of positions
    cov, ctrl_cov = th.compute_coverage(samp, engine=eng), th.compute_coverage(ctrl, engine=eng)
    covered = dict((cs, set(np.flatnonzero(cov[cs] > 0).tolist()) & set(np.flatnonzero(ctrl_cov[cs] > 0).tolist()))
                   for cs in set(cov) & set(ctrl_cov))
    for cs in set(r[0::3][:2] for r in regions):
        covered.setdefault(cs, set())
    want = th.get_unique_intervals(regions, covered)
    assert intervals == want and 2 < len(want) < len(regions)
    assert all(r[0::3][:2] != ('chrB', '+') for r in intervals)
    diffs = th.get_signal_differences(samp, ctrl, engine=eng)
    rows = np.stack([diffs[(c, st)][a:a + width] for c, a, _, st, _, _ in want])
    ref.same_bits(dists, ref.window_dists_loops(rows, slide_span))
    assert dists.shape == (len(want),) * 2 and np.any(dists[np.tril_indices(len(want), -1)] > 0)
    for name, (chrm, start, _, strand, _, _) in zip(names, want):
        seq, c, st, one_based = name.split('::')
        assert (c, st, int(one_based)) == (chrm, strand, start + 1) and len(seq) == width + 4
        assert seq == pc.genome().get_seq(chrm, start - 2, start + 2 + width)   # (covered by reads: no '-')
    assert ts.cluster_most_signif_dists(stats, samp, ctrl, 3, num_bases, slide_span, engine=eng)[2] is None


def test_cluster_most_signif_dists_region_at_a_chromosome_start(eng):
    """the reference widens every region by two bases for its column names and asks the genome index for them: a
    region that starts at 0 is refused there (th.TomboError), and here; without names it is computed"""
    rng = np.random.default_rng(5)
    samp, ctrl = level_reads(rng, 0.5), level_reads(rng, 0.0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dists, intervals, names = ts.cluster_most_signif_dists(pc.open_stats(), samp, ctrl, 40, 7, engine=eng)
        assert names is None and any(r[1] == 0 for r in intervals) and dists.shape[0] == len(intervals)
        with pytest.raises(th.TomboError, match='invalid genome sequence request'):
            ts.cluster_most_signif_dists(pc.open_stats(), samp, ctrl, 40, 7, genome_index=pc.genome(), with_seqs=True,
                                         engine=eng)


def test_cluster_most_signif_dists_without_common_coverage(eng):
    rng = np.random.default_rng(4)
    samp = level_reads(rng, 0.5)
    ctrl = {('chrZ', '+'): samp[('chrA', '+')]}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(th.TomboError, match='^No significant region is covered by both'):
            ts.cluster_most_signif_dists(pc.open_stats(), samp, ctrl, 10, 7, engine=eng)


def test_binding_constants_and_symbols():
    """the Python constants equal the kernel header's; the header declares the entries the binding calls"""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    text = open(os.path.join(root, 'tombo_amd', 'csrc', 'k_pdist.h')).read()
    assert int(re.search(r'#define PDIST_TILE (\d+)', text).group(1)) == _native.PDIST_TILE
    assert int(re.search(r'#define PDIST_LDS_ROW_MAX (\d+)', text).group(1)) == _native.PDIST_LDS_ROW_MAX
    assert int(re.search(r'#define PDIST_MAX_ROWS (\d+)', text).group(1)) == _native.PDIST_MAX_ROWS
    assert 2 * _native.PDIST_TILE * (_native.PDIST_LDS_ROW_MAX | 1) * 8 <= 65536
    header = open(os.path.join(root, 'include', 'tombo_amd.h')).read()
    assert '#define TBA_ABI_VERSION 13' in header
    for sym in ('tba_pairwise_window_dists', 'tba_pairwise_nanmean_dists', 'tba_pdist_tile', 'tba_pdist_lds_row_max'):
        assert re.search(r'\b%s\(' % sym, header), sym

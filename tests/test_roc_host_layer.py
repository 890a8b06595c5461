"""The host layer of the ROC feature over the numpy stand-in engine (no GPU): the helper functions against the live
reference's recorded results, the MotifStats interface, the argument checks of the engine methods, the NaN and
empty-name errors and the rule at chromosome edges."""
import os
import re
import warnings

import numpy as np
import pytest

import roc_cases as rc
from roc_stub_engine import NumpyRocEngine
from store_memh5 import StoreGroup
from tombo_amd import tombo_stats as ts, tombo_helper as th, _native

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


# ---- tombo_helper ---------------------------------------------------------------------------------
def test_fasta_get_seq():
    m, genome = rc.meta(), rc.genome()
    assert list(genome.iter_chrms()) == m['chrms'] and genome.has_rna_bases == m['has_rna_bases']
    assert 'chrA' in genome and 'chrZ' not in genome
    for (chrm, start, end), seq in zip(m['seq_reqs'], m['seqs']):
        assert genome.get_seq(chrm, start, end, error_end=False) == seq
    assert any(re.search('[a-z]', line) for line in open(rc.FASTA) if not line.startswith('>'))
    assert 'N' in genome.get_seq('chrA') and genome.get_seq('chrA') == genome.get_seq('chrA').upper()
    for chrm, start, end, error_end in m['seq_errs']:
        with pytest.raises(th.TomboError) as exc:
            genome.get_seq(chrm, start, end, error_end=error_end)
        assert str(exc.value) == m['seq_err_text'] == 'Encountered invalid genome sequence request.'


def test_fasta_uridines(tmp_path):
    fn = tmp_path / 'rna.fa'
    fn.write_text('>r1 x\nACGUUacgu\nGGU\n>r2\nAC\n')
    genome = th.Fasta(str(fn))
    assert genome.has_rna_bases and genome.get_seq('r1') == 'ACGTTACGTGGT' and genome.get_seq('r1', 3, 5) == 'TT'
    assert list(genome.iter_chrms()) == ['r1', 'r2']


def test_parse_motif_descs():
    m = rc.meta()
    for key, text in m['motif_sets'].items():
        got = [[motif.raw_motif, motif.mod_pos, motif.mod_base, name] for motif, name in th.parse_motif_descs(text)]
        assert got == m['parsed_motifs'][key]
    for bad in ('CG:1', 'CG:x:name', 'CG:1:a:b', 'CQ:1:a', 'CG:3:a'):
        with pytest.raises(th.TomboError) as exc:
            th.parse_motif_descs(bad)
        assert str(exc.value) in m['motif_err_text']
    assert 'Invalid motif decriptions format.' in m['motif_err_text']


@pytest.mark.parametrize('key,fn', [('mod', rc.MOD_BED), ('unmod', rc.UNMOD_BED)])
def test_parse_locs_file(key, fn):
    g, m = rc.gold(), rc.meta()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        locs = th.parse_locs_file(fn)
    keys = [tuple(cs) for cs in rc.js('locs_%s_keys' % key)]
    assert list(locs) == keys
    for cs in keys:
        assert rc.same(locs[cs], g['locs_%s|%s|%s' % ((key,) + cs)])
    if m['warn_text'][key]:
        assert len(caught) == 1 and str(caught[0].message).startswith('Some provided locations (2) were incorrectly')
        assert str(caught[0].message).split(fn)[0] in m['warn_text'][key].replace('\n\t', '')
    else:
        assert not caught


def test_parse_locs_file_all_bad(tmp_path):
    fn = tmp_path / 'bad.bed'
    fn.write_text('chrA\tx\n')
    with pytest.warns(UserWarning, match='All provided locations from .* were incorrectly formatted'):
        assert th.parse_locs_file(str(fn)) == {}
    assert 'All provided locations from' in rc.meta()['warn_text']['all_bad']


# ---- MotifStats -------------------------------------------------------------------------------------
def test_motif_stats_interface():
    ms = ts.MotifStats([0.5, -0.0, 0.25], [True, False, True])
    assert len(ms) == 3 and ms.stats.dtype == np.float64 and ms.has_mod.dtype == np.bool_
    assert list(ms) == [(0.5, True), (-0.0, False), (0.25, True)] and type(list(ms)[0][1]) is bool
    assert sorted(ms) == [(-0.0, False), (0.25, True), (0.5, True)]
    assert list(zip(*ms))[1] == (True, False, True)
    assert len(ts.MotifStats()) == 0 and list(ts.MotifStats()) == []
    with pytest.raises(ValueError):
        ts.MotifStats([1.0], [True, False])


def test_methods_on_the_three_containers():
    for cls in (ts.ModelStats, ts.LevelStats, ts.PerReadStats):
        for name in ('compute_motif_stats', 'compute_ground_truth_stats', 'compute_ctrl_motif_stats'):
            assert callable(getattr(cls, name))


def test_level_stats_uses_its_stat_slot():
    grp = StoreGroup()
    ls = ts.LevelStats(grp, 'ks_test', 100, 1, 10)
    poss = np.array([131, 132, 160, 163])           # chrA: CCAGG at 130 (mod C at 131), GATC at 160
    ls._write_stat_block(th.groupStats(np.array([0.5, 0.25, 0.125, 1.0]), poss, 'chrA', '+', 100,
                                       np.full(4, 3), np.full(4, 3)))
    ls.close()
    res = ts.TomboStats(grp).compute_motif_stats(rc.motif_descs('two'), rc.genome(), engine=NumpyRocEngine())
    seq = rc.genome().get_seq('chrA')
    want_a = [(s, p == 131) for s, p in zip([0.5, 0.25, 0.125, 1.0], poss) if seq[p] == 'C']
    assert list(res['a']) == want_a and (0.5, True) in want_a


# ---- errors -------------------------------------------------------------------------------------------
def test_nan_statistic_raises():
    with pytest.raises(ValueError, match='^NaN statistic$'):
        ts.prep_accuracy_rates({'x': ts.MotifStats([0.5, np.nan, 1.0], [True, False, True])}, engine=NumpyRocEngine())


def test_empty_name_raises_and_names_the_modification():
    with pytest.raises(ValueError, match='No statistics for modification 6mA'):
        ts.prep_accuracy_rates({'6mA': ts.MotifStats()}, engine=NumpyRocEngine())
    res = rc.run_case('motif_pr_cg_plain', NumpyRocEngine())
    res['none'] = []
    with pytest.raises(ValueError, match='none'):
        ts.prep_accuracy_rates(res, engine=NumpyRocEngine())


def test_prep_accuracy_rates_takes_lists_of_tuples():
    ms = rc.recorded('motif_pr_cg_plain')['x']
    a = ts.prep_accuracy_rates({'x': ms}, engine=NumpyRocEngine())
    b = ts.prep_accuracy_rates({'x': list(ms)}, engine=NumpyRocEngine())
    assert all(rc.same(np.array(u[:3]), np.array(v[:3])) for u, v in zip(a[:3], b[:3])) and a[3] == b[3]


def test_fewer_entries_than_plot_points():
    ms = ts.MotifStats([3.0, 1.0, 2.0], [True, False, True])
    tp, fp, prec = ts.sampled_accuracy_rates(ms, engine=NumpyRocEngine())
    want = ts.compute_accuracy_rates([False, True, True])
    assert rc.same(tp, want[0]) and rc.same(fp, want[1]) and rc.same(prec, want[2]) and prec.shape == (1000,)


def test_motifs_that_share_a_name_share_a_list():
    """as in the reference: per record (motif form) or per block (control form), in the order of motif_descs"""
    eng = NumpyRocEngine()
    for case in ('motif_pr_dup_plain', 'ctrl_pr_dup_plain', 'ctrl_ms_dup_limit'):
        res = rc.run_case(case, eng)
        assert list(res) == ['x']
        rc.check_case(case, res)
    with pytest.raises(ValueError, match='at least one motif'):
        rc.open_store('pr').compute_motif_stats([], rc.genome(), engine=eng)


# ---- bounded calls ------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['ctrl_pr_cg_limit', 'ctrl_pr_self_limit', 'ctrl_pr_dup_limit'])
def test_ctrl_limit_stops_sending_blocks(case, monkeypatch):
    """with a total_stats_limit the control form sends blocks in bounded groups and nothing after the limit"""
    monkeypatch.setattr(ts, '_ROC_LIMIT_MIN_RECORDS', 1)
    eng, everything = NumpyRocEngine(), NumpyRocEngine()
    rc.check_case(case, rc.run_case(case, eng))
    rc.check_case(case.replace('_limit', '_plain'), rc.run_case(case.replace('_limit', '_plain'), everything))
    sent = sum(n for _, n in eng.calls)
    assert len(eng.calls) > len(everything.calls) and 0 < sent < sum(n for _, n in everything.calls)
    # every block but the empty one is larger than the limit: one block per group, sample and control apart
    sizes = dict(((c, s, a), n) for c, s, a, n in rc.meta()['blocks'])
    n_first = [b[4].shape[0] for b in rc.open_store('pr')][0]
    assert eng.calls[0][1] == n_first == sizes[tuple(rc.meta()['blocks'][0][:3])]


@pytest.mark.parametrize('case', ['motif_pr_two_plain', 'ctrl_pr_two_plain', 'ctrl_pr_self_plain', 'truth_pr',
                                  'motif_pr_dup_sub', 'ctrl_pr_dup_limit'])
def test_groups_of_blocks_give_the_same_lists(case, monkeypatch):
    """a small bound on (record, motif) pairs per call: many calls, the same result"""
    monkeypatch.setattr(ts, '_ROC_MAX_PAIRS', 600)
    eng = NumpyRocEngine()
    rc.check_case(case, rc.run_case(case, eng))
    # a call holds one block (a block larger than the bound stands alone) or stays within the bound
    largest_block = max(n for _, _, _, n in rc.meta()['blocks'])
    n_motifs = 1 if case == 'truth_pr' else len(rc.motif_descs(rc.meta()['cases'][case]['motifs']))
    assert len(eng.calls) >= 2 and all(n <= max(600 // n_motifs, largest_block) for _, n in eng.calls)


def test_argument_checks():
    i64, f64 = np.int64, np.float64
    off, pos, stat = np.array([0, 2], dtype=i64), np.array([5, 6], dtype=i64), np.array([0.5, 0.25])
    minus, ss, s_off, seq = np.zeros(1, np.uint8), np.zeros(1, i64), np.array([0, 8], dtype=i64), np.zeros(8, np.uint8)
    motif = (2, 1, 1, np.array([2, 4], dtype=np.uint8))
    good = (minus, ss, s_off, seq, off, pos, stat, [motif])
    _native._check_roc_motif_args(*good)
    for k, bad in ((0, minus.astype(i64)), (3, seq.astype(np.int8)), (2, np.array([0, 7], dtype=i64)),
                   (2, np.array([1, 8], dtype=i64)), (4, np.array([0, 3], dtype=i64)), (5, pos.astype(np.int32)),
                   (6, stat.astype(np.float32)), (7, []), (7, [motif] * 65), (7, [(2, 3, 1, motif[3])]),
                   (7, [(3, 1, 1, motif[3])]), (7, [(2, 1, 1, np.array([2, 16], dtype=np.uint8))])):
        args = list(good)
        args[k] = bad
        with pytest.raises(ValueError):
            _native._check_roc_motif_args(*args)
    assert _native._check_roc_motif_args(*good[:7], [(2, 1, 9, motif[3])])[7][0, 2] == 255
    loc = np.array([[0, 2, 0, 1]], dtype=i64)
    mod, unmod = np.array([5, 9], dtype=i64), np.array([6], dtype=i64)
    _native._check_roc_loc_args(loc, mod, unmod, off, pos, stat)
    for args in ((loc, mod[::-1].copy(), unmod), (np.array([[0, 3, 0, 1]], dtype=i64), mod, unmod),
                 (np.array([[1, 0, 0, 1]], dtype=i64), mod, unmod), (loc.astype(np.int32), mod, unmod),
                 (loc, mod.astype(f64), unmod), (loc[0], mod, unmod)):
        with pytest.raises(ValueError):
            _native._check_roc_loc_args(*args, off, pos, stat)
    hm, ranks = np.array([True, False]), np.array([0, 1], dtype=i64)
    assert _native._check_roc_rank_args(stat, hm, ranks)[1].dtype == np.uint8
    for args in ((stat, hm.astype(np.uint8), ranks), (stat, hm, np.array([1, 0], dtype=i64)),
                 (stat, hm, np.array([0, 2], dtype=i64)), (stat, hm, np.array([-1], dtype=i64)),
                 (stat, hm[:1], ranks), (stat.astype(np.float32), hm, ranks), (stat, hm, ranks.astype(np.int32))):
        with pytest.raises(ValueError):
            _native._check_roc_rank_args(*args)


def test_sort_tile_is_exported():
    text = open(os.path.join(ROOT, 'tombo_amd', 'csrc', 'k_roc.h')).read()
    assert int(re.search(r'#define ROC_SORT_TILE (\d+)', text).group(1)) == _native.ROC_SORT_TILE
    hdr = open(os.path.join(ROOT, 'include', 'tombo_amd.h')).read()
    for sym in ('tba_roc_motif_labels', 'tba_roc_loc_labels', 'tba_roc_rank_counts', 'tba_roc_sort_tile'):
        assert re.search(r'\b%s\(' % sym, hdr)


# ---- the edge rule ---------------------------------------------------------------------------------------
def test_edge_rule(tmp_path):
    rc.check_edge_rule(NumpyRocEngine(), tmp_path)

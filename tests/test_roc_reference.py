"""The numpy restatement of the ROC entries (tests/roc_reference.py) pinned to the live reference's recorded results
(tests/golden/stats_roc.npz): labels of the three compute_*_stats forms, the sorted cumulative counts behind
prep_accuracy_rates, and the reference's own host arithmetic (compute_accuracy_rates, AUC, mean average precision).
No tolerance."""
import numpy as np
import pytest

import roc_cases as rc
import roc_reference as ref
from roc_stub_engine import NumpyRocEngine
from tombo_amd import tombo_stats as ts

CASES = sorted(rc.meta()['cases'])
RATE_CASES = sorted(rc.meta()['rates'])


def test_fixture_covers_what_it_should():
    m, g = rc.meta(), rc.gold()
    assert len(CASES) == 38 and set(c['kind'] for c in m['cases'].values()) == {'motif', 'ctrl', 'truth'}
    x = g['motif_pr_cg_plain|x|stat']
    assert np.any(np.signbit(x) & (x == 0)) and np.any(~np.signbit(x) & (x == 0))          # -0.0 and 0.0
    hm = g['motif_pr_cg_plain|x|has_mod']
    assert np.intersect1d(x[hm], x[~hm]).shape[0] > 10                                     # values across labels
    assert not np.isnan(x).any()
    assert g['motif_pr_cg_limit|x|stat'].shape[0] < x.shape[0]                             # the limit stops mid-file
    assert g['motif_pr_cg_sub|x|stat'].shape[0] < x.shape[0]
    assert len(m['cases']['motif_pr_dup_plain']['names']) == 1 and len(m['parsed_motifs']['dup']) == 3   # a shared name
    assert any(n == 0 for _, _, _, n in m['blocks'])                                       # an empty block
    assert any(s + m['region_size'] > m['chrm_lens'][c] for c, _, s, _ in m['blocks'])     # one past a chromosome end


@pytest.mark.parametrize('case', CASES)
def test_labels_match_the_reference(case):
    rc.check_case(case, rc.run_case(case, NumpyRocEngine()))


@pytest.mark.parametrize('case', RATE_CASES)
def test_rates_match_the_reference(case):
    rc.check_rates(case, NumpyRocEngine())


def test_rank_counts_is_sorted_of_tuples():
    """the ordering the reference gets from sorted() on (float, bool) tuples, -0.0 and 0.0 and +-inf included"""
    rng = np.random.default_rng(3)
    stats = rng.choice([-np.inf, -1.5, -0.0, 0.0, 5e-324, 0.25, np.inf], 400)
    has_mod = rng.integers(0, 2, 400).astype(bool)
    ordered = np.array(list(zip(*sorted(zip(stats.tolist(), has_mod.tolist()))))[1])
    tp_at, total, n_nan = ref.rank_counts(stats, has_mod, np.arange(400))
    assert np.array_equal(tp_at, np.cumsum(ordered)) and total == has_mod.sum() and n_nan == 0


@pytest.mark.parametrize('n,points', [(391, 1000), (37, 1000), (37, 10), (1, 5)])
def test_compute_accuracy_rates(n, points):
    g = rc.gold()
    ordered = g['acc_ordered'][:n]
    got = ts.compute_accuracy_rates(ordered, points)
    for k, v in zip('tfp', got):
        assert rc.same(v, g['acc|%d|%d|%s' % (n, points, k)]), (n, points, k)
    # the sampled form over the engine: any order of the same entries
    if points == 1000:
        perm = np.random.default_rng(n).permutation(n)
        stats = np.arange(n, dtype=np.float64)[perm]           # statistic = rank, so `ordered` is the sorted order
        got = ts.sampled_accuracy_rates(ts.MotifStats(stats, ordered[perm]), engine=NumpyRocEngine())
        for k, v in zip('tfp', got):
            assert rc.same(v, g['acc|%d|%d|%s' % (n, points, k)]), (n, points, k)


def test_default_plot_points():
    from tombo_amd._default_parameters import ROC_PLOT_POINTS
    assert ROC_PLOT_POINTS == 1000

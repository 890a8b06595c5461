"""The host layer of `compute_reg_stats_reads_batch` and `test_significance` on a numpy engine
(tests/site_reads_stub_engine.py, whose `site_fractions_reads` restates the pair geometry of
tba_site_fractions_reads pair by pair): the golden cases of the per-site fractions, reads shared between
regions, every way a pair fails, the driver against today's route, the argument checks and the C header."""
import os
import re

import numpy as np
import pytest

import site_reads_cases as cases
from site_reads_stub_engine import SiteReadsStubEngine
from stats_cases import gold, meta, model, alt_refs   # noqa: F401
from tombo_amd import tombo_stats as ts, tombo_helper as th, _native

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@pytest.mark.parametrize('at_once', [True, False])
@pytest.mark.parametrize('stat_type', cases.Z_TYPES)
def test_golden_cases(gold, meta, model, stat_type, at_once):
    assert cases.check_golden(gold, meta, model, SiteReadsStubEngine(), stat_type, at_once) >= 20


@pytest.mark.parametrize('fm', [0, 1, 3])
def test_reads_shared_between_regions(model, fm):
    assert cases.check_shared_reads(model, SiteReadsStubEngine(), fm) == 24


def test_failing_pairs(model):
    cases.check_failing_pairs(model, SiteReadsStubEngine())


def test_lengths_that_disagree_are_refused(model):
    index = cases.seeded_index(model, per_strand=3)
    rd = index[('chr1', '+')][0]
    for bad in (rd._replace(end=rd.end + 1), rd._replace(seq=rd.seq[:-1]), rd._replace(means=rd.means[:-1])):
        reg = th.regionData('chr1', '+', rd.start, rd.start + 50, [bad])
        with pytest.raises(ValueError, match='disagree'):
            ts.compute_reg_stats_reads_batch([reg], 0, 1, 0.3, None, None, model, None, False, ts.DE_NOVO_TXT, None,
                                             engine=SiteReadsStubEngine())


def test_model_compare_is_delegated(gold, meta, model, alt_refs):
    c = next(c for c in meta['cases'] if c['stat_type'] == ts.ALT_MODEL_TXT)
    args = cases.golden_case_args(gold, meta, model, c)
    args = args[:7] + (alt_refs,) + args[8:]
    eng = SiteReadsStubEngine()
    want = ts.compute_reg_stats_batch(*args, return_per_read=True, engine=eng)
    got = ts.compute_reg_stats_reads_batch(*args, return_per_read=True, engine=eng)
    assert eng.reads_calls == [] and len(want[0]) == len(got[0])
    for w, g in zip(want[0], got[0]):
        assert isinstance(g, Exception) == isinstance(w, Exception)
        if not isinstance(w, Exception):
            assert all(np.array_equal(a[1].reg_frac_standard_base, b[1].reg_frac_standard_base, equal_nan=True)
                       for a, b in zip(w, g))


# ---- the driver ------------------------------------------------------------------------------------
@pytest.mark.parametrize('stat_type,per_read,use_ref', cases.DRIVER_CASES)
def test_driver_equals_todays_route(model, alt_refs, stat_type, per_read, use_ref):
    n = cases.check_driver(model, alt_refs, SiteReadsStubEngine(), stat_type, per_read, use_ref)
    assert n >= 12 * (2 if per_read else 1)


def test_driver_file_names_and_refusals(model):
    assert ts.signif_store_names(ts.DE_NOVO_TXT, 'a', 'b') == ({'de_novo': 'a.tombo.stats'}, {'de_novo': 'b.tombo.per_read_stats'})
    assert ts.signif_store_names(ts.ALT_MODEL_TXT, 'a', 'b', [('5mC', None)]) == (
        {'5mC': 'a.5mC.tombo.stats'}, {'5mC': 'b.5mC.tombo.per_read_stats'})
    assert ts.signif_store_names(ts.KS_TEST_TXT, 'a') == ({'ks_test': 'a.tombo.stats'}, {})
    with pytest.raises(NotImplementedError):
        ts.test_significance({}, 'nonsense', 'a', 100, 1, 1, 10)
    with pytest.raises(ValueError, match='control reads'):
        ts.test_significance({}, ts.KS_TEST_TXT, 'a', 100, 1, 1, 10)
    with pytest.raises(ValueError, match='single_read_thresh'):
        ts.test_significance({}, ts.DE_NOVO_TXT, 'a', 100, 1, 1, 10, std_ref=model)


# ---- argument checks of the binding (shared with the numpy engine), the header -----------------------
def test_argument_checks():
    t = _native._check_site_reads_args(**cases.base_args())
    assert t.pos_off.tolist() == [0, 102, 204] and t.fm_offset == 1
    assert _native.site_reads_stat_bound(0, t, 6, 2).tolist() == [150 - 97 - 5, 203 - 150 - 5, 303 - 196 - 5]
    assert _native.site_reads_stat_bound(1, t).tolist() == [150 - 99, 201 - 150, 301 - 199]
    for change in cases.BAD_ARGS:
        with pytest.raises(ValueError):
            _native._check_site_reads_args(**dict(cases.base_args(), **change))
    ok = dict(cases.base_args(), form=1, seq=None, pos_means=np.zeros(204), pos_sds=np.ones(204))
    _native._check_site_reads_args(**ok)
    with pytest.raises(ValueError):
        _native._check_site_reads_args(**dict(ok, pos_sds=np.ones(203)))
    eng = SiteReadsStubEngine()
    with pytest.raises(ValueError, match='model'):
        eng.site_fractions_reads(*cases.base_args().values(), 1e-50, 0.3)


def test_header_declares_the_entry_and_raises_the_minor_number():
    hdr = open(os.path.join(ROOT, 'include', 'tombo_amd.h')).read()
    assert re.search(r'\bint tba_site_fractions_reads\(tba_engine \*e, int form,', hdr)
    assert re.search(r'#define TBA_ABI_VERSION 13\b', hdr)
    assert int(re.search(r'#define\s+TBA_ABI_MINOR\s+(\d+)', hdr).group(1)) >= 3
    assert 'tba_site_fractions_reads' in _native.PROTOTYPES
    names = list(_native.PROTOTYPES)
    assert names.index('tba_site_fractions_reads') == names.index('tba_site_fractions') + 1
    src = open(os.path.join(ROOT, 'tombo_amd', 'csrc', 'k_site.h')).read()
    assert '__global__ void __launch_bounds__(256) k_site_pair_plan(' in src and '__global__ void k_site_gather(' in src

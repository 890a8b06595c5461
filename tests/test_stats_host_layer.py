"""The host layer of the statistics (tombo_amd.tombo_stats: region clips, strand flips, motif
search, control levels, track building, per-read blocks, per-region assembly) without a GPU: the
golden cases of test_gpu_read_stats.py and test_gpu_site_stats.py with the numpy stand-in engine of
tests/stats_stub_engine.py passed as `engine=`.

Same comparisons and tolerances as on the device (tests/stats_cases.py holds them for both):
positions, coverages and fractions equal -- the fixture generator asserts that no recorded
statistic lies within 1e-9 relative of a threshold -- and per-read statistics to 1e-12 relative
(the constant-variance likelihood ratio bit-equal: no transcendental, terms in index order)."""
import pytest

from tombo_amd import tombo_stats as ts
from stats_cases import (gold, meta, model, alt_refs, load_read_cases, check_z_read_cases, check_alt_read_cases,   # noqa: F401
                         check_all_regions_at_once, check_one_region_at_a_time, check_per_read_blocks)
from stats_stub_engine import NumpyStatsEngine

ENGINE = NumpyStatsEngine()


def _only(res):
    if isinstance(res[0], Exception):
        raise res[0]
    return res[0]


def _de_novo(rd, std_ref, fm, reg):
    pv, poss = _only(ts.compute_de_novo_read_stats_batch([rd], std_ref, fm, reg, engine=ENGINE))
    return {ts.DE_NOVO_TXT: pv}, {ts.DE_NOVO_TXT: poss}, rd.read_id


def _sample_compare(rd, cm, cs, fm, reg):
    pv, poss = _only(ts.compute_sample_compare_read_stats_batch(
        [rd], [cm] if reg is None else cm, [cs] if reg is None else cs, fm, reg, engine=ENGINE))
    return {ts.SAMP_COMP_TXT: pv}, {ts.SAMP_COMP_TXT: poss}, rd.read_id


def _alt_model(rd, std_ref, alts, use_standard_llhr, reg):
    return _only(ts.compute_alt_model_read_stats_batch([rd], std_ref, alts, use_standard_llhr, reg,
                                                       engine=ENGINE)) + (rd.read_id,)


def test_de_novo_and_sample_compare_match_the_reference():
    assert check_z_read_cases(_de_novo, _sample_compare) >= 60


def test_alt_model_llhrs_match_the_reference():
    assert check_alt_read_cases(_alt_model) > 50


def test_golden_all_regions_at_once(gold, meta, model, alt_refs):
    assert check_all_regions_at_once(gold, meta, model, alt_refs, engine=ENGINE) > 60


def test_golden_one_region_at_a_time(gold, meta, model, alt_refs):
    check_one_region_at_a_time(gold, meta, model, alt_refs, engine=ENGINE)


def test_per_read_blocks(gold, meta, model, alt_refs):
    assert check_per_read_blocks(gold, meta, model, alt_refs, engine=ENGINE) > 10


def test_engine_argument_reaches_every_batch_function():
    """an engine that refuses every call shows that no per-read `*_batch` function falls back to the
    process-wide engine (the alternate-model one used to)"""
    class Refuses(object):
        def __getattr__(self, name):
            raise RuntimeError('engine method %s called' % name)
    _, _, std_ref, alts, reads = load_read_cases()
    cms = [[0.0] * (rd.end - rd.start) for rd in reads]
    for call in (lambda e: ts.compute_de_novo_read_stats_batch(reads, std_ref, 0, engine=e),
                 lambda e: ts.compute_sample_compare_read_stats_batch(reads, cms, cms, 0, engine=e),
                 lambda e: ts.compute_alt_model_read_stats_batch(reads, std_ref, alts, engine=e)):
        with pytest.raises(RuntimeError, match='engine method'):
            call(Refuses())

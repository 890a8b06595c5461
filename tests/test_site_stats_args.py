"""Argument checks of the per-site statistics (compute_reg_stats, compute_reg_stats_batch): raised or
returned on the host before anything reaches the engine, so no GPU is needed."""
import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th
from tombo_amd import _default_parameters as dp


def _reg(start=100, end=120, reads='one'):
    if isinstance(reads, str):
        reads = [th.resquiggledRead(90, 130, False, 0, '+', None, None, False, read_id='a',
                                    means=np.zeros(40), seq='ACGT' * 10)]
    return th.regionData('c', '+', start, end, reads)


MODEL = ts.TomboModel(seq_samp_type=th.seqSampleType('DNA', False))


def _batch(regions, stat_type=ts.DE_NOVO_TXT, fm=1, mtr=2, ctrl=None, std_ref=MODEL, alt_refs=None, **kw):
    return ts.compute_reg_stats_batch(regions, fm, mtr, 0.5, 0.15, ctrl, std_ref, alt_refs, False,
                                      stat_type, None, **kw)


def test_names_and_defaults():
    assert th.regionStats._fields == ('reg_frac_standard_base', 'reg_poss', 'chrm', 'strand', 'start',
                                      'reg_cov', 'ctrl_cov', 'valid_cov')
    assert dp.LLR_THRESH == {'DNA': (-1.5, 2.5), 'RNA': (-2.5, 2.5)}
    assert dp.SAMP_COMP_THRESH == {'DNA': (0.15, 0.5), 'RNA': (0.05, 0.4)}
    assert dp.DE_NOVO_THRESH == {'DNA': (0.15, 0.5), 'RNA': (0.05, 0.4)}
    assert list(dp.COV_DAMP_COUNTS) == [2, 0]


def test_unknown_stat_type():
    with pytest.raises(NotImplementedError, match='Unrecognized test type.'):
        _batch([_reg()], 'ks_test')


def test_mismatched_region_lists():
    with pytest.raises(ValueError):
        _batch([_reg()], ts.SAMP_COMP_TXT, ctrl=[])
    with pytest.raises(ValueError):
        _batch([_reg()], ts.SAMP_COMP_TXT, ctrl=None)
    with pytest.raises(ValueError):
        _batch([_reg()], ts.SAMP_COMP_TXT, ctrl=[_reg(100, 121)])


@pytest.mark.parametrize('fm, mtr', [(-1, 2), (65, 2), (1.5, 2), (1, 0)])
def test_fm_offset_out_of_range(fm, mtr):
    with pytest.raises(ValueError):
        _batch([_reg()], fm=fm, mtr=mtr)


def test_alt_without_alt_refs():
    with pytest.raises(ValueError):
        _batch([_reg()], ts.ALT_MODEL_TXT, alt_refs=None)
    with pytest.raises(ValueError):
        _batch([_reg()], ts.ALT_MODEL_TXT, alt_refs=[])
    with pytest.raises(ValueError):
        _batch([_reg()], ts.DE_NOVO_TXT, std_ref=None)


def test_region_without_reads_is_an_error_object():
    res = _batch([_reg(reads=[]), _reg(reads=None)])
    assert len(res) == 2
    for e in res:
        assert isinstance(e, th.TomboError) and str(e) == 'Reads contains no statistics in this region.'
    res, per_read = _batch([_reg(reads=[])], return_per_read=True)
    assert isinstance(res[0], th.TomboError) and per_read == [[]]
    with pytest.raises(th.TomboError, match='Reads contains no statistics'):
        ts.compute_reg_stats(_reg(reads=[]), 1, 2, 0.5, None, None, MODEL, None, False, None,
                             ts.DE_NOVO_TXT, None)
    # a control region without reads: the error of get_reads_ref
    res = _batch([_reg()], ts.SAMP_COMP_TXT, ctrl=[_reg(reads=[])], std_ref=None)
    assert isinstance(res[0], th.TomboError) and 'Must annotate region with reads' in str(res[0])


def test_empty_list():
    assert _batch([]) == []
    assert _batch([], return_per_read=True) == ([], [])


def test_damp_fraction_rounds_half_even():
    got = ts.calc_damp_fraction({'unmod': 2, 'mod': 0}, np.array([0.5, 0.5, np.nan]), np.array([5, 7, 0]))
    assert got[0] == (2 + 2) / 7 and got[1] == (4 + 2) / 9 and np.isnan(got[2])
    assert np.array_equal(ts.calc_damp_fraction((2, 0), np.array([0.5]), np.array([5])), got[:1])

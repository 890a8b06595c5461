"""The words tba_set_model keeps for a level model with ONE proven sd and hands to k_dp_c1 as arguments (made by
tba_one_sd_words: host code, no device): the sd, yh = RN(1 / sd) and yl = RN(RN(1 - sd yh) yh), held against the
exact-arithmetic restatement of tests/div_const_model.py (fractions.Fraction, every rounding spelled out) -- the same
bits the rows of k_dp_cdiv make of the sd per 64 rows -- and the cases in which the one-sd form is not offered."""
import numpy as np
import pytest

import div_const_model as model
from test_div_const_proof import DNA_SD, RNA_SD, BAD_SD


def words(sds):
    from tombo_amd import _native
    return _native.one_sd_words(np.asarray(sds, dtype=np.float64))


@pytest.mark.parametrize('name', ['DNA', 'RNA'])
def test_standard_models_words_equal_the_exact_restatement(name):
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    m = ts.TomboModel(seq_samp_type=th.seqSampleType(name, name == 'RNA'))
    sd = DNA_SD if name == 'DNA' else RNA_SD
    got = words(m.level_sds)
    assert got is not None
    yh, yl = model.recip_pair(sd)
    assert [float(w).hex() for w in got] == [float(sd).hex(), float(yh).hex(), float(yl).hex()]
    # (and the pair does what it is for: the two-operation quotient of a dividend is its IEEE quotient)
    for a in (1.0, -2.5, 123.456, 3.0e-7):
        assert model.fma(a, got[1], model.rn(model.Fraction(a) * model.Fraction(got[2]))) == a / sd


@pytest.mark.parametrize('sd', [0.25, 0.375, 3.0, DNA_SD, RNA_SD])
def test_any_single_proven_sd_gets_its_words(sd):
    yh, yl = model.recip_pair(sd)
    assert words([sd] * 7) == (sd, yh, yl)
    assert words([sd]) == (sd, yh, yl)


def test_tables_without_one_proven_sd_get_none():
    assert words([DNA_SD] * 5 + [RNA_SD]) is None          # two proven sds: the lane form's table
    assert words([RNA_SD] + [DNA_SD] * 5) is None
    assert words([BAD_SD] * 4) is None                     # one sd, unproven
    assert words([DNA_SD, BAD_SD]) is None
    assert words([0.0, -0.0]) is None and words([np.nan] * 3) is None
    assert words([]) is None

"""The prover of the forward pass's two-operation division (csrc/div_const_proof.h) through its C entry,
tba_prove_const_division: host code, no device.  For a divisor it calls proven, fma(a, yh, a * yl) is a / sd for
every dividend; the verdicts are held against fixed cases and against an exact-arithmetic restatement
(tests/div_const_model.py)."""
import numpy as np
import pytest

import div_const_model as model

DNA_SD = float.fromhex('0x1.69574c5f06820p-2')     # the one sd of Tombo's DNA model
RNA_SD = float.fromhex('0x1.cd5185c918344p-3')     # ... and of the RNA model
BAD_SD = float.fromhex('0x1.e3cf63ef4d557p-1')     # a divisor with a dividend the two-operation form gets wrong:
BAD_DIVIDEND = float.fromhex('0x1.bca5d32101e7bp+52')


def prove(sds):
    from tombo_amd import _native
    return _native.prove_const_division(sds)


def test_standard_models_have_one_sd_each_and_both_are_proven():
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    for name, sd, n in (('DNA', DNA_SD, 4096), ('RNA', RNA_SD, 1024)):
        m = ts.TomboModel(seq_samp_type=th.seqSampleType(name, name == 'RNA'))
        sds = np.asarray(m.level_sds, dtype=np.float64)
        assert sds.shape == (n,) and np.all(sds == sd), name
    assert prove([DNA_SD, RNA_SD]).tolist() == [True, True]
    assert model.proven(DNA_SD) and model.proven(RNA_SD)
    # DNA: five trailing zero bits, every boundary distance a multiple of 32: nothing within 16 at all
    assert model.candidates(DNA_SD, 16) == [] and len(model.candidates(RNA_SD, 16)) == 8


def test_the_failing_divisor_is_unproven_and_its_dividend_really_fails():
    assert prove([BAD_SD]).tolist() == [False] and not model.proven(BAD_SD)
    q2 = model.two_op_quotient(BAD_DIVIDEND, BAD_SD)
    assert q2 == float.fromhex('0x1.d68e47d408cccp+52') and BAD_DIVIDEND / BAD_SD == float.fromhex('0x1.d68e47d408ccdp+52')
    assert model.significand(BAD_DIVIDEND) in model.candidates(BAD_SD, 6)


@pytest.mark.parametrize('sd', [0.0, -0.0, -0.5, -DNA_SD, np.inf, -np.inf, np.nan, 5e-324, 1e-310,
                                float.fromhex('0x1.fffffffffffffp-1'), float.fromhex('0x1.fffffffffffffp+2'),
                                2.0 ** -300, 2.0 ** 300])
def test_divisors_outside_the_proof_are_unproven(sd):
    assert prove([sd]).tolist() == [False]


@pytest.mark.parametrize('sd', [0.25, 0.375, 1.0, 2.0 ** -200, 3.0])
def test_simple_divisors_are_proven(sd):
    assert prove([sd]).tolist() == [True] and model.proven(sd)


def test_verdicts_equal_the_exact_restatement_on_random_divisors():
    rng = np.random.RandomState(20261020)
    sds = np.concatenate([rng.uniform(0.05, 1.0, 440), rng.uniform(1.0, 40.0, 30),
                          np.ldexp(rng.randint(1, 1 << 12, 30).astype(np.float64), -10)])   # (short significands too)
    got = prove(sds)
    want = np.array([model.proven(float(s)) for s in sds])
    assert np.array_equal(got, want), sds[got != want]
    assert 0.9 * sds.shape[0] < got.sum() < sds.shape[0]       # most are proven, and some are not


def test_entry_takes_empty_input_and_refuses_null():
    from tombo_amd import _native
    L = _native.lib()
    assert L.tba_prove_const_division(None, 0, None) == 0
    assert L.tba_prove_const_division(None, 3, None) != 0
    assert prove(np.zeros(0)).shape == (0,)

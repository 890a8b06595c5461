"""The numpy restatement of ts.trim_rna (tests/trim_rna_reference.py) over the CPU oracle's change points and segment
SDs against what the live reference answered (tests/golden/stats_trim_rna.npz, cases in tests/trim_rna_cases.py): this pins
the restatement, which the GPU tests then take as the expected answer on any input."""
import hashlib
import json
import os

import numpy as np
import pytest

import trim_rna_cases as tc
import trim_rna_reference as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stats_trim_rna.npz')


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    return dict((k, g[k]) for k in g.files)


def expected(raw, case):
    """the restatement over the oracle -> the adapter end, or 'Class: text' of the reference's exception"""
    import oracle
    try:
        return tr.trim_rna(raw, case.seg, case.trim, oracle.valid_cpts, oracle.new_mean_stds)
    except tr.TomboErrorLike as e:
        return 'TomboError: %s' % e
    except ValueError as e:
        return 'ValueError: %s' % e


def recorded(golden, case):
    err = str(golden['err_' + case.name])
    return err if err else int(golden['f64_' + case.name])


@pytest.mark.parametrize('case', tc.CASES, ids=lambda c: c.name)
def test_restatement_equals_the_live_reference(golden, case):
    raw = tc.signal(case)
    assert hashlib.sha256(raw.tobytes()).hexdigest() == str(golden['sha_' + case.name])
    assert int(golden['ties_' + case.name]) == 0
    assert expected(raw, case) == recorded(golden, case)


def test_cases_cover_the_issue_and_the_branches(golden):
    by = tc.BY_NAME
    assert [by[k].n for k in ('n2234', 'n2235', 'n2249', 'n2250', 'n39999', 'n40000', 'n40001', 'n70000')] == \
        [2234, 2235, 2249, 2250, 39999, 40000, 40001, 70000]
    assert all(by[k].trim == tc.DEFAULT_TRIM and by[k].seg == tc.RNA_SEG for k in ('n2234', 'n40001', 'n70000'))
    assert sorted(c.trim[0] for c in tc.CASES if c.name.startswith('mw')) == [1, 8, 9, 128, 130]
    assert by['mr1'].trim[1] == 1 and by['ts0'].trim[2] == 0.0 and by['dna_seg'].seg == (5, 3, 5)
    assert by['cap_below'].trim[3] < by['cap_below'].n < by['cap_above'].trim[3]
    assert by['cap150k'].n == by['cap150k'].trim[3] == 150000
    assert 150000 // 15 - 1 - 50 + 1 > 8192             # more than one block of numpy's sum enters the mean
    assert str(golden['err_n2234']) == 'ValueError: negative dimensions are not allowed'
    assert str(golden['err_fewer_cpts']) == 'TomboError: Fewer changepoints found than requested'
    assert int(golden['f64_n2235']) == 0 and int(golden['f64_no_window']) == 0 and int(golden['f64_first_window']) > 0
    meta = json.loads(str(golden['meta']))
    assert len(meta['cases']) == len(tc.CASES) and meta['dac_differs'] >= 0

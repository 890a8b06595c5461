"""tests/filter_reference.py (the numpy restatement of the read filters) against the live reference's recorded
outputs in tests/golden/stats_filters.npz: output index tuples in order, counts through the message text, the
seeded draw.  Everything is integers, booleans and strings: compared exactly."""
import numpy as np
import pytest

import filter_reference as fref

DOC, LENS = fref.fixture()
CASES = [c for c in DOC['cases'] if c['error'] is None]


def test_fixture_holds_what_the_tests_rely_on():
    assert DOC['empty_percentile'] == 'IndexError'      # np.percentile of no lengths raises: such a read is stuck
    assert DOC['empty_index_error'] == 'Cannot replace with an empty index.'
    keys = [(c, s) for c, s, _ in DOC['index']]
    assert len(set(c for c, _ in keys)) == 2 and len(set(s for _, s in keys)) == 2
    assert any(len(recs) == 1 for _, _, recs in DOC['index'])
    recs = [r for _, _, rs in DOC['index'] for r in rs]
    assert any(r[fref.FILT] for r in recs) and any(r[fref.SMS] is None for r in recs)
    assert any(r[fref.MQ] is None for r in recs) and sorted(set(DOC['kind'])) == [0, 1, 2, 3]
    assert len(LENS) == len(recs) and {1, 2} <= set(len(v) for v in LENS)
    assert len([c for c in DOC['cases'] if c['error'] is not None]) == 5
    assert all(c['error'] == ['exit', 'No unfiltered reads present in current Tombo index.']
               for c in DOC['cases'] if c['error'] is not None)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_restatement_equals_the_reference(case):
    out, counts, text = fref.run_case(case, DOC, LENS)
    assert out == case['out']
    if counts is not None:
        assert fref.counts_message(*counts, filter_text=text) in case['messages']


def test_stuck_cases_sit_on_their_thresholds():
    """the fixture's edge reads: a percentile equal to the threshold stays, one above it is filtered"""
    for pairs, stays, goes in (([(99, 200)], 0, 1), ([(50, 8), (100, 5000)], 2, 3), ([(50, 8), (100, 5000)], 2, 4),
                               ([(0, 1)], 5, 6)):
        v_stay = [np.percentile(LENS[stays], p) for p, _ in pairs]
        assert any(v == t for v, (_, t) in zip(v_stay, pairs)) and not any(v > t for v, (_, t) in zip(v_stay, pairs))
        assert any(np.percentile(LENS[goes], p) > t for p, t in pairs)
    segs = np.concatenate([np.concatenate([[0], np.cumsum(v, dtype=np.int64)]) for v in LENS])
    off = np.concatenate([[0], np.cumsum([len(v) + 1 for v in LENS])]).astype(np.int64)
    vals, flags = fref.dwell_pctl_flags(segs, off, [(99, 200)])
    assert not flags[0] and flags[1] and vals[0, 0] == 200.0 and vals[1, 0] == 201.0
    assert np.isnan(vals[11, 0]) and flags[11]            # the empty table

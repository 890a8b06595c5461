"""The skipped-base stage (k_skip_plan, k_skip_dp<>, k_skip_dp_wave<> of k_tail.h) in every form, against the oracle:
both storages of the window planner (at most / more than SKP_LDS_DELS skipped bases), the column and the flat form out
of LDS, the three wave queues, the windows left to global scratch, and each status the planner gives.

The reads are the cases of tests/skip_cases.py, whose classes and statuses tests/test_skip_cases_reference.py holds to
the header's thresholds and to the oracle on the CPU.  Alone through rq.resolve_skipped_bases_with_raw, and all reads of
a sample type as one batch through the stage entry: there the window queues hold windows of several reads and a
failing read sits between reads that pass."""
import numpy as np
import pytest

import skip_cases as S

pytestmark = pytest.mark.gpu

CASES = S.cases()
_want = {}


def _oracle(case, default_args=False):
    key = (case.name, default_args)
    if key not in _want:
        _want[key] = S.oracle_result(case, **(dict(max_raw_cpts=200) if default_args else {}))
    return _want[key]


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_case_alone_vs_oracle_on_gpu(case):
    from tombo_amd import resquiggle as rq, errors, tombo_helper as th
    status, want = _oracle(case)
    assert status == case.status
    args = (S.dp_results(case), case.norm, S.rsqgl_params(case.samp))
    kw = dict(dict(max_raw_cpts=200), **case.kw)
    if status != 0:
        with pytest.raises(th.TomboError) as ei:
            rq.resolve_skipped_bases_with_raw(*args, **kw)
        assert str(ei.value) == errors.MESSAGES[status]
    else:
        np.testing.assert_array_equal(rq.resolve_skipped_bases_with_raw(*args, **kw), want)


def _run_batch(samp, cases):
    """the reads as one batch through the stage entry at the default arguments -> (boundaries, statuses, seg_off)"""
    from tombo_amd import _native as N, resquiggle as rq
    params = S.rsqgl_params(samp)
    eng = rq.get_engine()
    eng.ensure_model(rq._LevelsOnly)
    pad = 4 * int(params.running_stat_width) + 2
    norms = [np.concatenate([c.norm, np.zeros(max(0, pad - c.norm.shape[0]))]) for c in cases]
    eng.set_num_events([2] * len(cases))
    eng.upload(N.make_params(params), N.make_opts(max_raw_cpts=200), norms,
               [np.zeros(c.means.shape[0] + 1, np.uint8) for c in cases])
    assert eng.seg_off.tolist() == np.concatenate([[0], np.cumsum([c.segs.shape[0] for c in cases])]).tolist()
    eng.put(N.PUT_NORM, np.concatenate(norms))
    eng.put(N.PUT_REF_MEANS, np.concatenate([c.means for c in cases]))
    eng.put(N.PUT_REF_SDS, np.concatenate([c.sds for c in cases]))
    eng.put(N.PUT_DP_SEGS, np.concatenate([c.segs for c in cases]),
            per_read=np.array([[0, c.norm.shape[0]] for c in cases], np.int64).reshape(-1))
    eng.run_stages(N.STAGE_SKIP, N.STAGE_SKIP)
    return eng.get(N.GET_SEGS), eng.get(N.GET_STATUS), eng.seg_off.copy()


@pytest.mark.parametrize('samp', ['DNA', 'RNA'])
def test_batch_through_the_stage_entry_vs_oracle_on_gpu(samp):
    cases = [c for c in CASES if c.samp == samp]
    segs, status, off = _run_batch(samp, cases)
    want = [_oracle(c, default_args=True) for c in cases]
    assert status.tolist() == [st for st, _ in want]
    assert sorted(set(status.tolist())) == [0, S.TBA_NOT_ENOUGH_DEL_SIGNAL]
    for i, (c, (st, w)) in enumerate(zip(cases, want)):
        if st == 0:
            np.testing.assert_array_equal(segs[off[i]:off[i + 1]], w, err_msg=c.name)
    # run to run: the same bytes (the queues are filled by atomics, in whatever order the reads' planners get there)
    segs2, status2, _ = _run_batch(samp, cases)
    assert segs2.tobytes() == segs.tobytes() and status2.tobytes() == status.tobytes()

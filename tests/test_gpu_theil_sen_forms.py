"""k_theil_sen (csrc/k_tail.h) in every form it has, against a float64 reference on the CPU, bit for bit.

The kernel picks per read between the one-pass form (a sampled window, the pairs inside it listed and divided exactly)
and the generic two-pass select over all n (n - 1) / 2 slopes, and declines the one-pass form for four reasons.
TBA_GET_TS_FORM says which ran and why.  A natural read of 256 bases or more reports FAST -- the production
expectation, which the last test states on a 10 kb DNA batch -- so the reads here are the cases of
tests/theil_cases.py, fed to the kernel as exact points through the stage entry: each alone, and all as one batch with
a read that failed earlier in the middle.  tests/test_theil_cases_reference.py holds the cases to the properties they
are named for on the CPU.

Tolerance: none.  Columns 2 and 3 of TBA_GET_THEIL_SEN are -inter / slope and 1 / slope of np.median over
oracle.compute_slopes and over m - slope * e; columns 0 and 1 the kernel's own expression over the scale values read
back from the engine."""
import collections

import numpy as np
import pytest

import skip_cases
import theil_cases as TC

pytestmark = pytest.mark.gpu

CASES = TC.cases()
Run = collections.namedtuple('Run', 'status fit form prev')
_alone = {}


def _run_batch(cases):
    """the reads as one batch through the stage entry: skipped-base stage (no read of theil_cases has one), Theil-Sen,
    rescale -> Run of per-read arrays"""
    from tombo_amd import _native as N, resquiggle as rq
    eng = rq.get_engine()
    eng.ensure_model(rq._LevelsOnly)
    samp = None
    if any(getattr(c, 'samp_ind', None) is not None for c in cases):
        samp = N.pack_samp_inds([getattr(c, 'samp_ind', None) for c in cases])
    eng.set_num_events([2] * len(cases))
    eng.upload(N.make_params(skip_cases.rsqgl_params('DNA')), N.make_opts(max_raw_cpts=200), [c.norm for c in cases],
               [np.zeros(c.means.shape[0] + 1, np.uint8) for c in cases], samp_ind=samp)
    eng.put(N.PUT_NORM, np.concatenate([c.norm for c in cases]))
    eng.put(N.PUT_REF_MEANS, np.concatenate([c.means for c in cases]))
    eng.put(N.PUT_REF_SDS, np.concatenate([c.sds for c in cases]))
    eng.put(N.PUT_DP_SEGS, np.concatenate([c.segs for c in cases]),
            per_read=np.array([[0, c.norm.shape[0]] for c in cases], np.int64).reshape(-1))
    prev = eng.get(N.GET_SEG_SV)
    eng.run_stages(N.STAGE_SKIP, N.STAGE_RESCALE)
    return Run(eng.get(N.GET_STATUS), eng.get(N.GET_THEIL_SEN), eng.get(N.GET_TS_FORM), prev)


def _run_alone(case):
    if case.name not in _alone:
        r = _run_batch([case])
        _alone[case.name] = Run(int(r.status[0]), r.fit[0], r.form[0], r.prev[0])
    return _alone[case.name]


def _form_name(form):
    return TC.FORMS[int(form[0])]


def _same(a, b):
    """bit for bit, any NaN taken for any other"""
    a, b = np.float64(a), np.float64(b)
    return a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))


def _check_fit(case, run):
    from tombo_amd import _native as N
    ref = TC.reference_fit(case)
    assert run.status == ref.status == case.status, (case.name, run.status)
    n = ref.e.shape[0]
    assert 0 <= run.form[1] <= n * (n - 1) // 2 + n * (-n % 64)     # (pairs, and a row's partners in the padding to 64)
    if _form_name(run.form) in ('SMALL', 'NO_SCRATCH', 'NO_WINDOW'):
        assert run.form[1] == 0             # the pass over the pairs did not run
    if ref.status != TC.TBA_OK:
        return
    print('%s: form %s listed %d slope %r' % (case.name, _form_name(run.form), run.form[1], ref.slope))
    assert _same(run.fit[2], ref.shift_corr) and _same(run.fit[3], ref.scale_corr), (case.name, run.fit, ref[:5])
    with np.errstate(all='ignore'):         # (the kernel's expressions; the stage entry leaves shift = scale = 0)
        want0, want1 = run.prev[0] + (ref.shift_corr * run.prev[1]), run.prev[1] * ref.scale_corr
    assert _same(run.fit[0], want0) and _same(run.fit[1], want1), (case.name, run.fit, run.prev)
    assert N.TS_FORM_NONE == 0 and TC.FORMS[N.TS_FORM_WINDOW_MISS] == 'WINDOW_MISS'


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_case_alone_bit_for_bit_and_its_form(case):
    run = _run_alone(case)
    _check_fit(case, run)
    if case.form is not None:
        assert _form_name(run.form) == case.form, (case.name, run.form)
    if case.name in ('d_all_1.0', 'h_collinear', 'i_cancel', 'i_2pm160', 'i_2p200'):
        # every pair listed: each store past the list's cap went through the guard.  Infinite float copies list the
        # 24 partners that pad 1000 points to a multiple of 64 as well (theil_cases.listed_pairs)
        assert run.form[1] == 499500 + (24 * 1000 if case.name == 'i_2p200' else 0)


def test_scratch_edge_group_reaches_both_slices_and_the_overflow():
    """1000 points over 2048 .. 4200 raw samples: every fit exact (above), and -- a coverage condition of these
    inputs, not a correctness expectation -- the group holds a read whose list crossed from the first scratch slice
    into the second (FAST with more listed pairs than raw samples) and a read whose list overflowed"""
    g = [c for c in CASES if c.name.startswith('g_')]
    runs = [_run_alone(c) for c in g]
    seen = [(c.norm.shape[0], _form_name(r.form), int(r.form[1])) for c, r in zip(g, runs)]
    print(seen)
    for c, r in zip(g, runs):
        _check_fit(c, r)
        assert _form_name(r.form) in ('FAST', 'LIST_OVERFLOW', 'WINDOW_MISS'), seen
        assert (_form_name(r.form) == 'LIST_OVERFLOW') == (r.form[1] > 2 * c.norm.shape[0]), seen
    assert any(f == 'FAST' and listed > n_raw for n_raw, f, listed in seen), seen
    assert any(f == 'LIST_OVERFLOW' for _, f, _ in seen), seen


def test_all_cases_as_one_batch_equal_their_runs_alone():
    """every case in one batch, a read that failed in the skipped-base stage in the middle, the read that lists all
    its 499 500 pairs between two reads of the one-pass form (their lists are neighbours in the scratch: a store past
    the cap would land in one of them): every read as alone, bit for bit, and the same bytes run to run"""
    from tombo_amd import _native as N
    order = [c for c in CASES if c.name != 'd_all_1.0']
    at = [c.name for c in order].index('a_999')
    order.insert(at + 1, TC.by_name('d_all_1.0'))
    assert [c.name for c in order[at:at + 3]] == ['a_999', 'd_all_1.0', 'a_1000']
    failed = [c for c in skip_cases.cases() if c.name == 'dna_300_starved'][0]
    mid = len(order) // 2
    batch = order[:mid] + [failed] + order[mid:]
    run = _run_batch(batch)
    assert run.status[mid] == skip_cases.TBA_NOT_ENOUGH_DEL_SIGNAL
    assert run.form[mid].tolist() == [N.TS_FORM_NONE, 0] and not run.fit[mid].any()
    for k, c in enumerate(batch):
        if k == mid:
            continue
        alone = _run_alone(c)
        assert run.status[k] == alone.status and run.form[k].tolist() == alone.form.tolist(), c.name
        assert run.fit[k].tobytes() == alone.fit.tobytes(), c.name
    assert [_form_name(run.form[k]) for k in (at, at + 1, at + 2)] == ['FAST', 'LIST_OVERFLOW', 'FAST']
    again = _run_batch(batch)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(run, again))
    # every decline reason and both designed forms were reached
    assert {_form_name(f) for f in run.form} == set(TC.FORMS)


def test_natural_10kb_dna_reads_take_the_one_pass_form():
    """the production expectation the cases above deviate from: every read of a synthetic 10 kb DNA batch that
    reaches the fit (1000 subsampled points) reports FAST"""
    from tombo_amd import _native as N
    from test_gpu_determinism import _device_batch
    eng, gen = _device_batch('DNA', 64, 10000, 20261021)[:2]
    eng.run()
    status, form = eng.get(N.GET_STATUS), eng.get(N.GET_TS_FORM)
    eng.close(), gen.close()
    ok = status == 0
    assert ok.sum() >= 60, status
    assert (form[ok, 0] == N.TS_FORM_FAST).all(), form
    assert (form[ok, 1] > 0).all() and (form[ok, 1] < 65536).all()
    assert not form[~ok].any()

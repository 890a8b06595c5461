"""The cases of tests/skip_cases.py, held to what they claim on the CPU: each lands in the form of the skipped-base
stage (k_tail.h) it is there for, under the thresholds the header has today, and the oracle gives the status listed.
A moved threshold, a changed generator or an edited table that stops reaching a form fails here, not silently on the
GPU (test_gpu_skip_paths.py)."""
import collections

import numpy as np
import pytest

import skip_cases as S

CASES = S.cases()


def test_thresholds_are_read_from_the_header():
    T = S.thresholds()
    assert set(T) >= {'SKL_LEN', 'SKL_N', 'SKL_FLAT_N', 'SKL_FLAT_LEN', 'SKL_FLAT_WORDS', 'SKIP_WAVE_MIN', 'SKIP_LEN_S',
                      'SKIP_BITS_S', 'SKIP_LEN_M', 'SKIP_BITS_M', 'SKIP_LEN_B', 'SKIP_BITS_B', 'SKP_LDS_DELS'}
    assert all(v > 0 for v in T.values())
    # (the two derived ones, by hand from the header's expressions)
    assert T['SKL_FLAT_LEN'] == (T['SKL_LEN'] + 8) * 64 // T['SKL_FLAT_N'] - 8
    assert T['SKL_FLAT_WORDS'] == T['SKL_N'] * 64 // T['SKL_FLAT_N']
    assert T['SKIP_LEN_S'] < T['SKIP_LEN_M'] < T['SKIP_LEN_B'] and T['SKL_LEN'] < T['SKL_FLAT_LEN']


def test_the_planner_restatement_on_hand_made_boundaries():
    # one skipped base, windows of five bases: (n, len) = (5, 12 - 4 m); a neighbour two bases on joins the window
    segs = np.cumsum([0, 3, 3, 3, 0, 3, 3, 3, 3])
    assert S.get_deletion_windows(segs, 1) == (0, [(5, 8)])
    assert S.get_deletion_windows(segs, 2) == (0, [(7, 6)])        # 12 <= 6 * 2 * 1.1: widened once to 18 samples
    segs = np.cumsum([0, 3, 3, 3, 0, 3, 0, 3, 3, 3])
    assert S.get_deletion_windows(segs, 1) == (0, [(7, 9)])
    assert S.get_deletion_windows(segs, 1, max_raw_cpts=6) == (S.TBA_TOO_MANY_DELS, [])
    assert S.get_deletion_windows(segs, 1, max_raw_cpts=None, extra_sig_factor=9.0) == (S.TBA_NOT_ENOUGH_DEL_SIGNAL, [])
    assert S.get_deletion_windows(np.arange(9), 1) == (0, [])
    T = S.thresholds()
    assert S.window_class(T['SKL_N'], T['SKL_LEN'], 1, T) == 'column'
    assert S.window_class(T['SKL_N'] + 1, T['SKL_LEN'], 1, T) == S.window_class(2, T['SKL_LEN'] + 1, 1, T) == 'flat'
    assert S.window_class(2, T['SKL_FLAT_LEN'] + 1, 1, T) == 'arena'
    assert S.window_class(2, T['SKIP_WAVE_MIN'] // 2 - 1, 2, T) == 'arena'
    assert S.window_class(2, T['SKIP_LEN_S'], 2, T) == 'S' and S.window_class(2, T['SKIP_LEN_S'] + 1, 2, T) == 'M'
    assert S.window_class(2, T['SKIP_LEN_B'], 2, T) == 'B' and S.window_class(2, T['SKIP_LEN_B'] + 1, 2, T) == 'arena'


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_case_lands_in_its_class_and_status(case):
    status, ws = S.windows(case)
    assert status == case.status
    assert dict(collections.Counter(w[2] for w in ws)) == case.classes
    ost, segs = S.oracle_result(case)
    assert ost == case.status
    if ost == 0:
        assert np.all(np.diff(segs) >= 1) and segs[0] == case.segs[0] and segs[-1] == case.segs[-1]
        # only the interiors of windows move
        assert (segs != case.segs).sum() >= S.n_skipped(case)


def test_every_form_and_both_planners_are_reached():
    T = S.thresholds()
    reached = collections.Counter()
    for case in CASES:
        side = 'lds' if S.n_skipped(case) <= T['SKP_LDS_DELS'] else 'global'
        for cls in case.classes or [None]:
            reached[(side, case.samp, cls, case.status)] += 1
    by = lambda **kw: [k for k in reached if all(k['side samp cls status'.split().index(n)] == v for n, v in kw.items())]
    for cls, samp in (('column', 'DNA'), ('flat', 'DNA'), ('arena', 'DNA'), ('S', 'RNA'), ('M', 'RNA'), ('B', 'RNA'), ('arena', 'RNA')):
        assert by(samp=samp, cls=cls), (samp, cls)
    # the planner over global memory: every decision it repeats -- column, flat, the queues, the arena, each failure
    for samp, cls in (('DNA', 'column'), ('DNA', 'flat'), ('RNA', 'S'), ('RNA', 'arena')):
        assert by(side='global', samp=samp, cls=cls), (samp, cls)
    for status in (S.TBA_NOT_ENOUGH_DEL_SIGNAL, S.TBA_TOO_MANY_DELS):
        assert by(side='global', status=status), status
    assert by(side='lds', status=S.TBA_NOT_ENOUGH_DEL_SIGNAL)
    skipped = sorted(S.n_skipped(c) for c in CASES)
    assert T['SKP_LDS_DELS'] in skipped and T['SKP_LDS_DELS'] + 1 in skipped and 0 in skipped
    # more flat windows in one read than one round of the flat phase takes; arena windows past the flat form by flag
    # words and by length; an RNA window too long for the largest queue
    named = {c.name: c for c in CASES}
    assert named['dna_flat_rounds'].classes['flat'] > T['SKL_FLAT_N']
    (n, ln, _), = S.windows(named['dna_arena_words'])[1]
    assert ln <= T['SKL_FLAT_LEN'] and n * ((ln + 63) // 64) > T['SKL_FLAT_WORDS']
    (n, ln, _), = S.windows(named['dna_arena_len'])[1]
    assert ln > T['SKL_FLAT_LEN']
    lens = [(ln, cls) for _, ln, cls in S.windows(named['rna_every_form'])[1]]
    assert max(lens)[0] > T['SKIP_LEN_B'] and max(lens)[1] == 'arena' and min(lens)[1] == 'arena'
    # the widening case widens and merges: fewer windows than skipped bases, windows of more than five bases
    ws = S.windows(named['dna_300_widening'])[1]
    assert len(ws) < 300 and max(n for n, _, _ in ws) > T['SKL_N'] and min(n for n, _, _ in ws) == 5


@pytest.mark.parametrize('samp', ['DNA', 'RNA'])
def test_the_batch_of_a_sample_type_mixes_failing_and_passing_reads(samp):
    """at the default arguments (what the batch entry runs all reads with) at least one read fails between reads that
    pass, and the passing ones still cover every class of the sample type"""
    sts = [S.oracle_result(c, max_raw_cpts=200)[0] for c in CASES if c.samp == samp]
    assert S.TBA_NOT_ENOUGH_DEL_SIGNAL in sts[1:-1] and sts.count(0) >= 3 and sts[0] == 0 and sts[-1] == 0
    m = S.raw_min_obs(samp)
    classes, reads_of = set(), collections.Counter()
    for c in CASES:
        if c.samp == samp:
            st, ws = S.get_deletion_windows(c.segs, m)
            mine = set(S.window_class(n, ln, m) for n, ln in ws) if st == 0 else set()
            classes |= mine
            reads_of.update(mine)
    assert classes == ({'column', 'flat', 'arena'} if samp == 'DNA' else {'S', 'M', 'B', 'arena'})
    # every window queue of k_skip_dp_wave holds windows of more than one read of the batch
    assert samp == 'DNA' or all(reads_of[q] >= 2 for q in 'SMB'), reads_of

"""The traceback walkers off their fast paths, against the oracle: tbp_block's slow path of a row (k_tb_par.h: a stay
run that leaves the 64-cell window) in phase A, phase B, the verifier and the serial walk, the rows around chunk tops,
k_main_tb_long's ballot fallback (k_long.h), and the band-edge status whichever kernel finds it.

No read of the synthetic generator gets there (8-9 events per base at the most): the reads are the stutters of
tests/tb_cases.py, whose tables tests/test_tb_cases_reference.py holds to the oracle on the CPU.  Every read is compared
on everything compare_batch compares; TBA_GET_TB_FORM says which kernel finished it.  DNA only.

Not reached here either: tbp_block's walk through negative band positions (Python's wrap-around), which needs move rows
a genuine forward pass does not produce."""
import time

import numpy as np
import pytest

import tb_cases as T
from test_gpu_parity import run_batch, compare_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dna():
    return T.dna()


def _run(dna, bw, cases, label):
    """the batch through the engine and the oracle, equal on everything, the verifier silent
    -> (engine, out, oracles, tb_form, path)"""
    from tombo_amd import _native as N
    model, params = dna
    t0 = time.perf_counter()
    eng, out, oracles = run_batch(model, params[bw], 'DNA', [T.make_read(model, c) for c in cases])
    bad = compare_batch(eng, oracles, out, label)
    assert not bad, '%d mismatches\n' % len(bad) + '\n'.join(bad[:40])
    vf = eng.get(N.GET_TB_VERIFY_FAIL)
    assert not vf.any(), ('the traceback verifier disagreed', np.flatnonzero(vf).tolist())
    tb, path = eng.get(N.GET_TB_FORM), eng.get(N.GET_PATH)
    print('%s: %d reads, %.2f s, TB_FORM %s' % (label, len(cases), time.perf_counter() - t0,
                                               dict(zip(*[x.tolist() for x in np.unique(tb, return_counts=True)]))))
    return eng, out, oracles, tb, path


def _par_form(form):
    from tombo_amd import _native as N
    return N.TB_FORM_PAR64 if form == 'latency' else N.TB_FORM_PAR16


def _finished_by_the_chunk_kernel(tb, sel, form, cases, label):
    """the reads `sel` were finished by the chunk kernel of the form; a read it gave back (a chain without agreement:
    legal) was walked by k_main_tb -- named, and never more than half of the batch"""
    from tombo_amd import _native as N
    back = [i for i in sel if tb[i] != _par_form(form)]
    msg = '%s: reads the chunk kernel gave back: %s' % (label, [(i, int(tb[i]), tuple(cases[i])) for i in back])
    if back:
        print(msg)
    assert all(tb[i] == N.TB_FORM_LANE for i in back), msg
    assert 2 * len(back) <= len(sel), msg
    return back


@pytest.mark.parametrize('bw', [500, 300, 100, 1000])
def test_run_length_ladder_vs_oracle_on_gpu(dna, dispatch_form, bw):
    """one base with 10-16, 17-32, 33-47, 48-64, >= 66 and >= 100 events (W = 100: up to 47, W = 1000: from 66) next to
    the plain read; at W = 500 also runs of >= 66 events on the first bases after the masked start"""
    cases = [T.Case(bw, 2000, 3, None, 0)] + [c for _, c in T.LADDER[bw]]
    buckets = [(0, 9)] + [b for b, _ in T.LADDER[bw]]
    if bw == 500:
        cases += [c for _, c in T.AFTER_STATIC]
        buckets += [(66, None)] * len(T.AFTER_STATIC)
    label = 'ladder W=%d %s' % (bw, dispatch_form)
    eng, out, oracles, tb, path = _run(dna, bw, cases, label)
    for case, o, (fewest, most) in zip(cases, oracles, buckets):
        assert o['status'] == 0, case
        n = T.longest_run(o)[1]
        assert n >= fewest and (most is None or n <= most), (case, n)
    assert np.all(path[:, 0] == 1)
    _finished_by_the_chunk_kernel(tb, range(len(cases)), dispatch_form, cases, label)


@pytest.mark.parametrize('bw', [300, 500])
def test_run_length_sweep_vs_oracle_on_gpu(dna, dispatch_form, bw):
    """runs of 17 to 66 events on one base, nearly every length: the position the walk enters the row at on every cell
    in turn above the end of the run -- each alignment to the dwords and halves of tbp_block's window"""
    first, count = T.SWEEP[bw]
    cases = [first._replace(J=first.J + k) for k in range(count)]
    label = 'sweep W=%d %s' % (bw, dispatch_form)
    eng, out, oracles, tb, path = _run(dna, bw, cases, label)
    assert all(o['status'] == 0 for o in oracles)
    lengths = set(T.longest_run(o)[1] for o in oracles)
    assert set(range(25, 49)) <= lengths and len(lengths) >= 40, sorted(lengths)
    _finished_by_the_chunk_kernel(tb, range(len(cases)), dispatch_form, cases, label)


@pytest.mark.parametrize('bw', [300, 500])
def test_runs_that_end_under_the_window_vs_oracle_on_gpu(dna, dispatch_form, bw):
    """the run ends on the very cell where tbp_block's slow path takes over from the window: the restart position of
    `act && !fast` one cell off in either direction loses or repeats that cell"""
    cases = [c for c, _ in T.UNDER_WINDOW[bw]]
    label = 'under the window W=%d %s' % (bw, dispatch_form)
    eng, out, oracles, tb, path = _run(dna, bw, cases, label)
    for (case, leave), o in zip(T.UNDER_WINDOW[bw], oracles):
        assert o['status'] == 0 and int(T.run_profile(o)[1][case.where]) == leave, case
    _finished_by_the_chunk_kernel(tb, range(len(cases)), dispatch_form, cases, label)


@pytest.mark.parametrize('bw', [300, 500])
def test_long_runs_at_chunk_tops_vs_oracle_on_gpu(dna, dispatch_form, bw):
    """a run of >= 66 events in the row at +1, 0, -1, -2, -15, -16, -17 from the first, a middle and the last chunk
    top of the kernel of the form: the first row of a phase A, of a phase B, of its second block, of the verifier"""
    lanes = T.LANES[dispatch_form]
    rows = T.CHUNK_TOPS[(bw, lanes)]
    cases = [c for _, _, c in rows]
    label = 'tops W=%d %s' % (bw, dispatch_form)
    eng, out, oracles, tb, path = _run(dna, bw, cases, label)
    reached = set()
    for i, (case, o) in enumerate(zip(cases, oracles)):
        assert o['status'] == 0, case
        row, n = T.longest_run(o)
        assert n >= 66, (case, n)
        # the geometry the ENGINE walked this read with: its own n_static
        _, tops = T.chunk_tops(case.nb, int(path[i, 1]), lanes)
        c, off = T.top_offset(row, tops)
        which = {1: 'first', len(tops) // 2: 'middle', len(tops) - 1: 'last'}.get(c)
        reached.add((which, off))
    assert reached == set((w, off) for w in ('first', 'middle', 'last') for off in T.TOP_OFFSETS), sorted(reached, key=str)
    assert np.all(path[:, 0] == 1)
    _finished_by_the_chunk_kernel(tb, range(len(cases)), dispatch_form, cases, label)


def test_long_reads_with_long_runs_vs_oracle_on_gpu(dna, dispatch_form):
    """four reads of 24 800 bases (is_long): plain, a run of 20-31 events (past the 16 cells k_main_tb_long always looks
    back over), one of >= 66 (its ballot over the whole row), a failing stutter (its own band-edge exit).  Latency
    form: the chunk kernels do not take long reads, k_main_tb_long walks all four; throughput form: k_main_tb_par<64>
    through the index list"""
    from tombo_amd import _native as N
    cases = [c for _, c in T.LONG]
    label = 'long %s' % dispatch_form
    eng, out, oracles, tb, path = _run(dna, 500, cases, label)
    assert [o['status'] for o in oracles] == [0, 0, 0, T.TBA_BEYOND_BANDWIDTH]
    assert out['status'].tolist() == [0, 0, 0, T.TBA_BEYOND_BANDWIDTH]
    n = [T.longest_run(o)[1] for o in oracles[:3]]
    assert n[0] <= 16 and 20 <= n[1] <= 31 and n[2] >= 66, n
    if dispatch_form == 'latency':
        assert tb.tolist() == [N.TB_FORM_LONG] * 4
    else:
        assert tb[:3].tolist() == [N.TB_FORM_PAR64] * 3
        assert tb[3] in (N.TB_FORM_PAR64, N.TB_FORM_LONG)


@pytest.mark.parametrize('bw', [300, 500])
def test_band_edge_status_around_a_chunk_top_vs_oracle_on_gpu(dna, dispatch_form, bw):
    """failing stutters at 24 consecutive bases spanning a middle chunk top: every status the oracle's (a mix of 0 and
    TBA_BEYOND_BANDWIDTH).  A status 11 with the form of the chunk kernel is a phase A's on the true path; with
    TB_FORM_LANE a phase B met the violation first, the read went to k_main_tb and the serial walk's band-edge exit
    gave the status."""
    from tombo_amd import _native as N
    lanes = T.LANES[dispatch_form]
    first, want = T.BAND_EDGE[(bw, lanes)]
    cases = [first._replace(where=first.where + k) for k in range(len(want))]
    label = 'edge W=%d %s' % (bw, dispatch_form)
    eng, out, oracles, tb, path = _run(dna, bw, cases, label)
    assert [o['status'] for o in oracles] == want
    assert out['status'].tolist() == want
    failed = np.array(want) == T.TBA_BEYOND_BANDWIDTH
    n_par, n_lane = int((tb[failed] == _par_form(dispatch_form)).sum()), int((tb[failed] == N.TB_FORM_LANE).sum())
    print('%s: status 11 from the chunk kernel: %d, from k_main_tb: %d (reads %s)' % (
        label, n_par, n_lane, np.flatnonzero(failed & (tb == N.TB_FORM_LANE)).tolist()))
    assert n_par + n_lane == int(failed.sum()), np.unique(tb[failed]).tolist()
    assert n_par >= 1
    # (what the oracle cannot say, it has no row of the violation; measured on an MI355X: 3 / 6 of these reads in the
    # latency form at W = 300 / 500, 7 / 4 in the throughput form)
    assert n_lane >= 1, 'no read reached the band-edge exit of the serial walk'
    _finished_by_the_chunk_kernel(tb, np.flatnonzero(~failed).tolist(), dispatch_form, cases, label)

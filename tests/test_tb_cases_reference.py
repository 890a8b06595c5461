"""The case tables of tests/tb_cases.py, held to what they claim by the CPU oracle: the reads of test_gpu_tb_paths.py
reach the slow paths of the traceback walkers (k_tb_par.h, k_long.h) only while a stutter really gives one base its
run of events, in the row the table says.  An edited table, a changed generator or a changed oracle that stops
reaching a branch fails here, not silently on the GPU."""
import numpy as np
import pytest

import tb_cases as T

_cache = {}


@pytest.fixture(scope='module')
def orc():
    model, params = T.dna()

    def get(case):
        if case not in _cache:
            _cache[case] = T.oracle_read(model, params[case.bandwidth], case)
        return _cache[case]
    return get


def _run_on_its_base(o, case, fewest, most=None):
    """status 0, the longest run of the read on base `where` (row where + 1), fewest..most events long -> n_static"""
    assert o['status'] == 0, (case, o['status'])
    row, n = T.longest_run(o)
    assert row == case.where + 1, (case, row)
    assert n >= fewest and (most is None or n <= most), (case, n, fewest, most)
    # the run is one base's: its neighbours have what a plain read has
    per_base, _ = T.run_profile(o)
    assert np.delete(per_base, case.where).max() <= 16, case
    return int(o['dbg']['mask_seq_len'])


def test_the_stutter_is_what_the_docstring_says():
    from tombo_amd import synth
    model, _ = T.dna()
    seq0, raw0, starts = synth.synth_read(model, 300, 5, **synth.DNA_SYNTH)
    seq, raw = T.stutter_read(model, 300, 5, 100, 7)
    assert seq == seq0 and raw.shape[0] == raw0.shape[0] + 7 * 9
    b = int(starts[101])
    np.testing.assert_array_equal(raw[:b], raw0[:b])
    np.testing.assert_array_equal(raw[b + 63:], raw0[b:])
    level = raw0[int(starts[100]):b].mean()
    seg_means = raw[b:b + 63].reshape(7, 9).mean(axis=1) - level
    assert np.all(np.abs(np.abs(seg_means) - 2.0) < 1.0) and np.all(np.sign(seg_means) == [1, -1, 1, -1, 1, -1, 1])
    np.testing.assert_array_equal(T.stutter_read(model, 300, 5, 100, 7)[1], raw)      # deterministic
    np.testing.assert_array_equal(T.stutter_read(model, 300, 5, None, 0)[1], raw0)


def test_chunk_tops_restate_the_kernels_geometry():
    # (values worked out by hand from tbp_chunks, k_tb_par.h)
    assert T.chunk_tops(2000, 140, 16) == (116, [2000 - 116 * c for c in range(16)])
    assert T.chunk_tops(2000, 140, 64) == (64, [2000 - 64 * c for c in range(29)])
    assert T.chunk_tops(2000, 85, 16)[0] == 119 and len(T.chunk_tops(2000, 85, 64)[1]) == 30
    assert T.chunk_tops(100, 85, 16) == (64, [100])            # top_rows < 1 -> one chunk
    assert T.chunk_tops(24800, 140, 64)[0] == 386
    assert T.top_offset(1070, T.chunk_tops(2000, 140, 16)[1]) == (8, -2)


@pytest.mark.parametrize('bw', sorted(T.LADDER))
def test_ladder_covers_each_rung(orc, bw):
    want = {500: 6, 300: 6, 100: 3, 1000: 2}[bw]
    rungs = [(10, 16), (17, 32), (33, 47), (48, 64), (66, 99), (100, None)]
    assert [b for b, _ in T.LADDER[bw]] == (rungs[:3] if bw == 100 else rungs[-want:])
    for (fewest, most), case in T.LADDER[bw]:
        assert case.bandwidth == bw
        _run_on_its_base(orc(case), case, fewest, most)
    # what the plain read of the same seed has: nothing a walker leaves its fast path for
    plain = orc(T.Case(bw, 2000, 3, None, 0))
    assert plain['status'] == 0 and T.longest_run(plain)[1] <= 9


@pytest.mark.parametrize('bw', sorted(T.SWEEP))
def test_sweep_has_nearly_every_run_length(orc, bw):
    first, count = T.SWEEP[bw]
    lengths = []
    for k in range(count):
        case = first._replace(J=first.J + k)
        _run_on_its_base(orc(case), case, 17, 70)
        lengths.append(T.longest_run(orc(case))[1])
    assert lengths == sorted(lengths)
    # 24 consecutive lengths (the entering position at every alignment to a 16-cell dword and a 32-cell half), 40 in all
    assert set(range(25, 49)) <= set(lengths) and len(set(lengths) & set(range(17, 67))) >= 40, lengths


@pytest.mark.parametrize('bw', sorted(T.UNDER_WINDOW))
def test_runs_end_on_the_cell_under_the_window(orc, bw):
    assert T.strip_s0(500) == 208 and T.strip_s0(300) == -1 and T.strip_s0(1000) == 448 and T.strip_s0(100) == 0
    gaps = set()
    for case, leave in T.UNDER_WINDOW[bw]:
        o = orc(case)
        _run_on_its_base(o, case, 30)
        assert int(T.run_profile(o)[1][case.where]) == leave, case
        for lanes in (16, 64):
            ws = T.window_start(o, case, lanes)
            assert ws - leave in (1, 2), (case, lanes, ws)
            gaps.add(ws - leave)
    assert gaps == {1, 2}


def test_runs_just_after_the_masked_start(orc):
    assert [off for off, _ in T.AFTER_STATIC] == [0, 16, 17]
    for off, case in T.AFTER_STATIC:
        n_static = _run_on_its_base(orc(case), case, 66)
        assert case.bandwidth == 500 and case.where - n_static == off, (case, n_static)


def _top_index(which, tops):
    return {'first': 1, 'middle': len(tops) // 2, 'last': len(tops) - 1}[which]


@pytest.mark.parametrize('bw,lanes', sorted(T.CHUNK_TOPS))
def test_chunk_top_table_covers_every_offset(orc, bw, lanes):
    rows = T.CHUNK_TOPS[(bw, lanes)]
    assert sorted((w, off) for w, off, _ in rows) == sorted((w, off) for w in ('first', 'middle', 'last') for off in T.TOP_OFFSETS)
    for which, off, case in rows:
        assert case.bandwidth == bw
        n_static = _run_on_its_base(orc(case), case, 66)
        _, tops = T.chunk_tops(case.nb, n_static, lanes)
        c = _top_index(which, tops)
        assert 1 <= c < len(tops) and len({1, len(tops) // 2, len(tops) - 1}) == 3
        assert T.top_offset(case.where + 1, tops) == (c, off), (which, off, case, n_static)


@pytest.mark.parametrize('bw,lanes', sorted(T.BAND_EDGE))
def test_band_edge_table_is_a_mix_around_the_middle_top(orc, bw, lanes):
    first, want = T.BAND_EDGE[(bw, lanes)]
    assert first.bandwidth == bw and len(want) == 24
    got = [orc(first._replace(where=first.where + k))['status'] for k in range(24)]
    assert got == want
    assert want.count(0) >= 8 and want.count(T.TBA_BEYOND_BANDWIDTH) >= 8 and set(want) == {0, T.TBA_BEYOND_BANDWIDTH}
    # rows where + 1 .. where + 24 span the middle top -- itself, 11 rows under it and 12 above -- in every read that has a geometry
    for k in range(24):
        o = orc(first._replace(where=first.where + k))
        if o['status'] == 0:
            _, tops = T.chunk_tops(first.nb, int(o['dbg']['mask_seq_len']), lanes)
            assert tops[len(tops) // 2] == first.where + 12, (k, tops)


def test_long_read_table(orc):
    assert [name for name, _ in T.LONG] == ['plain', 'run 20-31', 'run >= 66', 'fail']
    cases = dict(T.LONG)
    assert all(24700 <= c.nb <= 25000 and c.bandwidth == 500 for c in cases.values())
    plain = orc(cases['plain'])
    assert plain['status'] == 0 and T.longest_run(plain)[1] <= 16
    _run_on_its_base(orc(cases['run 20-31']), cases['run 20-31'], 20, 31)
    _run_on_its_base(orc(cases['run >= 66']), cases['run >= 66'], 66)
    assert orc(cases['fail'])['status'] == T.TBA_BEYOND_BANDWIDTH


def test_inject_table(orc):
    offs = [off for off, _ in T.INJECT]
    assert offs.count(0) >= 2 and sum(-8 <= off < 0 for off in offs) >= 2 and len(offs) == offs.count(0) + sum(-8 <= off < 0 for off in offs)
    for off, case in T.INJECT:
        n_static = _run_on_its_base(orc(case), case, 66)
        _, tops = T.chunk_tops(case.nb, n_static, 16)
        assert case.bandwidth == 500 and case.where + 1 - tops[2] == off, (case, n_static)

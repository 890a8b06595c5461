"""The dwell-percentile kernel of csrc/k_filter.h (Engine.dwell_pctl_flags, batch_dwell_pctl_flags) against
np.percentile on np.diff of the boundaries and the strict comparison, and the stuck and coverage cases of
tests/golden/stats_filters.npz end to end through tombo_amd.filter_reads on the device.  Nothing is compared with
a tolerance: flags are booleans, percentile values are compared as bits.

Shapes: reads of 0 and 1 entries (no lengths), then 1, 2, 3 bases and bases around the wavefront (64), the
workgroup (256), the histogram (4096) and 70 000, mixed in one call so that neighbours differ in size; lengths
that stay below the histogram's last bin, that sit on its edge (4094, 4095, 4096) and that need the select
(65 535, 65 536, 3 000 000, up to 2^31 - 1); 2 000 reads in one call (more reads than workgroups)."""
import numpy as np
import pytest

import filter_cases as fc
import filter_reference as fref
from tombo_amd import _native, filter_reads as flt, resquiggle as rq

pytestmark = pytest.mark.gpu

BASES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70000]
LONG = np.array([4094, 4095, 4096, 65535, 65536, 3000000, 2 ** 31 - 1], dtype=np.int64)
PAIRS5 = [(0, 1), (1, 2.5), (50, 8), (99, 200), (100, 5000)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def pattern(rng, kind, n):
    if kind == 'equal':
        return np.full(n, int(rng.integers(1, 300)), dtype=np.int64)
    if kind == 'two':
        return rng.choice(np.array([3, 4094], dtype=np.int64), n)
    if kind == 'shuffled':
        return rng.permutation(np.arange(1, n + 1, dtype=np.int64))
    if kind == 'handful':                     # small values, a handful of long ones: ranks on both sides of the last bin
        v = rng.geometric(0.1, n).astype(np.int64)
        k = min(n, 9)
        v[rng.choice(n, k, replace=False)] = np.resize(LONG[3:6], k)
        return v
    assert kind == 'long'                     # every length in the last bin
    v = rng.integers(4095, 2 ** 31, n, dtype=np.int64)
    k = min(n, LONG.shape[0] - 1)
    v[rng.choice(n, k, replace=False)] = LONG[1:1 + k]
    return v


def mixed_reads(rng):
    """every pattern at every base count, neighbours of different size, the reads without lengths in between ->
    (segs, seg_off, entries per read)"""
    lens = [pattern(rng, kind, n) for kind in ('equal', 'two', 'shuffled', 'handful', 'long')
            for n in [BASES[i] for i in (12, 0, 9, 3, 6, 1, 10, 4, 7, 2, 11, 5, 8)]]
    segs = [int(rng.integers(0, 1000)) + np.concatenate([[0], np.cumsum(v)]) for v in lens]
    segs[7:7] = [np.zeros(0, dtype=np.int64)]
    segs[20:20] = [np.array([17], dtype=np.int64)]
    segs.append(np.zeros(0, dtype=np.int64))
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in segs])]).astype(np.int64)
    return np.concatenate(segs).astype(np.int64), off


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


@pytest.fixture(scope='module')
def mixed():
    segs, off = mixed_reads(np.random.default_rng(11))
    return segs, off, fref.dwell_pctl_flags(segs, off, PAIRS5)     # the reference once, for every test that needs it


def test_percentiles_and_flags_equal_numpy(eng, mixed):
    segs, off, (want_v, want_f) = mixed
    got_v, got_f = eng.dwell_pctl_flags(segs, off, PAIRS5)
    assert eng.last_filter_kernel_ms > 0.0
    same_bits(got_v, want_v)
    assert got_f.dtype == np.bool_ and np.array_equal(got_f, want_f)
    none = np.flatnonzero(np.diff(off) < 2)
    assert none.tolist() == [7, 20, off.shape[0] - 2] and np.isnan(got_v[none]).all() and got_f[none].all()
    assert 0 < got_f.sum() < got_f.shape[0]
    # the cases hold an integral (n - 1) q and a t of exactly 0.5
    n = np.diff(off) - 1
    assert ((n[n > 0] - 1) % 2 == 0).any() and ((n[n > 0] - 1) % 2 == 1).any()
    v2, f2 = eng.dwell_pctl_flags(segs, off, PAIRS5)             # the same call again: the same bytes
    assert v2.tobytes() == got_v.tobytes() and f2.tobytes() == got_f.tobytes()


@pytest.mark.parametrize('pairs', [[(50, 8)], [(99, 200), (100, 5000)], [(25, 3.5)]])
def test_one_and_two_pairs(eng, mixed, pairs):
    segs, off, _ = mixed
    want_v, want_f = fref.dwell_pctl_flags(segs, off, pairs)
    got_v, got_f = eng.dwell_pctl_flags(segs, off, pairs)
    same_bits(got_v, want_v)
    assert np.array_equal(got_f, want_f)


def test_threshold_on_the_percentile_and_one_step_below(eng, mixed):
    segs, off, (want_v, _) = mixed
    sizes = np.diff(off)
    for r in (int(np.flatnonzero(sizes == 70001)[3]), int(np.flatnonzero(sizes == 65)[3]), int(np.flatnonzero(sizes == 3)[4]),
              int(np.flatnonzero(sizes == 4097)[4])):
        s = segs[off[r]:off[r + 1]]
        o = np.array([0, s.shape[0]], dtype=np.int64)
        for j, (p, _) in enumerate(PAIRS5):
            v = want_v[r, j]
            on = eng.dwell_pctl_flags(s, o, [(p, v)])
            below = eng.dwell_pctl_flags(s, o, [(p, np.nextafter(v, -np.inf))])
            same_bits(on[0], [[v]])
            assert not on[1][0] and below[1][0], (r, p, v)


def test_many_short_reads(eng):
    rng = np.random.default_rng(12)
    lens = [rng.geometric(0.08, int(n)).astype(np.int64) for n in rng.integers(1, 301, 2000)]
    for v in lens[::97]:
        v[rng.integers(0, v.shape[0])] = int(rng.choice(LONG))
    segs = np.concatenate([np.concatenate([[0], np.cumsum(v)]) for v in lens]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum([v.shape[0] + 1 for v in lens])]).astype(np.int64)
    pairs = [(99, 200), (100, 5000)]
    want_v, want_f = fref.dwell_pctl_flags(segs, off, pairs)
    got_v, got_f = eng.dwell_pctl_flags(segs, off, pairs)
    same_bits(got_v, want_v)
    assert np.array_equal(got_f, want_f) and 0 < got_f.sum() < 2000


def test_bad_arguments_and_zero_reads(eng):
    segs, off = np.array([0, 3, 5, 0, 2], dtype=np.int64), np.array([0, 3, 3, 5], dtype=np.int64)
    q, th_ = np.array([0.5]), np.array([3.0])
    vals, flags = np.zeros((3, 1)), np.zeros(3, dtype=np.uint8)

    def call(segs=segs, off=off, n=3, n_pairs=1, q=q, th_=th_, vals=vals, flags=flags):
        eng._call('tba_dwell_pctl_flags', n, segs, off, n_pairs, q, th_, vals, flags, None)
    call()                                                      # (vals and the kernel time may be NULL)
    call(vals=None)
    assert flags.tolist() == [0, 1, 0] and vals[0, 0] == 2.5 and np.isnan(vals[1, 0]) and vals[2, 0] == 2.0
    bad = [dict(segs=None), dict(off=None), dict(q=None), dict(th_=None), dict(flags=None),
           dict(off=np.array([1, 3, 3, 5], dtype=np.int64)), dict(off=np.array([0, 3, 2, 5], dtype=np.int64)),
           dict(n_pairs=0), dict(q=np.array([1.5])), dict(q=np.array([-0.1])), dict(q=np.array([np.nan])),
           dict(th_=np.array([np.nan])), dict(segs=np.array([0, 3, 2, 0, 2], dtype=np.int64)),
           dict(segs=np.array([0, 3, 5, 0, 2 ** 31], dtype=np.int64)), dict(n=-1)]
    for change in bad:
        with pytest.raises(_native.EngineError) as exc:
            call(**change)
        assert '(-1)' in str(exc.value), change                  # TBA_E_ARG
    flags[:] = 7
    call(segs=None, off=np.zeros(1, dtype=np.int64), n=0)       # zero reads: nothing is launched or written
    assert flags.tolist() == [7, 7, 7]
    v, f = eng.dwell_pctl_flags(np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), [(50, 3)])
    assert v.shape == (0, 1) and f.shape == (0,) and eng.last_filter_kernel_ms == 0.0
    for args in ((segs, off, []), (segs, off, [(101, 1)]), (segs.astype(np.int32), off, [(50, 1)])):
        with pytest.raises(ValueError):
            eng.dwell_pctl_flags(*args)


def test_resident_batch_equals_the_array_form(eng):
    from tombo_amd import synth, tombo_stats as ts, tombo_helper as th
    samp = th.seqSampleType('DNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)
    rng = np.random.default_rng(13)
    mrs = [synth.synth_map_res(model, int(nb), 7000 + i, **synth.DNA_SYNTH)
           for i, nb in enumerate(rng.integers(300, 2001, 40))]
    mrs[5] = mrs[5]._replace(raw_signal=mrs[5].raw_signal[:400])     # a read that fails
    res = rq.resquiggle_batch(mrs, model, params, outlier_thresh=5.0, seq_samp_type=samp, engine=eng)
    assert isinstance(res[5], Exception) and sum(isinstance(r, Exception) for r in res) == 1
    before = eng.download(want_norm=False)
    pairs = [(50, 8), (99, 45), (100, 70)]
    vals, flags = eng.batch_dwell_pctl_flags(pairs)
    assert eng.last_filter_kernel_ms > 0.0
    after = eng.download(want_norm=False)
    for k in before:                                              # the batch's own downloads are unchanged
        assert (before[k] is None and after[k] is None) or before[k].tobytes() == after[k].tobytes(), k
    ok = before['status'] == 0
    seg_off = np.ascontiguousarray(eng.seg_off, dtype=np.int64)
    segs = before['segs'].copy()
    segs[seg_off[5]:seg_off[6]] = 0                              # (whatever the failed read left is no boundary)
    want_v, want_f = eng.dwell_pctl_flags(segs, seg_off, pairs)
    assert ok.sum() == 39 and not ok[5]
    same_bits(vals[ok], want_v[ok])
    assert np.array_equal(flags[ok], want_f[ok]) and 0 < flags.sum() < 39
    assert np.isnan(vals[5]).all() and not flags[5]
    for i in np.flatnonzero(ok)[:6]:                              # ... and numpy on the results' own boundaries
        lens = np.diff(res[i].segs)
        same_bits(vals[i], [np.percentile(lens, p) for p, _ in pairs])
    # the worker-loop rule for the batch, from the resident boundaries
    from tombo_amd import mapping
    fns = ['f%d' % i for i in range(len(res))]
    got = mapping.filter_and_index_records_batch(res, fns, 'G', 'BaseCalled_template', samp, 1.1, pairs, engine=eng,
                                                 resident=True)
    want = [None if isinstance(r, Exception) else
            mapping.filter_and_index_record(r, fn, 'G', 'BaseCalled_template', samp, 1.1, pairs) for r, fn in zip(res, fns)]
    assert got == want
    assert got == mapping.filter_and_index_records_batch(res, fns, 'G', 'BaseCalled_template', samp, 1.1, pairs, engine=eng)


@pytest.mark.parametrize('name', [n for n in sorted(fc.CASES) if n.startswith(('stuck', 'coverage', 'allfilt_stuck',
                                                                               'allfilt_coverage'))])
def test_fixture_cases_end_to_end(eng, name, tmp_path):
    fc.check_case(name, eng, tmp_path)

"""`tba_site_fractions_reads` (kernels k_site_pair_plan / k_site_gather of csrc/k_site.h), `compute_reg_stats_reads_batch`
and `test_significance` on the device.

The oracle is the route that exists without them: `compute_reg_stats_batch`, whose per-read preparation runs in
Python, and `write_stats_from_regions`.  Both routes hand the same float64 inputs to the same statistic kernels, so
every comparison is byte for byte; the golden cases are also held against the live reference's recorded results
with no tolerance (tests/test_gpu_site_stats.py states why none is needed).  The inputs and checks are those of
tests/test_site_reads_host_layer.py (tests/site_reads_cases.py), where the failing-pair conditions are established
on the numpy engine."""
import numpy as np
import pytest

import launch_caps
import site_reads_cases as cases
import stat_store_cases
from stats_cases import gold, meta, model, alt_refs   # noqa: F401
from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq, _native
from tombo_amd._default_parameters import SMALLEST_PVAL

pytestmark = pytest.mark.gpu
E_ARG = -1


@pytest.fixture(scope='module')
def eng():
    return rq.get_engine()


@pytest.mark.parametrize('at_once', [True, False])
@pytest.mark.parametrize('stat_type', cases.Z_TYPES)
def test_golden_cases(gold, meta, model, eng, stat_type, at_once):
    assert cases.check_golden(gold, meta, model, eng, stat_type, at_once) >= 20


@pytest.mark.parametrize('fm', [0, 1, 3])
def test_reads_shared_between_regions(model, eng, fm):
    assert cases.check_shared_reads(model, eng, fm) == 24


def test_failing_pairs(model, eng):
    cases.check_failing_pairs(model, eng)


# ---- size edges ----------------------------------------------------------------------------------
def spanning_regions(model, n_regions, depth, n_pos, extra, seed=31):
    """n_regions '+' regions of n_pos positions, each under `depth` reads that cover it with the k-mer lags and no
    more (n_pos statistics a pair at fm_offset 0); `extra` more reads on the last region"""
    rng = np.random.default_rng(seed)
    K, cp = model.kmer_width, model.central_pos
    regs = []
    for r in range(n_regions):
        start = 1000 + r * (n_pos + 200)
        seq = ''.join(rng.choice(list('ACGT'), n_pos + K - 1))
        lv, sd = model.get_exp_levels_from_seq(seq)
        reads = []
        for d in range(depth + (extra if r == n_regions - 1 else 0)):
            m = rng.normal(0.0, 1.0, n_pos + K - 1)
            m[cp:cp + n_pos] = lv + rng.normal(0.0, 1.3, n_pos) * sd
            reads.append(th.resquiggledRead(start - cp, start - cp + n_pos + K - 1, False, 0, '+', None, None, False,
                                            read_id='e%d_%d' % (r, d), means=m, seq=seq))
        regs.append(th.regionData('c', '+', start, start + n_pos, reads))
    return regs


@pytest.mark.parametrize('extra', [0, 1])
def test_statistics_around_one_grid_pass_and_pairs_past_a_scan_chunk(model, eng, extra):
    n_pos, single, lower = 953, 0.3, 0.05
    regs = spanning_regions(model, 11, 100, n_pos, extra)
    total = (1100 + extra) * n_pos
    assert 1100 + extra > launch_caps.SCAN_CHUNK
    assert 0 < (total - launch_caps.GRID_PASS if extra else launch_caps.GRID_PASS - total) < launch_caps.SCAN_CHUNK
    eng.ensure_model(model)
    want_in = ts._reg_stats_z_inputs(regs, 0, model, ts.DE_NOVO_TXT)
    want = want_in.site_fractions(eng, single, lower, cases.DAMP, True)
    got_in = ts._reg_stats_reads_inputs(regs, 0, ts.DE_NOVO_TXT)
    got = got_in.site_fractions(eng, single, lower, cases.DAMP, True)
    assert got_in.pair_ok.all() and np.array_equal(got_in.pair_off, want_in.off) and int(want_in.off[-1]) == total
    assert np.array_equal(got_in.pair_pos, want_in.read_pos) and np.array_equal(got_in.pair_reg, want_in.read_track)
    stat_store_cases.check_equal_results(want, got)
    sample = launch_caps.pass_sample(total, 5 + extra)
    assert got.per_read.shape[0] == total
    assert got.per_read[sample].tobytes() == want.per_read[sample].tobytes()
    assert not np.isnan(want.per_read[sample]).any()


# ---- TBA_E_ARG --------------------------------------------------------------------------------------
def raw_call(eng, a, null=(), per_read_cap=None):
    """straight at the C entry (the binding's own checks would stop these first) with outputs full of -3
    -> (return code, whether every output still holds -3 only)"""
    import ctypes as C
    f = dict((k, np.full(1024, -3.0)) for k in ('frac', 'damp', 'per_read'))
    q = dict((k, np.full(1024, -3, dtype=np.int64)) for k in ('pos', 'cov', 'valid', 'counts', 'n_stats', 'pair_pos', 'pair_off'))
    ok, ms = np.full(1024, -3, dtype=np.int32), np.full(2, -3.0)
    a, n_reg, n_reads = dict(a), a['reg_start'].shape[0], a['read_start'].shape[0]
    for k in null:
        a[k] = None
    out = lambda k, arr: None if k in null else arr   # noqa: E731
    rc = eng._L.tba_site_fractions_reads(
        eng._h, a['form'], n_reg, a['reg_start'], a['reg_end'], n_reads, a['read_start'],
        a['read_strand'], a['read_off'], a['means'], a['seq'], a['reg_pair_off'], a['pair_read'], a['pos_means'],
        a['pos_sds'], a['fm_offset'], SMALLEST_PVAL, 0.3, None, (C.c_double * 2)(2.0, 0.0), out('frac', f['frac']), q['pos'],
        q['cov'], q['valid'], f['damp'], q['counts'], q['n_stats'], out('pair_ok', ok), q['pair_pos'], q['pair_off'],
        None if per_read_cap is None else f['per_read'], per_read_cap or 0, ms)
    untouched = all(np.all(x == -3) for x in list(f.values()) + list(q.values()) + [ok, ms])
    return rc, untouched


def test_host_argument_errors_launch_nothing(model, eng):
    eng.ensure_model(model)
    base = cases.base_args()
    rc, untouched = raw_call(eng, base)
    assert rc == 0 and not untouched
    bad = [c for c in cases.BAD_ARGS if set(c) != {'means'} and c != dict(seq=None)]     # (what the C entry can see)
    assert len(bad) >= 13
    for change in bad:
        assert raw_call(eng, dict(base, **change)) == (E_ARG, True), change
    for null in ('seq', 'means', 'reg_start', 'read_off', 'pair_read', 'reg_pair_off', 'frac', 'pair_ok'):
        assert raw_call(eng, base, null=(null,)) == (E_ARG, True), null
    form1 = dict(base, form=1, seq=None, pos_means=np.zeros(204), pos_sds=np.ones(204))
    assert raw_call(eng, form1)[0] == 0
    assert raw_call(eng, form1, null=('pos_sds',)) == (E_ARG, True)
    fresh = _native.Engine(eng.device)          # form 0 without a model
    try:
        assert raw_call(fresh, base) == (E_ARG, True)
        assert raw_call(fresh, form1)[0] == 0
    finally:
        fresh.close()
    # per_read_cap below the statistics: found after the plan, nothing is written
    t = _native._check_site_reads_args(**base)
    total = int(_native.site_reads_stat_bound(0, t, model.kmer_width, model.central_pos).sum())
    assert raw_call(eng, base, per_read_cap=total - 1) == (E_ARG, True)
    assert b'per_read_cap' in eng._L.tba_last_error()
    rc, untouched = raw_call(eng, base, per_read_cap=total)
    assert rc == 0 and not untouched


def test_binding_refuses_what_the_entry_refuses(eng):
    for change in cases.BAD_ARGS:
        with pytest.raises(ValueError):
            eng.site_fractions_reads(*dict(cases.base_args(), **change).values(), SMALLEST_PVAL, 0.3)


# ---- the driver ------------------------------------------------------------------------------------
@pytest.mark.parametrize('stat_type,per_read,use_ref', cases.DRIVER_CASES)
def test_driver_equals_todays_route(model, alt_refs, eng, stat_type, per_read, use_ref):
    n = cases.check_driver(model, alt_refs, eng, stat_type, per_read, use_ref)
    assert n >= 12 * (2 if per_read else 1)

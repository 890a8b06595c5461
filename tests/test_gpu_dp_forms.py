"""Every forward-pass kernel against the oracle, and the report of which one ran.

The banded forward pass has more variants than event detection or the traceback: k_dp<CPL> per band
class, k_dp_multi for narrow bands, k_dp_wide for wide static bands, k_dp8_lowreg -- the 112-register
build of the 8-cell class, different machine code, chosen when several engines share the device and the
batch has more than 0.04 samples per DP cell (every RNA batch of a streaming pipeline) -- and for the
start-discovery retry k_dp_wg<4 / 8 / 12> or k_dp<CPL> in retry mode.  TBA_GET_DP_FORM names, per read,
the kernels that took it; these tests put each of them under the oracle and assert through the report
that it really was that kernel.  Every comparison is exact.
"""
import numpy as np
import pytest

import oracle

from conftest import check_forms
from test_gpu_parity import run_batch, compare_batch, _engine, _si

pytestmark = pytest.mark.gpu

LOWREG_SAMPLES_PER_CELL = 0.04      # dp_lowreg (tba_engine.hip)
CPL_CLASSES = (4, 5, 8, 12, 16, 24, 32, 48)     # cpl_class (k_dp.h)
WG_MAX_ROWS = 256                   # k_dp_wg.h

# (save_bw, start_bw, start_n_bases, TBA_DP_START_* of the retry, its class): every retry kernel.
# DNA alignment parameters (4.2, 4.2, 300, 1500, 20.0, 40, start_bw, save_bw, start_n_bases).
RETRY_SETS = (
    (900, 300, 120, 'wg', 4),
    (1800, 500, 200, 'wg', 8),
    (2500, 750, 250, 'wg', 12),
    (2500, 750, 300, 'k_dp', 48),   # 300 rows > WG_MAX_ROWS
    (3000, 1000, 250, 'wg', 12),
)
RETRY_LEADER_EVENTS = (lambda start_bw, save_bw: (0.8 * start_bw, 1.5 * start_bw, 0.6 * save_bw, 0.9 * save_bw,
                                                  1.3 * save_bw))


def cpl_class(w):
    return next((c for c in CPL_CLASSES if c * 64 >= w), 0)


def _model(samp_name):
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    samp = th.seqSampleType(samp_name, False)
    return samp, ts.TomboModel(seq_samp_type=samp)


class sharing(object):
    """the default engine under tba_engine_set_sharing(n); back to 1 on the way out"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.eng = _engine()
        self.eng.set_sharing(self.n)
        return self.eng

    def __exit__(self, *exc):      # (runs like a `finally`: also when the body raised)
        self.eng.set_sharing(1)
        return False


def samples_per_cell(eng):
    """the selector's ratio for the uploaded batch: samples / DP cells (tba_batch_stats)"""
    return float(eng.raw_off[-1]) / eng.stats()[1]


def check_dp_forms(eng, params, lowreg, oracles=None):
    """TBA_GET_DP_FORM of the last run against the dispatch rules, read by read: the main-pass kernel by the
    read's path and band width, the start-discovery columns by the number of start calls (the oracle's when
    `oracles` is given, else the engine's).  Returns the report."""
    from tombo_amd import _native as N
    form, path = eng.get(N.GET_DP_FORM), eng.get(N.GET_PATH)
    assert form.shape == (eng.n, 4) and form.dtype == np.int32
    bw = int(params.bandwidth)
    wcpl = 0
    if params.start_n_bases <= WG_MAX_ROWS:
        wcpl = 4 if params.start_save_bw <= 1024 else 8 if params.start_save_bw <= 2048 else 12
    retry = (N.DP_START_RETRY_WG, wcpl) if wcpl else (N.DP_START_RETRY_K_DP, cpl_class(params.start_save_bw))
    for i in range(eng.n):
        kind, w = int(path[i, 0]), int(path[i, 2])
        if kind == 0:
            want = (N.DP_FORM_NONE, 0)
        elif kind == 1 and w == bw and bw <= 128:
            want = (N.DP_FORM_MULTI, 4)
        elif cpl_class(w):
            want = (N.DP_FORM_K_DP8_LOWREG if cpl_class(w) == 8 and lowreg else N.DP_FORM_K_DP, cpl_class(w))
        else:
            assert kind == 2, (i, path[i])
            want = (N.DP_FORM_WIDE, 0)
        assert tuple(form[i, :2]) == want, (i, form[i].tolist(), path[i].tolist(), want)
        calls = int(path[i, 3]) if oracles is None else oracles[i]['dbg']['n_start_calls']
        if calls == 2:
            assert tuple(form[i, 2:]) == retry, (i, form[i].tolist(), retry)
        else:
            assert form[i, 2] in (N.DP_START_NONE, N.DP_START_FIRST_TRY) and form[i, 3] == 0, (i, form[i].tolist())
            if calls == 1:
                assert form[i, 2] == N.DP_START_FIRST_TRY, (i, form[i].tolist())
    return form


# ---- k_dp8_lowreg ---------------------------------------------------------------------------------
LOWREG_RNA_SPECS = ((600, {}), (900, {}), (1500, {}), (2100, {}), (700, dict(noise_sd=0.9)), (120, {}), (249, {}),
                    (800, dict(mean_dwell=12, min_dwell=3)), (1000, dict(lead=9000)), (650, {}), (1250, {}), (777, {}))
_cache = {}


def lowreg_rna_batch(golden_case):
    """(model, params, reads): twelve RNA reads at the RNA defaults (bandwidth 500) and a golden read that fails"""
    if 'rna' not in _cache:
        from tombo_amd import synth, tombo_stats as ts
        samp, model = _model('RNA')
        params = ts.load_resquiggle_parameters(samp)
        assert params.bandwidth == 500
        reads = []
        for k, (nb, kw) in enumerate(LOWREG_RNA_SPECS):
            seq, raw, _ = synth.synth_read(model, nb, 31000 + k, **dict(synth.RNA_SYNTH, **kw))
            reads.append((raw, seq, oracle.identify_stalls(raw), _si(nb, k)))
        c = golden_case('e_rna_trunc70_bandfail')
        assert c.params == params and c.error, (c.params, params)
        reads.append((c.raw, c.seq, c.stall_ints, c.samp_ind()))
        _cache['rna'] = (model, params, reads)
    return _cache['rna']


def test_lowreg_kernel_equals_the_oracle(golden_case, dispatch_form):
    """(a) an RNA batch under set_sharing(2) runs k_dp8_lowreg: every stage equal to the oracle's, in both
    dispatch forms, and the report names the kernel for every adaptive read of the batch bandwidth"""
    from tombo_amd import _native as N
    model, params, reads = lowreg_rna_batch(golden_case)
    with sharing(2):
        eng, out, oracles = run_batch(model, params, 'RNA', reads)
        assert eng.last_dp_lowreg()
        assert samples_per_cell(eng) > 1.25 * LOWREG_SAMPLES_PER_CELL, samples_per_cell(eng)
        bad = compare_batch(eng, oracles, out, 'lowreg')
        assert not bad, '\n'.join(bad[:40])
        check_forms(eng, dispatch_form, params)
        form = check_dp_forms(eng, params, True, oracles)
        path = eng.get(N.GET_PATH)
    assert all(o['status'] == 0 for o in oracles[:12]) and oracles[12]['status'] != 0
    assert [int(p) for p in path[5:8, 0]] == [2, 2, 2]          # static: a class by the read's own width
    adaptive = (path[:, 0] == 1) & (path[:, 2] == 500)
    assert adaptive.sum() >= 9
    assert np.all(form[adaptive, 0] == N.DP_FORM_K_DP8_LOWREG) and np.all(form[adaptive, 1] == 8), form.tolist()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _snapshot(eng, gets, download=True):
    snap = dict(('get%d' % g, eng.get(g)) for g in gets)
    if download:
        snap.update(eng.download())
    return snap


def _assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), '%s differs between k_dp8_lowreg and k_dp<8>' % k


def test_lowreg_kernel_is_bit_equal_to_k_dp8(golden_case):
    """(b) the same resident batch under set_sharing(2) and set_sharing(1): every forward-pass product, the
    stages after it and every output bit for bit the same"""
    from tombo_amd import _native as N
    model, params, reads = lowreg_rna_batch(golden_case)
    gets = (N.GET_BAND_STARTS, N.GET_LAST_ROW, N.GET_READ_TB, N.GET_DP_SEGS, N.GET_SEGS, N.GET_STATUS, N.GET_PATH)
    with sharing(2) as eng:
        run_batch(model, params, 'RNA', reads)
        assert eng.last_dp_lowreg()
        low = _snapshot(eng, gets)
        low_form = eng.get(N.GET_DP_FORM)
        eng.set_sharing(1)
        eng.run()
        assert not eng.last_dp_lowreg()
        ref = _snapshot(eng, gets)
        ref_form = check_dp_forms(eng, params, False)
    _assert_same(low, ref)
    took = low_form[:, 0] == N.DP_FORM_K_DP8_LOWREG
    assert took.sum() >= 9 and np.all(ref_form[took, 0] == N.DP_FORM_K_DP)
    assert np.array_equal(low_form[~took], ref_form[~took]) and np.array_equal(low_form[:, 1:], ref_form[:, 1:])


def _selector_reads(samp_name, n_bases, **kw):
    from tombo_amd import synth
    samp, model = _model(samp_name)
    base = synth.RNA_SYNTH if samp_name == 'RNA' else synth.DNA_SYNTH
    reads = []
    for k, nb in enumerate(n_bases):
        seq, raw, _ = synth.synth_read(model, nb, 52000 + k, **dict(base, **kw))
        reads.append((raw, seq, oracle.identify_stalls(raw) if samp_name == 'RNA' else None, _si(nb, k)))
    return samp, model, reads


@pytest.mark.parametrize('case', ['dna_w500_dwell9', 'dna_w500_dwell40', 'rna_w300'])
def test_lowreg_selector_on_both_sides(case):
    """(c) under set_sharing(2): DNA at bandwidth 500 stays on k_dp<8> (0.018 samples per cell); the same lengths
    with 40 samples per base (0.07) take k_dp8_lowreg -- DNA event detection beside it -- and match the oracle;
    RNA at bandwidth 300 is class 5 and has no low-register kernel to take"""
    from tombo_amd import _native as N, tombo_stats as ts
    if case == 'rna_w300':
        samp, model, reads = _selector_reads('RNA', (700, 1100, 1600, 900))
        bw, want_low = 300, False
    else:
        samp, model, reads = _selector_reads('DNA', (2000,) * 8, **(dict(mean_dwell=40) if case == 'dna_w500_dwell40' else {}))
        bw, want_low = 500, case == 'dna_w500_dwell40'
    params = ts.load_resquiggle_parameters(samp)._replace(bandwidth=bw)
    with sharing(2):
        eng, out, oracles = run_batch(model, params, samp.name, reads)
        ratio = samples_per_cell(eng)
        if case == 'dna_w500_dwell9':
            assert ratio < 0.75 * LOWREG_SAMPLES_PER_CELL, ratio
        else:
            assert ratio > 1.25 * LOWREG_SAMPLES_PER_CELL, ratio
        # (RNA at class 5: the selector says yes, and no kernel of the 8-cell class has a read to take)
        assert eng.last_dp_lowreg() == (want_low or case == 'rna_w300')
        bad = compare_batch(eng, oracles, out, case)
        assert not bad, '\n'.join(bad[:40])
        form = check_dp_forms(eng, params, eng.last_dp_lowreg(), oracles)
        path = eng.get(N.GET_PATH)
    assert all(o['status'] == 0 for o in oracles)
    adaptive = (path[:, 0] == 1) & (path[:, 2] == bw)
    assert adaptive.all()
    want = (N.DP_FORM_K_DP8_LOWREG, 8) if want_low else (N.DP_FORM_K_DP, cpl_class(bw))
    assert np.all(form[:, 0] == want[0]) and np.all(form[:, 1] == want[1]), form.tolist()


def test_lowreg_kernel_in_a_batch_of_thousands():
    """(d) 4 096 RNA reads from the device generator -- the batch size at which a register allocation alone made
    a kernel of this library wrong -- once on k_dp<8>, once on k_dp8_lowreg: the same traceback, band starts, last
    rows and statuses, and the traceback verifier silent in both"""
    from tombo_amd import _native as N
    from test_gpu_determinism import _device_batch
    eng, gen, model, params, raw_off, seq_off = _device_batch('RNA', 4096, 1500, 20261017)
    gets = (N.GET_READ_TB, N.GET_BAND_STARTS, N.GET_LAST_ROW, N.GET_STATUS)
    try:
        runs = []
        for n_engines, want_low in ((1, False), (2, True)):
            eng.set_sharing(n_engines)
            eng.run()
            assert eng.last_dp_lowreg() == want_low
            assert not eng.get(N.GET_TB_VERIFY_FAIL).any()
            form = check_dp_forms(eng, params, want_low)
            path = eng.get(N.GET_PATH)
            adaptive = (path[:, 0] == 1) & (path[:, 2] == 500)
            assert adaptive.sum() > 0.95 * eng.n
            assert np.all(form[adaptive, 0] == (N.DP_FORM_K_DP8_LOWREG if want_low else N.DP_FORM_K_DP)), np.bincount(form[:, 0])
            runs.append(_snapshot(eng, gets, download=False))
        assert (runs[0]['get%d' % N.GET_STATUS] == 0).sum() > 0.95 * eng.n
        _assert_same(runs[1], runs[0])
    finally:
        eng.set_sharing(1)
        eng.close(), gen.close()


def test_lowreg_kernel_under_real_sharing():
    """(e) two slots of a StreamPipeline over RNA reads as int16 DAC values, three batches, so that batches are on
    the device together: compact records and boundaries equal to the oracle's, and every slot ran k_dp8_lowreg"""
    from tombo_amd import streaming, synth, tombo_stats as ts, tombo_helper as th
    from tombo_amd._default_parameters import SIG_MATCH_THRESH, STALL_PARAMS
    samp, model = _model('RNA')
    params = ts.load_resquiggle_parameters(samp)
    rng = np.random.RandomState(77)
    reads = []
    for i in range(24):
        nb = int(rng.choice([600, 800, 1100, 1500]))
        seq, raw, _ = synth.synth_read(model, nb, 61000 + i, **synth.RNA_SYNTH)
        raw = np.round(raw / 0.1709 + 10.0).astype(np.int16)
        reads.append((seq, raw, rng.choice(nb, 1000, replace=False).astype(np.int64) if nb > 1000 else None))
    pipe = streaming.StreamPipeline(model, params, n_slots=2, outlier_thresh=5.0, seq_samp_type=samp,
                                    stall_params=th.stallParams(**STALL_PARAMS))
    try:
        batches = [streaming.ReadBatch.from_lists(
            [r for _, r, _ in reads[a:a + 8]], [ts.encode_seq(s) for s, _, _ in reads[a:a + 8]],
            samp_inds=[si for _, _, si in reads[a:a + 8]], tag=a, pinned=True) for a in (0, 8, 16)]
        p = oracle.make_params(params)
        o = oracle.make_opts(model.kmer_width, model.central_pos, outlier_thresh=5.0,
                             sig_match_thresh=SIG_MATCH_THRESH['RNA'])
        n_ok = n_seen = 0
        for res in pipe.run(batches):
            for k, (s, r, si) in enumerate(reads[res.tag:res.tag + 8]):
                raw = r.astype(np.float64)
                want = oracle.resquiggle_read(raw, ts.encode_seq(s), model.level_means, model.level_sds, p, o,
                                              stall_ints=oracle.identify_stalls(raw), samp_ind=si)
                rec = res.results[k]
                assert rec['status'] == want['status'], (res.tag, k)
                n_seen += 1
                if want['status'] == 0:
                    n_ok += 1
                    np.testing.assert_array_equal(res.segs_of(k), want['segs'])
                    assert rec['sig_match_score'] == want['sig_match_score']
                    assert rec['read_start_rel_to_raw'] == want['read_start_rel_to_raw']
                    assert rec['shift'] == want['scale_values'][0] and rec['scale'] == want['scale_values'][1]
        assert n_seen == 24 and n_ok >= 20
        assert [s.eng.last_dp_lowreg() for s in pipe.slots] == [True, True]
    finally:
        for s in pipe.slots:
            s.eng.set_sharing(1)
        pipe.close()


# ---- the start-discovery retry kernels --------------------------------------------------------------
def retry_reads(samp_name, model, start_bw, save_bw, obs_per_event):
    """five reads whose leaders put the sequence start inside the first band, between the bands, inside the save
    band and beyond it: (raw, seq, stall_ints, samp_ind)"""
    from tombo_amd import synth
    reads = []
    for k, f in enumerate(RETRY_LEADER_EVENTS(start_bw, save_bw)):
        nb, seed, lead = 500 + 111 * k, 4000 + 31 * k + save_bw, int(f * obs_per_event)
        if samp_name == 'RNA':
            # (the stall detector masks a leader of plain noise, and its events with it: the RNA leaders are the
            # signal of an unrelated sequence upstream of the read)
            seq, raw, _ = synth.synth_read(model, nb, seed, **dict(synth.RNA_SYNTH, lead=0))
            _, up, _ = synth.synth_read(model, lead // 40 + 50, seed + 7, **dict(synth.RNA_SYNTH, lead=0, n_trail=0))
            assert up.shape[0] >= lead
            raw = np.concatenate([up[:lead], raw])
            reads.append((raw, seq, oracle.identify_stalls(raw), _si(nb, k)))
        else:
            seq, raw, _ = synth.synth_read(model, nb, seed, **dict(synth.DNA_SYNTH, lead=lead))
            reads.append((raw, seq, None, _si(nb, k)))
    return reads


def retry_set(samp_name, table_row):
    """(model, params, reads) of one row of RETRY_SETS (DNA), or of the RNA defaults (table_row None)"""
    from tombo_amd import tombo_stats as ts
    samp, model = _model(samp_name)
    if table_row is None:
        params = ts.load_resquiggle_parameters(samp)
        assert (params.start_bw, params.start_save_bw, params.start_n_bases) == (1000, 3000, 250)
    else:
        save_bw, start_bw, n_bases = table_row[:3]
        params = ts.load_resquiggle_parameters(samp, (4.2, 4.2, 300, 1500, 20.0, 40, start_bw, save_bw, n_bases))
    return model, params, retry_reads(samp_name, model, params.start_bw, params.start_save_bw,
                                      params.mean_obs_per_event)


@pytest.mark.parametrize('row', list(range(len(RETRY_SETS))) + ['rna'])
def test_every_start_retry_kernel_equals_the_oracle(row, dispatch_form):
    """(f) k_dp_wg<4>, <8>, <12> and k_dp<48> in retry mode (more start bases than a workgroup holds rows): reads
    with leaders around and beyond both start bands, every stage against the oracle, and the report names the
    retry kernel for exactly the reads whose second start call the oracle counts"""
    from tombo_amd import _native as N
    if row == 'rna':
        model, params, reads = retry_set('RNA', None)
        kind, cls = 'wg', 12
    else:
        model, params, reads = retry_set('DNA', RETRY_SETS[row])
        kind, cls = RETRY_SETS[row][3:]
    with sharing(1):
        eng, out, oracles = run_batch(model, params, 'RNA' if row == 'rna' else 'DNA', reads)
        bad = compare_batch(eng, oracles, out, 'retry-%s' % (row,))
        assert not bad, '\n'.join(bad[:40])
        check_forms(eng, dispatch_form, params)
        form = check_dp_forms(eng, params, False, oracles)
    retried = np.array([o['dbg']['n_start_calls'] == 2 for o in oracles])
    assert retried.sum() >= 2, [o['dbg']['n_start_calls'] for o in oracles]
    want = N.DP_START_RETRY_WG if kind == 'wg' else N.DP_START_RETRY_K_DP
    assert np.all(form[retried, 2] == want) and np.all(form[retried, 3] == cls), form.tolist()
    assert np.all(form[~retried, 2] != N.DP_START_RETRY_WG) and np.all(form[~retried, 2] != N.DP_START_RETRY_K_DP)
    assert np.all(form[~retried, 3] == 0), form.tolist()


# ---- the report at the classes other tests reach ---------------------------------------------------
def _class_batch(bandwidth):
    from tombo_amd import synth, tombo_stats as ts
    samp, model = _model('DNA')
    if bandwidth == 100:        # test_many_seeds_w100_on_gpu
        params = ts.load_resquiggle_parameters(samp)._replace(bandwidth=100, band_bound_thresh=10)
        specs = [(2000, 9000 + seed, seed, synth.DNA_SYNTH) for seed in range(4)]
    elif bandwidth == 1500:     # test_wide_static_band_matches_oracle
        params = ts.load_resquiggle_parameters(samp, use_save_bandwidth=True)
        specs = [(nb, seed, seed, kw) for nb, seed, kw in [
            (20, 9, dict(lead=60000)), (100, 31, dict(mean_dwell=300)), (249, 32, dict(lead=30000)), (180, 33, {}),
            (1200, 34, {})]]
    else:                       # test_mixed_dna_batch_on_gpu
        params = ts.load_resquiggle_parameters(samp)._replace(bandwidth=bandwidth)
        specs = [(nb, 500 + seed, seed, dict(synth.DNA_SYNTH, **kw)) for nb, seed, kw in [
            (600, 1, {}), (150, 2, {}), (1200, 3, {}), (300, 4, {}), (1500, 5, dict(lead=5000)),
            (400, 7, dict(mean_dwell=400)), (2000, 8, {}), (260, 9, {})]]
    assert params.bandwidth == bandwidth
    reads = []
    for nb, seed, si_seed, kw in specs:
        seq, raw, _ = synth.synth_read(model, nb, seed, **kw)
        reads.append((raw, seq, None, _si(nb, si_seed)))
    return model, params, reads


@pytest.mark.parametrize('bandwidth', [100, 300, 700, 1500])
def test_dp_form_report_names_every_band_class(bandwidth):
    """(g) k_dp_multi at bandwidth 100, k_dp<5>, <12>, <24> at 300, 700, 1500 and k_dp_wide for the static bands
    wider than every class: the report, read by read, and the oracle's results beside it"""
    from tombo_amd import _native as N
    model, params, reads = _class_batch(bandwidth)
    with sharing(1):
        eng, out, oracles = run_batch(model, params, 'DNA', reads)
        bad = compare_batch(eng, oracles, out, 'w%d' % bandwidth)
        assert not bad, '\n'.join(bad[:40])
        assert not eng.last_dp_lowreg()
        form = check_dp_forms(eng, params, False, oracles)
        path = eng.get(N.GET_PATH)
    adaptive = (path[:, 0] == 1) & (path[:, 2] == bandwidth)
    assert adaptive.sum() >= 1, path.tolist()
    want = (N.DP_FORM_MULTI, 4) if bandwidth == 100 else (N.DP_FORM_K_DP, {300: 5, 700: 12, 1500: 24}[bandwidth])
    assert np.all(form[adaptive, 0] == want[0]) and np.all(form[adaptive, 1] == want[1]), form.tolist()
    if bandwidth == 100:
        assert adaptive.all()
    if bandwidth == 1500:
        assert np.all(form[:3, 0] == N.DP_FORM_WIDE) and np.all(form[:3, 1] == 0), form.tolist()
        assert form[3, 0] == N.DP_FORM_K_DP and form[3, 1] == cpl_class(path[3, 2])
    failed = path[:, 0] == 0
    assert np.all(form[failed, 0] == N.DP_FORM_NONE)

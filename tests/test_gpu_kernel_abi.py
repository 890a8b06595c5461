"""GPU: the per-kernel C ABI entry points (tba_c_*, bound with the Cython module's names in
tombo_amd/_c_dynamic_programming.py and _c_helper.py) against the oracle's kernel-level
restatements, on data from a synthetic read."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def read():
    import oracle
    from tombo_amd import synth, tombo_stats as ts, tombo_helper as th
    samp = th.seqSampleType('DNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)
    seq, raw, _ = synth.synth_read(model, 700, 4242, **synth.DNA_SYNTH)
    from tombo_amd._default_parameters import SIG_MATCH_THRESH
    o = oracle.resquiggle_read(
        raw, ts.encode_seq(seq), model.level_means, model.level_sds, oracle.make_params(params),
        oracle.make_opts(6, 2, outlier_thresh=5.0, sig_match_thresh=SIG_MATCH_THRESH['DNA']),
        debug=True)
    assert o['status'] == 0
    mu, sd = model.get_exp_levels_from_seq(seq)
    return dict(model=model, params=params, raw=raw, seq=seq, o=o, mu=mu, sd=sd)


def test_elementwise_kernels(read):
    import oracle
    from tombo_amd import _c_dynamic_programming as cdp, _c_helper as ch
    d = read['o']['dbg']
    sig = d['seg_norm_signal']
    z = cdp.c_base_z_scores(sig[:5000], 0.3, 0.35, True, 2.5)
    np.testing.assert_array_equal(z, oracle.base_z_scores(sig[:5000], 0.3, 0.35, True, 2.5))
    z = cdp.c_base_z_scores(sig[:100], -1.0, 0.7)
    np.testing.assert_array_equal(z, oracle.base_z_scores(sig[:100], -1.0, 0.7, False, 10.0))
    np.testing.assert_array_equal(ch.c_new_means(sig, d['valid_cpts']), d['event_means'])
    np.testing.assert_array_equal(ch.c_apply_outlier_thresh(sig, -0.5, 0.75),
                                  oracle.apply_outlier_thresh(sig, -0.5, 0.75))
    with pytest.raises(ValueError):
        ch.c_new_means(sig.astype(np.float32), d['valid_cpts'])


def test_segment_means_on_awkward_layouts():
    """c_new_means through the batch pipeline's own kernel (k_event_means -> wave_segment_sums, k_select.h):
    groups of 64 / 32 / ... / 4 segments per wavefront step, spans beyond the LDS slice staged piece by
    piece with running sums carried across the pieces, the software-pipelined group loop with one, two
    and many groups per wavefront, a first boundary past 0, odd offsets (16-byte loads that start on an
    8-byte boundary), single-sample and zero-length segments (0 / 0 = NaN, as the reference's division)"""
    import oracle
    from tombo_amd import _c_helper as ch
    rng = np.random.default_rng(20260927)

    def check(lengths, start=0, label=''):
        lengths = np.asarray(lengths, np.int64)
        segs = start + np.concatenate([[0], np.cumsum(lengths)])
        sig = rng.normal(0.0, 1.0, int(segs[-1]) + int(rng.integers(0, 5)))
        sig *= np.exp(rng.normal(0.0, 3.0, sig.shape[0]))          # (magnitudes apart: the order of the adds shows)
        got, want = ch.c_new_means(sig, segs), oracle.new_means(sig, segs)
        assert got.shape == want.shape, label
        with np.errstate(invalid='ignore'):
            assert np.array_equal(got, want, equal_nan=True), (label, np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8])

    for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4099):
        check(rng.integers(1, 12, n), start=int(rng.integers(0, 3)), label='short x %d' % n)
        check(rng.integers(5, 90, n), start=int(rng.integers(0, 3)), label='rna-like x %d' % n)
    # the widths around every slice size, alone and between short neighbours
    for w in (447, 448, 449, 767, 768, 769, 1279, 1280, 1281, 2559, 2561, 5000, 20001):
        check([w], label='one segment of %d' % w)
        check(np.concatenate([rng.integers(1, 9, 70), [w], rng.integers(1, 9, 70), [w, w], rng.integers(1, 9, 5)]),
              start=1, label='%d between short ones' % w)
    # heavy-tailed lengths: most groups fit, some spill
    for k in range(6):
        ln = np.maximum(1, (rng.pareto(1.3, 3000) * 6).astype(np.int64))
        check(ln, start=k, label='pareto %d' % k)
    # single samples only; zero-length segments among others
    check(np.ones(777, np.int64), label='ones')
    ln = rng.integers(0, 4, 500)
    ln[0] = 3
    check(ln, label='zero lengths')


def test_change_point_kernels(read):
    import oracle
    from tombo_amd import _c_helper as ch
    d = read['o']['dbg']
    sig = d['seg_norm_signal']
    n = len(d['valid_cpts'])
    np.testing.assert_array_equal(ch.c_valid_cpts_w_cap(sig, 3, 5, n), d['valid_cpts'])
    rc, want = oracle.valid_cpts(read['raw'], 6, 12, 400, ttest=True)
    assert rc == 0
    np.testing.assert_array_equal(ch.c_valid_cpts_w_cap_t_test(read['raw'], 6, 12, 400), want)
    # more change points than the signal can hold: the reference's error
    with pytest.raises(NotImplementedError, match='Fewer changepoints found than requested'):
        ch.c_valid_cpts_w_cap(sig[:600], 3, 5, 400)
    rc, _ = oracle.valid_cpts(sig[:600], 3, 5, 400)
    assert rc == 2


def test_change_points_with_exact_score_ties_and_tile_edges(dispatch_form):
    """quantised (integer) signal: many exactly equal scores, also at the threshold score ->
    priority falls to the higher index (DESIGN.md tie rule) like the oracle's ordering; lengths
    around the 3968-position tiles of the bit-sliced greedy; both exclusion radii.  In the
    throughput form the stand-alone entries run k_detect / k_detect_tt + k_pick (what they leave:
    the kernels that keep the scores), in the latency form k_cumsum_scores / k_scores_ttest + k_peaks."""
    import oracle
    from tombo_amd import _c_helper as _ch, _native as N
    forms = []

    class ch(object):   # every call also records which kernels answered it
        @staticmethod
        def c_valid_cpts_w_cap(*a):
            try:
                return _ch.c_valid_cpts_w_cap(*a)
            finally:
                forms.append(_ch.last_ed_form())

        @staticmethod
        def c_valid_cpts_w_cap_t_test(*a):
            try:
                return _ch.c_valid_cpts_w_cap_t_test(*a)
            finally:
                forms.append(_ch.last_ed_form())
    rng = np.random.default_rng(17)
    for n in (64, 700, 3968 + 10, 3968 + 74, 2 * 3968 + 9, 4096, 8192, 20011):
        sig = rng.integers(-3, 4, size=n).astype(np.float64)
        for frac in (0.02, 0.1, 0.19):
            k = max(2, int(n * frac))
            rc, want = oracle.valid_cpts(sig, 3, 5, k)
            if rc == 0:
                np.testing.assert_array_equal(ch.c_valid_cpts_w_cap(sig, 3, 5, k), want,
                                              err_msg='n=%d k=%d' % (n, k))
            else:
                with pytest.raises(NotImplementedError, match='Fewer changepoints'):
                    ch.c_valid_cpts_w_cap(sig, 3, 5, k)
        if n >= 700:
            k = max(2, n // 40)
            rc, want = oracle.valid_cpts(sig, 6, 12, k, ttest=True)
            if rc == 0:
                np.testing.assert_array_equal(ch.c_valid_cpts_w_cap_t_test(sig, 6, 12, k), want,
                                              err_msg='ttest n=%d k=%d' % (n, k))
    # window widths on both sides of the fused cumsum + score kernel's limit (2w <= 64), and
    # lengths around its 64-sample chunks
    for n, w in ((20011, 32), (20011, 33), (5000, 1), (64 * 7 + 1, 5), (64 * 7, 5), (64 * 7 - 1, 7)):
        sig = rng.normal(0, 1, n)
        k = max(2, n // 100)
        rc, want = oracle.valid_cpts(sig, 3, w, k)
        assert rc == 0
        np.testing.assert_array_equal(ch.c_valid_cpts_w_cap(sig, 3, w, k), want, err_msg='w=%d' % w)
    # continuous input around the tile edges
    for n in (3968 + 64 + 10 + 1, 3 * 3968 + 11):
        sig = rng.normal(0, 1, n)
        k = n // 6
        rc, want = oracle.valid_cpts(sig, 3, 5, k)
        assert rc == 0
        np.testing.assert_array_equal(ch.c_valid_cpts_w_cap(sig, 3, 5, k), want)
    fused = {N.ED_FORM_DETECT_PICK, N.ED_FORM_DETECT_TT_PICK}
    if dispatch_form == 'throughput':
        # the continuous signals and most of the quantised ones are finished by the score-free kernels
        assert sum(f == N.ED_FORM_DETECT_PICK for f in forms) >= 8, forms
        assert sum(f == N.ED_FORM_DETECT_TT_PICK for f in forms) >= 3, forms
    else:
        assert not (set(forms) & fused), forms


def test_forward_pass_and_traceback_kernels(read):
    import oracle
    from tombo_amd import _c_dynamic_programming as cdp
    p = read['params']
    ev = read['o']['dbg']['event_means']
    mu, sd = read['mu'], read['sd']
    # static band, as find_seq_start_in_events builds it (resquiggle.py:708-724)
    nb, bw = 120, 300
    z = np.empty((nb, bw))
    for r in range(nb):
        z[r] = p.z_shift - np.minimum(p.max_half_z_score, np.abs(ev[r:r + bw] - mu[r]) / sd[r])
    starts = np.arange(nb, dtype=np.int64)
    fwd, tb = cdp.c_banded_forward_pass(z, starts, p.skip_pen, p.stay_pen)
    ofwd, otb = oracle.banded_forward_pass(z, starts, p.skip_pen, p.stay_pen)
    np.testing.assert_array_equal(fwd, ofwd)
    np.testing.assert_array_equal(tb[1:], otb[1:])
    top = int(np.argmax(fwd[-1]))
    rc, want = oracle.banded_traceback(otb, starts, top)
    assert rc == 0
    np.testing.assert_array_equal(cdp.c_banded_traceback(tb, starts, top), want)
    with pytest.raises(NotImplementedError, match='extends beyond bandwidth'):
        cdp.c_banded_traceback(tb, starts, top, 140)
    # adaptive continuation from the static rows, in place (pyx:314-412)
    n_bases = 500
    fwd_a = np.zeros((n_bases + 1, bw))
    tb_a = np.zeros((n_bases + 1, bw), dtype=np.int64)
    st_a = np.zeros(n_bases, dtype=np.int64)
    fwd_a[:nb + 1], tb_a[:nb + 1], st_a[:nb] = fwd, tb, starts
    o_fwd, o_tb, o_st = fwd_a.copy(), tb_a.astype(np.int8), st_a.copy()
    rc = oracle.adaptive_banded_forward_pass(o_fwd, o_tb, o_st, ev, mu[:n_bases], sd[:n_bases],
                                             p.z_shift, p.skip_pen, p.stay_pen, nb, -15.0, True,
                                             p.max_half_z_score)
    assert rc == 0
    ret = cdp.c_adaptive_banded_forward_pass(
        fwd_a, tb_a, st_a, ev, mu[:n_bases], sd[:n_bases], p.z_shift, p.skip_pen, p.stay_pen, nb,
        -15.0, True, p.max_half_z_score)
    assert ret is None
    np.testing.assert_array_equal(st_a, o_st)
    np.testing.assert_array_equal(fwd_a, o_fwd)
    np.testing.assert_array_equal(tb_a[1:], o_tb[1:].astype(np.int64))
    # return_z_scores=True (pyx:339,387-388,409-410): same pass, plus the shifted z-scores of every row
    # it computed -- those are a function of the band starts it chose (pyx:361-386)
    fwd_z, tb_z, st_z = fwd_a.copy(), tb_a.copy(), st_a.copy()
    fwd_z[nb + 1:], tb_z[nb + 1:], st_z[nb:] = 0, 0, 0
    zs = cdp.c_adaptive_banded_forward_pass(
        fwd_z, tb_z, st_z, ev, mu[:n_bases], sd[:n_bases], p.z_shift, p.skip_pen, p.stay_pen, nb,
        -15.0, True, p.max_half_z_score, return_z_scores=True)
    np.testing.assert_array_equal(st_z, o_st)
    np.testing.assert_array_equal(fwd_z, o_fwd)
    assert zs.shape == (n_bases - nb, bw)
    want_z = np.full((n_bases - nb, bw), -15.0)
    for r in range(nb, n_bases):
        e = ev[o_st[r]:o_st[r] + bw]
        want_z[r - nb, :e.shape[0]] = p.z_shift - np.minimum(p.max_half_z_score, np.abs(e - mu[r]) / sd[r])
    np.testing.assert_array_equal(zs, want_z)
    # band start pushed past the last event (argmax at the right edge of a row that already sits
    # at the end of the events): the reference's error, pyx:349-357
    fwd_b, tb_b, st_b = fwd_a.copy(), tb_a.copy(), st_a.copy()
    fwd_b[nb] = np.arange(bw, dtype=np.float64)
    st_b[nb - 1] = ev.shape[0] - 10
    o_fwd, o_tb, o_st = fwd_b.copy(), tb_b.astype(np.int8), st_b.copy()
    rc = oracle.adaptive_banded_forward_pass(o_fwd, o_tb, o_st, ev, mu[:n_bases], sd[:n_bases],
                                             p.z_shift, p.skip_pen, p.stay_pen, nb, -15.0, True,
                                             p.max_half_z_score)
    assert rc == 10
    with pytest.raises(NotImplementedError, match='extended beyond raw signal'):
        cdp.c_adaptive_banded_forward_pass(
            fwd_b, tb_b, st_b, ev, mu[:n_bases], sd[:n_bases], p.z_shift, p.skip_pen,
            p.stay_pen, nb, -15.0, True, p.max_half_z_score)


@pytest.mark.parametrize('bw', [64, 100, 257, 300, 320, 321, 500, 700, 1000, 1500, 1610, 2000, 2500, 3072])
def test_row_engine_every_band_class(bw):
    """c_banded_forward_pass over random z-scores and random band offsets for every
    cells-per-lane instantiation of the wave-per-read kernel (CPL 4..48), noise-like scores with
    many exact ties (winsorised z) included"""
    import oracle
    from tombo_amd import _c_dynamic_programming as cdp
    rng = np.random.default_rng(bw)
    nb = 40
    z = 5.0 - np.abs(rng.normal(0, 6, size=(nb, bw)))
    z = np.maximum(z, -15.0)                       # winsorised floor -> exact ties
    z[rng.random(z.shape) < 0.02] = -15.0
    starts = np.cumsum(rng.integers(0, 4, size=nb)).astype(np.int64)
    starts[:5] = 0
    fwd, tb = cdp.c_banded_forward_pass(z, starts, 4.2, 4.2)
    ofwd, otb = oracle.banded_forward_pass(z, starts, 4.2, 4.2)
    np.testing.assert_array_equal(fwd, ofwd)
    np.testing.assert_array_equal(tb[1:], otb[1:])
    top = int(np.argmax(fwd[-1]))
    rc, want = oracle.banded_traceback(otb, starts, top)
    assert rc == 0
    np.testing.assert_array_equal(cdp.c_banded_traceback(tb, starts, top), want)


def test_row_constant_division_is_ieee():
    """div_by_recip (k_dp's z-score division by a per-row sd) == a / b bit for bit"""
    import ctypes as C
    from tombo_amd import resquiggle as rq
    eng = rq.get_engine(0)
    rng = np.random.default_rng(3)
    n = 1 << 21
    a = np.concatenate([
        rng.normal(0, 3, n // 4), rng.normal(0, 1e-3, n // 4), rng.uniform(-30, 30, n // 4),
        rng.normal(0, 1, n // 4) * 10.0 ** rng.uniform(-12, 6, n // 4)])
    b = np.concatenate([
        np.full(n // 4, 0.3528720791815676), np.full(n // 4, 0.2252531482690988),
        rng.uniform(0.05, 3.0, n // 4), 10.0 ** rng.uniform(-3, 3, n // 4)])
    a[:64] = 0.0
    a[64:128] = np.nextafter(b[64:128], 10)          # quotients next to 1
    a[128:192] = b[128:192] * (1 + 2.0 ** -52)
    out = np.empty(n)
    pd = C.POINTER(C.c_double)
    rc = eng._L.tba_selftest_division(eng._h, a.ctypes.data_as(pd), b.ctypes.data_as(pd),
                                      C.c_int64(n), out.ctypes.data_as(pd))
    assert rc == 0
    want = a / b
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, (bad[:5], a[bad[:5]], b[bad[:5]], out[bad[:5]], want[bad[:5]])


# ---- raw-signal DP kernels and the remaining helpers (K7-K9, H4, H6) -----------------------
def _kt():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                'kernels_tail.npz'))


def _rag(g, key, i):
    o = g[key + '_off']
    return g[key][o[i]:o[i + 1]]


def test_reg_z_forward_traceback_match_reference_vectors():
    """c_reg_z_scores -> c_base_forward_pass -> c_base_traceback chained like raw_forward_pass /
    raw_traceback (resquiggle.py:345-400), every call against the recorded reference output"""
    from tombo_amd._c_dynamic_programming import (
        c_reg_z_scores, c_base_forward_pass, c_base_traceback)
    g = _kt()
    for name in g['rz_names']:
        p = 'rz_%s_' % name
        rs, re_, mbs, m = (int(x) for x in g[p + 'args'])
        mh = float(g[p + 'mh'][0])
        res = c_reg_z_scores(g[p + 'sig'], g[p + 'means'], g[p + 'sds'], g[p + 'starts'], rs, re_,
                             mbs, m, max_half_z_score=None if np.isnan(mh) else mh)
        assert len(res) == re_ - rs
        for i, (z, b) in enumerate(res):
            assert b == tuple(g[p + 'bounds'][i])
            np.testing.assert_array_equal(z, _rag(g, p + 'z', i))
        # forward pass as raw_forward_pass drives it
        prev_data, (ps, pe) = res[0]
        fwd = np.cumsum(prev_data)
        ld = np.ones(pe - ps, dtype=np.int64) * m
        rows = [(fwd, (ps, pe))]
        for k, (b_data, (bs, be)) in enumerate(res[1:]):
            fwd, ld = c_base_forward_pass(b_data, bs, be, prev_data, ps, pe, fwd, ld, m)
            np.testing.assert_array_equal(fwd, _rag(g, p + 'fp_fwd', k))
            np.testing.assert_array_equal(ld, _rag(g, p + 'fp_last_diag', k))
            rows.append((fwd, (bs, be)))
            prev_data, ps, pe = b_data, bs, be
        # traceback as raw_traceback drives it
        new_segs = np.empty(len(rows) - 1, dtype=np.int64)
        sig_start = rows[-1][1][1] - 1
        for b in range(len(rows) - 1, 0, -1):
            cur, (cs, _) = rows[b]
            nxt, (ns, ne) = rows[b - 1]
            new_segs[b - 1] = c_base_traceback(cur, cs, nxt, ns, ne, sig_start, m)
            sig_start = new_segs[b - 1] - 1
        np.testing.assert_array_equal(new_segs, g[p + 'new_segs'])


def test_raw_dp_kernels_random_vs_oracle():
    import oracle
    from tombo_amd._c_dynamic_programming import (
        c_reg_z_scores, c_base_forward_pass, c_base_traceback)
    rng = np.random.default_rng(5)
    for trial in range(6):
        n, m = int(rng.integers(2, 11)), int(rng.integers(1, 4))
        L = int(rng.integers(n * m + 3, 200))
        starts = np.linspace(0, L, n + 1).astype(np.int64)
        sig, mu, sd = rng.normal(0, 1, L), rng.normal(0, 1, n), rng.uniform(0.1, 0.5, n)
        mh = None if trial % 2 else 4.0
        got = c_reg_z_scores(sig, mu, sd, starts, 0, n, n, m, max_half_z_score=mh)
        want = oracle.reg_z_scores(sig, mu, sd, starts, 0, n, n, m, mh)
        for (gz, gb), (wz, wb) in zip(got, want):
            assert gb == wb
            np.testing.assert_array_equal(gz, wz)
        prev, (ps, pe) = got[0]
        fwd, ld = np.cumsum(prev), np.full(pe - ps, m, np.int64)
        for b_data, (bs, be) in got[1:]:
            f2, l2 = c_base_forward_pass(b_data, bs, be, prev, ps, pe, fwd, ld, m)
            rc, of, ol = oracle.base_forward_pass(b_data, bs, be, prev, ps, pe, fwd, ld, m)
            assert rc == 0
            np.testing.assert_array_equal(f2, of)
            np.testing.assert_array_equal(l2, ol)
            tb = c_base_traceback(f2, bs, fwd, ps, pe, be - 1, m)
            assert (-1 if tb is None else tb) == oracle.base_traceback(f2, bs, fwd, ps, pe,
                                                                        be - 1, m)
            prev, ps, pe, fwd, ld = b_data, bs, be, f2, l2
    # running off the scan returns None like the Cython function
    assert c_base_traceback(np.zeros(3), 5, np.zeros(3), 9, 12, 2, 10) is None


def test_slopes_and_mean_stds_match_reference_vectors():
    import oracle
    from tombo_amd._c_helper import c_compute_slopes, c_new_mean_stds
    g = _kt()
    np.testing.assert_array_equal(c_compute_slopes(g['sl_ev'], g['sl_md']), g['sl_out'])
    np.testing.assert_array_equal(c_compute_slopes(g['sl_ev'], g['sl_md'], 5.0), g['sl_out_max5'])
    m, s = c_new_mean_stds(g['ms_sig'], g['ms_segs'])
    np.testing.assert_array_equal(m, g['ms_means'])
    np.testing.assert_array_equal(s, g['ms_stds'])
    # the size the Theil-Sen fit uses (1000 sampled bases -> 499 500 slopes)
    rng = np.random.default_rng(2)
    ev, md = rng.normal(0, 1, 1000), rng.normal(0, 1, 1000)
    ev[17] = ev[400]
    got = c_compute_slopes(ev, md)
    np.testing.assert_array_equal(got, oracle.compute_slopes(ev, md))
    assert got.shape[0] == 499500 and (got == 1000.0).sum() == 1


def test_approximate_quotient_stays_inside_its_guard_band():
    """k_theil_sen sorts slope pairs against its window with a * (rcp(b) + one Newton step) and a
    1e-5 guard band (exact division only inside the band): the approximation has to stay orders
    of magnitude inside it, including tiny and huge denominators"""
    import ctypes as C
    from tombo_amd import resquiggle as rq
    eng = rq.get_engine(0)
    rng = np.random.default_rng(9)
    n = 1 << 20
    a = rng.normal(0, 2, n)
    b = rng.normal(0, 1, n)
    b[:4096] = rng.normal(0, 1, 4096) * 10.0 ** rng.integers(-16, 3, 4096)   # |e_i - e_j| tiny .. large
    b[b == 0] = 1.0
    out = np.empty(n)
    pd = C.POINTER(C.c_double)
    rc = eng._L.tba_selftest_approx_quotient(eng._h, a.ctypes.data_as(pd), b.ctypes.data_as(pd),
                                             C.c_int64(n), out.ctypes.data_as(pd))
    assert rc == 0
    exact = a / b
    rel = np.abs(out - exact) / np.maximum(np.abs(exact), 1e-300)
    assert rel.max() < 1e-9, rel.max()


def test_llh_ratio_kernels_match_reference_vectors():
    """row N4: the model-comparison log-likelihood ratio kernels against vectors recorded from the
    reference's compiled functions; the constant-variance form has no transcendental and is bit
    equal, the others use the device log / exp / pow (tolerance 1e-12 relative)"""
    from tombo_amd import _c_helper as ch
    g = _kt()
    kw = int(g['llh_kw'][0])
    m, r, a = g['llh_means'], g['llh_ref_means'], g['llh_alt_means']
    rv, av = g['llh_ref_vars'], g['llh_alt_vars']
    sf, hf, hp = (float(x) for x in g['llh_scaled_params'])
    n = g['llh_var'].shape[0]
    starts = np.arange(n, dtype=np.int64)
    got_var = ch.llh_ratio_windows(0, m, r, a, rv, starts, kw, alt_vars=av)
    got_const = ch.llh_ratio_windows(1, m, r, a, rv, starts, kw)
    got_scaled = ch.llh_ratio_windows(2, m, r, a, rv, starts, kw, scale_factor=sf,
                                      density_height_factor=hf, density_height_power=hp)
    np.testing.assert_array_equal(got_const, g['llh_const'])
    np.testing.assert_allclose(got_var, g['llh_var'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got_scaled, g['llh_scaled'], rtol=1e-12, atol=1e-13)
    # one window per call == the Cython signatures
    for i in (0, 7, 55, n - 1):
        sl = slice(i, i + kw)
        assert ch.c_calc_llh_ratio_const_var(m[sl], r[sl], a[sl], rv[i]) == g['llh_const'][i]
        assert abs(ch.c_calc_llh_ratio(m[sl], r[sl], a[sl], rv[sl], av[sl]) - g['llh_var'][i]) \
            <= 1e-12 * max(1.0, abs(g['llh_var'][i]))
        assert abs(ch.c_calc_scaled_llh_ratio_const_var(m[sl], r[sl], a[sl], rv[i], sf, hf, hp)
                   - g['llh_scaled'][i]) <= 1e-12 * max(1.0, abs(g['llh_scaled'][i]))


# ---- host-side argument checks and early returns of the per-kernel entries ---------------------
# Each row passes one bad input straight to the C entry (the Python wrappers reject most of these
# before the call) and pins the return code and the tba_last_error() text.  Every call is either
# rejected on the host or runs a normal small kernel.  A row whose expected text is None must not
# touch the last error: it is set to a sentinel before the call.
E_ARG, INTERNAL = -1, 100
_SENTINEL = 'engine is NULL'


def _v(a):
    return a.ctypes.data_as(C.c_void_p)  # (keeps a temporary array alive until the call returns)


def _f(*shape):
    return np.zeros(shape, np.float64)


def _i(*shape):
    return np.zeros(shape, np.int64)


def _adaptive_fwd(L, e, b, starts, bandwidth):
    n_bases, n_events = 10, 50
    fwd, tb = _f((n_bases + 1) * 8), _i((n_bases + 1) * 8)
    return L.tba_c_adaptive_banded_forward_pass_z(
        e, _v(fwd), _v(tb), C.c_int64(n_bases), C.c_int64(bandwidth), _v(starts),
        _v(_f(n_events)), C.c_int64(n_events), _v(_f(n_bases)), _v(np.ones(n_bases)),
        C.c_double(0.0), C.c_double(1.0), C.c_double(1.0), C.c_int64(3), C.c_double(0.0),
        C.c_int(0), C.c_double(5.0), None)


def _banded_fwd(L, e, b):
    n_bases, bw = 6, 8
    starts = np.array([-1, 0, 1, 2, 3, 4], np.int64)
    return L.tba_c_banded_forward_pass(e, _v(_f(n_bases, bw)), C.c_int64(n_bases), C.c_int64(bw),
                                       _v(starts), C.c_double(1.0), C.c_double(1.0),
                                       _v(_f(n_bases + 1, bw)), _v(_i(n_bases + 1, bw)))


def _banded_tb(L, e, b):
    n_bases, bw = 6, 8
    return L.tba_c_banded_traceback(e, _v(_i(n_bases + 1, bw)), C.c_int64(n_bases), C.c_int64(bw),
                                    _v(np.arange(n_bases, dtype=np.int64)), C.c_int64(bw),
                                    C.c_int64(10), _v(_i(n_bases + 1)))


def _new_means(L, e, b, stds):
    sig, segs = _f(20), np.array([0, 5, 21], np.int64)
    if stds:
        return L.tba_c_new_mean_stds(e, _v(sig), C.c_int64(20), _v(segs), C.c_int64(2),
                                     _v(_f(2)), _v(_f(2)))
    return L.tba_c_new_means(e, _v(sig), C.c_int64(20), _v(segs), C.c_int64(2), _v(_f(2)))


def _slopes(L, e, b):
    n = 65536
    return L.tba_c_compute_slopes(e, _v(_f(n)), _v(_f(n)), C.c_int64(n), C.c_double(1.0), _v(_f(1)))


def _reg_z(L, e, b, n_b_starts, z_cap):
    n_sig, n_bases, reg_start, reg_end = 100, 10, 2, 5
    b_starts = np.arange(0, 110, 10, dtype=np.int64)
    bounds, z_off = _i(2 * (reg_end - reg_start)), np.full(reg_end - reg_start + 1, -7, np.int64)
    rc = L.tba_c_reg_z_scores(
        e, _v(np.linspace(-1.0, 1.0, n_sig)), C.c_int64(n_sig), _v(_f(n_bases)), _v(np.ones(n_bases)),
        C.c_int64(n_bases), _v(b_starts), C.c_int64(n_b_starts), C.c_int64(reg_start),
        C.c_int64(reg_end), C.c_int64(0), C.c_int64(1), C.c_int(0), C.c_double(5.0), _v(bounds),
        _v(z_off), _v(_f(max(z_cap, 1))), C.c_int64(z_cap))
    if z_cap < 30 and n_b_starts > reg_end:  # filled before the capacity is checked
        assert z_off.tolist() == [0, 10, 20, 30]
        assert not bounds.any()
    return rc


def _base_fwd(L, e, b, b_start, b_end):
    b_fwd, last = np.full(4, 3.5), np.full(4, 9, np.int64)
    rc = L.tba_c_base_forward_pass(e, _v(_f(4)), C.c_int64(b_start), C.c_int64(b_end), _v(_f(2)),
                                   C.c_int64(0), C.c_int64(2), _v(_f(2)), _v(_i(2)), C.c_int64(1),
                                   _v(b_fwd), _v(last))
    assert (b_fwd == 3.5).all() and (last == 9).all()  # untouched on a non-OK status
    return rc


def _valid_cpts(L, e, b):
    n, width = 10, 6
    return L.tba_c_valid_cpts_w_cap(e, _v(_f(n)), C.c_int64(n), C.c_int64(3), C.c_int64(width),
                                    C.c_int64(2), _v(_i(2)))


def _llh(L, e, b, kind, starts):
    n = 10
    return L.tba_llh_ratio_windows(e, C.c_int(kind), _v(_f(n)), _v(_f(n)), _v(_f(n)), _v(np.ones(n)),
                                   _v(np.ones(n)), C.c_int64(n), C.c_int64(3), _v(starts),
                                   C.c_int64(starts.shape[0]), _v(_f(3)), _v(_f(starts.shape[0])))


def _pvals(L, e, b, off):
    n_reads = off.shape[0] - 1
    return L.tba_read_pvals(e, _v(_f(8)), _v(_f(8)), _v(np.ones(8)), _v(off), C.c_int64(n_reads),
                            C.c_int64(1), C.c_int(1), C.c_double(1e-50), _v(_f(8)))


def _stalls(L, e, b):
    n_ints = np.full(1, -7, np.int64)
    rc = L.tba_identify_stalls(e, _v(_f(500)), C.c_int(0), C.c_int64(500), C.c_int64(100),
                               C.c_int64(7), C.c_int64(20), C.c_double(1.0), C.c_int64(100),
                               C.c_int64(10), _v(_i(8)), C.c_int64(4), _v(n_ints))
    assert n_ints[0] == -7
    return rc


def _division(L, e, b):
    return L.tba_selftest_division(e, _v(_f(1)), _v(np.ones(1)), C.c_int64(0), _v(_f(1)))


def _batch_get(L, e, b, what, short):
    h, n = b
    out = np.full(n, -7, np.int32)
    nbytes = out.nbytes - (4 if short else 0)
    rc = L.tba_batch_get(h, C.c_int(what), _v(out), C.c_int64(nbytes))
    assert (out == -7).all()
    return rc


def _empty(L, e, b, fn):
    out = np.full(3, 2.5)
    if fn == 'tba_c_base_z_scores':
        rc = L.tba_c_base_z_scores(e, _v(_f(3)), C.c_int64(0), C.c_double(0.0), C.c_double(1.0),
                                   C.c_int(1), C.c_double(5.0), _v(out))
    else:
        rc = L.tba_c_apply_outlier_thresh(e, _v(_f(3)), C.c_int64(0), C.c_double(-1.0),
                                          C.c_double(1.0), _v(out))
    assert (out == 2.5).all()
    return rc


_DEC = np.array([0, 3, 2, 4, 5, 6, 7, 8, 9, 10], np.int64)
_INC = np.array([0, 2, 3, 4, 5, 6, 7, 8, 9, 10], np.int64)
_GUARD_ROWS = [
    ('adaptive_fwd_decreasing_starts', lambda L, e, b: _adaptive_fwd(L, e, b, _DEC, 8), E_ARG,
     'event_starts must be non-decreasing inside [0, n_events)'),
    ('adaptive_fwd_bandwidth_1', lambda L, e, b: _adaptive_fwd(L, e, b, _INC, 1), E_ARG, 'bad arguments'),
    ('banded_fwd_negative_start', _banded_fwd, E_ARG, 'event_starts must be non-negative and non-decreasing'),
    ('banded_tb_band_pos', _banded_tb, E_ARG, 'bad arguments'),
    ('new_means_past_signal', lambda L, e, b: _new_means(L, e, b, False), E_ARG,
     'segment boundaries outside the signal'),
    ('new_mean_stds_past_signal', lambda L, e, b: _new_means(L, e, b, True), E_ARG,
     'segment boundaries outside the signal'),
    ('slopes_too_many_points', _slopes, E_ARG, 'too many points'),
    ('reg_z_region_outside', lambda L, e, b: _reg_z(L, e, b, 5, 100), E_ARG,
     'region outside the bases / base starts'),
    ('reg_z_cap_too_small', lambda L, e, b: _reg_z(L, e, b, 11, 5), E_ARG, 'z-score buffer too small'),
    ('base_fwd_empty_interval', lambda L, e, b: _base_fwd(L, e, b, 3, 3), E_ARG, 'empty base interval'),
    ('base_fwd_status_internal', lambda L, e, b: _base_fwd(L, e, b, 10, 12), INTERNAL, None),
    ('valid_cpts_too_wide', _valid_cpts, INTERNAL, None),
    ('llh_kind_3', lambda L, e, b: _llh(L, e, b, 3, np.array([0], np.int64)), E_ARG, 'bad arguments'),
    ('llh_window_outside', lambda L, e, b: _llh(L, e, b, 1, np.array([0, 8], np.int64)), E_ARG,
     'window outside the arrays'),
    ('pvals_offset_start', lambda L, e, b: _pvals(L, e, b, np.array([1, 4, 8], np.int64)), E_ARG,
     'offset arrays must start at 0'),
    ('pvals_offset_decreasing', lambda L, e, b: _pvals(L, e, b, np.array([0, 5, 4], np.int64)), E_ARG,
     'offset arrays must be non-decreasing'),
    ('stalls_window_size', _stalls, E_ARG, 'bad stall detection parameters'),
    ('selftest_division_n0', _division, E_ARG, 'bad arguments'),
    ('batch_get_unknown_selector', lambda L, e, b: _batch_get(L, e, b, 1000, False), E_ARG,
     'unknown TBA_GET_* selector'),
    ('batch_get_short_output', lambda L, e, b: _batch_get(L, e, b, 18, True), E_ARG,  # (TBA_GET_STATUS)
     'output buffer too small'),
    ('base_z_scores_n0', lambda L, e, b: _empty(L, e, b, 'tba_c_base_z_scores'), 0, None),
    ('apply_outlier_thresh_n0', lambda L, e, b: _empty(L, e, b, 'tba_c_apply_outlier_thresh'), 0, None),
]


@pytest.fixture(scope='module')
def run_batch(read):
    """a private engine holding one finished batch of the module's read (for tba_batch_get)"""
    from tombo_amd import _native as N, tombo_stats as ts
    eng = N.Engine(0)
    m = read['model']
    eng.set_model(m.level_means, m.level_sds, m.kmer_width, m.central_pos)
    eng.upload(N.make_params(read['params']), N.make_opts(outlier_thresh=5.0),
               [read['raw']] * 2, [ts.encode_seq(read['seq'])] * 2)
    eng.run()
    yield eng
    eng.close()


@pytest.mark.parametrize('row', _GUARD_ROWS, ids=[r[0] for r in _GUARD_ROWS])
def test_entry_argument_checks_and_early_returns(row, run_batch):
    from tombo_amd import _native as N
    from tombo_amd import resquiggle as rq
    _, call, want_rc, want_msg = row
    L = N.lib()
    assert L.tba_batch_sync(None) == E_ARG
    assert L.tba_last_error().decode() == _SENTINEL
    rc = call(L, rq.get_engine(0)._h, (run_batch._h, 2))
    assert rc == want_rc
    assert L.tba_last_error().decode() == (_SENTINEL if want_msg is None else want_msg)

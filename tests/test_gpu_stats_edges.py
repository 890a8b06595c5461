"""The statistics kernels (k_read_pvals in k_cabi.h, the pileup kernels of k_group.h) at the
edges the small golden fixtures do not reach, against tests/stats_reference.py (pinned to the
live reference by test_stats_reference.py) and tests/golden/stats_wide.npz:
  - Fisher's method at every window width up to fm_offset 64 with window sums hx from 0 through
    the band where exp(-hx) underflows (~700 - 1100) to fully floored windows;
  - window means over np_sum's eight-accumulator path and its split above 128 values;
  - the three sort size classes (64 / 4096 levels) at their boundaries in one call;
  - get_reads_ref at numpy's pairwise-sum edges (8, 128, 8192 values);
  - batches of 1000+ regions; the branch points of the special functions.

Tolerances: statistics, window means, medians, means, stds, positions and coverages bit-equal;
p-values 1e-12 relative (t test 1e-11) with atol 1e-305; NaN patterns identical.
"""
import numpy as np
import pytest

import stats_reference as sr
from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq
from tombo_amd._default_parameters import SMALLEST_PVAL

pytestmark = pytest.mark.gpu

FMS = [1, 2, 3, 4, 7, 8, 16, 32, 61, 62, 63, 64]
LOG_FLOOR = -np.log(1e-50)


def _read(start, means, strand='+', seq=None):
    return th.resquiggledRead(start, start + means.shape[0], False, 0, strand, None, None, False,
                              read_id='x', means=means, seq=seq)


def _close(got, want, rtol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if rtol == 0:
        assert np.array_equal(got[ok], want[ok])
    else:
        np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=1e-305)


def _rtol(stat_type):
    return 0 if 'stat' in stat_type else (1e-11 if stat_type == 't_test' else 1e-12)


def _z_profile(fm, rng, lo=-3.0, hi=1.6):
    """|z| on a log ramp lo -> hi, a plateau longer than the window at 10^hi (p floored), a ramp
    back and a quiet tail longer than the window: the window sums of width 2 fm + 1 run from ~0
    to saturation"""
    w = 2 * fm + 1
    u = np.concatenate([np.linspace(lo, hi, 90), np.full(w + 12, hi), np.linspace(hi, lo, 70),
                        np.full(w + 5, lo)])
    return 10.0 ** (u + rng.normal(0, 0.04, u.shape[0]))


def _assert_hx_band(hx, fm, low=5.0):
    """the windows cover hx from below `low` to saturation, the underflow band included"""
    hx = hx[~np.isnan(hx)]
    w = 2 * fm + 1
    assert hx.min() < low and hx.max() > LOG_FLOOR * w - 1e-6
    if w * LOG_FLOOR > 730:
        assert ((hx > 718) & (hx < min(1100, LOG_FLOOR * w - 1))).sum() >= 3


# ---- 4a: Fisher's method ------------------------------------------------------------------------
@pytest.mark.parametrize('fm', FMS)
def test_fisher_sweep_per_read(fm):
    """sample-compare (batch form) and de novo (array form) across the whole hx range"""
    rng = np.random.default_rng(100 + fm)
    reads, cms, css, dn = [], [], [], []
    for k, strand in enumerate('+-'):
        z = _z_profile(fm, rng) * np.where(rng.random(1) < 0.5, 1, -1)
        n = z.shape[0]
        cs = np.abs(rng.normal(0.3, 0.05, n + 2 * fm)) + 0.05
        cm = rng.normal(0, 1, n + 2 * fm)
        gm = cm[fm:fm + n] + z * cs[fm:fm + n]                    # genome order
        gm[[5, 6, 150]] = cm[fm + np.array([5, 6, 150])]           # p == 1 exactly
        cm[fm + 40] = np.nan                                       # NaN inside windows
        gm[110] = np.nan
        reads.append(_read(1000 * (k + 1), gm[::-1].copy() if strand == '-' else gm, strand))
        cms.append(cm)
        css.append(cs)
        ref_m = rng.normal(0, 1, n)
        ref_s = np.abs(rng.normal(0.3, 0.05, n)) + 0.05
        dmeans = ref_m + z * ref_s
        dmeans[[5, 6]] = ref_m[[5, 6]]
        dmeans[100] = np.nan
        dn.append((dmeans, ref_m, ref_s))
    got = ts.compute_sample_compare_read_stats_batch(reads, cms, css, fm)
    for rd, cm, cs, g in zip(reads, cms, css, got):
        want_p, want_pos = sr.sample_compare_read_pvals(rd.means, rd.start, rd.end, rd.strand, cm, cs, fm)
        assert np.array_equal(g[1], want_pos)
        _close(g[0], want_p, 1e-12)
    off = np.concatenate([[0], np.cumsum([d[0].shape[0] for d in dn])])
    pv = rq.get_engine().read_pvals(np.concatenate([d[0] for d in dn]), np.concatenate([d[1] for d in dn]),
                                    np.concatenate([d[2] for d in dn]), off, fm, True, SMALLEST_PVAL)
    for k, d in enumerate(dn):
        _close(pv[off[k]:off[k + 1]], sr.de_novo_pvals(d[0], d[1], d[2], fm), 1e-12)
        _assert_hx_band(sr.window_hx(sr.z_pvals(d[0], d[1], d[2]), fm), fm)


def _shift_region(start, fm, rng, n_reads=6, lo=-2.0, hi=7.0, strand='+'):
    """n_reads sample and control reads over the region extended by fm; the control levels
    shifted on a log ramp (plateau longer than the window at 10^hi, then a quiet tail)"""
    w = 2 * fm + 1
    u = np.concatenate([np.linspace(lo, hi, 90), np.full(w + 12, hi), np.linspace(hi, lo, 70),
                        np.full(w + 5, lo)])
    shift = 10.0 ** (u + rng.normal(0, 0.04, u.shape[0]))
    L = shift.shape[0]
    a = start - fm
    groups = []
    for ctrl in (0, 1):
        rs = []
        for k in range(n_reads):
            m = rng.normal(0, 1, L) + (shift if ctrl else 0.0)
            if k == 0:
                m[rng.random(L) < 0.03] = np.nan
            rs.append(_read(a, m[::-1].copy() if strand == '-' else m, strand))
        groups.append(rs)
    end = a + L - fm
    return groups[0], groups[1], end


@pytest.mark.parametrize('stat_type', ['ks_test', 'u_test', 't_test'])
def test_fisher_sweep_group(stat_type):
    rng = np.random.default_rng(7 + len(stat_type))
    for fm in FMS:
        w = 2 * fm + 1
        samp, ctrl, end = _shift_region(3000, fm, rng, strand='-' if fm % 2 else '+')
        strand = samp[0].strand
        got = ts.compute_group_reg_stats(th.regionData('c', strand, 3000, end, samp),
                                         th.regionData('c', strand, 3000, end, ctrl), fm, 3, stat_type)
        want = sr.compute_group_reg_stats(samp, ctrl, 3000, end, strand, fm, 3, stat_type)
        gs = got[0][1]
        assert np.array_equal(gs.reg_poss, want[1]) and np.array_equal(gs.reg_cov, want[2])
        assert np.array_equal(gs.ctrl_cov, want[3])
        _close(gs.reg_stats, want[0], _rtol(stat_type))
        if stat_type == 't_test':
            raw = sr.compute_group_reg_stats(samp, ctrl, 3000 - fm, end + fm, strand, 0, 3, stat_type)[0]
            _assert_hx_band(sr.window_hx(raw, fm), fm, low=2.0 * w)


def test_resident_batch_de_novo_wide_window():
    """tba_batch_de_novo_stats at fm 16 and 64 == the array form, and == the restatement"""
    from tombo_amd import resquiggle as rq, synth
    samp = th.seqSampleType('DNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)
    mrs = [synth.synth_map_res(model, nb, 5100 + nb, **synth.DNA_SYNTH) for nb in (400, 650, 900)]
    res, tabs = rq.resquiggle_batch_events(mrs, model, params, outlier_thresh=5.0, seq_samp_type=samp)
    n_checked = 0
    for fm in (16, 64):
        got = rq.batch_de_novo_stats(fm_offset=fm)
        for i, r in enumerate(res):
            if isinstance(r, Exception):
                continue
            rd = th.read_from_results(r, tabs[i]['norm_mean'])
            want = ts.compute_de_novo_read_stats_batch([rd], model, fm)[0]
            if isinstance(want, Exception):
                assert got[i] is None
                continue
            np.testing.assert_array_equal(got[i][0], want[0])
            np.testing.assert_array_equal(got[i][1], want[1])
            K, cp = model.kmer_width, model.central_pos
            lb, le = (cp, K - cp - 1) if rd.strand == '+' else (K - cp - 1, cp)
            gm = np.asarray(rd.means)[::-1] if rd.strand == '-' else np.asarray(rd.means)
            ref_m, ref_s = model.get_exp_levels_from_seq(rd.seq, rd.strand == '-')
            _close(want[0], sr.de_novo_pvals(gm[lb:gm.shape[0] - le], ref_m, ref_s, fm), 1e-12)
            n_checked += 1
    assert n_checked >= 4


# ---- 4b: window means ---------------------------------------------------------------------------
def _runs_region(start, fm, rng, lens, gap=3):
    """coverage runs of the given lengths (3 sample + 3 control reads each), the first starting at
    the extended region's first position, the last ending at its last"""
    a = start - fm
    samp, ctrl, pos = [], [], a
    for k, L in enumerate(lens):
        for rs in (samp, ctrl):
            for _ in range(3):
                rs.append(_read(pos, rng.normal(0, 1, L) + 0.3 * len(rs)))
        pos += L + (gap if k < len(lens) - 1 else 0)
    return samp, ctrl, pos - fm


@pytest.mark.parametrize('fm', [4, 8, 63, 64])
@pytest.mark.parametrize('stat_type', ['ks_stat_test', 'u_stat_test', 't_stat_test'])
def test_window_means_bit_equal(fm, stat_type):
    rng = np.random.default_rng(fm)
    w = 2 * fm + 1
    lens = [w, 2 * fm, w + 37, 1, 2 * fm, w]   # kept, dropped, kept, dropped, dropped, kept (edge)
    samp, ctrl, end = _runs_region(800, fm, rng, lens)
    got = ts.compute_group_reg_stats(th.regionData('c', '+', 800, end, samp),
                                     th.regionData('c', '+', 800, end, ctrl), fm, 3, stat_type)
    want = sr.compute_group_reg_stats(samp, ctrl, 800, end, '+', fm, 3, stat_type)
    gs = got[0][1]
    assert gs.reg_poss.shape[0] == 3 * w + 37
    assert np.array_equal(gs.reg_poss, want[1])
    _close(gs.reg_stats, want[0], 0)


# ---- 4c: golden ---------------------------------------------------------------------------------
def test_stats_wide_golden():
    import os
    from conftest import GOLDEN_DIR
    from test_stats_reference import group_golden_reads, wide_read_case
    g = np.load(os.path.join(GOLDEN_DIR, 'stats_wide.npz'))
    fms, mtr = [int(f) for f in g['fm_offsets']], int(g['min_test_reads'])
    n_regs = g['reg_start'].shape[0]
    samp, ctrl = [], []
    for ri in range(n_regs):
        s_r, c_r = group_golden_reads(g, ri)
        args = ('chr1', '-' if g['reg_minus'][ri] else '+', int(g['reg_start'][ri]), int(g['reg_end'][ri]))
        samp.append(th.regionData(*args, reads=[_read(r.start, r.means, r.strand) for r in s_r]))
        ctrl.append(th.regionData(*args, reads=[_read(r.start, r.means, r.strand) for r in c_r]))
    for st in sr.STATS:
        for fm in fms:
            res = ts.compute_group_reg_stats_batch(samp, ctrl, fm, mtr, st)
            for ri in range(n_regs):
                key = 'g_%s_fm%d_m%d_r%d' % (st, fm, mtr, ri)
                assert len(res[ri]) == int(g[key + '_n']), key
                if not res[ri]:
                    continue
                gs = res[ri][0][1]
                assert np.array_equal(gs.reg_poss, g[key + '_poss']), key
                assert np.array_equal(gs.reg_cov, g[key + '_cov']), key
                assert np.array_equal(gs.ctrl_cov, g[key + '_ctrl_cov']), key
                _close(gs.reg_stats, g[key + '_stats'], _rtol(st))
    model = ts.TomboModel(seq_samp_type=th.seqSampleType('DNA', False))
    for ci in range(int(g['n_read_cases'])):
        means, start, n, strand, cm, cs, _ = wide_read_case(g, ci, model)
        rd = _read(start, means, strand, seq=str(g['pr%d_seq' % ci]))
        for fm in fms:
            tag = 'w%d_fm%d' % (ci, fm)
            p, pos = ts.compute_sample_compare_read_stats_batch(
                [rd], [cm[64 - fm:64 + n + fm]], [cs[64 - fm:64 + n + fm]], fm)[0]
            assert np.array_equal(pos, g[tag + '_sc_pos'])
            _close(p, g[tag + '_sc_p'], 1e-12)
            p, pos = ts.compute_de_novo_read_stats_batch([rd], model, fm)[0]
            assert np.array_equal(pos, g[tag + '_dn_pos'])
            _close(p, g[tag + '_dn_p'], 1e-12)


# ---- 4d: sort size classes ----------------------------------------------------------------------
COVS = [1, 2, 3, 63, 64, 65, 127, 128, 4095, 4096, 4097]


def _pointwise_region(start, levels):
    """one length-1 read per level: levels[i] = (sample levels, control levels) of position
    start + i"""
    samp, ctrl = [], []
    for i, (s, c) in enumerate(levels):
        samp += [_read(start + i, np.array([v])) for v in s]
        ctrl += [_read(start + i, np.array([v])) for v in c]
    end = start + len(levels)
    return th.regionData('c', '+', start, end, samp), th.regionData('c', '+', start, end, ctrl)


def _check_pointwise(levels, stat_types, start=100):
    samp, ctrl = _pointwise_region(start, levels)
    for st in stat_types:
        gs = ts.compute_group_reg_stats(samp, ctrl, 0, 1, st)[0][1]
        assert gs.reg_poss.tolist() == list(range(start, start + len(levels)))
        assert gs.reg_cov.tolist() == [len(s) for s, _ in levels]
        assert gs.ctrl_cov.tolist() == [len(c) for _, c in levels]
        want = np.array([sr.group_stat(st, s, c) for s, c in levels])
        _close(gs.reg_stats, want, _rtol(st))


def _class_pairs(rng):
    i = np.arange(len(COVS))
    return list(zip(COVS, np.array(COVS)[rng.permutation(i)])) + list(zip(rng.permutation(COVS), COVS))


def test_sort_classes_continuous():
    rng = np.random.default_rng(11)
    levels = [(rng.normal(0, 1, ns), rng.normal(0.2, 1.3, nc)) for ns, nc in _class_pairs(rng)]
    _check_pointwise(levels, sr.STATS)


def test_sort_classes_quantised_ties():
    """ties within groups everywhere; KS / t also across groups; U: sample levels on even and
    control levels on odd multiples of the quantum (cross-group ties rank in an unstated order in
    the reference)"""
    rng = np.random.default_rng(12)
    q = 0.125
    pairs = _class_pairs(rng)
    tied = [(np.round(rng.normal(0, 1, ns) / q) * q, np.round(rng.normal(0.1, 1, nc) / q) * q)
            for ns, nc in pairs]
    _check_pointwise(tied, ['ks_test', 'ks_stat_test', 't_test', 't_stat_test'])
    disjoint = [(2 * np.round(rng.normal(0, 3, ns)) * q, (2 * np.round(rng.normal(0.5, 3, nc)) + 1) * q)
                for ns, nc in pairs]
    _check_pointwise(disjoint, ['u_test', 'u_stat_test'])


# ---- 4e: get_reads_ref at numpy's summation edges ----------------------------------------------
REF_NS = [1, 2, 7, 8, 9, 16, 127, 128, 129, 136, 255, 256, 257, 8191, 8192, 8193, 16384, 16385, 16392]


def test_reads_ref_summation_edges():
    rng = np.random.default_rng(13)
    levels = [rng.normal(0, 1, n) * 10 ** rng.uniform(-3, 3) + rng.uniform(-50, 50) for n in REF_NS]
    levels.append(np.full(5, 0.37))                                # all equal: sd 0 -> NaN
    start = 400
    reads = [_read(start + i, np.array([v])) for i, lv in enumerate(levels) for v in lv]
    end = start + len(levels)
    reg = th.regionData('c', '+', start, end, reads)
    for est_mean in (False, True):
        lm, ls, cov = ts.get_reads_ref(reg, 1, 0, est_mean=est_mean)
        want_m, want_s, want_c = sr.get_reads_ref(reads, start, end, '+', 1, 0, est_mean=est_mean)
        _close(lm, want_m, 0)
        _close(ls, want_s, 0)
        assert [cov[p] for p in range(start, end)] == want_c.tolist()
        assert np.isnan(lm[-1]) and np.isnan(ls[-1])
    # the prior blend: model levels over the region's k-mers
    model = ts.TomboModel(seq_samp_type=th.seqSampleType('DNA', False))
    K, cp = model.kmer_width, model.central_pos
    seq = ''.join('ACGT'[c] for c in rng.integers(0, 4, end - start + 2 * (K - 1)))
    reg = th.regionData('c', '+', start, end, reads, seq=seq)
    pm, ps = model.get_exp_levels_from_seq_with_gaps(seq[K - 1 - cp:len(seq) - cp], False)
    for est_mean in (False, True):
        lm, ls, _ = ts.get_reads_ref(reg, 1, 0, model, (7.5, 3.0), est_mean)
        want_m, want_s, _ = sr.get_reads_ref(reads, start, end, '+', 1, 0, pm, ps, (7.5, 3.0), est_mean)
        _close(lm, want_m, 0)
        _close(ls, want_s, 0)


# ---- 4f: batch geometry -------------------------------------------------------------------------
def _geometry_batch(rng, fm, n_regions=1000):
    regs, edges = [], [63, 64, 65, 127, 128]
    for r in range(n_regions):
        L = int(np.exp(rng.uniform(0, np.log(600))))
        start = 10000 * (r + 1)
        strand = '+-'[r % 2]
        ext = L + 2 * fm
        a0 = start - fm
        groups = []
        for ctrl in (0, 1):
            rs = []
            kind = r % 7
            for k in range(4):
                if kind == 6:                      # too few reads / other strand: nothing covered
                    st, en, s_ = a0, a0 + ext, ('+-'[(r + 1) % 2] if k < 3 else strand)
                elif kind in (0, 1) and ext > 130:  # runs starting / ending at the chunk edges
                    e = edges[(r // 7) % 5]
                    st, en = (a0 + e, a0 + ext) if kind == 0 else (a0, a0 + e)
                    s_ = strand
                else:
                    st = a0 + int(rng.integers(-5, max(ext // 2, 1)))
                    en = st + int(rng.integers(1, ext + 10))
                    s_ = strand
                m = rng.normal(0.25 * ctrl, 1, en - st)
                if k == 1:
                    m[rng.random(en - st) < 0.05] = np.nan
                rs.append(_read(st, m[::-1].copy() if s_ == '-' else m, s_))
            groups.append(rs)
        regs.append((start, start + L, strand, groups[0], groups[1]))
    return regs


@pytest.mark.parametrize('fm', [0, 1, 7, 64])
def test_batch_geometry(fm):
    rng = np.random.default_rng(200 + fm)
    regs = _geometry_batch(rng, fm)
    samp = [th.regionData('c', st, s, e, sr_) for s, e, st, sr_, _ in regs]
    ctrl = [th.regionData('c', st, s, e, cr) for s, e, st, _, cr in regs]
    stat_type = 'ks_test' if fm % 2 else 't_stat_test'
    batch = ts.compute_group_reg_stats_batch(samp, ctrl, fm, 3, stat_type)
    assert sum(1 for b in batch if not b) >= 100
    for ri in range(len(regs)):
        one = ts.compute_group_reg_stats(samp[ri], ctrl[ri], fm, 3, stat_type)
        assert len(one) == len(batch[ri])
        if one:
            a, b = one[0][1], batch[ri][0][1]
            for f in ('reg_stats', 'reg_poss', 'reg_cov', 'ctrl_cov'):
                assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), (ri, f)
        if ri % 10 == 0:
            s, e, strand, sr_, cr = regs[ri]
            want = sr.compute_group_reg_stats(sr_, cr, s, e, strand, fm, 3, stat_type)
            assert (want is None) == (not batch[ri])
            if want is not None:
                gs = batch[ri][0][1]
                assert np.array_equal(gs.reg_poss, want[1]) and np.array_equal(gs.reg_cov, want[2])
                _close(gs.reg_stats, want[0], _rtol(stat_type))
    # get_reads_ref over the control reads, the region strand and no strand filter
    for strand_none in (False, True):
        regions = [th.regionData('c', None if strand_none else st, s, e, cr) for s, e, st, _, cr in regs]
        res = ts.get_reads_ref_batch(regions, 3, fm)
        for ri in range(0, len(regs), 10):
            s, e, st, _, cr = regs[ri]
            want_m, want_s, want_c = sr.get_reads_ref(cr, s, e, None if strand_none else st, 3, fm)
            lm, ls, cov = res[ri]
            _close(lm, want_m, 0)
            _close(ls, want_s, 0)
            assert (want_c is None) == (cov == {})


# ---- 4g: special-function regimes ---------------------------------------------------------------
def test_special_function_regimes():
    rng = np.random.default_rng(14)
    levels = []
    # KS: interleaved groups, control shifted by k steps: d = (k + 1) / n;
    # x = (en + 0.12 + 0.11 / en) d: 0.0413, 0.0406 (n = 310), 0.785 / 0.8205 about 0.82, d = 1
    for n, k in ((300, 0), (310, 0), (400, 0), (400, 2), (400, 21), (400, 22), (400, 59), (64, 63),
                 (5, 4), (400, 399)):
        s = 2.0 * np.arange(n)
        levels.append((s, s + 2.0 * k + 1.0))
    # U: the z of partially overlapping groups out to the full separation (z -> -sqrt(3))
    for shift in (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 6.0, 40.0):
        levels.append((rng.normal(0, 1, 40), rng.normal(shift, 1, 45)))
    # t: dof 1, 2, 3, 4 and >= 8000, t on both sides of -2
    # (evenly spaced levels, the control shifted to a target t)
    for ns, nc in ((2, 1), (2, 2), (3, 2), (3, 3), (4001, 4001), (4200, 3900)):
        s, c = np.linspace(-1, 1, ns), np.linspace(-1.3, 1.3, nc)
        sp = np.sqrt(((ns - 1) * np.var(s) + (nc - 1) * np.var(c)) / (ns + nc - 2))
        for t in (0.05, 0.6, 1.6, 1.99, 2.01, 2.6, 8.0, 60.0):
            levels.append((s, c + t * sp * np.sqrt(1.0 / ns + 1.0 / nc)))
    ks_x = np.array([sr.group_special_args('ks_test', s, c) for s, c in levels[:10]])
    assert (ks_x < 0.0406).any() and ((ks_x > 0.0407) & (ks_x < 0.82)).any() and (ks_x > 0.82).any()
    assert ((ks_x > 0.75) & (ks_x < 0.82)).any() and ((ks_x > 0.82) & (ks_x < 0.86)).any()
    assert (ks_x > 14).any()
    u_z = np.array([sr.group_special_args('u_test', s, c) for s, c in levels[10:18]])
    assert (u_z > -0.7).any() and (u_z < -1.72).any()
    targs = [sr.group_special_args('t_test', s, c) for s, c in levels[18:]]
    for dof in (1, 2, 3, 4):
        ts_ = [t for t, k in targs if k == dof]
        assert min(ts_) < -2 < max(ts_)
    assert min(t for t, k in targs if k >= 8000) < -2 < max(t for t, k in targs if k >= 8000)
    _check_pointwise(levels, ['ks_test', 'u_test', 't_test'])

"""Golden vectors of the statistics at wide Fisher / mean windows from the REFERENCE (build
container only).

    python tests/golden/gen_golden_wide_windows.py   # writes tests/golden/stats_wide.npz

(The `stats_` prefix keeps the file out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference's compute_group_reg_stats (all six test types),
compute_sample_compare_read_stats and compute_de_novo_read_stats at fm_offset 4, 7, 16 and 64 on
synthetic reads with strong signals: the z scores / group shifts climb on a log scale from ~0 to
far beyond the 1e-50 p-value floor, hold there for more than the widest window, and fall back, so
that the window sums hx = -sum(log p) of every width run from 0 through the band where exp(-hx)
underflows (hx ~ 700 - 1100) to fully floored windows.  Level accessors are pointed at in-memory
arrays as in gen_golden_group_stats.py / gen_golden_stats.py; only data is written.

Group levels are continuous draws, so no sample level equals a control level (the U test's rank
order of cross-group ties is unstated in the reference).
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_oracle  # noqa: E402
import stats_reference as sr  # noqa: E402
from tombo_amd import tombo_stats as my_ts, tombo_helper as my_th  # noqa: E402

rq, ts, th = ref_oracle.load()
STORE = {}
STATS = ['ks_test', 'u_test', 't_test', 'ks_stat_test', 'u_stat_test', 't_stat_test']
FMS = (4, 7, 16, 64)
MIN_READS = 3


class FakeFile(object):
    def __init__(self, fn, mode='r'):
        self.fn = fn

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class _Rd(object):
    def __init__(self, start, end, strand, means):
        self.start, self.end, self.strand, self.means = start, end, strand, means


class _Slot(object):
    def __init__(self, rid):
        self.attrs = {'read_id': rid}


def install():
    ts.h5py.File = FakeFile
    th.get_multiple_slots_read_centric = lambda f, names, grp=None: [STORE[f.fn][n] for n in names]
    th.get_single_slot_read_centric = lambda r, name, grp=None: STORE[getattr(r, 'fn', r)][name]
    th.get_raw_read_slot = lambda f: _Slot(STORE[f.fn]['read_id'])


def profile(n, lo, hi, rng):
    """log-scale ramp lo -> hi over ~n/4, a plateau of at least 140 positions at hi, ramp back,
    a quiet tail; the ramps are jittered so window sums do not repeat"""
    up = max(n // 4, 20)
    flat = max(140, n // 3)
    down = max(n // 5, 20)
    u = np.concatenate([np.linspace(lo, hi, up), np.full(flat, hi), np.linspace(hi, lo, down)])
    u = np.concatenate([u, np.full(max(n - u.shape[0], 0), lo)])[:n]
    return 10.0 ** (u + rng.normal(0, 0.05, n))


def main():
    install()
    rng = np.random.default_rng(2252)
    out = {'fm_offsets': np.array(FMS), 'min_test_reads': np.array(MIN_READS)}

    # ---- group statistics: (start, end, strand, sample reads, control reads, log10 shift range)
    regs = [(2000, 2300, '+', 6, 6, (-2.0, 7.0)), (5000, 5090, '-', 5, 5, (-1.5, 6.5))]
    rd_start, rd_len, rd_minus, rd_ctrl, rd_reg, rd_means = [], [], [], [], [], []
    ref_regs, ref_ctrl, plain = [], [], []
    for ri, (s, e, strand, ns, nc, (lo, hi)) in enumerate(regs):
        a, b = s - 64 - 3, e + 64 + 3
        shift = profile(b - a, lo, hi, rng)                         # genome order
        reads, mine = {0: [], 1: []}, {0: [], 1: []}
        for ctrl, depth in ((0, ns), (1, nc)):
            for k in range(depth + 1):
                minus = strand == '-'
                st, en = a, b
                if k == depth:            # a read of the other strand: skipped by the pileup
                    minus = not minus
                elif k == 1:              # starts inside the window range, ends early
                    st, en = a + 70, b - 40
                m = rng.normal(0.0, 1.0, en - st) + (shift[st - a:en - a] if ctrl else 0.0)
                if k == 2:
                    m[rng.random(m.shape[0]) < 0.02] = np.nan
                rc = m[::-1].copy() if minus else m          # read-centric
                fn = 'g%d' % len(STORE)
                STORE[fn] = {'norm_mean': rc}
                reads[ctrl].append(th.readData(st, en, False, 0, '-' if minus else '+', fn, 'grp',
                                               False, 0.0, 10.0, fn))
                mine[ctrl].append(_Rd(st, en, '-' if minus else '+', rc))
                rd_start.append(st); rd_len.append(en - st); rd_minus.append(minus)
                rd_ctrl.append(ctrl); rd_reg.append(ri); rd_means.append(rc)
        ref_regs.append(th.intervalData('chr1', s, e, strand, reads=reads[0]))
        ref_ctrl.append(th.intervalData('chr1', s, e, strand, reads=reads[1]))
        plain.append(mine)
    out.update(reg_start=np.array([r[0] for r in regs]), reg_end=np.array([r[1] for r in regs]),
               reg_minus=np.array([r[2] == '-' for r in regs]),
               rd_start=np.array(rd_start), rd_len=np.array(rd_len), rd_minus=np.array(rd_minus),
               rd_ctrl=np.array(rd_ctrl), rd_reg=np.array(rd_reg), rd_means=np.concatenate(rd_means))
    hx_seen = {}
    for st in STATS:
        for fm in FMS:
            for ri in range(len(regs)):
                res = ts.compute_group_reg_stats(ref_regs[ri], ref_ctrl[ri], fm, MIN_READS, st)
                key = 'g_%s_fm%d_m%d_r%d' % (st, fm, MIN_READS, ri)
                out[key + '_n'] = np.array(len(res))
                if res:
                    gs = res[0][1]
                    out[key + '_stats'] = gs.reg_stats
                    out[key + '_poss'] = gs.reg_poss
                    out[key + '_cov'] = gs.reg_cov
                    out[key + '_ctrl_cov'] = gs.ctrl_cov
                if st in ('t_test', 'ks_test'):   # (diagnostics only: windows across run gaps)
                    s, e, strand = regs[ri][:3]
                    raw = sr.compute_group_reg_stats(plain[ri][0], plain[ri][1], s - fm,
                                                     e + fm, strand, 0, MIN_READS, st)[0]
                    hx_seen.setdefault(fm, []).append(sr.window_hx(raw, fm))

    # ---- per-read statistics: one '+' and one '-' read, control levels over [start - 64, end + 64)
    my_model = my_ts.TomboModel(seq_samp_type=my_th.seqSampleType('DNA', False))
    kmers = sorted(my_model.means.keys())
    std_ref = ts.TomboModel(kmer_ref=[(k, my_model.means[k], my_model.sds[k]) for k in kmers],
                            central_pos=my_model.central_pos,
                            seq_samp_type=th.seqSampleType('DNA', False))
    K, cp = my_model.kmer_width, my_model.central_pos
    cases = [(700, 330, '+'), (9000, 220, '-')]
    out['n_read_cases'] = np.array(len(cases))
    for ci, (start, n, strand) in enumerate(cases):
        minus = strand == '-'
        lag_b, lag_e = (cp, K - cp - 1) if not minus else (K - cp - 1, cp)
        seq = ''.join('ACGT'[c] for c in rng.integers(0, 4, n))     # read-centric bases
        ref_m, ref_s = my_model.get_exp_levels_from_seq(seq, minus)  # genome order, n - K + 1
        z = profile(n - K + 1, -2.5, 1.6, rng) * np.where(rng.random(n - K + 1) < 0.5, -1, 1)
        z[[3, 4, 40]] = 0.0                                          # p == 1 exactly
        gm = np.concatenate([rng.normal(0, 1, lag_b), ref_m + z * ref_s, rng.normal(0, 1, lag_e)])
        gm[[60, 61, n // 2]] = np.nan                                # NaN inside windows
        # control levels: z scores of the same profile shape, shifted along the read
        cs = np.abs(rng.normal(0.3, 0.05, n + 128)) + 0.05
        zc = np.concatenate([np.zeros(64), np.roll(profile(n, -2.5, 1.6, rng), n // 7), np.zeros(64)])
        cm = np.concatenate([rng.normal(0, 1, 64), gm, rng.normal(0, 1, 64)]) - zc * cs
        cm[64 + 10] = gm[10]                                          # p == 1 exactly
        cm[[64 + 90, 64 + 91]] = np.nan
        cs[[64 + 90, 64 + 91]] = np.nan
        rc = gm[::-1].copy() if minus else gm
        fn = 'p%d' % ci
        STORE[fn] = dict(norm_mean=rc, base=np.frombuffer(seq.encode(), dtype='S1'), read_id=fn)
        r_data = th.readData(start=start, end=start + n, filtered=False, read_start_rel_to_raw=0,
                             strand=strand, fn=fn, corr_group='grp', rna=False)
        out.update({'pr%d_means' % ci: rc, 'pr%d_start' % ci: np.array(start),
                    'pr%d_strand' % ci: np.array(strand), 'pr%d_seq' % ci: np.array(seq),
                    'pr%d_cm' % ci: cm, 'pr%d_cs' % ci: cs})
        for fm in FMS:
            tag = 'w%d_fm%d' % (ci, fm)
            pv, ps, _ = ts.compute_sample_compare_read_stats(
                r_data, cm[64 - fm:64 + n + fm], cs[64 - fm:64 + n + fm], fm, None)
            out[tag + '_sc_p'] = pv[ts.SAMP_COMP_TXT]
            out[tag + '_sc_pos'] = ps[ts.SAMP_COMP_TXT]
            pv, ps, _ = ts.compute_de_novo_read_stats(r_data, std_ref, fm, None)
            out[tag + '_dn_p'] = pv[ts.DE_NOVO_TXT]
            out[tag + '_dn_pos'] = ps[ts.DE_NOVO_TXT]
            zz = np.abs(gm[lag_b:n - lag_e] - ref_m) / ref_s
            hx_seen[fm].append(sr.window_hx(sr.z_pvals(zz, 0, 1), fm))

    for fm in FMS:
        h = np.concatenate(hx_seen[fm])
        h = h[~np.isnan(h)]
        print('fm %2d: %4d windows, hx %.1f .. %.1f, %d in [718, 1100], %d fully floored'
              % (fm, h.shape[0], h.min(), h.max(), ((h >= 718) & (h <= 1100)).sum(),
                 (h >= 115.129 * (2 * fm + 1)).sum()))
    path = os.path.join(HERE, 'stats_wide.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

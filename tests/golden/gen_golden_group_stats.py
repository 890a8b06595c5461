"""Golden vectors of the pileup statistics from the REFERENCE (build container only).

    python tests/golden/gen_golden_group_stats.py   # writes tests/golden/stats_group.npz

(The `stats_` prefix keeps the file out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference's compute_group_reg_stats (level_sample_compare, all six test types) and
get_reads_ref (tombo/tombo_stats.py:3627-3673, 4336-4398) on synthetic reads.  The reference loads
`norm_mean` of each read from its FAST5 file and the region sequence from the genome index; here
those two accessors (`th.get_single_slot_read_centric`, `intervalData.add_seq`) are pointed at
in-memory arrays -- everything after them is the reference's own numpy / scipy code.  Only data is
written: the reads, the regions, the genome and the outputs.

Levels are continuous draws, so no level of a sample read equals one of a control read (the U
test's ranks of cross-group ties depend on the reference's unstable argsort).
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import ref_oracle  # noqa: E402
from tombo_amd import tombo_stats as my_ts, tombo_helper as my_th  # noqa: E402

rq, ts, th = ref_oracle.load()
STORE = {}
GENOME = {}
STATS = ['ks_test', 'u_test', 't_test', 'ks_stat_test', 'u_stat_test', 't_stat_test']


def install():
    th.get_single_slot_read_centric = lambda r, name, grp=None: STORE[r.fn][name]
    th.intervalData.add_seq = lambda self, *a, **k: self.update(seq=GENOME['chr1'][self.start:self.end])


def make_reads(rng, spec):
    """spec: (start, length, strand, ctrl, nan_frac) -> reference readData, flat arrays"""
    reads, rows = [], []
    for k, (s, n, strand, ctrl, nan_frac) in enumerate(spec):
        m = rng.normal(0.0, 1.0, n) + 0.3 * np.sin(np.arange(n) * 0.7) + (0.4 if ctrl else 0.0)
        m[rng.random(n) < nan_frac] = np.nan
        fn = 'r%d' % len(STORE)
        STORE[fn] = {'norm_mean': m}
        reads.append(th.readData(s, s + n, False, 0, strand, fn, 'grp', False, 0.0, 10.0, fn))
        rows.append((s, n, strand == '-', ctrl, m))
    return reads, rows


def main():
    install()
    rng = np.random.default_rng(4236)
    GENOME['chr1'] = ''.join(rng.choice(list('ACGT'), 8000))
    g = list(GENOME['chr1'])
    g[1040:1046] = 'NNNNNN'
    GENOME['chr1'] = ''.join(g)
    # regions: (start, end, strand, read spec)
    regs = []
    # A: + strand, reads starting / ending inside, spanning, NaNs, a few '-' reads to skip
    spec = []
    for ctrl in (0, 1):
        for k in range(7):
            s = 960 + int(rng.integers(0, 80))
            spec.append((s, int(rng.integers(60, 200)), '+', ctrl, 0.05))
        spec.append((900, 400, '+', ctrl, 0.0))          # spans the region
        spec.append((1050, 30, '+', ctrl, 0.3))          # inside, many NaNs
        spec.append((980, 100, '-', ctrl, 0.0))          # other strand: skipped
    regs.append((1000, 1100, '+', spec))
    # B: - strand
    spec = []
    for ctrl in (0, 1):
        for k in range(6):
            s = 2950 + int(rng.integers(0, 120))
            spec.append((s, int(rng.integers(40, 160)), '-', ctrl, 0.08))
        spec.append((2990, 20, '-', ctrl, 0.0))          # short, starts inside
        spec.append((2900, 300, '+', ctrl, 0.0))         # other strand
    regs.append((3000, 3080, '-', spec))
    # C: deep pileup (workgroup sort class: > 64 levels per group and position)
    spec = [(5000 - int(rng.integers(0, 10)), 60, '+', ctrl, 0.02) for ctrl in (0, 1) for _ in range(90)]
    regs.append((5010, 5040, '+', spec))
    # D: sparse: coverage hovers around min_test_reads, runs shorter than the window
    spec = [(6000 + 9 * k, 14, '+', ctrl, 0.1) for ctrl in (0, 1) for k in range(12)]
    regs.append((6005, 6100, '+', spec))

    out = {'genome': np.frombuffer(GENOME['chr1'].encode(), dtype=np.uint8)}
    rd_start, rd_len, rd_minus, rd_ctrl, rd_reg, rd_means = [], [], [], [], [], []
    ref_regs, ref_ctrl_regs = [], []
    for ri, (s, e, strand, spec) in enumerate(regs):
        reads, rows = make_reads(rng, spec)
        for (st, n, minus, ctrl, m) in rows:
            rd_start.append(st); rd_len.append(n); rd_minus.append(minus); rd_ctrl.append(ctrl)
            rd_reg.append(ri); rd_means.append(m)
        samp = [r for r, row in zip(reads, rows) if not row[3]]
        ctrl = [r for r, row in zip(reads, rows) if row[3]]
        ref_regs.append(th.intervalData('chr1', s, e, strand, reads=samp))
        ref_ctrl_regs.append(th.intervalData('chr1', s, e, strand, reads=ctrl))
    out.update(reg_start=np.array([r[0] for r in regs]), reg_end=np.array([r[1] for r in regs]),
               reg_minus=np.array([r[2] == '-' for r in regs]),
               rd_start=np.array(rd_start), rd_len=np.array(rd_len), rd_minus=np.array(rd_minus),
               rd_ctrl=np.array(rd_ctrl), rd_reg=np.array(rd_reg), rd_means=np.concatenate(rd_means))
    for st in STATS:
        for fm in (0, 1, 3):
            for mtr in (3, 5):
                for ri in range(len(regs)):
                    res = ts.compute_group_reg_stats(ref_regs[ri], ref_ctrl_regs[ri], fm, mtr, st)
                    key = 'g_%s_fm%d_m%d_r%d' % (st, fm, mtr, ri)
                    out[key + '_n'] = np.array(len(res))
                    if res:
                        gs = res[0][1]
                        out[key + '_stats'] = gs.reg_stats
                        out[key + '_poss'] = gs.reg_poss
                        out[key + '_cov'] = gs.reg_cov
                        out[key + '_ctrl_cov'] = gs.ctrl_cov
    # get_reads_ref over the control reads, with and without the model prior
    my_model = my_ts.TomboModel(seq_samp_type=my_th.seqSampleType('DNA', False))
    kmers = sorted(my_model.means.keys())
    std_ref = ts.TomboModel(kmer_ref=[(k, my_model.means[k], my_model.sds[k]) for k in kmers],
                            central_pos=my_model.central_pos,
                            seq_samp_type=th.seqSampleType('DNA', False))
    for ri in range(len(regs)):
        for fm in (0, 1):
            for est_mean in (False, True):
                for use_ref in (False, True):
                    lm, ls, cov = ts.get_reads_ref(ref_ctrl_regs[ri], 3, fm,
                                                   std_ref if use_ref else None, None, est_mean)
                    key = 'ref_r%d_fm%d_e%d_s%d' % (ri, fm, est_mean, use_ref)
                    out[key + '_means'] = lm
                    out[key + '_sds'] = ls
                    out[key + '_cov_pos'] = np.array(sorted(cov.keys()), dtype=np.int64)
                    out[key + '_cov'] = np.array([cov[k] for k in sorted(cov.keys())], dtype=np.int64)
    path = os.path.join(HERE, 'stats_group.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

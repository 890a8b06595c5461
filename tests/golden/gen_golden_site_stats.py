"""Golden vectors of the per-site modified fractions from the REFERENCE (build container only).

    python tests/golden/gen_golden_site_stats.py   # writes tests/golden/stats_site.npz

(The `stats_` prefix keeps the file out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference's compute_reg_stats (tombo/tombo_stats.py:4180-4229: de_novo,
sample_compare, model_compare), calc_damp_fraction (:2537-2552) and the array expression of
ModelStats._write_stat_block (:2752-2764) on synthetic reads.  The reference loads `norm_mean` /
`base` of each read from its FAST5 file and the region sequence from the genome index; here those
accessors (`h5py.File`, `th.get_multiple_slots_read_centric`, `th.get_single_slot_read_centric`,
`th.get_raw_read_slot`, `intervalData.add_seq`) are pointed at in-memory arrays -- everything after
them is the reference's own code.  Only data is written: the reads, the regions, the genome and the
outputs.  The two alternate-model tables are the ones stats_reads.npz already holds (made up by
gen_golden_stats.py); they are read from there, here and in the tests.

Condition on the inputs: device p-values agree with scipy to 1e-12 relative, so a statistic that
close to a threshold could be counted either way.  Levels are continuous draws, and the generator
asserts that no recorded statistic lies within 1e-9 relative of a threshold; under that condition
every recorded output is exact.
"""
import os
import sys
import json
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
MARGIN = 1e-9
COV_DAMP = {'unmod': 2, 'mod': 0}
MIN_TEST_READS = 3
# (single_read_thresh, lower_thresh) with and without the lower threshold
THRESH = {'de_novo': [(0.5, None), (0.5, 0.15)], 'sample_compare': [(0.5, None), (0.5, 0.15)],
          'model_compare': [(2.0, None), (2.5, -1.5)]}


class FakeFile(object):
    def __init__(self, fn, mode='r'):
        self.fn = fn

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class _Slot(object):
    def __init__(self, rid):
        self.attrs = {'read_id': rid}


class Queue(list):
    put = list.append


def install():
    ts.h5py.File = FakeFile
    th.get_multiple_slots_read_centric = lambda f, names, grp=None: [STORE[f.fn][n] for n in names]
    th.get_single_slot_read_centric = lambda f, name, grp=None: STORE[f.fn][name]
    th.get_raw_read_slot = lambda f: _Slot(STORE[f.fn]['read_id'])
    th.intervalData.add_seq = lambda self, *a, **k: self.update(seq=GENOME['chr1'][self.start:self.end])


def make_reads(rng, model, spec):
    """spec rows (start, length, strand, ctrl, nan_frac, shift) -> reference readData + table rows.
    Levels: the model's level of the read's own k-mers plus continuous noise (plus `shift` on a third
    of the bases, so that fractions spread); NaN with probability nan_frac."""
    K, cp = model.kmer_width, model.central_pos
    reads, rows = [], []
    for (s, n, strand, ctrl, nan_frac, shift) in spec:
        gseq = GENOME['chr1'][s:s + n]
        seq = gseq if strand == '+' else my_th.rev_comp(gseq)
        m = rng.normal(0.0, 0.6, n)
        if n >= K:
            lv, sd = model.get_exp_levels_from_seq(seq)
            m[cp:cp + lv.shape[0]] = lv + rng.normal(0.0, 1.0, lv.shape[0]) * sd * 1.3
        m = m + shift * (rng.random(n) < 0.33)
        m[rng.random(n) < nan_frac] = np.nan
        rid = 'r%d' % len(STORE)
        STORE[rid] = {'norm_mean': m, 'base': np.frombuffer(seq.encode(), dtype='S1'),
                      'read_id': rid.encode()}
        reads.append(th.readData(s, s + n, False, 0, strand, rid, 'grp', False, 0.0, 10.0, rid))
        rows.append((s, n, strand == '-', ctrl, m))
    return reads, rows


def check_margin(stats, thresholds, what):
    stats = np.asarray(stats, dtype=np.float64)
    for t in thresholds:
        if t is None or stats.shape[0] == 0:
            continue
        rel = np.abs(stats - t) / max(abs(t), 1e-300)
        assert rel.min() > MARGIN, '%s: a statistic lies within %g of the threshold %r' % (what, MARGIN, t)


def main():
    install()
    rng = np.random.default_rng(4180)
    my_model = my_ts.TomboModel(seq_samp_type=my_th.seqSampleType('DNA', False))
    kmers = sorted(my_model.means.keys())
    std_ref = ts.TomboModel(kmer_ref=[(k, my_model.means[k], my_model.sds[k]) for k in kmers],
                            central_pos=my_model.central_pos,
                            seq_samp_type=th.seqSampleType('DNA', False))
    reads_gold = np.load(os.path.join(HERE, 'stats_reads.npz'))
    alt_refs = []
    for am in json.loads(str(reads_gold['meta']))['alt_models']:
        tab = reads_gold[am['key']]
        alt_refs.append((am['name'], ts.AltModel(
            kmer_ref=[(r['kmer'].decode(), int(r['pos']), float(r['mean']), float(r['sd'])) for r in tab],
            central_pos=std_ref.central_pos, alt_base=am['alt_base'], name=am['name'],
            motif=th.TomboMotif(am['motif'], am['mod_pos']))))

    g = ''.join(rng.choice(list('ACGT'), 9000))
    g = g[:6900] + g[6900:7300].replace('GATC', 'GTTC') + g[7300:]   # region E: no GATC hit
    GENOME['chr1'] = g
    regs = []   # (start, end, strand, read spec)
    # A: + strand; reads starting / ending inside, spanning, NaN levels, one on the other strand;
    # a control read with NaN levels inside
    spec = []
    for ctrl in (0, 1):
        for k in range(7):
            spec.append((960 + int(rng.integers(0, 80)), int(rng.integers(60, 200)), '+', ctrl, 0.04, 1.5))
        spec.append((900, 400, '+', ctrl, 0.0, 1.0))
        spec.append((1050, 30, '+', ctrl, 0.3, 0.0))
        spec.append((980, 100, '-', ctrl, 0.0, 0.0))
    regs.append((1000, 1100, '+', spec))
    # B: - strand
    spec = []
    for ctrl in (0, 1):
        for k in range(6):
            spec.append((2950 + int(rng.integers(0, 120)), int(rng.integers(40, 160)), '-', ctrl, 0.06, -1.2))
        spec.append((2990, 20, '-', ctrl, 0.0, 0.0))
        spec.append((2900, 300, '+', ctrl, 0.0, 0.0))
    regs.append((3000, 3080, '-', spec))
    # C: deep pileup (more than 64 reads on a position)
    spec = [(5000 - int(rng.integers(0, 10)), 60, '+', 0, 0.02, 1.4) for _ in range(80)] + \
           [(4995, 70, '+', 1, 0.02, 0.0) for _ in range(12)]
    regs.append((5010, 5030, '+', spec))
    # D: every read fails (shorter than a k-mer, no level)
    spec = [(6050 + k, 2, '+', ctrl, 1.0, 0.0) for ctrl in (0, 1) for k in range(4)]
    regs.append((6040, 6080, '+', spec))
    # E: no GATC in reach: model_compare fails the whole region on its second alternate model
    spec = [(6990 + 5 * k, 90, '+', ctrl, 0.03, 1.0) for ctrl in (0, 1) for k in range(6)]
    regs.append((7020, 7080, '+', spec))

    out = {'genome': np.frombuffer(GENOME['chr1'].encode(), dtype=np.uint8)}
    rd_start, rd_len, rd_minus, rd_ctrl, rd_reg, rd_means = [], [], [], [], [], []
    ref_regs, ref_ctrl_regs = [], []
    for ri, (s, e, strand, spec) in enumerate(regs):
        reads, rows = make_reads(rng, my_model, spec)
        for (st, n, minus, ctrl, m) in rows:
            rd_start.append(st); rd_len.append(n); rd_minus.append(minus); rd_ctrl.append(ctrl)
            rd_reg.append(ri); rd_means.append(m)
        ref_regs.append(th.intervalData('chr1', s, e, strand, reads=[r for r, row in zip(reads, rows) if not row[3]]))
        ref_ctrl_regs.append(th.intervalData('chr1', s, e, strand, reads=[r for r, row in zip(reads, rows) if row[3]]))
    out.update(reg_start=np.array([r[0] for r in regs]), reg_end=np.array([r[1] for r in regs]),
               reg_minus=np.array([r[2] == '-' for r in regs]),
               rd_start=np.array(rd_start), rd_len=np.array(rd_len), rd_minus=np.array(rd_minus),
               rd_ctrl=np.array(rd_ctrl), rd_reg=np.array(rd_reg), rd_means=np.concatenate(rd_means))

    cases, errs, n_checked = [], set(), 0
    for stat_type in ('de_novo', 'sample_compare', 'model_compare'):
        fms = (0,) if stat_type == 'model_compare' else (0, 1, 3)
        use_refs = (0, 1) if stat_type == 'sample_compare' else (1,)
        for fm in fms:
            for li, (single, lower) in enumerate(THRESH[stat_type]):
                for use_ref in use_refs:
                    cases.append(dict(stat_type=stat_type, fm=fm, li=li, single=single, lower=lower,
                                      use_ref=use_ref))
                    for ri in range(len(regs)):
                        key = '%s_fm%d_l%d_s%d_r%d' % (stat_type, fm, li, use_ref, ri)
                        q = Queue()
                        keep_pr = li == 0 and use_ref == 1 and fm < 3
                        try:
                            res = ts.compute_reg_stats(
                                ref_regs[ri], fm, MIN_TEST_READS, single, lower, ref_ctrl_regs[ri],
                                std_ref if use_ref else None, alt_refs, False, q, stat_type, None)
                            err = ''
                        except th.TomboError as e:
                            res, err = [], str(e)
                        errs.add(err)
                        out[key + '_err'] = np.array(err)
                        out[key + '_names'] = np.array([n for n, _ in res], dtype='U')
                        # every statistic the reference collated (the blocks are put before a
                        # region can fail): the margin condition, and the per-read golden blocks
                        # (they do not depend on the thresholds: kept for the first pair, fm_offset 0 and 1)
                        for k, (name, (blk, lookup, chrm, strand, start)) in enumerate(q):
                            thr = (single, lower) if stat_type != 'model_compare' else \
                                ((single, lower) if lower is not None else (single, -single))
                            check_margin(blk['stat'], thr, key)
                            n_checked += blk.shape[0]
                            if keep_pr:
                                inv = dict((v, int(rid[1:])) for rid, v in lookup.items())
                                out['%s_pr%d_name' % (key, k)] = np.array(name)
                                out['%s_pr%d_pos' % (key, k)] = blk['pos'].astype(np.uint32)
                                out['%s_pr%d_stat' % (key, k)] = blk['stat']
                                out['%s_pr%d_read' % (key, k)] = np.array(
                                    [inv[v] for v in blk['read_id']], dtype=np.uint16)
                        out[key + '_npr'] = np.array(len(q) if keep_pr else -1)
                        for k, (name, rs) in enumerate(res):
                            damp = ts.calc_damp_fraction(COV_DAMP, rs.reg_frac_standard_base, rs.valid_cov)
                            blk = np.array(
                                [p for p in zip(damp, rs.reg_frac_standard_base, rs.reg_poss, rs.reg_cov,
                                                rs.ctrl_cov, rs.valid_cov) if not np.isnan(p[0])],
                                dtype=[(str('damp_frac'), 'f8'), (str('frac'), 'f8'), (str('pos'), 'u4'),
                                       (str('cov'), 'u4'), (str('control_cov'), 'u4'), (str('valid_cov'), 'u4')])
                            p = '%s_n%d_' % (key, k)
                            out[p + 'frac'] = rs.reg_frac_standard_base
                            out[p + 'poss'] = np.asarray(rs.reg_poss, dtype=np.int32)
                            out[p + 'cov'] = np.asarray(rs.reg_cov, dtype=np.int32)
                            out[p + 'ctrl_cov'] = np.asarray(rs.ctrl_cov, dtype=np.int32)
                            out[p + 'valid_cov'] = np.asarray(rs.valid_cov, dtype=np.int32)
                            out[p + 'damp'] = damp
                            out[p + 'block'] = blk
                            assert (rs.chrm, rs.strand, rs.start) == ('chr1', regs[ri][2], regs[ri][0])
    out['meta'] = np.array(json.dumps(dict(
        cases=cases, cov_damp_counts=COV_DAMP, min_test_reads=MIN_TEST_READS, margin=MARGIN,
        alt_tables_from='stats_reads.npz')))
    path = os.path.join(HERE, 'stats_site.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays;', n_checked,
          'statistics checked against the threshold margin')
    print('errors seen:', sorted(errs))


if __name__ == '__main__':
    main()

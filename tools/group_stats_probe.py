"""Throughput of the pileup statistics (level_sample_compare, csrc/k_group.h) on a synthetic genome.

    timeout -k 10 600 python tools/group_stats_probe.py [--regions 1000] [--batch 100] [--out F]

Workload: regions of 10 000 bases on '+', each with 50 sample + 50 control reads of 10 kb per
strand (the '-' reads are skipped by the strand filter), levels N(0, 1) (+0.2 for the control),
2 % NaN.  Per test type: positions/s of compute_group_reg_stats_batch over all regions (wall
time of the engine calls, host packing included and reported apart), and the time of a
single-core numpy restatement of the reference's per-position loop on a few regions, scaled up.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/group_stats_probe.py` for the
kernel split.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from tombo_amd import tombo_stats as ts, tombo_helper as th  # noqa: E402

REG_LEN, READ_LEN, DEPTH = 10000, 10000, 50


def make_regions(n, rng):
    samp, ctrl = [], []
    for r in range(n):
        start = 1_000_000 + r * REG_LEN
        groups = []
        for g in (0, 1):
            reads = []
            for strand in ('+', '-'):
                for k in range(DEPTH):
                    s = start - int(rng.integers(0, READ_LEN - REG_LEN + 1)) if READ_LEN > REG_LEN else start
                    m = rng.normal(0.2 * g, 1.0, READ_LEN)
                    m[rng.random(READ_LEN) < 0.02] = np.nan
                    reads.append(th.resquiggledRead(s, s + READ_LEN, False, 0, strand, None, None,
                                                    False, read_id='r', means=m))
            groups.append(th.regionData('c', '+', start, start + REG_LEN, reads))
        samp.append(groups[0])
        ctrl.append(groups[1])
    return samp, ctrl


def numpy_loop(samp, ctrl, stat_type, fm, mtr):
    """the reference's per-position loop (np.sort / searchsorted / argsort / scipy per position),
    restated in numpy: sample and control levels of one region as columns"""
    from scipy import stats as sps

    def levels(reg):
        cols = []
        for rd in reg.reads:
            if rd.strand != reg.strand:
                continue
            col = np.full(reg.end - reg.start + 2 * fm, np.nan)
            lo = max(rd.start, reg.start - fm)
            hi = min(rd.end, reg.end + fm)
            col[lo - (reg.start - fm):hi - (reg.start - fm)] = rd.means[lo - rd.start:hi - rd.start]
            cols.append(col)
        return np.column_stack(cols)

    t0 = time.perf_counter()
    S, C = levels(samp), levels(ctrl)
    out = []
    for i in range(S.shape[0]):
        s, c = np.sort(S[i][~np.isnan(S[i])]), np.sort(C[i][~np.isnan(C[i])])
        if s.shape[0] < mtr or c.shape[0] < mtr:
            continue
        ns, nc = s.shape[0], c.shape[0]
        al = np.concatenate([s, c])
        if stat_type == ts.KS_TEST_TXT:
            d = np.max(np.abs(np.searchsorted(s, al, side='right') / ns -
                              np.searchsorted(c, al, side='right') / nc))
            en = np.sqrt(ns * nc / float(ns + nc))
            out.append(sps.distributions.kstwobign.sf((en + 0.12 + 0.11 / en) * d))
        elif stat_type == ts.U_TEST_TXT:
            ranks = np.empty(ns + nc, int)
            ranks[al.argsort()] = np.arange(1, ns + nc + 1)
            u1 = ranks[:ns].sum() - (ns * (ns + 1)) / 2
            u = min(u1, ns * nc - u1)
            out.append(sps.norm.cdf((u - ns * nc / 2) / np.sqrt(ns * nc * (ns * nc + 1) / 12)) * 2)
        else:
            sm, ssd, cm, csd = s.mean(), s.std(), c.mean(), c.std()
            sp = np.sqrt((((ns - 1) * ssd ** 2) + (nc - 1) * csd ** 2) / (ns + nc - 2))
            t = -np.abs(sm - cm) / (sp * np.sqrt(1 / ns + 1 / nc))
            out.append(sps.t.cdf(t, ns + nc - 2) * 2)
    return time.perf_counter() - t0, S.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--fm', type=int, default=1)
    ap.add_argument('--min-test-reads', type=int, default=40)
    ap.add_argument('--numpy-regions', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    samp, ctrl = make_regions(a.batch, rng)   # one batch of regions, run regions / batch times
    n_batches = max(1, a.regions // a.batch)
    from tombo_amd import resquiggle as rq
    rq.get_engine()
    ts.compute_group_reg_stats_batch(samp[:2], ctrl[:2], a.fm, a.min_test_reads, ts.KS_TEST_TXT)  # warm-up
    res = {'regions': n_batches * a.batch, 'region_bases': REG_LEN, 'reads_per_group_and_strand': DEPTH,
           'read_len': READ_LEN, 'fm_offset': a.fm, 'min_test_reads': a.min_test_reads, 'types': {}}
    for st in (ts.KS_TEST_TXT, ts.U_TEST_TXT, ts.T_TEST_TXT, ts.KS_STAT_TEST_TXT):
        t0 = time.perf_counter()
        n_pos = 0
        for _ in range(n_batches):
            out = ts.compute_group_reg_stats_batch(samp, ctrl, a.fm, a.min_test_reads, st)
            n_pos += sum(len(o[0][1].reg_poss) for o in out if o)
        wall = time.perf_counter() - t0
        ent = {'positions': n_pos, 'wall_s': wall, 'positions_per_s': n_pos / wall}
        if st != ts.KS_STAT_TEST_TXT and a.numpy_regions > 0:
            tn, npos = 0.0, 0
            for k in range(a.numpy_regions):
                dt, n = numpy_loop(samp[k], ctrl[k], st, a.fm, a.min_test_reads)
                tn += dt
                npos += n
            ent['numpy_single_core_s_per_position'] = tn / npos
            ent['numpy_single_core_s_scaled'] = tn / npos * n_pos
        res['types'][st] = ent
        print(st, json.dumps(ent), flush=True)
    # host side alone: packing the CSR inputs of one batch
    t0 = time.perf_counter()
    ts._pileup_inputs(samp, [samp, ctrl], a.fm)
    res['host_pack_s_per_batch'] = time.perf_counter() - t0
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as fp:
            json.dump(res, fp, indent=1)


if __name__ == '__main__':
    main()

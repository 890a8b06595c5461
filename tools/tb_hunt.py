"""The chunk-parallel traceback under repetition: one resident batch run K times; read_tb, status, tb_form and the
verifier's count of every run against run 0 (round-6 fault hunt; profiles/r06_traceback_rootcause.txt).

    TBA_LIB_PATH=<build> python tools/tb_hunt.py [--rna] [--reads N] [--bases B] [--runs K]

One line per run that differs, and a summary
    HUNT <tag> <DNA|RNA> runs K DISTINCT_RESULTS D (minority runs M) bad_reads .. verify_fail_rows_per_run [..]
(D = 1: every run gave the same bytes)."""
import os
import sys
import argparse
import collections
import zlib
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=10000)
    ap.add_argument('--bases', type=int, default=3000)
    ap.add_argument('--bandwidth', type=int, default=500)
    ap.add_argument('--rna', action='store_true')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--tag', default=os.path.basename(os.environ.get('TBA_LIB_PATH', 'tree')))
    a = ap.parse_args()
    from tombo_amd import _native as N, tombo_stats as ts, tombo_helper as th
    from tombo_amd._default_parameters import SIG_MATCH_THRESH, STALL_PARAMS
    sn = 'RNA' if a.rna else 'DNA'
    samp = th.seqSampleType(sn, a.rna)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)._replace(bandwidth=a.bandwidth)
    bases = np.full(a.reads, a.bases, np.int64)
    seqs, raws, _ = bench.make_reads(bases, 1000003, min(32, os.cpu_count() or 8), sn, False)
    rng = np.random.RandomState(1)
    si = np.stack([rng.choice(a.bases, 1000, replace=False) for _ in range(a.reads)]) if a.bases > 1000 else None
    eng = N.Engine(0)
    eng.set_model(model.level_means, model.level_sds, model.kmer_width, model.central_pos)
    eng.upload(N.make_params(params),
               N.make_opts(outlier_thresh=5.0, sig_match_thresh=SIG_MATCH_THRESH[sn],
                           stall_params=th.stallParams(**STALL_PARAMS) if a.rna else None),
               raws, [ts.encode_seq(q) for q in seqs], samp_ind=si)
    off = np.asarray(eng.seg_off)

    def read_of(pos):
        return np.unique(np.searchsorted(off, pos, side='right') - 1)

    digests, vfail, bad_reads = [], [], set()
    for k in range(a.runs):
        eng.run()
        tb = eng.get(N.GET_READ_TB)
        st = eng.get(N.GET_STATUS)
        fm = eng.get(N.GET_TB_FORM)
        vf = eng.get(N.GET_TB_VERIFY_FAIL)
        vfail.append(int(vf.sum()))
        if vf.any():
            w = np.flatnonzero(vf)
            print('run %d: the verifier disagreed on %d rows of reads %s (wavefronts %s); their tb_form now %s' % (
                k, vfail[-1], w[:12].tolist(), sorted(set((w // 4).tolist()))[:6], fm[w[:12]].tolist()), flush=True)
        digests.append(zlib.crc32(tb.tobytes()) ^ zlib.crc32(st.tobytes()))
        if k == 0:
            tb0, st0, fm0 = tb, st, fm
            continue
        d = np.flatnonzero(tb != tb0)
        ds = np.flatnonzero(st != st0)
        df = np.flatnonzero(fm != fm0)
        if d.size or ds.size or df.size:
            rd = read_of(d)
            bad_reads.update(rd.tolist())
            print('run %d: read_tb differs from run 0 at %d entries of reads %s (wavefronts %s); status differs %s; tb_form differs %s' % (
                k, d.size, rd[:16].tolist(), sorted(set((rd // 4).tolist()))[:8], ds[:8].tolist(),
                [(int(i), int(fm0[i]), int(fm[i])) for i in df[:8]]), flush=True)
    cnt = collections.Counter(digests)
    print('HUNT %s %s runs %d DISTINCT_RESULTS %d (minority runs %d) bad_reads %d %s forms %s ok %d verify_fail_rows_per_run %s' % (
        a.tag, sn, a.runs, len(cnt), a.runs - max(cnt.values()), len(bad_reads), sorted(bad_reads)[:12],
        dict(collections.Counter(fm0.tolist())), int((st0 == 0).sum()), vfail), flush=True)


if __name__ == '__main__':
    main()

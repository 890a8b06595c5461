"""K-mer level distributions (`tombo plot kmer`): Engine.kmer_dist (csrc/k_kmer_dist.h) against the numpy restatement,
on the same box.

    python tools/kmer_dist_timing.py [--out profiles/kmer_dist_timing.json]

The job is the plot's own size: 100 synthetic reads of 10 000 bases (uniform random bases, full-mantissa levels), all
taken (kmer_thresh 1 at K = 4: every read shows all 256 4-mers; kmer_thresh 0 at K = 6), for K = 4 and K = 6 and both
forms (per-read means / every level).  The GPU step runs in a child process under its own `timeout`.  In that ONE
process, after a warm-up call per configuration, five rounds, host clock:
  (a) engine: Engine.kmer_dist, the count call and the fill call with their uploads and downloads; the time of the
      kernels alone comes from the hipEvents inside the entry (`last_kmer_dist_kernel_ms`);
  (b) numpy: tests/kmer_dist_reference.kmer_dist on the same arrays.
The outputs are compared bit for bit before anything is timed.  Needs a GPU: there is no fallback.  Reads nothing but
this repository."""
import os
import sys
import json
import time
import argparse
import subprocess
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CONFIGS = [(4, 1, 1, True), (4, 1, 1, False), (6, 2, 0, True), (6, 2, 0, False)]   # K, central_pos, kmer_thresh, read_mean


def spread(ts_):
    return dict(median=float(np.median(ts_)), min=float(min(ts_)), max=float(max(ts_)), all=[float(t) for t in ts_])


def same(got, want):
    return all((g == w) if not isinstance(w, np.ndarray) else
               (g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()) for g, w in zip(got, want))


def child(a):
    import kmer_dist_reference as kr
    from tombo_amd import resquiggle as rq
    eng = rq.get_engine()   # raises without a GPU
    rng = np.random.default_rng(41)
    means = rng.standard_normal(a.reads * a.bases) * 1.3 + rng.random(a.reads * a.bases) * 1e-3
    codes = rng.integers(0, 4, a.reads * a.bases).astype(np.uint8)
    off = np.arange(a.reads + 1, dtype=np.int64) * a.bases
    results, equal = [], True
    for K, cp, thresh, read_mean in CONFIGS:
        args = (means, codes, off, K, cp, thresh, a.reads, read_mean)
        got, want = eng.kmer_dist(*args), kr.kmer_dist(*args)     # warm-up and the comparison
        ok = bool(same(got, want))
        equal = equal and ok
        wall, kern, numpy_s = [], [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter(); eng.kmer_dist(*args); t1 = time.perf_counter()
            kern.append(eng.last_kmer_dist_kernel_ms)
            kr.kmer_dist(*args); t2 = time.perf_counter()
            wall.append((t1 - t0) * 1e3)
            numpy_s.append(t2 - t1)
        results.append(dict(
            kmer_width=K, central_pos=cp, kmer_thresh=thresh, read_mean=read_mean, reads_taken=int(got[1]),
            values=int(got[4][-1]), kmers_with_entries=int(np.count_nonzero(got[3])), outputs_equal=ok,
            engine_kernel_ms=spread(kern), engine_end_to_end_ms=spread(wall), numpy_restatement_s=spread(numpy_s),
            numpy_over_engine_end_to_end=float(np.median(numpy_s) * 1e3 / np.median(wall))))
    out = dict(
        what='tombo plot kmer numbers of %d reads x %d bases' % (a.reads, a.bases), reads=a.reads, bases_per_read=a.bases,
        rounds=a.rounds, outputs_equal=equal, configurations=results,
        engine_end_to_end_what='Engine.kmer_dist: argument checks, the count call and the fill call of tba_kmer_dist, '
                               'each with upload, kernels, download',
        engine_kernel_what='hipEvent time of the kernels of both calls',
        numpy_what='tests/kmer_dist_reference.kmer_dist on the same arrays, same process, same box (numpy per read, a '
                   'Python loop over the (k-mer, read) segments)')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
    if not equal:
        sys.exit('engine and numpy differ')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmer_dist_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reads', type=int, default=100)
    ap.add_argument('--bases', type=int, default=10000)
    ap.add_argument('--timeout', type=int, default=420, help='seconds the GPU step may take')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child', '--out', a.out,
           '--rounds', str(a.rounds), '--reads', str(a.reads), '--bases', str(a.bases)]
    sys.exit(subprocess.call(cmd))


if __name__ == '__main__':
    main()

"""K-mer model estimation: `ts.extract_kmer_levels` + `ts.tabulate_kmer_levels` on the device against the numpy
restatement of the reference (tests/kmer_est_reference.py) on the same machine.

    python tools/kmer_est_timing.py [--out profiles/kmer_est_timing.json]

Input: a 6-mer model (upstrm 2, dnstrm 3) from synthetic reads of 5 kb at 30x on each strand of a 1 Mb chromosome,
regions of 10 kb, cov_thresh 10, medians (est_mean off), no subsampling.  After --warmup runs of the device route,
the median of --rounds device runs and of --numpy-rounds runs of the restatement, in ONE process.  The device
route is split into
  engine_s   the region_key_levels / segment_medians / coverage calls: copies to the device, kernels, copies back,
  host_s     the rest: overlap lists, region sequences, k-mer codes, entries, the concatenation per key.
The parent commit has no route of its own, so the restatement -- the reference's loop per position, in numpy --
is the yardstick.  Host clock around calls that end in a synchronise.  Single-threaded numpy; nothing here starts
threads.  Needs a GPU: there is no fallback."""
import os
import sys
import json
import time
import argparse
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from tombo_amd import tombo_helper as th, tombo_stats as ts, resquiggle as rq  # noqa: E402
import kmer_est_reference as kr  # noqa: E402

UP, DN = 2, 3


class Timed(object):
    """the engine with the time spent inside its calls added up"""

    def __init__(self, eng):
        self.eng, self.seconds, self.by_call = eng, 0.0, {}

    def __getattr__(self, name):
        fn = getattr(self.eng, name)
        if not callable(fn):
            return fn

        def call(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                dt = time.perf_counter() - t0
                self.seconds += dt
                self.by_call[name] = self.by_call.get(name, 0.0) + dt
        return call


def make_reads(rng, chrm_len, read_len, cov):
    genome = ''.join(rng.choice(list('ACGT'), chrm_len))
    comp = th.rev_comp(genome)    # comp[chrm_len - e:chrm_len - s] is the minus-strand read over [s, e)
    pool = rng.normal(size=1 << 22)
    index = {}
    for strand in '+-':
        n = cov * chrm_len // read_len
        starts = rng.integers(0, chrm_len - read_len + 1, n)
        at = rng.integers(0, (1 << 22) - read_len, n)
        index[('chr1', strand)] = [th.resquiggledRead(
            int(s), int(s) + read_len, False, 0, strand, None, None, False, read_id='%s%d' % (strand, i),
            means=pool[a:a + read_len],
            seq=genome[s:s + read_len] if strand == '+' else comp[chrm_len - s - read_len:chrm_len - s])
            for i, (s, a) in enumerate(zip(starts.tolist(), at.tolist()))]
    return index


def device_route(index, a):
    eng = Timed(rq.get_engine())
    t0 = time.perf_counter()
    table = ts.extract_kmer_levels(index, a.region_size, a.cov_thresh, UP, DN, None, engine=eng)
    t1 = time.perf_counter()
    rows = ts.tabulate_kmer_levels(table, 1, engine=eng)
    t2 = time.perf_counter()
    return (table, rows), dict(total_s=t2 - t0, extract_s=t1 - t0, tabulate_s=t2 - t1, engine_s=eng.seconds,
                               host_s=t2 - t0 - eng.seconds, **dict(('call_' + k, v) for k, v in eng.by_call.items()))


def numpy_route(index, a):
    t0 = time.perf_counter()
    regs = list(th.iter_cov_regs(index, a.cov_thresh, a.region_size))
    all_regs = kr.extract(index, regs, a.region_size, a.cov_thresh, UP, DN, None)
    keys = kr.all_kmers(UP + DN + 1)
    off, lv, sd = kr.table(*kr.flatten(all_regs, keys))
    res = (off, lv, sd, kr.medians(lv, off), kr.medians(sd, off))
    return res, time.perf_counter() - t0


def med(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), all=[float(x) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmer_est_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--numpy-rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--chrm-len', type=int, default=1000000)
    ap.add_argument('--read-len', type=int, default=5000)
    ap.add_argument('--coverage', type=int, default=30)
    ap.add_argument('--region-size', type=int, default=10000)
    ap.add_argument('--cov-thresh', type=int, default=10)
    a = ap.parse_args()
    rq.get_engine()   # raises without a GPU
    index = make_reads(np.random.default_rng(1716), a.chrm_len, a.read_len, a.coverage)
    for _ in range(max(a.warmup, 1)):              # warm-up: the engine's buffers and the allocator settle
        (table, rows), _ = device_route(index, a)
    print('device warm-up done: %d pairs under %d keys' % (table.levels.shape[0], len(table.keys)), flush=True)
    dev, host, want = [], [], None
    for i in range(max(a.rounds, a.numpy_rounds)):
        if i < a.rounds:
            dev.append(device_route(index, a)[1])
        if i < a.numpy_rounds:
            want, dt = numpy_route(index, a)
            host.append(dt)
        print('round %d done' % i, flush=True)
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    got_tab = np.array([r[1:] for r in rows], dtype=np.float64)
    equal = np.array_equal(table.off, want[0]) and np.array_equal(bits(table.levels), bits(want[1])) and \
        np.array_equal(bits(table.sds), bits(want[2])) and np.array_equal(bits(got_tab[:, 0]), bits(want[3])) and \
        np.array_equal(bits(got_tab[:, 1]), bits(want[4]))
    n_levels = sum(len(rd.means) for rds in index.values() for rd in rds)
    res = dict(
        what='k-mer model estimation: %d-mer, reads of %d bases at %dx on both strands of a %d-position chromosome, '
             'regions of %d, cov_thresh %d' % (UP + DN + 1, a.read_len, a.coverage, a.chrm_len, a.region_size, a.cov_thresh),
        rounds=a.rounds, numpy_rounds=a.numpy_rounds, warmup=a.warmup, outputs_equal=bool(equal), levels=int(n_levels),
        pairs=int(table.levels.shape[0]), regions=int(table.n_regions),
        device=dict((k, med([d[k] for d in dev])) for k in sorted(dev[0])),
        numpy_restatement_s=med(host),
        device_faster_than_numpy=bool(np.median([d['total_s'] for d in dev]) < np.median(host)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
    print(json.dumps(res))
    if not equal:
        sys.exit('the device and the restatement differ')


if __name__ == '__main__':
    main()

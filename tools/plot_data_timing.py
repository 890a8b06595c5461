"""Region plot data: the three engine calls of csrc/k_plot.h against the numpy restatement, on the same box.

    python tools/plot_data_timing.py [--out profiles/plot_data_timing.json]

The job: 200 regions of 21 bases with 100 reads each (both strands, reads that hang over either end, full-mantissa
levels), about 10 raw samples per base.  In ONE process, after a warm-up, five rounds, host clock:
  (a) engine: Engine.region_level_piles (piles, five linear and twelve nearest percentiles), Engine.segment_percentiles
      on those piles, Engine.region_raw_signal of every (read, region) pair -- each with its upload and download; the
      time of the kernels alone comes from the hipEvents inside the entries (`last_plot_kernel_ms`);
  (b) numpy: tests/plot_reference.py (level_piles, segment_percentiles, raw_signal) on the same arrays.
The outputs are compared bit for bit before anything is timed.  Needs a GPU: there is no fallback.  Reads nothing but
this repository."""
import os
import sys
import json
import time
import argparse
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import plot_reference as ref  # noqa: E402
from tombo_amd import resquiggle as rq  # noqa: E402

Q_LIN = np.true_divide([0, 25, 50, 75, 100], 100)
Q_NEAR = np.true_divide([1, 10, 20, 30, 40, 49, 99, 90, 80, 70, 60, 51], 100)


def spread(ts_):
    return dict(median=float(np.median(ts_)), min=float(min(ts_)), max=float(max(ts_)), all=[float(t) for t in ts_])


def make_job(rng, n_regions, n_bases, n_reads, samples):
    csr = (lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64))
    rs, rm, means, segs, raws, rsr, st, en = [], [], [], [], [], [], [], []
    for r in range(n_regions):
        start = 1000 + 100 * r
        st.append(start)
        en.append(start + n_bases)
        for _ in range(n_reads):
            a = start + int(rng.integers(-n_bases + 1, n_bases // 2))
            n = int(rng.integers(n_bases, 2 * n_bases + 1))
            s = np.concatenate([[0], np.cumsum(rng.integers(2, 2 * samples - 1, n))]).astype(np.int64)
            rs.append(a)
            rm.append(rng.random() < 0.5)
            means.append(ref.full_mantissa(rng, n))
            segs.append(s)
            rsr.append(int(rng.integers(0, 50)))
            raws.append(rng.integers(200, 900, rsr[-1] + int(s[-1])).astype(np.int16))
    n = len(rs)
    roff = np.arange(n_regions + 1, dtype=np.int64) * n_reads
    piles = (np.array(rs, dtype=np.int64), np.array(rm, dtype=np.uint8), csr(means), np.concatenate(means), roff,
             np.arange(n, dtype=np.int64), np.array(st, dtype=np.int64), np.array(en, dtype=np.int64))
    pair_reg = np.repeat(np.arange(n_regions), n_reads)
    signal = (np.concatenate(raws), csr(raws), np.concatenate(segs), csr(segs), piles[0], np.array(rsr, dtype=np.int64),
              piles[1], np.zeros(n, dtype=np.uint8), 500 + rng.standard_normal(n), 80 + rng.random(n), np.full(n, -2.5),
              np.full(n, 2.5), np.arange(n, dtype=np.int64), piles[6][pair_reg], piles[7][pair_reg])
    return piles, signal


def same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint64) if np.asarray(g).dtype.kind == 'f' else g,
                              np.asarray(w).view(np.uint64) if np.asarray(w).dtype.kind == 'f' else w)
               for g, w in zip(got, want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plot_data_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--regions', type=int, default=200)
    ap.add_argument('--bases', type=int, default=21)
    ap.add_argument('--reads', type=int, default=100)
    ap.add_argument('--samples', type=int, default=10)
    a = ap.parse_args()
    eng = rq.get_engine()   # raises without a GPU
    piles, signal = make_job(np.random.default_rng(31), a.regions, a.bases, a.reads, a.samples)
    # warm-up and the comparison
    got_p = eng.region_level_piles(*piles, q_linear=Q_LIN, q_nearest=Q_NEAR)
    pile_off, levels = ref.level_piles(*piles)
    want_q = ref.segment_percentiles(levels, pile_off, Q_LIN, Q_NEAR)
    got_q = eng.segment_percentiles(levels, pile_off, Q_LIN, Q_NEAR)
    got_s = eng.region_raw_signal(*signal)
    equal = bool(same(got_p, (pile_off, levels) + want_q) and same(got_q, want_q) and same(got_s, ref.raw_signal(*signal)))
    names = ('region_level_piles', 'segment_percentiles', 'region_raw_signal')
    wall, kern, numpy_s = dict((n, []) for n in names), dict((n, []) for n in names), dict((n, []) for n in names)
    calls = (lambda: eng.region_level_piles(*piles, q_linear=Q_LIN, q_nearest=Q_NEAR),
             lambda: eng.segment_percentiles(levels, pile_off, Q_LIN, Q_NEAR), lambda: eng.region_raw_signal(*signal))
    refs = (lambda: ref.segment_percentiles(*ref.level_piles(*piles)[::-1], Q_LIN, Q_NEAR),
            lambda: ref.segment_percentiles(levels, pile_off, Q_LIN, Q_NEAR), lambda: ref.raw_signal(*signal))
    for _ in range(a.rounds):
        for name, call, restated in zip(names, calls, refs):
            t0 = time.perf_counter(); call(); t1 = time.perf_counter()
            kern[name].append(eng.last_plot_kernel_ms)
            restated(); t2 = time.perf_counter()
            wall[name].append((t1 - t0) * 1e3)
            numpy_s[name].append(t2 - t1)
    out = dict(
        what='plot data of %d regions x %d bases x %d reads, about %d raw samples per base' % (
            a.regions, a.bases, a.reads, a.samples),
        regions=a.regions, bases=a.bases, reads_per_region=a.reads, samples_per_base=a.samples, rounds=a.rounds,
        positions=int(pile_off.shape[0] - 1), piled_levels=int(levels.shape[0]), linear_fractions=int(Q_LIN.shape[0]),
        nearest_fractions=int(Q_NEAR.shape[0]), pairs=int(signal[12].shape[0]), raw_samples_in=int(signal[0].shape[0]),
        signal_samples_out=int(got_s[0][-1]), outputs_equal=equal,
        engine_kernel_ms=dict((n, spread(kern[n])) for n in names),
        engine_end_to_end_ms=dict((n, spread(wall[n])) for n in names),
        engine_end_to_end_what='the Engine method: argument checks, upload, kernels, download',
        numpy_restatement_s=dict((n, spread(numpy_s[n])) for n in names),
        numpy_what='tests/plot_reference.py on the same arrays, same process, same box (Python loops over regions, reads '
                   'and bases, as the reference has them)',
        numpy_over_engine_end_to_end=dict((n, float(np.median(numpy_s[n]) * 1e3 / np.median(wall[n]))) for n in names))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
    if not equal:
        sys.exit('engine and numpy differ')


if __name__ == '__main__':
    main()

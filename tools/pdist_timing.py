"""Pairwise distances between the most significant regions: the engine's kernel and call against numpy.

    python tools/pdist_timing.py [--out profiles/pdist_timing.json]

The job of `tombo plot cluster_most_significant`: 2000 regions, num_bases 21, slide_span 3, so 2000 signal-difference
profiles of 27 values (full-mantissa random doubles), 2 001 000 pairs of 49 window pairs each.  In ONE process, after
a warm-up, five rounds, host clock:
  (a) engine: tombo_stats.get_pairwise_dists -- one Engine.pairwise_window_dists call with the upload of the rows and
      the download of the 2000 x 2000 matrix; the time of the kernel alone comes from the hipEvents inside the entry;
  (b) numpy, on a SUBSAMPLE of the rows only, then SCALED to the full job by the ratio of the pair counts (the work
      is the same for every pair): the reference's own statements pair by pair (tests/pdist_reference.py
      window_dists_loops, what each worker process of the reference runs) on the first 96 rows, and the vectorised
      restatement (window_dists) on the first 256.
The engine's rows for both subsamples are compared bit for bit with numpy's before anything is timed; the order_reads
metric (Engine.pairwise_nanmean_dists) is timed the same way on 2000 reads of 27 positions with a fifth of the values
NaN.  Needs a GPU: there is no fallback.  Reads nothing but this repository."""
import os
import sys
import json
import time
import argparse
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pdist_reference as ref  # noqa: E402
from tombo_amd import resquiggle as rq, tombo_stats as ts  # noqa: E402


def pairs(n):
    return n * (n + 1) // 2


def spread(ts_):
    return dict(median=float(np.median(ts_)), min=float(min(ts_)), max=float(max(ts_)), all=[float(t) for t in ts_])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pdist_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--regions', type=int, default=2000)
    ap.add_argument('--num-bases', type=int, default=21)
    ap.add_argument('--slide-span', type=int, default=3)
    ap.add_argument('--loop-rows', type=int, default=96)
    ap.add_argument('--vector-rows', type=int, default=256)
    a = ap.parse_args()
    eng = rq.get_engine()   # raises without a GPU
    rng = np.random.default_rng(29)
    row_len = a.num_bases + 2 * a.slide_span
    rows = ref.full_mantissa(rng, (a.regions, row_len))
    n_loop, n_vec = min(a.loop_rows, a.regions), min(a.vector_rows, a.regions)
    full = ts.get_pairwise_dists(rows, a.slide_span, engine=eng)   # warm-up
    want_loop, want_vec = ref.window_dists_loops(rows[:n_loop], a.slide_span), ref.window_dists(rows[:n_vec], a.slide_span)
    equal = bool(np.array_equal(full[:n_loop, :n_loop], want_loop) and np.array_equal(full[:n_vec, :n_vec], want_vec) and
                 np.array_equal(eng.pairwise_window_dists(rows[:n_vec], a.slide_span), want_vec))
    t_eng, k_ms, t_loop, t_vec = [], [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); ts.get_pairwise_dists(rows, a.slide_span, engine=eng); t1 = time.perf_counter()
        k_ms.append(eng.last_pdist_kernel_ms)
        ref.window_dists_loops(rows[:n_loop], a.slide_span); t2 = time.perf_counter()
        ref.window_dists(rows[:n_vec], a.slide_span); t3 = time.perf_counter()
        t_eng.append(t1 - t0); t_loop.append(t2 - t1); t_vec.append(t3 - t2)
    scale_loop, scale_vec = pairs(a.regions) / pairs(n_loop), pairs(a.regions) / pairs(n_vec)
    # the order_reads metric
    reads = rows.copy()
    reads[rng.random(reads.shape) < 0.2] = np.nan
    cond = eng.pairwise_nanmean_dists(reads)
    n_sub = min(512, a.regions)
    nan_equal = bool(np.array_equal(eng.pairwise_nanmean_dists(reads[:n_sub]), ref.nanmean_dists(reads[:n_sub]),
                                    equal_nan=True))
    t_nan, k_nan, t_nan_np = [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); eng.pairwise_nanmean_dists(reads); t1 = time.perf_counter()
        k_nan.append(eng.last_pdist_kernel_ms)
        ref.nanmean_dists(reads[:n_sub]); t2 = time.perf_counter()
        t_nan.append(t1 - t0); t_nan_np.append(t2 - t1)
    scale_nan = (a.regions * (a.regions - 1) // 2) / max(n_sub * (n_sub - 1) // 2, 1)
    k_med, e_med = float(np.median(k_ms)), float(np.median(t_eng))
    out = dict(
        what='get_pairwise_dists of %d regions, num_bases %d, slide_span %d: %d pairs x %d window pairs of %d values' % (
            a.regions, a.num_bases, a.slide_span, pairs(a.regions), (2 * a.slide_span + 1) ** 2, a.num_bases),
        regions=a.regions, row_len=row_len, slide_span=a.slide_span, rounds=a.rounds, outputs_equal_on_subsamples=equal,
        engine_kernel_ms=spread(k_ms), engine_end_to_end_ms=spread([t * 1e3 for t in t_eng]),
        engine_end_to_end_what='tombo_stats.get_pairwise_dists: stack, upload, kernel, download of the %d x %d matrix' % (
            a.regions, a.regions),
        numpy_loops=dict(rows=n_loop, measured_s=spread(t_loop), scale=scale_loop,
                         scaled_to_full_job_s=float(np.median(t_loop)) * scale_loop,
                         what='SCALED: the reference\'s statements pair by pair on the first %d rows, times the ratio '
                              'of the pair counts' % n_loop),
        numpy_vectorised=dict(rows=n_vec, measured_s=spread(t_vec), scale=scale_vec,
                              scaled_to_full_job_s=float(np.median(t_vec)) * scale_vec,
                              what='SCALED: tests/pdist_reference.py window_dists on the first %d rows, times the ratio '
                                   'of the pair counts' % n_vec),
        scaled_loops_over_engine_end_to_end=float(np.median(t_loop)) * scale_loop / e_med,
        scaled_loops_over_engine_kernel=float(np.median(t_loop)) * scale_loop / (k_med / 1e3) if k_med > 0 else None,
        window_sums_per_s_kernel=pairs(a.regions) * (2 * a.slide_span + 1) ** 2 / (k_med / 1e3) if k_med > 0 else None,
        nanmean=dict(reads=a.regions, positions=row_len, nan_share=0.2, pairs=int(cond.shape[0]), outputs_equal_on_subsample=nan_equal,
                     engine_kernel_ms=spread(k_nan), engine_end_to_end_ms=spread([t * 1e3 for t in t_nan]),
                     numpy_vectorised=dict(rows=n_sub, measured_s=spread(t_nan_np), scale=scale_nan,
                                           scaled_to_full_job_s=float(np.median(t_nan_np)) * scale_nan,
                                           what='SCALED: nanmean_dists on the first %d reads' % n_sub)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
    if not (equal and nan_equal):
        sys.exit('engine and numpy differ')


if __name__ == '__main__':
    main()

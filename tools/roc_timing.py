"""ROC numbers from per-read records: the numpy restatement on the host against the engine's three ROC entries.

    python tools/roc_timing.py [--out profiles/roc_timing.json]

5 000 000 synthetic per-read records in 50 blocks (both strands, random sequence with a few non-bases, normally
distributed statistics: every byte of the sort keys varies, so the sort runs all eight passes) against the two
motifs CG:1 and CCWGG:2 under the rule of compute_motif_stats, then for each motif the true-positive counts at the
1000 + 1000 ranks of compute_accuracy_rates.  After a warm-up of each route, five rounds alternating in ONE process,
host clock:
  (a) host route: tests/roc_reference.py -- vectorised sequence lookups, np.lexsort, np.cumsum (not the reference's
      per-record Python loop and sorted() of tuples, which would take minutes);
  (b) engine route: one `Engine.roc_motif_labels` call and one `Engine.roc_rank_counts` call per motif, uploads and
      downloads included; the time of the kernels alone comes from the hipEvents inside the entries, split into the
      labels (count, scan, scatter), the sort (keys and passes) and the ranks (label scan, gather).
The outputs of the two routes are compared bit for bit before anything is timed.  Needs a GPU: there is no
fallback.  Reads nothing but this repository."""
import os
import sys
import json
import time
import argparse
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import roc_reference as ref  # noqa: E402
from tombo_amd import resquiggle as rq, tombo_stats as ts, tombo_helper as th  # noqa: E402

MOTIFS = 'CG:1:x::CCWGG:2:a'
POINTS = 1000


def make_inputs(n_blocks, per_block, region, seed=23):
    rng = np.random.default_rng(seed)
    flank = 4
    lens = np.full(n_blocks, region + 2 * flank, dtype=np.int64)
    seq = rng.choice(np.array([0, 1, 2, 3, 4], dtype=np.uint8), int(lens.sum()), p=[.2475, .2475, .2475, .2475, .01])
    starts = np.arange(n_blocks, dtype=np.int64) * region + 1000
    pos = (starts[:, None] + rng.integers(0, region, (n_blocks, per_block))).ravel().astype(np.int64)
    return (np.arange(n_blocks, dtype=np.uint8) % 2, starts - flank, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
            seq, np.arange(n_blocks + 1, dtype=np.int64) * per_block, pos, rng.standard_normal(pos.shape[0]))


def plot_ranks(n):
    return np.union1d(np.linspace(0, n - 1, POINTS).astype(np.int64),
                      np.linspace(0, n - 1, POINTS + 1).astype(np.int64)[1:])


def route_host(args, motifs):
    out = []
    for stats, has_mod, _ in ref.motif_labels(*args, motifs):
        out.append((stats, has_mod) + ref.rank_counts(stats, has_mod, plot_ranks(stats.shape[0])))
    return out


def route_engine(eng, args, motifs, ms):
    out = []
    labelled = eng.roc_motif_labels(*args, motifs)
    ms['labels'] += eng.last_roc_kernel_ms
    for stats, has_mod in labelled:
        out.append((stats, has_mod) + eng.roc_rank_counts(stats, has_mod, plot_ranks(stats.shape[0])))
        ms['sort'] += eng.last_roc_sort_ms
        ms['ranks'] += eng.last_roc_gather_ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'roc_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=50)
    ap.add_argument('--per-block', type=int, default=100000)
    ap.add_argument('--region', type=int, default=10000)
    a = ap.parse_args()
    eng = rq.get_engine()   # raises without a GPU
    args = make_inputs(a.blocks, a.per_block, a.region)
    motifs = [ts.motif_base_sets(m) for m, _ in th.parse_motif_descs(MOTIFS)]
    want = route_host(args, motifs)   # warm-up of both routes
    got = route_engine(eng, args, motifs, dict(labels=0.0, sort=0.0, ranks=0.0))
    equal = all(np.array_equal(g[0].view(np.uint64), w[0].view(np.uint64)) and np.array_equal(g[1], w[1]) and
                np.array_equal(g[2], w[2]) and g[3:] == w[3:] for g, w in zip(got, want))
    t_a, t_b, k_ms = [], [], []
    for _ in range(a.rounds):
        ms = dict(labels=0.0, sort=0.0, ranks=0.0)
        t0 = time.perf_counter(); route_host(args, motifs); t1 = time.perf_counter()
        route_engine(eng, args, motifs, ms); t2 = time.perf_counter()
        t_a.append(t1 - t0); t_b.append(t2 - t1); k_ms.append(ms)
    n_rec, kept = int(args[5].shape[0]), [int(w[0].shape[0]) for w in want]
    med_b = float(np.median(t_b))
    k_med = dict((k, float(np.median([m[k] for m in k_ms]))) for k in ('labels', 'sort', 'ranks'))
    k_total = sum(k_med.values()) / 1e3
    out = dict(
        what='(statistic, has_mod) pairs of %s under compute_motif_stats, then tp counts at %d + %d ranks per motif' % (
            MOTIFS, POINTS, POINTS),
        blocks=a.blocks, records=n_rec, region=a.region, kept_per_motif=kept, rounds=a.rounds, outputs_equal=bool(equal),
        host_route_s=dict(median=float(np.median(t_a)), min=min(t_a), max=max(t_a), all=t_a,
                          what='tests/roc_reference.py: numpy lookups, np.lexsort, np.cumsum'),
        engine_route_s=dict(median=med_b, min=min(t_b), max=max(t_b), all=t_b,
                            what='three engine calls with uploads, downloads and the host glue between them'),
        kernel_ms=dict(median=k_med, all=k_ms, what='hipEvents inside the entries: labels = count / scan / scatter; '
                       'sort = keys and radix passes of both motifs; ranks = label scan and gather'),
        kernel_total_s=k_total, kernel_share_of_engine_route=k_total / med_b,
        speedup_with_transfers=float(np.median(t_a)) / med_b, speedup_kernels_only=float(np.median(t_a)) / k_total,
        bytes_uploaded=int(16 * n_rec + args[3].shape[0] + 9 * sum(kept)), bytes_downloaded=int(9 * sum(kept)),
        sort_keys_per_s=sum(kept) / (k_med['sort'] / 1e3) if k_med['sort'] > 0 else None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
    if not equal:
        sys.exit('outputs of the two routes differ')


if __name__ == '__main__':
    main()

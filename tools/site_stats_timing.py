"""Per-site fractions: the route a caller had before `compute_reg_stats_batch` against that call.

    python tools/site_stats_timing.py [--out profiles/site_stats_timing.json]

On the seeded de_novo batch of tests/site_stats_reference.py (64 regions x 10 000 positions x 50
reads), after a warm-up of each route, five rounds alternating in ONE process:
  (a) parent route: `tba_read_pvals` through `Engine.read_pvals`, every per-read p-value copied back, then
      the numpy collation of tests/site_stats_reference.py region by region;
  (b) `compute_reg_stats_batch` without the per-read output.
Both routes run the same host preparation (`_reg_stats_z_inputs`) inside the timed span.  Host clock
around calls that end in the entry's synchronise.  Needs a GPU: there is no fallback."""
import os
import sys
import json
import time
import argparse
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq  # noqa: E402
from tombo_amd._default_parameters import SMALLEST_PVAL  # noqa: E402
import site_stats_reference as ssr  # noqa: E402

FM, SINGLE, LOWER = 1, 0.5, 0.15


def route_parent(regions, model):
    inp = ts._reg_stats_z_inputs(regions, FM, model, ts.DE_NOVO_TXT)
    pv = rq.get_engine().read_pvals(inp.means, inp.ref_means, inp.ref_sds, inp.off, FM, True, SMALLEST_PVAL)
    lens = np.diff(inp.off)
    locs = np.repeat(inp.read_pos - inp.off[:-1], lens) + np.arange(pv.shape[0])
    trk = np.repeat(inp.read_track, lens)
    bounds = np.concatenate([[0], np.flatnonzero(np.diff(trk)) + 1, [trk.shape[0]]])
    out = [ssr.collate(pv[bounds[r]:bounds[r + 1]], locs[bounds[r]:bounds[r + 1]], SINGLE, LOWER, False)
           for r in range(len(regions))]
    return out, pv.nbytes


def route_batch(regions, model):
    return ts.compute_reg_stats_batch(regions, FM, 1, SINGLE, LOWER, None, model, None, False,
                                      ts.DE_NOVO_TXT, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'site_stats_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--regions', type=int, default=64)
    ap.add_argument('--positions', type=int, default=10000)
    ap.add_argument('--depth', type=int, default=50)
    a = ap.parse_args()
    rq.get_engine()   # raises without a GPU
    model = ts.TomboModel(seq_samp_type=th.seqSampleType('DNA', False))
    regions = ssr.seeded_batch(th, model, a.regions, a.positions, a.depth)
    want, bytes_a = route_parent(regions, model)   # warm-up of both routes
    got = route_batch(regions, model)
    equal = all(
        np.array_equal(rs.reg_frac_standard_base, w[0], equal_nan=True) and np.array_equal(rs.reg_poss, w[1])
        and np.array_equal(rs.reg_cov, w[2]) and rs.ctrl_cov == w[3] and np.array_equal(rs.valid_cov, w[4])
        for ((_, rs),), w in zip(got, want))
    n_sites = sum(w[1].shape[0] for w in want)
    # (b) copies back frac f8 + pos / cov / valid_cov i64 per track position, two counts per track
    n_trk_pos = sum(r.end - r.start + 2 * FM for r in regions)
    bytes_b = n_trk_pos * 32 + len(regions) * 16
    t_a, t_b = [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); route_parent(regions, model); t1 = time.perf_counter()
        route_batch(regions, model); t2 = time.perf_counter()
        t_a.append(t1 - t0); t_b.append(t2 - t1)
    res = dict(
        what='per-site fractions, de_novo, fm_offset %d, thresholds (%g, %g)' % (FM, LOWER, SINGLE),
        regions=a.regions, positions=a.positions, depth=a.depth,
        statistics=int(sum(len(r.reads) for r in regions) * (a.positions + 2 * FM)), sites=int(n_sites),
        rounds=a.rounds, outputs_equal=bool(equal),
        parent_route_s=dict(median=float(np.median(t_a)), min=min(t_a), max=max(t_a), all=t_a),
        batch_call_s=dict(median=float(np.median(t_b)), min=min(t_b), max=max(t_b), all=t_b),
        bytes_copied_back=dict(parent_route=int(bytes_a), batch_call=int(bytes_b)),
        not_slower=bool(np.median(t_b) <= np.median(t_a) + (max(t_a) - min(t_a))))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
    print(json.dumps(res))
    if not equal:
        sys.exit('outputs of the two routes differ')


if __name__ == '__main__':
    main()

"""aggregate_per_read_stats: the host route over stored per-read blocks against `Engine.site_aggregate`.

    python tools/stat_agg_timing.py [--out profiles/stat_agg_timing.json]

64 blocks x 10 000 positions x 50 reads = 32 M stored records (the shape of profiles/site_stats_timing.json), each
block laid out as it is stored: read after read, a read's positions ascending.  After a warm-up of each route, five
rounds alternating in ONE process, host clock:
  (a) host route: the arithmetic of the reference's _agg_stats_worker / apply_per_read_thresh block by block in numpy --
      stable sort by position, site boundaries, thresholds -- with the per-site Python loops of the reference
      replaced by np.add.reduceat (the fastest form this arithmetic has on the host);
  (b) one `Engine.site_aggregate` call over all blocks, upload of the records and download of the per-site
      arrays included; the time of its kernels alone comes from the hipEvents inside the entry.
The two outputs must be equal.  Needs a GPU: there is no fallback."""
import os
import sys
import json
import time
import argparse
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)

from tombo_amd import resquiggle as rq, _native  # noqa: E402

SINGLE, LOWER, DAMP = 0.5, 0.15, (2.0, 0.0)


def make_blocks(n_blocks, n_pos, depth, seed=11):
    rng = np.random.default_rng(seed)
    starts = np.arange(n_blocks, dtype=np.int64) * n_pos
    rec = np.empty(n_blocks * n_pos * depth, dtype=_native.PER_READ_DTYPE)
    rec['pos'] = (starts[:, None, None] + np.arange(n_pos)[None, None, :] + np.zeros((1, depth, 1), np.int64)).ravel()
    rec['stat'] = rng.random(rec.shape[0])
    rec['read_id'] = np.tile(np.repeat(np.arange(depth), n_pos), n_blocks)
    off = np.arange(n_blocks + 1, dtype=np.int64) * (n_pos * depth)
    return starts, starts + n_pos, off, rec


def route_host(starts, ends, off, rec):
    out = []
    for t in range(starts.shape[0]):
        block = rec[off[t]:off[t + 1]]
        order = np.argsort(block['pos'], kind='stable')
        pos, stat = block['pos'][order], block['stat'][order]
        first = np.flatnonzero(np.concatenate([[1], np.diff(pos)]))
        ge = stat >= SINGLE
        valid = ge | (stat <= LOWER)
        cov = np.diff(np.concatenate([first, [pos.shape[0]]]))
        n_valid = np.add.reduceat(valid.astype(np.int64), first)
        n_ge = np.add.reduceat((ge & valid).astype(np.int64), first)
        with np.errstate(invalid='ignore'):
            frac = np.where(n_valid > 0, n_ge / n_valid, np.nan)
            damp = (np.round(frac * n_valid) + DAMP[0]) / (n_valid + DAMP[0] + DAMP[1])
        out.append((frac, pos[first].astype(np.int64), cov, n_valid, damp))
    return out


def route_engine(eng, starts, ends, off, rec):
    return eng.site_aggregate(starts, ends, off, rec, SINGLE, LOWER, False, DAMP)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stat_agg_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=64)
    ap.add_argument('--positions', type=int, default=10000)
    ap.add_argument('--depth', type=int, default=50)
    a = ap.parse_args()
    eng = rq.get_engine()   # raises without a GPU
    args = make_blocks(a.blocks, a.positions, a.depth)
    want = route_host(*args)   # warm-up of both routes
    res = route_engine(eng, *args)
    equal = True
    for t, w in enumerate(want):
        lo = int(res.pos_off[t])
        hi = lo + int(res.counts[t])
        got = (res.frac[lo:hi], res.poss[lo:hi], res.cov[lo:hi], res.valid[lo:hi], res.damp[lo:hi])
        equal = equal and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, w))
    t_a, t_b, k_ms = [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); route_host(*args); t1 = time.perf_counter()
        route_engine(eng, *args); t2 = time.perf_counter()
        t_a.append(t1 - t0); t_b.append(t2 - t1); k_ms.append(eng.last_site_aggregate_kernel_ms)
    n_rec, n_pos = int(args[3].shape[0]), a.blocks * a.positions
    med_b, med_k = float(np.median(t_b)), float(np.median(k_ms)) / 1e3
    out = dict(
        what='per-site fractions from stored per-read records, thresholds (%g, %g), damp counts %s' % (LOWER, SINGLE, DAMP),
        blocks=a.blocks, positions=a.positions, depth=a.depth, records=n_rec, rounds=a.rounds, outputs_equal=bool(equal),
        host_route_s=dict(median=float(np.median(t_a)), min=min(t_a), max=max(t_a), all=t_a),
        engine_call_s=dict(median=med_b, min=min(t_b), max=max(t_b), all=t_b),
        kernel_ms=dict(median=float(np.median(k_ms)), min=min(k_ms), max=max(k_ms), all=k_ms,
                       what='hipEvents around the counter reset, k_site_rec and k_site_finish'),
        bytes_uploaded=int(16 * n_rec + 8 * (3 * a.blocks + 1)), bytes_downloaded=int(40 * n_pos + 16 * a.blocks),
        upload_GBps_if_all_of_the_call=16e-9 * n_rec / med_b,
        kernel_share_of_call=med_k / med_b,
        kernel_record_GBps=16e-9 * n_rec / med_k if med_k > 0 else None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
    if not equal:
        sys.exit('outputs of the two routes differ')


if __name__ == '__main__':
    main()

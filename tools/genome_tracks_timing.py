"""Genome tracks: `GenomeTracks.add_reads` + `finish` and `get_largest_signal_differences`' selection on the device
against the numpy restatement of the reference (tests/tracks_reference.py) on the same machine.

    python tools/genome_tracks_timing.py [--out profiles/genome_tracks_timing.json]

Input: 20 000 reads of 10 kb, half on each strand of a 5 Mb chromosome, three slots (norm_mean, norm_stdev, length);
the reads' columns are views into one pool of random values.  After one warm-up of each route, the median of five
rounds, alternating in ONE process.  The device route is split into
  gather_s   add_reads: the per-read Python loop that copies the reads' columns into flat arrays,
  lists_s    the tile lists (vectorised numpy),
  engine_s   the tracks_begin / tracks_add / tracks_finish calls: host-to-device copies, kernels, copies back,
  kernel_ms  of which kernels (hipEvents around the launches); transfer_s = engine_s - kernel_ms / 1000.
The parent commit has no route of its own, so the numpy loop over the reads is the yardstick.  The restatement adds
a whole 10 kb read per numpy call, so it runs near the host's memory bandwidth: long reads are its best case.
Host clock around calls that end in a synchronise.  Single-threaded numpy; nothing here starts threads.  Needs a
GPU: there is no fallback."""
import os
import sys
import json
import time
import argparse
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from tombo_amd import tombo_helper as th, resquiggle as rq  # noqa: E402
import tracks_reference as tr  # noqa: E402

SLOTS = ('norm_mean', 'norm_stdev', 'length')


def make_reads(rng, n_reads, read_len, chrm_len):
    pool = dict(norm_mean=rng.normal(size=1 << 20), norm_stdev=np.abs(rng.normal(size=1 << 20)),
                length=rng.integers(1, 400, 1 << 20).astype(np.float64))
    index, cols = {}, {}
    for strand in '+-':
        starts = rng.integers(0, chrm_len - read_len + 1, n_reads // 2)
        at = rng.integers(0, (1 << 20) - read_len, n_reads // 2)
        cl = [dict((s, pool[s][a:a + read_len]) for s in SLOTS) for a in at]
        index[('chr1', strand)] = [tr.Read(int(s), int(s) + read_len, strand, None, c['norm_mean'])
                                   for s, c in zip(starts, cl)]
        cols[('chr1', strand)] = cl
    return index, cols


def device_route(index, slots, sizes):
    t0 = time.perf_counter()
    tracks = th.GenomeTracks(sizes, slots=SLOTS)
    for (chrm, strand), reads in index.items():
        tracks.add_reads(chrm, strand, reads, dict((s, slots[s][(chrm, strand)]) for s in SLOTS))
    t1 = time.perf_counter()
    res = tracks.finish()
    t2 = time.perf_counter()
    tm = dict(tracks.timing, gather_s=t1 - t0, total_s=t2 - t0)
    tm['transfer_s'] = tm['engine_s'] - tm['kernel_ms'] / 1000.0
    return res, tm


def numpy_route(index, cols, sizes):
    t0 = time.perf_counter()
    out = {}
    for cs, reads in index.items():
        out[cs] = [tr.slot_mean(reads, cols[cs], sizes[cs[0]], s) for s in SLOTS]
    return out, time.perf_counter() - t0


def med(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), all=[float(x) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'genome_tracks_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reads', type=int, default=20000)
    ap.add_argument('--read-len', type=int, default=10000)
    ap.add_argument('--chrm-len', type=int, default=5000000)
    ap.add_argument('--top', type=int, default=100)
    a = ap.parse_args()
    eng = rq.get_engine()   # raises without a GPU
    rng = np.random.default_rng(7)
    index, cols = make_reads(rng, a.reads, a.read_len, a.chrm_len)
    slots, sizes = tr.slot_maps(cols), {'chr1': a.chrm_len}
    got, _ = device_route(index, slots, sizes)      # warm-up of both routes
    want, _ = numpy_route(index, cols, sizes)
    equal = all(np.array_equal(got[cs].means[k], want[cs][k], equal_nan=True) for cs in want for k in range(3))
    dev, host = [], []
    for _ in range(a.rounds):
        dev.append(device_route(index, slots, sizes)[1])
        host.append(numpy_route(index, cols, sizes)[1])
    # the quick sample-against-control scan: the two strands' mean signal stand in for sample and control
    x, y = want[('chr1', '+')][0], want[('chr1', '-')][0]
    top_dev, top_np = eng.tracks_topn(x, y, a.top), tr.top_n(x, y, a.top)
    top_equal = np.array_equal(top_dev[0], top_np[0]) and np.array_equal(top_dev[1], top_np[1])
    t_dev, t_np = [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); eng.tracks_topn(x, y, a.top); t1 = time.perf_counter()
        tr.top_n(x, y, a.top); t2 = time.perf_counter()
        t_dev.append(t1 - t0); t_np.append(t2 - t1)
    n_values = a.reads * a.read_len
    positions = 2 * a.chrm_len
    # per position and slot the kernel reads and writes a sum and a coverage (32 B) and, per covering read, one
    # value (8 B); the read coverage adds 16 B per position
    kernel_bytes = positions * (3 * 32 + 16) + 3 * 8 * n_values
    kernel_s = float(np.median([d['kernel_ms'] for d in dev])) / 1000.0
    res = dict(
        what='genome tracks: %d reads of %d bases on both strands of a %d-position chromosome, slots %s' % (
            a.reads, a.read_len, a.chrm_len, ', '.join(SLOTS)),
        rounds=a.rounds, outputs_equal=bool(equal), values_added=int(3 * n_values),
        device=dict((k, med([d[k] for d in dev])) for k in ('total_s', 'gather_s', 'lists_s', 'engine_s',
                                                            'transfer_s')),
        device_kernel_ms=med([d['kernel_ms'] for d in dev]),
        numpy_restatement_s=med(host),
        kernel_bytes_per_position=float(kernel_bytes) / positions,
        kernel_GBps=float(kernel_bytes) / kernel_s / 1e9 if kernel_s > 0 else None,
        bytes_uploaded=int(3 * 8 * n_values), bytes_copied_back=int(positions * (3 * 16 + 8)),
        device_faster_than_numpy=bool(np.median([d['total_s'] for d in dev]) < np.median(host)),
        top_n=dict(n=a.top, positions=a.chrm_len, outputs_equal=bool(top_equal), device_s=med(t_dev),
                   numpy_s=med(t_np), device_faster_than_numpy=bool(np.median(t_dev) < np.median(t_np))))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
    print(json.dumps(res))
    if not (equal and top_equal):
        sys.exit('the device and the restatement differ')


if __name__ == '__main__':
    main()

"""Whole-sample modified base detection: the route a caller could assemble before `test_significance` against
that call.

    python tools/test_signif_timing.py [--out profiles/test_signif_timing.json]

One seeded reads index ('+' and '-' strand of one chromosome, every read spanning several regions), de_novo,
fm_offset 1.  After a warm-up of each route, five rounds alternating in ONE process:
  (a) today's route: `th.iter_cov_regs`, `intervalData.add_reads`, `compute_reg_stats_batch` (per-read
      preparation in Python, 24 bytes uploaded per statistic) over the region batches of
      `iter_signif_region_batches`, `write_stats_from_regions`;
  (b) `test_significance` (`compute_reg_stats_reads_batch`: every read uploaded once, preparation on the device).
Both write a ModelStats file into an in-memory store (tests/store_memh5.py) and the two files are compared.
Recorded besides the medians: the time of the region batches alone (coverage, regions, add_reads: common to both
routes), the device time of the new kernels and of the statistic kernels behind them (hipEvents inside
tba_site_fractions_reads), and the bytes each route hands to its site-fractions entry.  Host clock around calls
that end in the entry's synchronise.  Needs a GPU: there is no fallback."""
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
from store_memh5 import StoreGroup, flat_tree, same_array  # noqa: E402

FM, SINGLE, LOWER, DAMP, MIN_READS, N_SIGNIF = 1, 0.5, 0.15, (2, 0), 1, 1000


def seeded_index(model, n_regions, region_size, depth, seed=4574):
    """{('chr1', strand): reads}: per strand reads of 2.5 to 4 region sizes placed at random over n_regions regions, as
    many as give `depth` on average (levels: the model's plus continuous noise, a shift on some bases)"""
    rng = np.random.default_rng(seed)
    K, cp = model.kmer_width, model.central_pos
    size = n_regions * region_size
    genome = ''.join(rng.choice(list('ACGT'), size))
    index = {}
    for strand in '+-':
        reads, bases = [], 0
        while bases < depth * size:
            n = int(rng.integers(int(2.5 * region_size), 4 * region_size + 1))
            s = int(rng.integers(0, size - n + 1))
            seq = genome[s:s + n] if strand == '+' else th.rev_comp(genome[s:s + n])
            lv, sd = model.get_exp_levels_from_seq(seq)
            m = rng.normal(0.0, 1.0, n)
            nl = n - K + 1
            m[cp:cp + nl] = lv + rng.normal(0.0, 1.3, nl) * sd + 1.2 * (rng.random(nl) < 0.3)
            reads.append(th.resquiggledRead(s, s + n, False, 0, strand, None, None, False,
                                            read_id='t%s%d' % (strand, len(reads)), means=m, seq=seq))
            bases += n
        index[('chr1', strand)] = reads
    return index


class Meter(object):
    """the engine with its two site-fractions entries metered: bytes of the arrays handed over, device time"""

    def __init__(self, eng):
        self.eng = eng
        self.reset()

    def reset(self):
        self.bytes, self.calls, self.new_kernel_ms, self.stat_kernel_ms = 0, 0, 0.0, 0.0

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def _count(self, args):
        self.calls += 1
        self.bytes += sum(a.nbytes for a in args if isinstance(a, np.ndarray))

    def site_fractions_z(self, *args, **kw):
        self._count(args)
        return self.eng.site_fractions_z(*args, **kw)

    def site_fractions_reads(self, *args, **kw):
        self._count(args)
        out = self.eng.site_fractions_reads(*args, **kw)
        self.new_kernel_ms += self.eng.last_site_reads_kernel_ms[0]
        self.stat_kernel_ms += self.eng.last_site_reads_kernel_ms[1]
        return out


def batches(index, model, region_size, eng):
    return list(ts.iter_signif_region_batches(index, ts.DE_NOVO_TXT, region_size, FM, std_ref=model, engine=eng))


def route_today(index, model, region_size, eng):
    store = StoreGroup()
    stats = ts.ModelStats(store, ts.DE_NOVO_TXT, region_size, DAMP, MIN_READS, N_SIGNIF)
    for regs, _ in batches(index, model, region_size, eng):
        res = ts.compute_reg_stats_batch(regs, FM, MIN_READS, SINGLE, LOWER, None, model, None, False, ts.DE_NOVO_TXT,
                                         None, engine=eng)
        ts.write_stats_from_regions(res, [[] for _ in regs], stats)
    stats.close()
    return store


def route_test_significance(index, model, region_size, eng):
    store = StoreGroup()
    ts.test_significance(index, ts.DE_NOVO_TXT, 'timing', region_size, 1, MIN_READS, N_SIGNIF, None, SINGLE, LOWER, DAMP,
                         FM, None, model, engine=eng, stores={'timing.tombo.stats': store})
    return store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'test_signif_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--regions', type=int, default=200)
    ap.add_argument('--region-size', type=int, default=1000)
    ap.add_argument('--depth', type=int, default=30)
    a = ap.parse_args()
    eng = Meter(rq.get_engine())   # raises without a GPU
    model = ts.TomboModel(seq_samp_type=th.seqSampleType('DNA', False))
    index = seeded_index(model, a.regions, a.region_size, a.depth)
    want = route_today(index, model, a.region_size, eng)   # warm-up of both routes
    bytes_a, calls_a = eng.bytes, eng.calls
    eng.reset()
    got = route_test_significance(index, model, a.region_size, eng)
    bytes_b, calls_b = eng.bytes, eng.calls
    fa, fb = flat_tree(want), flat_tree(got)
    equal = list(fa) == list(fb) and all(same_array(fa[k], fb[k]) for k in fa)
    bt = batches(index, model, a.region_size, eng)
    n_regions = sum(len(r) for r, _ in bt)
    n_pairs = sum(len(reg.reads) for r, _ in bt for reg in r)
    n_stats = sum(int(v.shape[0]) for k, v in fa.items() if k.endswith('/block_stats'))
    t_a, t_b, t_r, k_new, k_stat = [], [], [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); route_today(index, model, a.region_size, eng); t1 = time.perf_counter()
        eng.reset()
        route_test_significance(index, model, a.region_size, eng); t2 = time.perf_counter()
        batches(index, model, a.region_size, eng); t3 = time.perf_counter()
        t_a.append(t1 - t0); t_b.append(t2 - t1); t_r.append(t3 - t2)
        k_new.append(eng.new_kernel_ms); k_stat.append(eng.stat_kernel_ms)
    span = lambda t: dict(median=float(np.median(t)), min=min(t), max=max(t), all=t)   # noqa: E731
    n_reads = sum(len(v) for v in index.values())
    res = dict(
        what='test_significance, de_novo, fm_offset %d, thresholds (%g, %g), one ModelStats file' % (FM, LOWER, SINGLE),
        strands=2, regions_per_strand=a.regions, region_size=a.region_size, mean_depth=a.depth, reads=n_reads,
        read_bases=int(sum(rd.end - rd.start for v in index.values() for rd in v)), regions_tested=n_regions,
        region_read_pairs=n_pairs, sites_written=n_stats, engine_calls=dict(today=calls_a, test_significance=calls_b),
        rounds=a.rounds, outputs_equal=bool(equal),
        today_route_s=span(t_a), test_significance_s=span(t_b), region_batches_alone_s=span(t_r),
        test_significance_kernel_ms=dict(plan_scan_gather=span(k_new), statistics_and_collation=span(k_stat)),
        bytes_to_site_entry=dict(today=int(bytes_a), test_significance=int(bytes_b)),
        speedup_median=float(np.median(t_a) / np.median(t_b)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
    print(json.dumps(res))
    if not equal:
        sys.exit('outputs of the two routes differ')


if __name__ == '__main__':
    main()

"""Time the centring of a k-mer model on one MI355X: the per-read form against the batch form.

    python tools/center_timing.py [--reads 5000] [--bases 1000] [--out profiles/center_timing.json]

Synthetic reads of about `--bases` bases (seeded, made on the host): DNA at the standard DNA model's levels
(5-12 samples a base, int16 DAC), RNA at the standard RNA model's (25-45 samples a base at level * 70 + 450, noise
of sd 9, samples in acquisition order).  max_reads = the number of reads, so both forms fit every read.
  * DNA, per-read form: ts.center_model_to_median_norm -- wall time over all reads; the kernel time of its two
    pipeline slices is summed in a second, instrumented pass over the first --kernel-reads reads (reading the
    event times after every slice would slow the timed pass);
  * DNA, batch form: ts.center_model_to_median_norm_batch -- wall time, and the kernel time the two entries report
    per chunk (device events around their kernels);
  * RNA, batch form: the same (the per-read form refuses RNA).
Both forms run once on --warmup reads first (code objects, buffers).  Wall times are host clocks around calls that
end in a device synchronise.  The factors of the two DNA forms are compared bit for bit.  There is no fallback:
without a device the engine cannot be created and the tool fails."""
import os
import sys
import json
import time
import argparse
import warnings

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq, _native  # noqa: E402


def model_of(rna):
    return ts.TomboModel(seq_samp_type=th.seqSampleType(ts.RNA_SAMP_TYPE if rna else ts.DNA_SAMP_TYPE, rna))


def make_reads(rng, n_reads, n_bases, rna):
    model = model_of(rna)
    K, up = model.kmer_width, model.central_pos
    reads = []
    for _ in range(n_reads):
        n = int(rng.integers(n_bases - n_bases // 10, n_bases + n_bases // 10 + 1))
        codes = rng.integers(0, 4, n + K - 1)
        idx = np.zeros(n, dtype=np.int64)
        for j in range(K):
            idx = idx * 4 + codes[j:j + n]
        lv = model.level_means[idx]
        seq = ''.join('ACGT'[c] for c in codes[up:up + n])      # base j sits at the model's central position
        rsr = int(rng.integers(20, 60))
        if rna:
            dwell = rng.integers(25, 46, n)
            body = np.repeat(lv * 70.0 + 450.0 + rng.normal(0, 3.0, n), dwell) + rng.normal(0, 9.0, int(dwell.sum()))
            lead, tail = rng.normal(450, 60, rsr), rng.normal(450, 60, 25)
        else:
            dwell = rng.integers(5, 13, n)
            body = np.repeat(lv * 12.0 + 90.0 + rng.normal(0, 0.6, n), dwell) + rng.normal(0, 1.5, int(dwell.sum()))
            lead, tail = rng.normal(95, 6, rsr), rng.normal(95, 6, 25)
        sig = np.round(np.concatenate([lead, body, tail])).astype(np.int16)
        start = np.concatenate([[0], np.cumsum(dwell)[:-1]]).astype(np.int64)
        reads.append(ts.CenterRead(sig[::-1].copy() if rna else sig, start, seq, rsr, rna, n))
    return reads


def off_centre(rna):
    model = model_of(rna)
    model._center_model(0.15, 1.2)
    return model


class Timed(object):
    """an engine that sums the kernel times of the centring entries (batch form) or of run_stages (per-read form)"""

    def __init__(self, engine, per_read_kernels=False):
        self._engine, self.kernel_ms, self.calls, self._per_read = engine, 0.0, 0, per_read_kernels

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def center_fit(self, *a, **kw):
        res = self._engine.center_fit(*a, **kw)
        self.kernel_ms += sum(self._engine.last_center_kernel_ms)
        self.calls += 1
        return res

    def run_stages(self, first, last):
        self._engine.run_stages(first, last)
        if self._per_read:
            self.kernel_ms += float(self._engine.get(_native.GET_KERNEL_MS)[_native.STAGE_NAMES.index('total')])
        self.calls += 1


def centre(form, reads, rna, engine):
    """-> (seconds, factors handed to _center_model)"""
    model, got = off_centre(rna), []
    real = model._center_model
    model._center_model = lambda a, b: (got.append((float(a), float(b))), real(a, b))[1]
    np.random.seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        t0 = time.perf_counter()
        form(list(reads), model, len(reads), engine=engine)
        dt = time.perf_counter() - t0
    return dt, got[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=5000)
    ap.add_argument('--bases', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--kernel-reads', type=int, default=500)
    ap.add_argument('--out', default=os.path.join('profiles', 'center_timing.json'))
    a = ap.parse_args()
    eng = rq.get_engine()
    rng = np.random.default_rng(20261021)
    res = dict(reads=a.reads, bases=a.bases, warmup=a.warmup, kernel_reads=a.kernel_reads)
    dna = make_reads(rng, a.reads, a.bases, False)
    res['dna_samples'] = int(sum(len(rd.raw_signal) for rd in dna))
    for form in (ts.center_model_to_median_norm, ts.center_model_to_median_norm_batch):
        centre(form, dna[:a.warmup], False, eng)
    t_eng = Timed(eng)
    res['dna_per_read_wall_s'], f_per_read = centre(ts.center_model_to_median_norm, dna, False, t_eng)
    res['dna_per_read_engine_runs'] = t_eng.calls
    k_eng = Timed(eng, per_read_kernels=True)
    n_k = min(a.kernel_reads, a.reads)
    centre(ts.center_model_to_median_norm, dna[:n_k], False, k_eng)
    res['dna_per_read_kernel_ms_per_read'] = k_eng.kernel_ms / n_k
    res['dna_per_read_kernel_s_scaled'] = k_eng.kernel_ms / n_k * a.reads / 1e3
    b_eng = Timed(eng)
    res['dna_batch_wall_s'], f_batch = centre(ts.center_model_to_median_norm_batch, dna, False, b_eng)
    res['dna_batch_kernel_s'], res['dna_batch_chunks'] = b_eng.kernel_ms / 1e3, b_eng.calls
    res['dna_factors'] = list(f_batch)
    res['dna_same_bits'] = bool(np.array_equal(np.array(f_per_read).view(np.int64), np.array(f_batch).view(np.int64)))
    res['dna_wall_ratio'] = res['dna_per_read_wall_s'] / res['dna_batch_wall_s']
    del dna
    rna = make_reads(rng, a.reads, a.bases, True)
    res['rna_samples'] = int(sum(len(rd.raw_signal) for rd in rna))
    centre(ts.center_model_to_median_norm_batch, rna[:a.warmup], True, eng)
    r_eng = Timed(eng)
    res['rna_batch_wall_s'], f_rna = centre(ts.center_model_to_median_norm_batch, rna, True, r_eng)
    res['rna_batch_kernel_s'], res['rna_batch_chunks'] = r_eng.kernel_ms / 1e3, r_eng.calls
    res['rna_factors'] = list(f_rna)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1, sort_keys=True)
        fp.write('\n')


if __name__ == '__main__':
    main()

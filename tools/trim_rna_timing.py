"""RNA adapter trimming and estimate_global_scale (csrc/k_trim_rna.h) on a batch of synthetic direct-RNA reads.

    python tools/trim_rna_timing.py [--out profiles/trim_rna_timing.json]

The batch: device-made int16 RNA reads in acquisition order (tombo_amd.synth's RNA parameters, about 130 000 samples
each) downloaded to host arrays.  The GPU step runs in a child process under its own `timeout`.  In that ONE process,
after a warm-up call per configuration, `--rounds` rounds in which the configurations that are compared alternate; host
clock around work that ends in a device synchronise, medians reported beside every single time:
  (a) tombo_stats.trim_rna_batch over all reads: packing of the 40 000-sample prefixes, upload, kernels, download; the
      time of the kernels alone comes from the hipEvents inside the entry (`last_trim_kernel_ms`);
  (b) on `--route-reads` of the reads, trim_rna_batch against the route that was open before it: per read
      c_valid_cpts_w_cap + c_new_mean_stds through the per-kernel entries, and the window stage in numpy;
  (c) on `--prep-reads` of the reads, one resquiggle_batch_iters(device_prep=True) pass with and without
      trim_rna_adapter (max_scaling_iters 1, no save parameters);
  (d) estimate_global_scale on `--scale-reads` whole reads against np.median on one thread.
Before anything is timed (b)'s two routes and (d)'s two are compared: the same answers.  Needs a GPU: there is no
fallback.  Reads nothing but this repository."""
import os
import sys
import json
import time
import argparse
import subprocess
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)


def spread(ts_):
    return dict(median=float(np.median(ts_)), min=float(min(ts_)), max=float(max(ts_)), all=[float(t) for t in ts_])


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def per_read_route(raw, params, trim):
    """trim_rna of one read through the per-kernel entries and numpy (the reference's own steps)"""
    from tombo_amd import _c_helper
    x = raw[:trim.max_raw_obs].astype(np.float64)
    cpts = np.sort(_c_helper.c_valid_cpts_w_cap(x, params.min_obs_per_base, params.running_stat_width,
                                                x.shape[0] // params.mean_obs_per_event))
    _, sds = _c_helper.c_new_mean_stds(x, cpts)
    means = np.lib.stride_tricks.sliding_window_view(sds, trim.moving_window_size).mean(-1)
    thresh = means.mean() * trim.thresh_scale
    mins = np.lib.stride_tricks.sliding_window_view(means, trim.min_running_values).min(-1)
    above = np.flatnonzero(mins > thresh)
    return int(cpts[above[0]]) if above.shape[0] else 0


def child(a):
    from tombo_amd import _native, synth, tombo_stats as ts, tombo_helper as th, resquiggle as rq
    eng = rq.get_engine()   # raises without a GPU
    samp = th.seqSampleType('RNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)
    trim = ts.DEFAULT_TRIM_RNA_PARAMS
    gen = _native.Synth(model, 0)
    _, raw_off, _, seq_off = gen.generate(_native.make_synth_params(reverse=True, **synth.RNA_SYNTH), 1,
                                          np.full(a.reads, a.bases), raw_dtype=np.int16)
    raw, seq = gen.download()
    raws = [raw[i:j] for i, j in zip(raw_off[:-1], raw_off[1:])]
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    n_route, n_prep, n_scale = min(a.route_reads, a.reads), min(a.prep_reads, a.reads), min(a.scale_reads, a.reads)
    mrs = [th.resquiggleResults(
        align_info=th.alignInfo('read_%d' % k, 'BaseCalled_template', 0, 0, 0, 0, a.bases, 0),
        genome_loc=th.genomeLocation(0, '+', 'synth'), genome_seq=letters[seq[seq_off[k]:seq_off[k + 1]]].tobytes().decode(),
        mean_q_score=10.0, raw_signal=raws[k]) for k in range(n_prep)]

    def batch(reads):
        return ts.trim_rna_batch(reads, params, trim, engine=eng)

    def route(reads):
        return [per_read_route(r, params, trim) for r in reads]

    def prep(trim_on):
        return rq.resquiggle_batch_iters(mrs, model, params, outlier_thresh=5.0, seq_samp_type=samp, max_scaling_iters=1,
                                         engine=eng, device_prep=True, trim_rna_adapter=trim_on)

    def scale_np():
        return np.mean([np.median(np.abs(r - np.median(r))) for r in raws[:n_scale]])

    def scale_dev():
        st = np.random.get_state()
        try:
            return ts.estimate_global_scale(list(raws[:n_scale]), n_scale, engine=eng)
        finally:
            np.random.set_state(st)

    ends, errs = batch(raws[:n_route])
    same_ends = bool(all(e is None for e in errs) and ends.tolist() == route(raws[:n_route]))
    same_scale = bool(scale_dev() == scale_np())
    batch(raws), prep(False), prep(True)            # warm-up of the remaining configurations
    t = dict((k, []) for k in ('batch_all', 'kernel_all', 'batch_route', 'kernel_route', 'route', 'prep_off', 'prep_on',
                               'scale_dev', 'kernel_scale', 'scale_np'))
    for _ in range(a.rounds):
        t['batch_all'].append(timed(lambda: batch(raws))); t['kernel_all'].append(eng.last_trim_kernel_ms)
        t['batch_route'].append(timed(lambda: batch(raws[:n_route]))); t['kernel_route'].append(eng.last_trim_kernel_ms)
        t['route'].append(timed(lambda: route(raws[:n_route])))
        t['prep_off'].append(timed(lambda: prep(False)))
        t['prep_on'].append(timed(lambda: prep(True)))
        t['scale_dev'].append(timed(scale_dev)); t['kernel_scale'].append(eng.last_med_mad_kernel_ms)
        t['scale_np'].append(timed(scale_np))
    out = dict(
        what='%d int16 RNA reads x %d bases (%d samples, %.0f per read), default trimming parameters' % (
            a.reads, a.bases, int(raw_off[-1]), raw_off[-1] / float(a.reads)),
        reads=a.reads, bases_per_read=a.bases, samples=int(raw_off[-1]), rounds=a.rounds,
        trim_rna_batch_all_reads=dict(end_to_end_ms=spread(t['batch_all']), kernel_ms=spread(t['kernel_all'])),
        per_read_route=dict(reads=n_route, same_answers=same_ends,
                            trim_rna_batch=dict(end_to_end_ms=spread(t['batch_route']), kernel_ms=spread(t['kernel_route'])),
                            per_kernel_entries_and_numpy=dict(end_to_end_ms=spread(t['route']))),
        device_prep_pass=dict(reads=n_prep, without_trimming_ms=spread(t['prep_off']), with_trimming_ms=spread(t['prep_on'])),
        estimate_global_scale=dict(reads=n_scale, same_answer=same_scale, device=dict(
            end_to_end_ms=spread(t['scale_dev']), kernel_ms=spread(t['kernel_scale'])),
            numpy_one_thread_ms=spread(t['scale_np'])),
        end_to_end_what='host clock: packing, upload, kernels, download, the result lists',
        kernel_what='hipEvent time of the kernels inside the entry')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
    if not (same_ends and same_scale):
        sys.exit('the routes disagree')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'trim_rna_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reads', type=int, default=10000)
    ap.add_argument('--bases', type=int, default=3000, help='43 samples per base on average: about 130 000 per read')
    ap.add_argument('--route-reads', type=int, default=500)
    ap.add_argument('--prep-reads', type=int, default=1000)
    ap.add_argument('--scale-reads', type=int, default=1000)
    ap.add_argument('--timeout', type=int, default=900, help='seconds the GPU step may take')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child', '--out', a.out,
           '--rounds', str(a.rounds), '--reads', str(a.reads), '--bases', str(a.bases), '--route-reads',
           str(a.route_reads), '--prep-reads', str(a.prep_reads), '--scale-reads', str(a.scale_reads)]
    sys.exit(subprocess.call(cmd))


if __name__ == '__main__':
    main()

"""normalize_raw_signal_batch (csrc/k_norm_api.h) per norm type on a batch of synthetic reads, and beside it the
pipeline's segmentation stage, which holds k_normalize, on the same batch.

    python tools/norm_api_timing.py [--out profiles/norm_api_timing.json]

The batch: device-made int16 DNA reads (tombo_amd.synth's parameters) downloaded to host arrays.  The GPU step runs in
a child process under its own `timeout`.  In that ONE process, after a warm-up call per configuration, five rounds, host
clock around work that ends in a device synchronise:
  (a) tombo_stats.normalize_raw_signal_batch with outlier_thresh 5 for 'none', 'pA_raw', 'median',
      'median_const_scale' and 'robust_median': packing, upload, k_norm_scale, k_norm_apply, download, the result list;
      the time of the two kernels alone comes from the hipEvents inside the entry (`last_normalize_raw_kernel_ms`);
  (b) for 'median': Engine.upload + run_stages(STAGE_SEGMENT) + sync on the same reads, and the kernel time the engine
      reports for its normalize and whole-segment steps (k_normalize and the event detection that is attached to it).
Before anything is timed the scale values of (a) 'median' are compared with the stage's, bit for bit.  Needs a GPU:
there is no fallback.  Reads nothing but this repository."""
import os
import sys
import json
import time
import argparse
import subprocess
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)

NORM_TYPES = ('none', 'pA_raw', 'median', 'median_const_scale', 'robust_median')


def spread(ts_):
    return dict(median=float(np.median(ts_)), min=float(min(ts_)), max=float(max(ts_)), all=[float(t) for t in ts_])


def child(a):
    from tombo_amd import _native, synth, tombo_stats as ts, tombo_helper as th, resquiggle as rq
    eng = rq.get_engine()   # raises without a GPU
    samp = th.seqSampleType('DNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    gen = _native.Synth(model, 0)
    _, raw_off, _, seq_off = gen.generate(_native.make_synth_params(**synth.DNA_SYNTH), 1, np.full(a.reads, a.bases),
                                          raw_dtype=np.int16)
    raw, seq = gen.download()
    raws = [raw[i:j] for i, j in zip(raw_off[:-1], raw_off[1:])]
    seqs = [seq[i:j] for i, j in zip(seq_off[:-1], seq_off[1:])]
    channel = [th.channelInfo(-3.0, 1437.5, 8192.0, 1, 4000.0)] * a.reads
    params = _native.make_params(ts.load_resquiggle_parameters(samp))
    opts = _native.make_opts(outlier_thresh=5.0)
    eng.ensure_model(model)

    def api(norm_type):
        return ts.normalize_raw_signal_batch(raws, norm_type=norm_type, outlier_thresh=5.0, channel_infos=channel,
                                             const_scale=37.25, engine=eng)

    def stage():
        eng.upload(params, opts, raws, seqs)
        eng.run_stages(_native.STAGE_SEGMENT, _native.STAGE_SEGMENT)
        eng.sync()

    stage()
    sv_stage = eng.get(_native.GET_SEG_SV)
    sv_api = np.array([[r[1].shift, r[1].scale, r[1].lower_lim, r[1].upper_lim] for r in api('median')])
    equal = bool(sv_api.tobytes() == np.ascontiguousarray(sv_stage[:, :4], dtype=np.float64).tobytes())
    results = {}
    for norm_type in NORM_TYPES:
        api(norm_type)
        wall, kern = [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter(); api(norm_type); wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(eng.last_normalize_raw_kernel_ms)
        results[norm_type] = dict(end_to_end_ms=spread(wall), kernel_ms=spread(kern))
    wall, k_norm, k_all = [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); stage(); wall.append((time.perf_counter() - t0) * 1e3)
        ms = eng.get(_native.GET_KERNEL_MS)
        k_norm.append(float(ms[_native.STAGE_NAMES.index('normalize')]))
        k_all.append(float(sum(ms[:_native.STAGE_NAMES.index('event_means')])))
    out = dict(
        what='normalize_raw_signal_batch of %d int16 reads x %d bases (%d samples), outlier_thresh 5' % (
            a.reads, a.bases, int(raw_off[-1])),
        reads=a.reads, bases_per_read=a.bases, samples=int(raw_off[-1]), rounds=a.rounds,
        median_scale_values_equal_stage_segment=equal, normalize_raw_signal_batch=results,
        stage_segment_median=dict(end_to_end_ms=spread(wall), kernel_ms_normalize=spread(k_norm),
                                  kernel_ms_segment_steps=spread(k_all)),
        end_to_end_what='host clock: packing, upload, kernels, download (the API also builds the per-read result list; '
                        'the stage also detects events and downloads nothing)',
        kernel_what='API: hipEvent time of k_norm_scale + k_norm_apply inside the entry; stage: the hipEvent times the '
                    'engine keeps per step')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
    if not equal:
        sys.exit('the scale values differ from the segmentation stage')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'norm_api_timing.json'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reads', type=int, default=200)
    ap.add_argument('--bases', type=int, default=10000)
    ap.add_argument('--timeout', type=int, default=300, help='seconds the GPU step may take')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child', '--out', a.out,
           '--rounds', str(a.rounds), '--reads', str(a.reads), '--bases', str(a.bases)]
    sys.exit(subprocess.call(cmd))


if __name__ == '__main__':
    main()

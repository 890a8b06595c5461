"""The observations-per-base ("stuck read") rule: the host loop of the worker against the engine's kernel.

    python tools/read_filter_timing.py [--out profiles/read_filter_timing.json]

10 000 synthetic DNA reads of 10 000 bases (drawn on the device, _native.Synth) are resquiggled as one resident
batch; the boundaries that batch gives are what all three forms work on, with the pairs [(99, 200), (100, 5000)]:
  (a) the host rule of mapping.filter_and_index_record: np.diff and one np.percentile per pair, read by read, one
      thread, wall time on this host;
  (b) Engine.dwell_pctl_flags on the same boundaries: the call (argument checks, upload of the boundaries, kernel,
      download of values and flags) by the host clock, the kernel by the hipEvents inside the entry;
  (c) Engine.batch_dwell_pctl_flags on the resident batch: the call and the kernel, beside the kernel time of the
      resquiggle pass that made the batch (TBA_GET_KERNEL_MS: its `total` slot and the sum of its steps).
In ONE process, after a warm-up of each form; the flags of the three forms are compared before anything is timed.
Needs a GPU: there is no fallback.  Reads nothing but this repository."""
import os
import sys
import json
import time
import argparse
import datetime

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)

from tombo_amd import _native, resquiggle as rq, synth, tombo_stats as ts, tombo_helper as th  # noqa: E402


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), all=[float(t) for t in v])


def host_rule(segs, off, pairs):
    """the parent's rule, read by read (mapping.filter_and_index_record)"""
    flags = np.zeros(off.shape[0] - 1, dtype=bool)
    for i in range(off.shape[0] - 1):
        base_lens = np.diff(segs[off[i]:off[i + 1]])
        flags[i] = any(np.percentile(base_lens, pctl) > thresh for pctl, thresh in pairs)
    return flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'read_filter_timing.json'))
    ap.add_argument('--reads', type=int, default=10000)
    ap.add_argument('--bases', type=int, default=10000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=3)
    a = ap.parse_args()
    pairs = [(99, 200), (100, 5000)]
    eng = rq.get_engine()   # raises without a GPU
    samp = th.seqSampleType('DNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)
    gen = _native.Synth(model, eng.device)
    raw, raw_off, seq, seq_off = gen.generate(_native.make_synth_params(**synth.DNA_SYNTH), 20261020,
                                              np.full(a.reads, a.bases, np.int64), raw_dtype=np.int16)
    eng.ensure_model(model)
    eng.upload_packed(_native.make_params(params),
                      _native.make_opts(outlier_thresh=5.0, seq_samp_type=samp, skip_norm_out=True, subsample_seed=7),
                      raw, raw_off, seq, seq_off, wait=True)
    eng.run()
    eng.sync()
    stage_ms = eng.get(_native.GET_KERNEL_MS)[:len(_native.STAGE_NAMES)]
    dl = eng.download(want_norm=False)
    ok = dl['status'] == 0
    off = np.ascontiguousarray(eng.seg_off, dtype=np.int64)
    segs = dl['segs'].copy()
    for i in np.flatnonzero(~ok):
        segs[off[i]:off[i + 1]] = 0     # (a failed read has no boundaries: one length-0 base per entry)
    # warm-up and agreement
    f_host = host_rule(segs, off, pairs)
    v_arr, f_arr = eng.dwell_pctl_flags(segs, off, pairs)
    v_res, f_res = eng.batch_dwell_pctl_flags(pairs)
    equal = bool(np.array_equal(f_host, f_arr) and np.array_equal(f_arr[ok], f_res[ok]) and
                 np.array_equal(v_arr[ok].view(np.int64), v_res[ok].view(np.int64)) and not f_res[~ok].any())
    t_host = []
    for _ in range(a.host_rounds):
        t0 = time.perf_counter(); host_rule(segs, off, pairs); t_host.append(time.perf_counter() - t0)
    t_arr, k_arr, t_res, k_res = [], [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); eng.dwell_pctl_flags(segs, off, pairs); t1 = time.perf_counter()
        k_arr.append(eng.last_filter_kernel_ms)
        eng.batch_dwell_pctl_flags(pairs); t2 = time.perf_counter()
        k_res.append(eng.last_filter_kernel_ms)
        t_arr.append(t1 - t0); t_res.append(t2 - t1)
    steps = dict(zip(_native.STAGE_NAMES, (float(x) for x in stage_ms)))
    out = dict(
        what='observations-per-base rule, pairs %s, on the boundaries of %d resquiggled synthetic reads of %d bases '
             '(%d boundaries, %d reads succeeded)' % (pairs, a.reads, a.bases, segs.shape[0], int(ok.sum())),
        date=datetime.date.today().isoformat(), reads=a.reads, bases=a.bases, pairs=pairs, rounds=a.rounds,
        flags_equal=equal, reads_flagged=int(f_host.sum()), boundary_bytes=int(segs.nbytes),
        a_host_rule_s=spread(t_host),
        a_what='np.diff + np.percentile per pair, read by read, one thread (mapping.filter_and_index_record)',
        b_array_call_ms=spread([t * 1e3 for t in t_arr]), b_array_kernel_ms=spread(k_arr),
        b_what='Engine.dwell_pctl_flags: argument checks, upload of the boundaries, kernel, download',
        c_resident_call_ms=spread([t * 1e3 for t in t_res]), c_resident_kernel_ms=spread(k_res),
        c_what='Engine.batch_dwell_pctl_flags on the resident batch: only the pairs are uploaded',
        resquiggle_pass_kernel_ms=dict(total=steps.get('total'), sum_of_steps=float(sum(
            v for k, v in steps.items() if k not in ('total', 'stalls'))), steps=steps),
        host_over_array_call=float(np.median(t_host) / np.median(t_arr)),
        host_over_resident_call=float(np.median(t_host) / np.median(t_res)),
        resident_kernel_share_of_pass=float(np.median(k_res) / steps['total']) if steps.get('total') else None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
    if not equal:
        sys.exit('the three forms differ')


if __name__ == '__main__':
    main()

"""Golden vectors of center_model_to_median_norm on RNA reads from the REFERENCE (build container only).

    python tests/golden/gen_golden_center_rna.py   # writes tests/golden/stats_center_rna.npz

Runs the live reference's center_model_to_median_norm (tombo/tombo_stats.py:1599-1705) with its RNA branch
(:1630-1634, get_event_scale_values :1603-1622): `h5py.File`, `th.get_raw_read_slot` and
`th.get_multiple_slots_read_centric` are pointed at in-memory arrays, as in gen_golden_kmer_est.py; everything
after that is the reference's own code.  Only data is written: the reads, the runs and the outputs.

The reference cannot take int16 here: identify_stalls allocates its metric in the signal's dtype and assigns NaN
(:312-313), a ValueError the bare `except` of the read loop swallows, so every RNA read is skipped.  As in
gen_golden_stalls.py the reference is handed the DAC values as float64; the fixture stores them as int16.

Reads, in read direction (the fixture stores the samples in acquisition order, reversed, as a FAST5 file has
them), levels at level * 70 + 450 DAC units with noise of sd 9 (the stall detector's threshold is 40 raw units):
    0-3  250-400 bases, 25-45 samples a base
    4    the same with a stall of 1500 samples inside one base
    5    1100 bases, 20-30 samples a base: 1098 points, its Theil-Sen points are drawn with np.random.choice
    6    1200 bases, 5-6 samples a base: fails in valid_cpts_w_cap_t_test ("Fewer changepoints found than
         requested"), BEFORE the fit, so it must not consume a draw although it has more than 1000 points
    7    a homopolymer of 200 bases over an ordinary signal: every expected level is equal, the slope is 0 and the
         read fails after the fit
    8    300 bases, 10-14 samples a base, mapped length 5 above its bases: compute_num_events takes
         int(map_len * 1.1), not the signal's share
Runs: all reads with max_reads above the successes (warning), below them, equal to them, and the two failing reads
alone (error).  Per run the seed, the factors handed to _center_model, the centred levels, the reads the reference
processed in order, those that reached the fit, those that drew, those that succeeded and their own factors (the
medians alone would hide a wrong draw on a read that is not the middle one).
"""
import os
import sys
import json
from itertools import product

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import ref_oracle  # noqa: E402

rq, ts, th = ref_oracle.load()

CENTER = {}     # read id -> {'raw' (float64, acquisition order), 'start', 'base'}
MESSAGES, FACTORS = [], []
TRACE = {'processed': [], 'fitted': [], 'drew': [], 'succeeded': [], 'read_factors': []}
N_READS = 9
FAILING = [6, 7]


class RefExit(Exception):
    pass


def _exit(msg):
    raise RefExit(msg)


class FakeFile(object):
    def __init__(self, fn, mode='r'):
        self.fn = fn

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class ReadsIndex(object):
    def __init__(self, reads):
        self.reads = reads

    def iter_reads(self):
        return iter(self.reads)


def install():
    ts.h5py.File = FakeFile

    def raw_slot(f):
        TRACE['processed'].append(int(f.fn[1:]))
        return {'Signal': CENTER[f.fn]['raw']}
    th.get_raw_read_slot = raw_slot
    th.get_multiple_slots_read_centric = lambda f, names, grp=None: [CENTER[f.fn][n] for n in names]
    real_center = ts.TomboModel._center_model

    def recording_center(self, shift, scale):
        FACTORS.append((float(shift), float(scale)))
        return real_center(self, shift, scale)
    ts.TomboModel._center_model = recording_center
    real_fit = ts.calc_kmer_fitted_shift_scale

    def recording_fit(*a, **kw):
        TRACE['fitted'].append(TRACE['processed'][-1])
        res = real_fit(*a, **kw)
        TRACE['succeeded'].append(TRACE['processed'][-1])
        TRACE['read_factors'].append([float(res[2]), float(res[3])])
        return res
    ts.calc_kmer_fitted_shift_scale = recording_fit
    real_choice = np.random.choice

    def recording_choice(*a, **kw):
        TRACE['drew'].append(TRACE['processed'][-1])
        return real_choice(*a, **kw)
    np.random.choice = recording_choice
    th.error_message_and_exit = _exit
    th.warning_message = MESSAGES.append


def make_reads(rng, level):
    specs = [(int(n), 25, 45, 0) for n in rng.integers(250, 401, 4)] + \
        [(int(rng.integers(250, 401)), 25, 45, 1500), (1100, 20, 30, 0), (1200, 5, 6, 0), (200, 25, 45, 0), (300, 10, 14, 0)]
    assert len(specs) == N_READS
    reads = []
    for i, (n, lo, hi, stall) in enumerate(specs):
        seq = 'A' * n if i == 7 else ''.join(rng.choice(list('ACGT'), n))
        sig_seq = ''.join(rng.choice(list('ACGT'), n)) if i == 7 else seq     # (the homopolymer's signal is an ordinary one)
        rsr = int(rng.integers(20, 60))
        dwell = rng.integers(lo, hi + 1, n)
        lv = np.array([level.get(sig_seq[max(j - 1, 0):j + 2], 0.0) for j in range(n)]) * 70.0 + 450.0 + rng.normal(0, 3.0, n)
        if stall:
            dwell[n // 2] += stall
        body = np.repeat(lv, dwell) + rng.normal(0, 9.0, int(dwell.sum()))
        if stall:
            at = int(dwell[:n // 2].sum()) + 10
            body[at:at + stall] = lv[n // 2] + rng.normal(0, 2.0, stall)
        sig = np.round(np.concatenate([rng.normal(450, 60, rsr), body, rng.normal(450, 60, 25)])).astype(np.int16)
        start = np.concatenate([[0], np.cumsum(dwell)[:-1]]).astype(np.uint32)
        map_len = n + 5 if i == 8 else n
        rid = 'c%d' % i
        CENTER[rid] = {'raw': sig[::-1].astype(np.float64), 'dac': sig[::-1].copy(), 'start': start,
                       'base': np.frombuffer(seq.encode(), dtype='S1'), 'rsr': rsr, 'map_len': map_len}
        reads.append(th.readData(100, 100 + map_len, False, rsr, '+', rid, 'grp', True, 0.0, 10.0, rid))
    return reads


def run(meta, out, level, kmers3, reads, name, sel, seed, max_reads):
    del MESSAGES[:], FACTORS[:]
    for v in TRACE.values():
        del v[:]
    model = ts.TomboModel(kmer_ref=[(k, level[k], 0.2) for k in kmers3], central_pos=1)
    np.random.seed(seed)
    rec = dict(name=name, reads=sel, seed=seed, max_reads=max_reads, error=None, factors=None)
    try:
        ts.center_model_to_median_norm(ReadsIndex([reads[i] for i in sel]), model, max_reads)
        rec['factors'] = list(FACTORS[0])
        out['run_' + name + '_means'] = np.array([model.means[k] for k in kmers3])
    except RefExit as e:
        rec['error'] = str(e)
    rec['warning'] = MESSAGES[0] if MESSAGES else None
    rec.update((k, list(v)) for k, v in TRACE.items())
    rec['skipped'] = [i for i in rec['processed'] if i not in rec['succeeded']]
    print('%-22s seed %d factors %s warning %s error %s\n    processed %s drew %s skipped %s' % (
        name, seed, rec['factors'], bool(rec['warning']), rec['error'], rec['processed'], rec['drew'], rec['skipped']))
    meta['runs'].append(rec)
    return rec


def main():
    install()
    rng = np.random.default_rng(2110)
    kmers3 = [''.join(p) for p in product('ACGT', repeat=3)]
    level = dict(zip(kmers3, (rng.permutation(np.linspace(-2.4, 2.4, 64)) + rng.normal(0, 0.02, 64)).tolist()))
    reads = make_reads(rng, level)
    rows = [CENTER['c%d' % i] for i in range(N_READS)]
    out = {
        'init': np.array([(level[k], 0.2) for k in kmers3]),
        'rsr': np.array([c['rsr'] for c in rows], dtype=np.int32),
        'map_len': np.array([c['map_len'] for c in rows], dtype=np.int32),
        'raw_off': np.concatenate([[0], np.cumsum([len(c['dac']) for c in rows])]).astype(np.int32),
        'raw': np.concatenate([c['dac'] for c in rows]),
        'off': np.concatenate([[0], np.cumsum([len(c['start']) for c in rows])]).astype(np.int32),
        'start': np.concatenate([c['start'] for c in rows]),
        'seq': np.frombuffer(b''.join(c['base'].tobytes() for c in rows), dtype=np.uint8),
    }
    assert out['raw'].dtype == np.int16
    meta = {'runs': []}
    everything = list(range(N_READS))
    n_ok = N_READS - len(FAILING)
    # the seeds: under 3 the shuffle puts read 6 (no change points, more than 1000 points) before read 5 (drawn)
    runs = [run(meta, out, level, kmers3, reads, *spec) for spec in (
        ('all_reads', everything, 3, 50), ('first_three', everything, 3, 3),
        ('max_equals_successes', everything, 4, n_ok), ('only_the_failing_reads', FAILING, 3, 50))]
    by = dict((r['name'], r) for r in runs)
    a = by['all_reads']
    assert sorted(a['succeeded']) == [i for i in everything if i not in FAILING], 'the number of successes'
    assert sorted(a['skipped']) == FAILING and a['drew'] == [5] and 6 not in a['fitted'] and 7 in a['fitted']
    assert a['processed'].index(6) < a['processed'].index(5), 'the read without change points must come before the drawn one'
    assert a['warning'] and not by['first_three']['warning'] and not by['max_equals_successes']['warning']
    assert by['only_the_failing_reads']['error'] and a['factors'] != by['first_three']['factors']
    drawn = [r['read_factors'][r['succeeded'].index(5)] for r in (a, by['max_equals_successes'])]
    assert drawn[0] != drawn[1], 'another seed, another draw: the factors of the drawn read must tell'
    assert len(by['first_three']['succeeded']) == 3 and len(by['first_three']['processed']) < N_READS
    assert len(by['max_equals_successes']['succeeded']) == n_ok
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'stats_center_rna.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()

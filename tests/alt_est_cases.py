"""TEST INFRASTRUCTURE: the recorded cases of tests/golden/stats_alt_est.npz (written by
tests/golden/gen_golden_alt_est.py from the live reference) as the objects the alternate-model
estimation takes, and the comparisons the CPU and GPU tests share."""
import os
import json

import numpy as np

from tombo_amd import tombo_stats as ts, tombo_helper as th

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stats_alt_est.npz'))
META = json.loads(str(GOLD['meta']))
K, CP = META['kmer_width'], META['central_pos']
KMERS = ts._all_kmers(K)
SAVE_X = np.linspace(-5, 5, 500)
SAVE_G = np.linspace(-5, 5, META['g_est'])
PARSE_CASES = dict((c['name'], c) for c in META['parse_cases'])


def std_ref():
    return ts.TomboModel(kmer_ref=list(zip(KMERS, GOLD['model_means'].tolist(), GOLD['model_sds'].tolist())),
                         central_pos=CP)


def reads(name):
    off, seq, means = GOLD[name + '_off'], GOLD[name + '_seq'].tobytes().decode(), GOLD[name + '_means']
    return [th.resquiggledRead(0, int(b - a), False, 0, '+', None, None, False, read_id='%s%d' % (name, i),
                               means=means[a:b], seq=seq[a:b])
            for i, (a, b) in enumerate(zip(off[:-1].tolist(), off[1:].tolist()))]


def parse_case(name, engine):
    c = PARSE_CASES[name]
    return ts.parse_base_levels(reads(c['reads']), std_ref(), c['batch'], c['kmer_obs_thresh'],
                                c['max_kmer_obs'], c['min_kmer_obs_to_est'], engine=engine)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_levels_bit_equal(got, name):
    levels, lv_off = got
    assert np.array_equal(lv_off, GOLD[name + '_lv_off'])
    assert np.array_equal(bits(levels), bits(GOLD[name + '_levels']))   # same levels in the same order


def assert_density_close(got, want):
    """1e-12 relative where the recorded density is at least 1e-10 (the cut below which
    isolate_alt_density ignores a density), 1e-20 absolute elsewhere"""
    assert got.shape == want.shape
    big = want >= 1e-10
    rel = np.abs(got[big] - want[big]) / want[big]
    ab = np.abs(got[~big] - want[~big])
    print('density: max relative %.3g above the cut, max absolute %.3g below' %
          (rel.max() if rel.size else 0.0, ab.max() if ab.size else 0.0))
    assert np.all(rel <= 1e-12), rel.max()
    assert np.all(ab <= 1e-20), ab.max()


def assert_model_close(alt_ref, table):
    """an AltModel against a recorded (kmer, pos, mean, sd) table: same entries in the same order,
    levels to 1e-12 relative"""
    assert [(k, p) for k, p in alt_ref.means] == [(r['kmer'].decode(), int(r['pos'])) for r in table]
    got = np.array([alt_ref.means[kp] for kp in alt_ref.means])
    assert np.all(np.abs(got - table['mean']) <= 1e-12 * np.abs(table['mean'])), np.max(np.abs(got - table['mean']))
    assert np.array_equal(np.array([alt_ref.sds[kp] for kp in alt_ref.sds]), table['sd'])


def estimate(engine, **files):
    """estimate_alt_model as the generator ran the reference"""
    e = META['est_kernel_density']
    return ts.estimate_alt_model(
        reads('alt'), reads('ctrl'), std_ref(), META['alt_base'], META['alt_frac_pctl'], e['kmer_obs_thresh'],
        files.get('density_basename'), META['bw_est'], files.get('alt_dens_fn'), files.get('std_dens_fn'),
        num_dens_points=META['g_est'], engine=engine, shuffle=False,
        parse_levels_batch_size=e['parse_levels_batch_size'], max_kmer_obs=e['max_kmer_obs'],
        min_kmer_obs_to_est=e['min_kmer_obs_to_est'])

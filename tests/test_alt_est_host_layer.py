"""Argument checks and batching rules of the alternate-model estimation's host layer (no GPU): the
checks the binding makes before anything becomes a device address, on the numpy stand-in engine."""
import numpy as np
import pytest

from tombo_amd import _native, tombo_stats as ts, tombo_helper as th, _default_parameters as dp
import alt_est_cases as ac
from alt_est_stub_engine import AltEstStubEngine


def _args(**kw):
    a = dict(means=np.zeros(7), codes=np.zeros(7, dtype=np.uint8), read_off=np.array([0, 3, 7], dtype=np.int64),
             kmer_width=3, central_pos=1, completed=np.zeros(64, dtype=np.uint8))
    a.update(kw)
    return a


def test_abi_version_and_symbols():
    assert _native.ABI_VERSION == 13
    hdr = open(_native.os.path.join(_native._HERE, '..', 'include', 'tombo_amd.h')).read()
    assert '#define TBA_ABI_VERSION 13' in hdr and 'int tba_kmer_levels(' in hdr and 'int tba_kde_eval(' in hdr
    assert callable(_native.Engine.kmer_levels) and callable(_native.Engine.kde_eval)


@pytest.mark.parametrize('bad', [
    dict(means=np.zeros(7, dtype=np.float32)), dict(codes=np.zeros(7, dtype=np.int8)),
    dict(completed=np.zeros(64, dtype=bool)), dict(read_off=np.array([0, 3, 7], dtype=np.int32)),
    dict(read_off=np.array([0, 5, 3, 7], dtype=np.int64)), dict(read_off=np.array([1, 3, 7], dtype=np.int64)),
    dict(read_off=np.array([0, 3, 8], dtype=np.int64)), dict(central_pos=3), dict(central_pos=-1),
    dict(kmer_width=0), dict(kmer_width=11), dict(completed=np.zeros(16, dtype=np.uint8)),
    dict(codes=np.zeros(6, dtype=np.uint8))])
def test_kmer_levels_rejects(bad):
    with pytest.raises(ValueError):
        AltEstStubEngine().kmer_levels(**_args(**bad))


@pytest.mark.parametrize('bad', [
    dict(levels=np.zeros(4, dtype=np.float32)), dict(x=np.zeros(3, dtype=np.float32)),
    dict(lv_off=np.array([0, 3, 2, 4], dtype=np.int64)), dict(lv_off=np.array([0, 2, 5], dtype=np.int64)),
    dict(lv_off=np.array([0.0, 4.0])), dict(bandwidth=0.0), dict(bandwidth=-1.0), dict(bandwidth=np.inf),
    dict(bandwidth=np.nan)])
def test_kde_eval_rejects(bad):
    a = dict(levels=np.zeros(4), lv_off=np.array([0, 2, 4], dtype=np.int64), x=np.zeros(3), bandwidth=0.05)
    a.update(bad)
    with pytest.raises(ValueError):
        AltEstStubEngine().kde_eval(**a)


def test_kmer_levels_stub_windows():
    """window i pairs with the level central_pos + i; N windows and completed k-mers are skipped; a NaN
    level is kept; reads shorter than K contribute nothing"""
    seqs = ['ACGTA', 'AC', 'ACG', 'ACNACG']
    codes = np.concatenate([ts.encode_seq(s) for s in seqs])
    means = np.arange(codes.shape[0], dtype=np.float64)
    means[1] = np.nan
    off = ts._csr_offsets([len(s) for s in seqs])
    done = np.zeros(64, dtype=np.uint8)
    done[ts.TomboModel._kmer_code('CGT')] = 1
    counts, levels, lv_off = AltEstStubEngine().kmer_levels(means, codes, off, 3, 1, done)
    acg, gta = ts.TomboModel._kmer_code('ACG'), ts.TomboModel._kmer_code('GTA')
    assert counts.sum() == 4 and counts[acg] == 3 and counts[gta] == 1
    got = levels[lv_off[acg]:lv_off[acg + 1]]
    assert np.isnan(got[0]) and got[1:].tolist() == [8.0, 14.0]
    assert levels[lv_off[gta]] == 3.0


def test_reads_without_levels_and_mismatched_reads():
    ref = ac.std_ref()
    rd = ac.reads('edge')
    none = th.resquiggledRead(0, 5, False, 0, '+', None, None, False, read_id='x')
    a = ts._kmer_levels_batch(rd[:4] + [none], ac.K, ac.CP, np.zeros(64, dtype=np.uint8), AltEstStubEngine())
    b = ts._kmer_levels_batch(rd[:4], ac.K, ac.CP, np.zeros(64, dtype=np.uint8), AltEstStubEngine())
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    bad = rd[0]._replace(seq=rd[0].seq[:-1])
    with pytest.raises(ValueError):
        ts.parse_base_levels([bad], ref, 10, 1, 10, 0, engine=AltEstStubEngine())
    with pytest.raises(ValueError):
        ts.parse_base_levels(rd, ref, 0, 1, 10, 0, engine=AltEstStubEngine())


def test_est_kernel_density_needs_two_observations_and_is_one_call():
    ref = ac.std_ref()
    eng = AltEstStubEngine()
    with pytest.warns(UserWarning), pytest.raises(th.TomboError, match='at least two observations'):
        ts.est_kernel_density(ac.reads('edge')[:1], ref, 5, None, ac.SAVE_G, 0.05, min_kmer_obs_to_est=0,
                              engine=eng, shuffle=False)
    eng = AltEstStubEngine()
    dens = ts.est_kernel_density(ac.reads('ctrl'), ref, 50, None, ac.SAVE_G, 0.08, parse_levels_batch_size=20,
                                 engine=eng, shuffle=False)
    assert list(dens) == ac.KMERS and [k for k, _ in eng.calls].count('kde_eval') == 1
    assert eng.calls[-1] == ('kde_eval', 64)


def test_default_parameters():
    assert (dp.ALT_EST_BATCH, dp.MAX_KMER_OBS, dp.MIN_KMER_OBS_TO_EST, dp.KERNEL_DENSITY_RANGE, dp.ALT_EST_PCTL,
            dp.NUM_DENS_POINTS, dp.KERNEL_DENSITY_BW) == (1000, 10000, 50, (-5, 5), 5, 500, 0.05)

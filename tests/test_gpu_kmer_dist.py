"""`tombo plot kmer` on the device (csrc/k_kmer_dist.h, tba_kmer_dist) against the live reference's recorded frames
(tests/golden/stats_kmer_dist.npz) and against the numpy restatement (tests/kmer_dist_reference.py).  No tolerance
anywhere: labels, counts, offsets, values and means are compared by bits."""
import ctypes as C

import numpy as np
import pytest

from tombo_amd import _native, resquiggle as rq
import kmer_dist_cases as kc
import kmer_dist_reference as kr
import model_overlay_cases as mc

pytestmark = pytest.mark.gpu
NAMES = ('read_label', 'n_sel', 'n_examined', 'counts', 'off', 'values', 'value_label', 'kmer_mean')


def assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                                  w.view(np.uint64) if w.dtype == np.float64 else w), name
        else:
            assert g == w, name


@pytest.mark.parametrize('case', kc.kmer_cases(), ids=lambda c: c['name'])
def test_recorded_case(case):
    eng = rq.get_engine()
    eng.last_kmer_dist_kernel_ms = 0.0
    kc.check_case(case, eng)
    if any(r.means is not None for r in kc.case_reads(case)):
        assert eng.last_kmer_dist_kernel_ms > 0


@pytest.mark.parametrize('case', mc.meta()['body_cases'], ids=lambda c: c['name'])
def test_model_overlay_and_per_read_bodies_on_the_device(case):
    """the frames of plot_model_single_sample, plot_motif_centered_with_stats and plot_per_read_modification with
    their numbers (level piles, raw signal, read order) from the real engine"""
    mc.check_body_case(case, rq.get_engine())


def _seq(rng, n):
    return ''.join('ACGT'[i] for i in rng.integers(0, 4, n))


def edge_reads(rng, K):
    """reads of K - 1, K, K + 63 .. K + 65 bases, of one chunk (4096 positions) - 1, + 0, + 1 and of three chunks
    and more, homopolymer reads whose one segment holds 1, 7, 8, 9, 128, 129 and 9000 levels"""
    seqs = [_seq(rng, n) for n in (K - 1, K, K + 63, K + 64, K + 65, 4095, 4096, 4097, 3 * 4096 + 17)]
    seqs += ['ACGT'[i % 4] * (n + K - 1) for i, n in enumerate((1, 7, 8, 9, 128, 129, 9000))]
    return [(rng.standard_normal(len(s)) * 2 + 80, s) for s in seqs]


@pytest.mark.parametrize('K,cp', [(1, 0), (2, 1), (4, 2), (6, 0)])
@pytest.mark.parametrize('read_mean', [True, False])
def test_edge_sizes_against_the_restatement(K, cp, read_mean):
    rng = np.random.default_rng(100 + K)
    args = kr.pack_reads(edge_reads(rng, K)) + (K, cp, 0, 100, read_mean)
    before = [a.copy() for a in args[:3]]
    want = kr.kmer_dist(*args)
    assert want[1] == 16 and want[3].max() > (1 if read_mean else 8192)
    eng = rq.get_engine()
    got, again = eng.kmer_dist(*args), eng.kmer_dist(*args)
    assert_same(got, want)
    assert_same(again, want)
    assert all(g.tobytes() == a.tobytes() for g, a in zip(got, again) if isinstance(g, np.ndarray))
    assert all(np.array_equal(a, b) for a, b in zip(args[:3], before))
    assert eng.last_kmer_dist_kernel_ms > 0


@pytest.mark.parametrize('K,thresh', [(1, 1), (2, 1), (2, 5), (3, 2)])
@pytest.mark.parametrize('read_mean', [True, False])
def test_rejected_reads_between_accepted_ones(K, thresh, read_mean):
    rng = np.random.default_rng(200 + K + thresh)
    reads = []
    for i in range(12):
        n = int(rng.integers(40, 90)) if i % 3 == 1 else int(rng.integers(2000, 9000))
        reads.append((rng.standard_normal(n), _seq(rng, n)))
    reads[4] = (reads[4][0], reads[4][1].replace('A', 'C'))
    args = kr.pack_reads(reads) + (K, K - 1, thresh, 7, read_mean)
    want = kr.kmer_dist(*args)
    label = want[0]
    assert want[1] == 7 and (label[:np.flatnonzero(label)[-1]] == 0).any() and want[2] < 12
    assert_same(rq.get_engine().kmer_dist(*args), want)


def test_k9_three_short_reads():
    rng = np.random.default_rng(9)
    args = kr.pack_reads([(rng.standard_normal(n), _seq(rng, n)) for n in (8, 9, 75)]) + (9, 4, 0, 3, True)
    want = kr.kmer_dist(*args)
    assert want[1] == 3 and want[3].sum() >= 67
    assert_same(rq.get_engine().kmer_dist(*args), want)
    assert_same(rq.get_engine().kmer_dist(*(args[:-1] + (False,))), kr.kmer_dist(*(args[:-1] + (False,))))


@pytest.mark.parametrize('num_reads,last', [(50, 69), (0, 0), (10 ** 6, 299), (None, 299)])
def test_selection_rule(num_reads, last):
    """300 reads, two in seven without a T; num_reads reached at read 70, at the first read, never, at the last read"""
    rng = np.random.default_rng(3)
    reads = []
    for i in range(300):
        s = _seq(rng, 30) + 'ACGT'
        reads.append((rng.standard_normal(34), s.replace('T', 'G') if i % 7 in (2, 5) or i == 299 else s))
    if num_reads is None:
        reads[299] = (reads[299][0], reads[298][1])
        num_reads = sum('T' in s for _, s in reads)
    packed = kr.pack_reads(reads)
    want = kr.kmer_dist(*packed, 1, 0, 1, num_reads, True)
    got = rq.get_engine().kmer_dist(*packed, 1, 0, 1, num_reads, True)
    assert_same(got, want)
    assert got[2] == last + 1 and (got[0][last + 1:] == 0).all()
    valid = np.array(['T' in s for _, s in reads])
    assert np.array_equal(got[0][:last + 1] > 0, valid[:last + 1])


def _raw_call(eng, means, codes, off, n_reads, K, cp, thresh=0, num_reads=3, read_mean=1, fill=False, cap=0, label=True):
    n_kmers = 4 ** min(max(int(K), 1), 9)
    out = dict(label=np.zeros(max(n_reads, 1), dtype=np.int64), counts=np.zeros(n_kmers, dtype=np.int64),
               off=np.zeros(n_kmers + 1, dtype=np.int64), values=np.zeros(max(cap, 1)), vlabel=np.zeros(max(cap, 1), dtype=np.int64),
               kmean=np.zeros(n_kmers))
    n_sel, n_exam, ms = C.c_int64(-5), C.c_int64(-5), C.c_double(-1.0)
    rc = eng._L.tba_kmer_dist(eng._h, means, codes, off, n_reads, K, cp, thresh, num_reads, read_mean,
                              out['label'] if label else None, C.byref(n_sel), C.byref(n_exam), out['counts'], out['off'],
                              out['values'] if fill else None, out['vlabel'] if fill else None, cap,
                              out['kmean'] if fill else None, C.byref(ms))
    return rc, n_sel.value, n_exam.value, out


def test_empty_input_and_argument_errors():
    eng = rq.get_engine()
    m, c, off = np.arange(8) * 0.5, np.zeros(8, dtype=np.uint8), np.array([0, 3, 8], dtype=np.int64)
    rc, n_sel, n_exam, out = _raw_call(eng, None, None, np.zeros(1, dtype=np.int64), 0, 2, 1, fill=True)
    assert (rc, n_sel, n_exam) == (0, 0, 0) and not out['counts'].any() and not out['off'].any()
    assert np.isnan(out['kmean']).all()
    got = eng.kmer_dist(np.empty(0), np.empty(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), 2, 1, 0, 3, True)
    assert got[1:3] == (0, 0) and got[5].shape == (0,) and np.isnan(got[7]).all()
    # reads without bases are still taken under kmer_thresh 0
    got = eng.kmer_dist(np.empty(0), np.empty(0, dtype=np.uint8), np.zeros(4, dtype=np.int64), 2, 1, 0, 2, False)
    assert got[0].tolist() == [1, 2, 0] and got[1:3] == (2, 2) and not got[3].any()
    E_ARG = -1
    big = np.array([0, 2 ** 31], dtype=np.int64)
    many = np.zeros(2 ** 27 // 4 ** 9 + 2, dtype=np.int64)
    bad = [
        dict(means=None, codes=c, off=off, n_reads=2, K=2, cp=1), dict(means=m, codes=None, off=off, n_reads=2, K=2, cp=1),
        dict(means=m, codes=c, off=None, n_reads=2, K=2, cp=1), dict(means=m, codes=c, off=off, n_reads=2, K=2, cp=1, label=False),
        dict(means=m, codes=c, off=np.array([1, 3, 8], dtype=np.int64), n_reads=2, K=2, cp=1),
        dict(means=m, codes=c, off=np.array([0, 5, 3], dtype=np.int64), n_reads=2, K=2, cp=1),
        dict(means=m, codes=c, off=off, n_reads=-1, K=2, cp=1),
        dict(means=m, codes=c, off=off, n_reads=2, K=0, cp=0), dict(means=m, codes=c, off=off, n_reads=2, K=10, cp=0),
        dict(means=m, codes=c, off=off, n_reads=2, K=2, cp=2), dict(means=m, codes=c, off=off, n_reads=2, K=2, cp=-1),
        dict(means=m, codes=c, off=big, n_reads=1, K=2, cp=1),
        dict(means=m, codes=c, off=many, n_reads=many.shape[0] - 1, K=9, cp=0),
        dict(means=m, codes=c, off=off, n_reads=2, K=2, cp=1, fill=True, cap=4),       # 6 values
        dict(means=m, codes=c, off=off, n_reads=2, K=2, cp=1, fill=True, cap=-1),
    ]
    for kw in bad:
        rc, _, _, _ = _raw_call(eng, kw.pop('means'), kw.pop('codes'), kw.pop('off'), kw.pop('n_reads'), kw.pop('K'),
                                kw.pop('cp'), read_mean=0, **kw)
        assert rc == E_ARG, kw
        assert eng._L.tba_last_error()
    rc, n_sel, n_exam, out = _raw_call(eng, m, c, off, 2, 2, 1, read_mean=0, fill=True, cap=6)
    assert (rc, n_sel, n_exam) == (0, 2, 2) and out['off'][-1] == 6     # the engine is usable afterwards
    assert np.array_equal(out['values'], m[[1, 2, 4, 5, 6, 7]]) and out['vlabel'].tolist() == [1, 1, 2, 2, 2, 2]

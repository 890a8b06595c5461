"""K-mer model estimation on the device (csrc/k_kmer_est.h) against the live reference
(tests/golden/stats_kmer_est.npz, written by gen_golden_kmer_est.py) under the parity rule of kmer_est_cases:
bit for bit against the reference run with a stable sort in get_reads_events (read order, the order the device
uses); against the reference as it is, counts and medians bit for bit and the order-dependent columns within four
times the spread recorded between the two reference runs."""
import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq
import kmer_est_cases as kc
import kmer_est_reference as kr
import kmer_est_stub_engine as stub

pytestmark = pytest.mark.gpu

TABULATED = ['canon_med', 'canon_mean', 'canon_cs', 'canon_clean', 'motif_cg']
# segments of both sides of the wavefront (64) and workgroup (4096) sorter classes, a big one between small ones
SEG_SIZES = [0, 1, 2, 63, 64, 65, 4095, 12003, 4096, 4097, 7, 0, 10]


def same_table(a, b):
    return list(a.keys) == list(b.keys) and np.array_equal(a.off, b.off) and \
        np.array_equal(kc.bits(a.levels), kc.bits(b.levels)) and np.array_equal(kc.bits(a.sds), kc.bits(b.sds))


@pytest.mark.parametrize('name', sorted(kc.CASES))
def test_extract_matches_the_reference_lists(name):
    """every recorded case (kmer_est_cases.CASES: medians and means, subsampled reads, the 4-mer with unequal
    flanks, both motifs, the deep pile), twice: the runs are bit-equal"""
    got, again = kc.extract(name, None), kc.extract(name, None)
    kc.assert_table(got, name)
    assert same_table(got, again)


@pytest.mark.parametrize('name', sorted(kc.CASES))
def test_tabulate_matches_the_reference(name):
    c = kc.CASES[name]
    table = kc.extract(name, None)
    if name in TABULATED:
        kc.assert_tabulated(kc.tabulate(table, name, None), name)
        return
    with pytest.raises(th.TomboError) as err:
        kc.tabulate(table, name, None)
    if c['error'] == 'NameError':   # the reference dies here; the message it meant, with the least count
        assert str(err.value) == ts._FEW_OBS_MSG % int(np.diff(table.off).min())
    else:
        assert str(err.value) == c['error']


@pytest.mark.parametrize('name', ['canon_mean', 'motif_cg', 'deep_med'])
def test_one_region_per_call_gives_the_same_table(name):
    class Counting(object):
        def __init__(self, eng):
            self.eng, self.calls = eng, 0

        def __getattr__(self, attr):
            return getattr(self.eng, attr)

        def region_key_levels(self, *a):
            self.calls += 1
            return self.eng.region_key_levels(*a)
    one, each = Counting(rq.get_engine()), Counting(rq.get_engine())
    together, apart = kc.extract(name, one), kc.extract(name, each, max_levels=1)
    assert one.calls == 1 and each.calls > 1
    assert same_table(together, apart)


def random_call(rng, n_reads, n_regions, n_keys, n_pos, n_ent, est_mean):
    lens = rng.integers(1, 60, n_reads)
    off = ts._csr_offsets(lens)
    means = rng.normal(0, 1, int(off[-1]))
    means[rng.random(means.shape[0]) < 0.002] = np.nan
    per_reg = [rng.permutation(n_reads)[:rng.integers(0, min(n_reads, 90))] for _ in range(n_regions)]
    ek = rng.integers(0, n_keys, n_ent)
    ek[rng.random(n_ent) < 0.6] = n_keys // 3     # one very common key
    return (est_mean, rng.integers(0, 200, n_reads).astype(np.int64), (rng.random(n_reads) < 0.5).astype(np.uint8),
            off, means, ts._csr_offsets([len(p) for p in per_reg]), np.concatenate(per_reg).astype(np.int64),
            rng.integers(0, n_regions, n_pos).astype(np.int64), rng.integers(-5, 265, n_pos).astype(np.int64),
            rng.integers(0, n_pos, n_ent).astype(np.int64), ek.astype(np.int64), n_keys)


@pytest.mark.parametrize('est_mean,n_keys,n_ent', [(False, 64, 9001), (True, 1000, 4097), (False, 1, 130), (True, 5, 0),
                                                   (False, 2, 4096), (True, 5, 8192)])
def test_region_key_levels_against_the_numpy_form(est_mean, n_keys, n_ent):
    """several chunks of entries (4096 each: one and two that are exactly full among them), a key most entries share,
    keys nobody uses, one key (no key bits) and a key count that is no power of two, positions no read covers,
    regions without reads: counts, offsets and both columns bit-equal to the definition written out in numpy"""
    eng = rq.get_engine()
    args = random_call(np.random.default_rng(n_keys + n_ent), 300, 9, n_keys, 700, n_ent, est_mean)
    want = stub.region_key_levels(*args[:-1], n_keys=n_keys)
    for _ in range(2):
        got = eng.region_key_levels(*args)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(kc.bits(got[2]), kc.bits(want[2])) and np.array_equal(kc.bits(got[3]), kc.bits(want[3]))


def test_region_key_levels_checks_its_arguments_first():
    eng = rq.get_engine()
    args = list(random_call(np.random.default_rng(3), 20, 2, 8, 30, 40, False))
    for i, bad in ((6, np.full_like(args[6], 20)), (7, np.full_like(args[7], 2)), (9, np.full_like(args[9], 30)),
                   (10, np.full_like(args[10], 8)), (10, args[10].astype(np.int32)), (4, args[4][:-1])):
        broken = list(args)
        broken[i] = bad
        with pytest.raises(ValueError):
            eng.region_key_levels(*broken)


def test_c_entry_refuses_indices_outside_the_batch():
    """the C entry checks every index again, for callers that do not come through the binding: reg_reads, pos_reg,
    ent_pos, ent_key out of range and offsets that do not start at 0 give TBA_E_ARG before anything reaches the
    device"""
    import ctypes as C
    from tombo_amd._native import i64, f64
    _p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    eng = rq.get_engine()
    good = [np.ascontiguousarray(a) for a in random_call(np.random.default_rng(4), 20, 2, 8, 30, 40, False)[1:11]]
    rs, rm, off, m, roff, rr, pr, pg, ep, ek = good

    def call(rs, rm, off, m, roff, rr, pr, pg, ep, ek, n_keys=8):
        counts, koff = np.empty(n_keys, np.int64), np.empty(n_keys + 1, np.int64)
        lv, sd = np.empty(ep.shape[0]), np.empty(ep.shape[0])
        return eng._L.tba_region_key_levels(
            eng._h, C.c_int(0), i64(rs.shape[0]), _p(rs, i64), _p(rm, C.c_uint8), _p(off, i64), _p(m, f64),
            i64(roff.shape[0] - 1), _p(roff, i64), _p(rr, i64), i64(pr.shape[0]), _p(pr, i64), _p(pg, i64),
            i64(ep.shape[0]), _p(ep, i64), _p(ek, i64), i64(n_keys), _p(counts, i64), _p(koff, i64), _p(lv, f64),
            _p(sd, f64))
    assert call(*good) == 0
    for i, bad in ((5, np.full_like(rr, 20)), (5, np.full_like(rr, -1)), (6, np.full_like(pr, 2)), (8, np.full_like(ep, 30)),
                   (9, np.full_like(ek, 8)), (9, np.full_like(ek, -1)), (2, off + 1), (4, roff[::-1].copy())):
        broken = list(good)
        broken[i] = bad
        assert call(*broken) != 0, i
    assert call(*good, n_keys=0) != 0


def test_segment_medians_every_segment_size():
    eng = rq.get_engine()
    rng = np.random.default_rng(1454)
    segs = [rng.normal(rng.uniform(-2, 2), 1.0, n) for n in SEG_SIZES]
    segs[10][3] = np.nan
    values, off = np.concatenate(segs), ts._csr_offsets(SEG_SIZES)
    before = values.copy()
    got, again = eng.segment_medians(values, off), eng.segment_medians(values, off)
    want = kr.medians(values, off)
    assert np.isnan(want[[0, 10, 11]]).all() and not np.isnan(np.delete(want, [0, 10, 11])).any()
    assert got.dtype == np.float64 and np.array_equal(kc.bits(got), kc.bits(want))
    assert np.array_equal(kc.bits(got), kc.bits(again))
    assert np.array_equal(kc.bits(values), kc.bits(before))     # the input is not sorted in place
    assert eng.segment_medians(np.empty(0), np.zeros(1, dtype=np.int64)).shape == (0,)
    with pytest.raises(ValueError):
        eng.segment_medians(values, off[:-1])


@pytest.mark.parametrize('name', sorted(kc.CENTER_RUNS))
def test_centring_gives_the_reference_factors(name):
    """center_model_to_median_norm on slices of the resident pipeline: eight reads of 150-400 bases, one of 1200
    (its points are drawn), one whose slope is 0; max_reads below, at and above the number of successes; no
    success at all.  Factors and centred levels bit for bit (they do not depend on the sort of the parity rule)"""
    kc.assert_centring(name, None)


def test_estimators_end_to_end():
    """estimate_kmer_model (tabulated, centred on the recorded reads; k-mer specific and constant sd) and
    estimate_motif_alt_model give the models the reference's lines give, and write_model leaves the tree the
    reference's writer leaves"""
    kc.assert_models(kc.end_to_end_models(None))

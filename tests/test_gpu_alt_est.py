"""Alternate-model estimation on the device (csrc/k_kde.h: k_key_partition over KmerSrc / k_kde_eval) against the live
reference (tests/golden/stats_alt_est.npz, written by gen_golden_alt_est.py).

The gather has no tolerance: counts and levels are bit-equal and in the reference's order.  Densities:
1e-12 relative where the recorded scipy density is at least 1e-10 (below that isolate_alt_density
ignores a density), 1e-20 absolute elsewhere; a direct float64 evaluation of the same sum differs from
scipy by 8.5e-14 relative on these segments (recorded in the golden file).  The generator asserts that
no discrete step of isolate_alt_density is within 1e-9 of flipping, so the final levels are compared at
1e-12 relative."""
import warnings

import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, resquiggle as rq
import alt_est_cases as ac
import alt_est_stub_engine as stub

pytestmark = pytest.mark.gpu

# sizes of the recorded segments: both sides of the wavefront (64) and workgroup (4096) sorter classes
SEG_SIZES = [2, 63, 64, 65, 4095, 4096, 4097, 12003, 342, 200]


@pytest.mark.parametrize('name', ['a_overshoot', 'a2_batch_of_7', 'b_reads_run_out'])
def test_kmer_levels_match_the_reference_lists(name):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = ac.parse_case(name, None)
        again = ac.parse_case(name, None)
    ac.assert_levels_bit_equal(got, name)
    ac.assert_levels_bit_equal(again, name)


def test_kmer_levels_one_call_many_chunks_and_a_completed_mask():
    """all reads of both samples and the edge reads in one call (several chunks of positions, a
    homopolymer read in front), k-mers masked out"""
    eng = rq.get_engine()
    reads = ac.reads('edge') + ac.reads('alt') + ac.reads('ctrl')
    means = [np.full(700, 0.25)] + [np.asarray(r.means) for r in reads]
    codes = [np.zeros(700, dtype=np.uint8)] + [ts.encode_seq(r.seq) for r in reads]
    means[0][::7] = np.arange(100) * 0.5
    off = ts._csr_offsets([m.shape[0] for m in means])
    done = (np.arange(64) % 5 == 2).astype(np.uint8)
    args = (np.concatenate(means), np.concatenate(codes), off, ac.K, ac.CP, done)
    want = stub.kmer_levels(*args)
    assert want[0][0] >= 698 and off[-1] > 3 * 4096   # (698 AAA windows from the first read alone)
    for _ in range(2):
        counts, levels, lv_off = eng.kmer_levels(*args)
        assert counts.dtype == np.int64 and np.array_equal(counts, want[0]) and np.array_equal(lv_off, want[2])
        assert np.array_equal(ac.bits(levels), ac.bits(want[1]))
    full = 3 * 4096   # the same batch cut off where its third chunk of 4096 positions is exactly full
    cut = (args[0][:full], args[1][:full], np.minimum(off, full)) + args[3:]
    want = stub.kmer_levels(*cut)
    counts, levels, lv_off = eng.kmer_levels(*cut)
    assert 0 < counts.sum() < full and np.array_equal(counts, want[0]) and np.array_equal(lv_off, want[2])
    assert np.array_equal(ac.bits(levels), ac.bits(want[1]))
    empty = eng.kmer_levels(np.empty(0), np.empty(0, dtype=np.uint8), np.zeros(3, dtype=np.int64), ac.K, ac.CP, done)
    assert empty[0].sum() == 0 and empty[1].shape == (0,) and not empty[2].any()


def test_kde_eval_every_segment_size():
    eng = rq.get_engine()
    assert np.diff(ac.GOLD['dens_lv_off']).tolist() == SEG_SIZES
    got = eng.kde_eval(ac.GOLD['dens_levels'], ac.GOLD['dens_lv_off'], ac.SAVE_X, ac.META['bw'])
    again = eng.kde_eval(ac.GOLD['dens_levels'], ac.GOLD['dens_lv_off'], ac.SAVE_X, ac.META['bw'])
    assert got.shape == (len(SEG_SIZES), 500) and np.array_equal(ac.bits(got), ac.bits(again))
    ac.assert_density_close(got, ac.GOLD['dens_scipy'])


def test_kde_eval_big_segment_among_small_ones():
    """the 12003-level segment between 63 small ones, with an empty segment, single levels and a NaN
    level among them: every row is its own segment's"""
    eng = rq.get_engine()
    lv, off = ac.GOLD['dens_levels'], ac.GOLD['dens_lv_off']
    seg = lambda i: lv[off[i]:off[i + 1]]
    small = [0, 1, 2, 3, 8, 9]
    order = [small[i % 6] for i in range(63)]
    order.insert(20, 7)
    segs = [seg(i) for i in order]
    want = [ac.GOLD['dens_scipy'][i] for i in order]
    nan_row = np.full(500, np.nan)
    for pos, s in ((5, np.empty(0)), (33, np.array([0.5])), (50, np.concatenate([seg(1)[:30], [np.nan], seg(1)[30:]]))):
        segs.insert(pos, s)
        want.insert(pos, nan_row)
    levels, lv_off = np.concatenate(segs), ts._csr_offsets([s.shape[0] for s in segs])
    before = levels.copy()
    got = eng.kde_eval(levels, lv_off, ac.SAVE_X, ac.META['bw'])
    want = np.array(want)
    assert np.array_equal(ac.bits(levels), ac.bits(before))   # the input is not sorted in place
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want[:, 0])
    ac.assert_density_close(got[ok], want[ok])
    assert np.array_equal(ac.bits(got), ac.bits(eng.kde_eval(levels, lv_off, ac.SAVE_X, ac.META['bw'])))


def test_estimate_alt_model_end_to_end(tmp_path):
    base = str(tmp_path / 'dens')
    model = ac.estimate(None, density_basename=base)
    ac.assert_model_close(model, ac.GOLD['g_model'])
    dens = ts.parse_kmer_densities_file(base + '.alternate_density.txt')
    ac.assert_density_close(np.array([dens[k] for k in ac.KMERS]), ac.GOLD['g_alt_dens'])
    from_files = ac.estimate(None, alt_dens_fn=base + '.alternate_density.txt', std_dens_fn=base + '.control_density.txt')
    ac.assert_model_close(from_files, ac.GOLD['g_model_from_files'])

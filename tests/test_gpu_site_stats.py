"""Per-site modified fractions on the device (compute_reg_stats_batch, csrc/k_site.h) against the live
reference (tests/golden/stats_site.npz, written by gen_golden_site_stats.py).

No tolerance: the generator asserts that no recorded statistic lies within 1e-9 relative of a
threshold (device p-values agree with scipy to 1e-12), so positions, coverages and control coverages
are equal and the fractions / dampened fractions bit-equal (integer counts, one rounding, one
division).  The per-read statistics themselves keep the stated tolerance of k_read_pvals /
k_c_llh_windows (1e-12 relative)."""
import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th, resquiggle as rq
from tombo_amd._default_parameters import SMALLEST_PVAL
import site_stats_reference as ssr
from stats_cases import (gold, meta, model, alt_refs, run_site_case as _run, site_key as _key,   # noqa: F401
                         check_all_regions_at_once, check_one_region_at_a_time, check_per_read_blocks)

pytestmark = pytest.mark.gpu


def test_golden_all_regions_at_once(gold, meta, model, alt_refs):
    assert check_all_regions_at_once(gold, meta, model, alt_refs) > 60


def test_golden_one_region_at_a_time(gold, meta, model, alt_refs):
    check_one_region_at_a_time(gold, meta, model, alt_refs)


def test_single_region_form_and_queue(gold, meta, model, alt_refs):
    for c in meta['cases']:
        if c['fm'] == 3 or c['li'] != 0:
            continue
        samp, ctrl = ssr.golden_regions(gold, th, c['fm'], model.kmer_width)
        both = _run(gold, meta, model, alt_refs, c)
        for ri in range(len(samp)):
            q = []

            class Q(object):
                put = staticmethod(q.append)
            args = (samp[ri], c['fm'], meta['min_test_reads'], c['single'], c['lower'], ctrl[ri],
                    model if c['use_ref'] else None, alt_refs, False)
            if isinstance(both[ri], Exception):
                with pytest.raises(th.TomboError, match=str(both[ri])):
                    ts.compute_reg_stats(*args, Q, c['stat_type'], None)
            else:
                one = ts.compute_reg_stats(*args, Q, c['stat_type'], None)
                assert [n for n, _ in one] == [n for n, _ in both[ri]]
                for (_, a), (_, b) in zip(one, both[ri]):
                    assert np.array_equal(a.reg_frac_standard_base, b.reg_frac_standard_base, equal_nan=True)
                    assert np.array_equal(a.reg_poss, b.reg_poss) and list(a.ctrl_cov) == list(b.ctrl_cov)
                assert [n for n, _ in q] == [n for n, _ in one]
                assert ts.compute_reg_stats(*args, None, c['stat_type'], None)[0][0] == one[0][0]


def test_per_read_blocks(gold, meta, model, alt_refs):
    assert check_per_read_blocks(gold, meta, model, alt_refs) > 10


def test_region_stats_block(gold, meta, model, alt_refs):
    n = 0
    for c in meta['cases']:
        res = _run(gold, meta, model, alt_refs, c)
        for ri, reg_res in enumerate(res):
            if isinstance(reg_res, Exception):
                continue
            for k, (name, rs) in enumerate(reg_res):
                want = gold['%s_n%d_block' % (_key(c, ri), k)]
                got = ts.region_stats_block(rs, meta['cov_damp_counts'])
                assert got.dtype == want.dtype and np.array_equal(got, want), _key(c, ri)
                damp = ts.calc_damp_fraction(meta['cov_damp_counts'], rs.reg_frac_standard_base, rs.valid_cov)
                assert np.array_equal(damp, gold['%s_n%d_damp' % (_key(c, ri), k)], equal_nan=True)
                n += 1
    assert n > 60


@pytest.fixture(scope='module')
def big(model):
    return ssr.seeded_batch(th, model)


def test_user_size_batch_counts_and_determinism(big, model):
    """64 regions x 10 000 positions x 50 reads: the counts against the numpy restatement on the
    statistics `tba_read_pvals` gives for the same inputs (the same device code, so exact), and the
    same batch twice gives identical bytes"""
    fm, single, lower = 1, 0.5, 0.15
    damp = {'unmod': 2, 'mod': 0}
    args = (big, fm, 1, single, lower, None, model, None, False, ts.DE_NOVO_TXT, None)
    res = ts.compute_reg_stats_batch(*args, cov_damp_counts=damp)
    again = ts.compute_reg_stats_batch(*args, cov_damp_counts=damp)
    inp = ts._reg_stats_z_inputs(big, fm, model, ts.DE_NOVO_TXT)
    pv = rq.get_engine().read_pvals(inp.means, inp.ref_means, inp.ref_sds, inp.off, fm, True, SMALLEST_PVAL)
    lens = np.diff(inp.off)
    locs = np.repeat(inp.read_pos - inp.off[:-1], lens) + np.arange(pv.shape[0])
    trk = np.repeat(inp.read_track, lens)
    bounds = np.concatenate([[0], np.flatnonzero(np.diff(trk)) + 1, [trk.shape[0]]])
    assert bounds.shape[0] == len(big) + 1
    for r in range(len(big)):
        (name, rs), (_, rs2) = res[r][0], again[r][0]
        a, b = bounds[r], bounds[r + 1]
        frac, poss, cov, cc, valid = ssr.collate(pv[a:b], locs[a:b], single, lower, False)
        assert np.array_equal(rs.reg_poss, poss) and np.array_equal(rs.reg_cov, cov)
        assert np.array_equal(rs.valid_cov, valid) and rs.ctrl_cov == cc
        assert np.array_equal(rs.reg_frac_standard_base, frac, equal_nan=True)
        assert np.array_equal(rs.damp_frac, ssr.damp_fraction(damp, frac, valid), equal_nan=True)
        assert poss.shape[0] == 10000 and cov.max() == 50
        for x, y in zip(rs[:2] + rs[5:] + (rs.damp_frac,), rs2[:2] + rs2[5:] + (rs2.damp_frac,)):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()

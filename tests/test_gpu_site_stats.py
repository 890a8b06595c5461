"""Per-site modified fractions on the device (compute_reg_stats_batch, csrc/k_site.h) against the live
reference (tests/golden/stats_site.npz, written by gen_golden_site_stats.py).

No tolerance: the generator asserts that no recorded statistic lies within 1e-9 relative of a
threshold (device p-values agree with scipy to 1e-12), so positions, coverages and control coverages
are equal and the fractions / dampened fractions bit-equal (integer counts, one rounding, one
division).  The per-read statistics themselves keep the stated tolerance of k_read_pvals /
k_c_llh_windows (1e-12 relative)."""
import os
import json
import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th
import site_stats_reference as ssr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLDEN, 'stats_site.npz'))


@pytest.fixture(scope='module')
def meta(gold):
    return json.loads(str(gold['meta']))


@pytest.fixture(scope='module')
def model():
    return ts.TomboModel(seq_samp_type=th.seqSampleType('DNA', False))


@pytest.fixture(scope='module')
def alt_refs(model):
    g = np.load(os.path.join(GOLDEN, 'stats_reads.npz'))
    out = []
    for am in json.loads(str(g['meta']))['alt_models']:
        rows = [(r['kmer'].decode(), int(r['pos']), float(r['mean']), float(r['sd'])) for r in g[am['key']]]
        out.append((am['name'], ts.AltModel(rows, model.central_pos, am['alt_base'], name=am['name'],
                                            motif=th.TomboMotif(am['motif'], am['mod_pos']))))
    return out


def _run(gold, meta, model, alt_refs, c, which=None, **kw):
    samp, ctrl = ssr.golden_regions(gold, th, c['fm'], model.kmer_width)
    if which is not None:
        samp, ctrl = [samp[i] for i in which], [ctrl[i] for i in which]
    std_ref = model if c['use_ref'] else None
    return ts.compute_reg_stats_batch(
        samp, c['fm'], meta['min_test_reads'], c['single'], c['lower'], ctrl, std_ref, alt_refs, False,
        c['stat_type'], None, **kw)


def _key(c, ri):
    return '%s_fm%d_l%d_s%d_r%d' % (c['stat_type'], c['fm'], c['li'], c['use_ref'], ri)


def _check_region(gold, key, res, start, strand, damp=False):
    err = str(gold[key + '_err'])
    if err:
        assert isinstance(res, th.TomboError) and str(res) == err, key
        return 0
    assert not isinstance(res, Exception), (key, res)
    assert [n for n, _ in res] == gold[key + '_names'].tolist(), key
    for k, (name, rs) in enumerate(res):
        p = '%s_n%d_' % (key, k)
        assert isinstance(rs, th.regionStats) and (rs.chrm, rs.strand, rs.start) == ('chr1', strand, start)
        assert np.array_equal(rs.reg_poss, gold[p + 'poss']), key
        assert np.array_equal(rs.reg_cov, gold[p + 'cov']), key
        assert np.array_equal(rs.valid_cov, gold[p + 'valid_cov']), key
        assert list(rs.ctrl_cov) == gold[p + 'ctrl_cov'].tolist(), key
        assert np.array_equal(rs.reg_frac_standard_base, gold[p + 'frac'], equal_nan=True), key
        if damp:
            assert np.array_equal(rs.damp_frac, gold[p + 'damp'], equal_nan=True), key
    return len(res)


def test_golden_all_regions_at_once(gold, meta, model, alt_refs):
    n = 0
    for c in meta['cases']:
        res = _run(gold, meta, model, alt_refs, c, cov_damp_counts=meta['cov_damp_counts'])
        for ri in range(len(res)):
            n += _check_region(gold, _key(c, ri), res[ri], int(gold['reg_start'][ri]),
                               '-' if gold['reg_minus'][ri] else '+', damp=True)
    assert n > 60


def test_golden_one_region_at_a_time(gold, meta, model, alt_refs):
    for c in meta['cases']:
        for ri in range(gold['reg_start'].shape[0]):
            res = _run(gold, meta, model, alt_refs, c, which=[ri])
            _check_region(gold, _key(c, ri), res[0], int(gold['reg_start'][ri]),
                          '-' if gold['reg_minus'][ri] else '+')


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
    """return_per_read: the reference's per-read blocks after mapping ids back to strings; statistics
    to the stated tolerance of the per-read kernels, positions and reads equal (both sorted by
    (read, position): the reference concatenates reads in region order, as the batch does)"""
    n = 0
    for c in meta['cases']:
        if c['li'] != 0 or c['use_ref'] != 1 or c['fm'] >= 3:
            continue
        res, per_read = _run(gold, meta, model, alt_refs, c, return_per_read=True)
        for ri in range(len(res)):
            key = _key(c, ri)
            assert len(per_read[ri]) == int(gold[key + '_npr']), key
            for k, (name, (blk, lookup, chrm, strand, start)) in enumerate(per_read[ri]):
                assert name == str(gold['%s_pr%d_name' % (key, k)])
                assert (chrm, start) == ('chr1', int(gold['reg_start'][ri]))
                assert blk.dtype == np.dtype([('pos', 'u4'), ('stat', 'f8'), ('read_id', 'u4')])
                inv = dict((v, rid) for rid, v in lookup.items())
                got_ids = [inv[v] for v in blk['read_id']]
                assert got_ids == ['r%d' % q for q in gold['%s_pr%d_read' % (key, k)]], key
                assert np.array_equal(blk['pos'], gold['%s_pr%d_pos' % (key, k)]), key
                np.testing.assert_allclose(blk['stat'], gold['%s_pr%d_stat' % (key, k)], rtol=1e-12, atol=0)
                n += 1
    assert n > 10


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
    pv = ts._read_pvals(inp['means'], inp['ref_means'], inp['ref_sds'], inp['off'], fm, True)
    lens = np.diff(inp['off'])
    locs = np.repeat(inp['read_pos'] - inp['off'][:-1], lens) + np.arange(pv.shape[0])
    trk = np.repeat(inp['read_track'], lens)
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

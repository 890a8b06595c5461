"""The golden cases of the per-read and per-site statistics (tests/golden/stats_reads.npz,
stats_site.npz) as inputs, and the comparisons against their recorded results.  A plain module
(not a conftest): the GPU tests (test_gpu_read_stats.py, test_gpu_site_stats.py) run the cases on
the device, tests/test_stats_host_layer.py runs the same cases through the numpy stand-in engine."""
import os
import json

import numpy as np
import pytest

from tombo_amd import tombo_stats as ts, tombo_helper as th
import site_stats_reference as ssr

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
RTOL = 1e-12


# ---- per-read statistics (stats_reads.npz) -------------------------------------------------------
def load_read_cases():
    g = np.load(os.path.join(GOLDEN, 'stats_reads.npz'))
    meta = json.loads(str(g['meta']))
    model = ts.TomboModel(seq_samp_type=th.seqSampleType('DNA', False))
    alts = []
    for am in meta['alt_models']:
        rows = g[am['key']]
        alts.append((am['name'], ts.AltModel(
            [(r['kmer'], r['pos'], r['mean'], r['sd']) for r in rows], model.central_pos,
            am['alt_base'], name=am['name'], motif=th.TomboMotif(am['motif'], am['mod_pos']))))
    reads = []
    for ci, c in enumerate(meta['cases']):
        reads.append(th.resquiggledRead(
            start=c['start'], end=c['start'] + c['n'], filtered=False, read_start_rel_to_raw=0,
            strand=c['strand'], fn=c['fn'], corr_group='RawGenomeCorrected_000/BaseCalled_template',
            rna=False, read_id=c['read_id'], means=g['c%d_means' % ci], seq=str(g['c%d_seq' % ci])))
    return g, meta, model, alts, reads


class Reg(object):
    def __init__(self, se):
        self.start, self.end = se


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    np.testing.assert_allclose(a[ok], b[ok], rtol=RTOL, atol=0)


# ---- per-site fractions (stats_site.npz) ---------------------------------------------------------
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


def run_site_case(gold, meta, model, alt_refs, c, which=None, **kw):
    samp, ctrl = ssr.golden_regions(gold, th, c['fm'], model.kmer_width)
    if which is not None:
        samp, ctrl = [samp[i] for i in which], [ctrl[i] for i in which]
    std_ref = model if c['use_ref'] else None
    return ts.compute_reg_stats_batch(
        samp, c['fm'], meta['min_test_reads'], c['single'], c['lower'], ctrl, std_ref, alt_refs, False,
        c['stat_type'], None, **kw)


def site_key(c, ri):
    return '%s_fm%d_l%d_s%d_r%d' % (c['stat_type'], c['fm'], c['li'], c['use_ref'], ri)


def check_site_region(gold, key, res, start, strand, damp=False):
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


def check_all_regions_at_once(gold, meta, model, alt_refs, **kw):
    n = 0
    for c in meta['cases']:
        res = run_site_case(gold, meta, model, alt_refs, c, cov_damp_counts=meta['cov_damp_counts'], **kw)
        for ri in range(len(res)):
            n += check_site_region(gold, site_key(c, ri), res[ri], int(gold['reg_start'][ri]),
                                   '-' if gold['reg_minus'][ri] else '+', damp=True)
    return n


def check_one_region_at_a_time(gold, meta, model, alt_refs, **kw):
    for c in meta['cases']:
        for ri in range(gold['reg_start'].shape[0]):
            res = run_site_case(gold, meta, model, alt_refs, c, which=[ri], **kw)
            check_site_region(gold, site_key(c, ri), res[0], int(gold['reg_start'][ri]),
                              '-' if gold['reg_minus'][ri] else '+')


def check_per_read_blocks(gold, meta, model, alt_refs, **kw):
    """return_per_read: the reference's per-read blocks after mapping ids back to strings; statistics
    to the stated tolerance of the per-read kernels, positions and reads equal (both sorted by
    (read, position): the reference concatenates reads in region order, as the batch does)"""
    n = 0
    for c in meta['cases']:
        if c['li'] != 0 or c['use_ref'] != 1 or c['fm'] >= 3:
            continue
        res, per_read = run_site_case(gold, meta, model, alt_refs, c, return_per_read=True, **kw)
        for ri in range(len(res)):
            key = site_key(c, ri)
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
    return n


# ---- the per-read golden cases -------------------------------------------------------------------
def check_z_read_cases(de_novo, sample_compare):
    """every golden case through de_novo(read, model, fm_offset, region) and sample_compare(read,
    ctrl_means, ctrl_sds, fm_offset, region), both with the single-read functions' return shape and
    errors -> number of checks"""
    g, meta, model, alts, reads = load_read_cases()
    n_checked = 0
    for ci, (c, rd) in enumerate(zip(meta['cases'], reads)):
        for ri, reg in enumerate(c['regions']):
            regd = None if reg is None else Reg(reg)
            for fm in meta['fm_offsets']:
                tag = 'c%d_r%d_fm%d' % (ci, ri, fm)
                err = str(g[tag + '_dn_err'])
                if err:
                    with pytest.raises(th.TomboError, match=err[:30]):
                        de_novo(rd, model, fm, regd)
                else:
                    pv, ps, rid = de_novo(rd, model, fm, regd)
                    close(pv[ts.DE_NOVO_TXT], g[tag + '_dn_p'])
                    np.testing.assert_array_equal(ps[ts.DE_NOVO_TXT], g[tag + '_dn_pos'])
                    assert rid == c['read_id']
                err = str(g[tag + '_sc_err'])
                cm, cs = g[tag + '_sc_cm'], g[tag + '_sc_cs']
                if err:
                    with pytest.raises(th.TomboError, match=err[:30]):
                        sample_compare(rd, cm, cs, fm, regd)
                else:
                    pv, ps, rid = sample_compare(rd, cm, cs, fm, regd)
                    close(pv[ts.SAMP_COMP_TXT], g[tag + '_sc_p'])
                    np.testing.assert_array_equal(ps[ts.SAMP_COMP_TXT], g[tag + '_sc_pos'])
                n_checked += 2
    return n_checked


def check_alt_read_cases(alt_model):
    """every golden case through alt_model(read, model, alt_refs, use_standard_llhr, region) -> number
    of log-likelihood ratios checked"""
    g, meta, model, alts, reads = load_read_cases()
    hits = 0
    for ci, (c, rd) in enumerate(zip(meta['cases'], reads)):
        for ri, reg in enumerate(c['regions']):
            regd = None if reg is None else Reg(reg)
            for std_llhr in (False, True):
                tag = 'c%d_r%d_llhr%d' % (ci, ri, int(std_llhr))
                err = str(g[tag + '_am_err'])
                if err:
                    with pytest.raises(th.TomboError, match=err[:30]):
                        alt_model(rd, model, alts, std_llhr, regd)
                    continue
                ll, ps, rid = alt_model(rd, model, alts, std_llhr, regd)
                for name, _ in alts:
                    want = g[tag + '_am_%s_v' % name]
                    np.testing.assert_array_equal(ps[name], g[tag + '_am_%s_pos' % name])
                    if std_llhr:
                        np.testing.assert_array_equal(ll[name], want)   # constant variance: bit-equal
                    else:
                        np.testing.assert_allclose(ll[name], want, rtol=RTOL, atol=1e-300)
                    hits += want.shape[0]
    return hits

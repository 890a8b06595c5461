"""tests/tracks_reference.py (the genome-track functions restated in numpy) equals the live reference's recorded
output, tests/golden/stats_tracks.npz (written by tests/golden/gen_golden_tracks.py), exactly."""
import numpy as np
import pytest

import tracks_reference as tr
from tracks_cases import Case, same_bits, exact, SLOTS


@pytest.fixture(scope='module')
def c():
    return Case()


def test_chrm_sizes(c):
    for tag, got in (('s', tr.chrm_sizes(c.samp)), ('sc', tr.chrm_sizes(c.samp, c.ctrl))):
        assert got == dict((c.names[k], int(n)) for k, n in zip(c.g['sizes_%s_chrm' % tag], c.g['sizes_%s' % tag]))


def test_slot_means(c):
    for which, index, cols in ((0, c.samp, c.samp_cols), (1, c.ctrl, c.ctrl_cols)):
        for (chrm, strand), reads in index.items():
            for slot in SLOTS:
                same_bits(tr.slot_mean(reads, cols[(chrm, strand)], c.sizes[chrm], slot),
                          c.g['mean_%d_%s_%s_%s' % (which, chrm, strand, slot)])


def test_the_deep_stack_tells_a_reordered_sum(c):
    reads, cols = c.samp[('chrD', '+')], c.samp_cols[('chrD', '+')]
    fwd = tr.slot_mean(reads, cols, c.sizes['chrD'], 'norm_mean')
    rev = tr.slot_mean(reads[::-1], cols[::-1], c.sizes['chrD'], 'norm_mean')
    covered = ~np.isnan(fwd)
    assert 3 * int((fwd[covered] != rev[covered]).sum()) >= int(covered.sum())


def test_coverage_regions_and_cov_regs(c):
    for tag, ctrl in (('s', None), ('sc', c.ctrl)):
        regs = tr.coverage_regions(c.samp, ctrl)
        assert [(r[0], r[1]) for r in regs] == [c.cs(r) for r in c.g['covreg_%s_cs' % tag]]
        for i, r in enumerate(regs):
            exact(r[2], c.g['covreg_%s_%d_cov' % (tag, i)])
            exact(r[3], c.g['covreg_%s_%d_starts' % (tag, i)])
        for thresh in (1, 5, int(c.g['max_cov']) + 1):
            for rs in (100, None):
                want = c.g['covregs_%s_t%d_r%s' % (tag, thresh, rs)]
                got = tr.cov_regs(c.samp, thresh, rs, ctrl)
                assert got == [c.cs(w) + tuple(int(x) for x in w[2:]) for w in want]


def test_cov_regs_keeps_the_stretches_between_runs(c):
    """the reference pairs consecutive threshold crossings: with two qualifying runs the stretch between them is
    yielded as a region of its own (recorded, so it is what callers of the reference get)"""
    want = c.g['covregs_s_t5_rNone']
    rows = [w for w in want if c.cs(w) == ('chrA', '-')]
    assert len(rows) >= 3 and all(rows[i][3] == rows[i + 1][2] for i in range(len(rows) - 1))


def test_differences(c):
    got = tr.signal_differences(c.samp, c.samp_cols, c.ctrl, c.ctrl_cols)
    assert list(got) == [c.cs(r) for r in c.g['diff_cs']]
    for i, d in enumerate(got.values()):
        same_bits(d, c.g['diff_%d' % i])
    for n in (1, 5, int(c.g['n_nonzero'])):
        res = tr.largest_signal_differences(c.samp, c.samp_cols, c.ctrl, c.ctrl_cols, n, int(c.g['num_bases']))
        same_bits(np.array([r[0] for r in res]), c.g['largest_%d_val' % n])
        assert [(r[1], r[2], r[3]) for r in res] == [(int(x[0]),) + c.cs(x[1:]) for x in c.g['largest_%d_rest' % n]]


def test_browser_files(c):
    for tag, ctrl, ctrl_cols in (('s', None, None), ('sc', c.ctrl, c.ctrl_cols)):
        files = tr.browser_files('trk', tr.WIG_TYPES, c.samp, c.samp_cols, ctrl, ctrl_cols)
        names = [str(x) for x in c.g['files_%s_names' % tag]]
        assert sorted(files) == names
        for i, name in enumerate(names):
            assert files[name].encode() == c.g['files_%s_%d' % (tag, i)].tobytes(), name

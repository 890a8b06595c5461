"""numpy restatement of the reference's collation of per-read statistics into per-site records:
collate_reg_stats / apply_per_read_thresh (tombo_stats.py:4084-4178) and calc_damp_fraction
(:2537-2552), on given per-read statistics.  This is what a caller had to run on the host, region by
region, before `compute_reg_stats_batch` (tools/site_stats_timing.py times it as the parent route)."""
import numpy as np


def collate(stats, stat_locs, single_read_thresh, lower_thresh, is_alt, ctrl_cov=None,
            is_samp_comp=False):
    """-> (frac, poss, cov, ctrl_cov list, valid_cov) or None when no statistic is left"""
    stats, stat_locs = np.asarray(stats, dtype=np.float64), np.asarray(stat_locs)
    ok = ~np.isnan(stats)
    stats, stat_locs = stats[ok], stat_locs[ok]
    if stats.shape[0] == 0:
        return None
    order = np.argsort(stat_locs, kind='stable')
    stat_locs, stats = stat_locs[order], stats[order]
    poss = np.unique(stat_locs)
    base_stats = np.split(stats, np.where(np.concatenate([[0], np.diff(stat_locs)]) > 0)[0])
    cov = np.array([b.shape[0] for b in base_stats])
    if lower_thresh is not None:
        base_stats = [b[np.logical_or(b <= lower_thresh, b >= single_read_thresh)] for b in base_stats]
    elif is_alt:
        base_stats = [b[np.abs(b) >= single_read_thresh] for b in base_stats]
    valid = np.array([b.shape[0] for b in base_stats])
    if is_samp_comp:
        cc = [ctrl_cov[p] if ctrl_cov is not None and p in ctrl_cov else 0 for p in stat_locs.tolist()]
    else:
        cc = [0] * stat_locs.shape[0]
    frac = np.array([np.greater_equal(b, single_read_thresh).sum() / b.shape[0]
                     if b.shape[0] > 0 else np.nan for b in base_stats])
    return frac, poss, cov, cc, valid


def damp_fraction(cov_damp_counts, fracs, valid_cov):
    return (np.round(fracs * valid_cov) + cov_damp_counts['unmod']) / (
        valid_cov + sum(list(cov_damp_counts.values())))


def stat_block(frac, poss, cov, ctrl_cov, valid, cov_damp_counts):
    damp = damp_fraction(cov_damp_counts, frac, valid)
    return np.array([p for p in zip(damp, frac, poss, cov, ctrl_cov, valid) if not np.isnan(p[0])],
                    dtype=[('damp_frac', 'f8'), ('frac', 'f8'), ('pos', 'u4'), ('cov', 'u4'),
                           ('control_cov', 'u4'), ('valid_cov', 'u4')])


# ---- the golden file (tests/golden/stats_site.npz) as inputs ------------------------------------
def golden_reads(g):
    """per read of the golden file: (global index, region, start, length, minus, ctrl, means)"""
    off = np.concatenate([[0], np.cumsum(g['rd_len'])])
    return [(q, int(g['rd_reg'][q]), int(g['rd_start'][q]), int(g['rd_len'][q]), bool(g['rd_minus'][q]),
             bool(g['rd_ctrl'][q]), g['rd_means'][off[q]:off[q + 1]]) for q in range(g['rd_len'].shape[0])]


def ctrl_cov_dict(g, ri, fm, min_test_reads):
    """the coverage dict of get_reads_ref (tombo_stats.py:3642-3666) over the control reads of region
    ri: non-NaN levels of the reads on the region's strand per position of [start - fm, end + fm);
    {} when no position reaches min_test_reads"""
    lo, hi = int(g['reg_start'][ri]) - fm, int(g['reg_end'][ri]) + fm
    cov = np.zeros(hi - lo, dtype=np.int64)
    for (q, r, s, n, minus, ctrl, m) in golden_reads(g):
        if r != ri or not ctrl or minus != bool(g['reg_minus'][ri]):
            continue
        lv = m[::-1] if minus else m
        a, b = max(s, lo), min(s + n, hi)
        if b > a:
            cov[a - lo:b - lo] += ~np.isnan(lv[a - s:b - s])
    if not (cov >= min_test_reads).any():
        return {}
    return dict(zip(range(lo, hi), cov.tolist()))


def golden_regions(g, th, fm=0, kmer_width=None):
    """golden reads -> (sample regions, control regions) of th.regionData, reads in the generator's
    order with ids 'r<global index>'; kmer_width given: control regions carry the sequence the prior
    blend of get_reads_ref needs"""
    genome = g['genome'].tobytes().decode()
    samp, ctrl = [], []
    rows = golden_reads(g)
    for ri in range(g['reg_start'].shape[0]):
        strand = '-' if g['reg_minus'][ri] else '+'
        rs = {False: [], True: []}
        for (q, r, s, n, minus, is_ctrl, m) in rows:
            if r != ri:
                continue
            seq = genome[s:s + n]
            rs[is_ctrl].append(th.resquiggledRead(
                s, s + n, False, 0, '-' if minus else '+', None, None, False, read_id='r%d' % q,
                means=m, seq=th.rev_comp(seq) if minus else seq))
        start, end = int(g['reg_start'][ri]), int(g['reg_end'][ri])
        samp.append(th.regionData('chr1', strand, start, end, rs[False]))
        cseq = None if kmer_width is None else genome[start - fm - kmer_width + 1:end + fm + kmer_width - 1]
        ctrl.append(th.regionData('chr1', strand, start, end, rs[True], seq=cseq))
    return samp, ctrl


def seeded_batch(th, model, n_regions=64, n_pos=10000, depth=50, seed=4180):
    """a de_novo batch at a user's size: n_regions '+' regions of n_pos positions, depth reads
    spanning each (levels: the model's plus continuous noise, a shift on some bases)"""
    rng = np.random.default_rng(seed)
    K, cp = model.kmer_width, model.central_pos
    pad = 8   # the reads reach past the region, so every position of it is tested for fm_offset <= pad
    regions = []
    for r in range(n_regions):
        start = 1000 + r * (n_pos + 500)
        n_lv = n_pos + 2 * pad
        n = n_lv + K - 1
        seq = ''.join(rng.choice(list('ACGT'), n))
        lv, sd = model.get_exp_levels_from_seq(seq)
        reads = []
        for d in range(depth):
            m = np.zeros(n)
            m[cp:cp + n_lv] = lv + rng.normal(0.0, 1.3, n_lv) * sd + 1.2 * (rng.random(n_lv) < 0.3)
            reads.append(th.resquiggledRead(start - pad - cp, start - pad - cp + n, False, 0, '+', None,
                                            None, False, read_id='s%d_%d' % (r, d), means=m, seq=seq))
        regions.append(th.regionData('c', '+', start, start + n_pos, reads))
    return regions

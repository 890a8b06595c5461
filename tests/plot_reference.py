"""TEST INFRASTRUCTURE: the arithmetic of the region plot frames (tombo/_plot_commands.py:784-984) restated in numpy,
statement by statement where the reference has statements: the pile-up of intervalData.get_base_levels with the NaN
removal of the frame functions, the two np.percentile forms written out (numpy's _quantile / _lerp), and
th.get_raw_signal + normalize_raw_signal + the per-base np.linspace spread.  tests/test_plot_reference.py pins it to
the live reference's recorded frames (tests/golden/stats_plot_data.npz) bit for bit; the GPU tests then use it as the
yardstick beyond the fixture.  The argument layout is that of the Engine methods (tombo_amd/_native.py)."""
import numpy as np


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == 'f':
        bad = np.flatnonzero(got.view(np.uint64).ravel() != want.view(np.uint64).ravel())
        assert bad.size == 0, 'first of %d differing values at %d: %r != %r' % (
            bad.size, bad[0], got.ravel()[bad[0]].hex(), want.ravel()[bad[0]].hex())
    else:
        assert np.array_equal(got, want)


def full_mantissa(rng, shape):
    """doubles whose last bits are all in use: a changed operation order shows"""
    return rng.standard_normal(shape) + rng.random(shape) * 1e-3


def base_levels(rs, rm, off, m, reads, start, end):
    """get_base_levels (tombo_helper.py:1976-2032) of one region: [end - start, len(reads)], NaN outside a read"""
    cols = []
    for q in reads:
        r_means = m[off[q]:off[q + 1]][::-1] if rm[q] else m[off[q]:off[q + 1]]
        r_start, r_end = int(rs[q]), int(rs[q]) + r_means.shape[0]
        col = np.full(end - start, np.nan)
        lo, hi = max(r_start, start), min(r_end, end)
        if lo < hi:
            col[lo - start:hi - start] = r_means[lo - r_start:hi - r_start]
        cols.append(col)
    return np.column_stack(cols) if cols else np.empty((end - start, 0))


def level_piles(rs, rm, off, m, roff, rr, st, en):
    """-> (pile offsets int64[n_pos + 1], levels): per region and position the non-NaN levels in read order"""
    piles = []
    for r in range(st.shape[0]):
        for row in base_levels(rs, rm, off, m, rr[roff[r]:roff[r + 1]].tolist(), int(st[r]), int(en[r])):
            piles.append(row[~np.isnan(row)])
    sizes = [p.shape[0] for p in piles]
    return (np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
            np.concatenate(piles) if piles else np.empty(0, dtype=np.float64))


def _linear_sorted(v, q):
    """numpy's _quantile / _lerp for one fraction on a sorted, NaN-free v"""
    n = v.shape[0]
    vi = (n - 1) * q
    lo = int(np.floor(vi))
    a, b, t = v[lo], v[min(lo + 1, n - 1)], vi - np.floor(vi)
    return b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t


def _nearest_sorted(v, q):
    return v[int(np.around((v.shape[0] - 1) * q))]


def percentile_linear(v, q):
    """np.percentile(v, 100 q) of a NaN-free v"""
    return _linear_sorted(np.sort(v), q)


def percentile_nearest(v, q):
    """np.percentile(v, 100 q, interpolation='nearest') of a NaN-free v"""
    return _nearest_sorted(np.sort(v), q)


def segment_percentiles(values, off, ql, qn):
    """-> (lin [n_seg, n_ql], near [n_seg, n_qn]); NaN rows for an empty segment and one with a NaN"""
    n_seg = off.shape[0] - 1
    lin, near = np.full((n_seg, ql.shape[0]), np.nan), np.full((n_seg, qn.shape[0]), np.nan)
    for s in range(n_seg):
        v = values[off[s]:off[s + 1]]
        if v.shape[0] == 0 or np.isnan(v).any():
            continue
        v = np.sort(v)
        lin[s] = [_linear_sorted(v, q) for q in ql.tolist()]
        near[s] = [_nearest_sorted(v, q) for q in qn.tolist()]
    return lin, near


def get_raw_signal(all_sig, segs, r_start, rsrtr, minus, rna, int_start, int_end):
    """th.get_raw_signal (tombo_helper.py:2107-2137) on arrays -> (r_sig, overlap_seg_data, start_offset)"""
    if rna:
        all_sig = all_sig[::-1]
    if minus:
        segs = (segs[::-1] * -1) + segs[-1]
    if int_start < r_start:
        start_offset = r_start - int_start
        overlap_seg_data = segs[:int_end - r_start + 1]
    else:
        start_offset = 0
        overlap_seg_data = segs[int_start - r_start:int_end - r_start + 1]
    num_reg_obs = overlap_seg_data[-1] - overlap_seg_data[0]
    if not minus:
        reg_start_rel_raw = rsrtr + overlap_seg_data[0]
        r_sig = all_sig[reg_start_rel_raw:reg_start_rel_raw + num_reg_obs]
    else:
        reg_start_rel_raw = rsrtr + segs[-1] - overlap_seg_data[-1]
        r_sig = all_sig[reg_start_rel_raw:reg_start_rel_raw + num_reg_obs][::-1]
    return r_sig, overlap_seg_data, start_offset


def raw_signal(raw, roff, segs, soff, rs, rsr, mn, rn, sh, sc, lo, hi, pr, ps, pe, genome_centric=True):
    """-> (sig_off, position, signal, base_i) of the pairs, as Engine.region_raw_signal lays them out"""
    sizes, position, signal, base = [], [], [], []
    for q, int_start, int_end in zip(pr.tolist(), ps.tolist(), pe.tolist()):
        r_sig, ov, start_offset = get_raw_signal(raw[roff[q]:roff[q + 1]], segs[soff[q]:soff[q + 1]], int(rs[q]),
                                                 int(rsr[q]), bool(mn[q]), bool(rn[q]), int_start, int_end)
        r_sig = (r_sig - sh[q]) / sc[q]                         # normalize_raw_signal, tombo_stats.py:554
        if not np.isnan(lo[q]) and not np.isnan(hi[q]):         # c_apply_outlier_thresh
            r_sig = np.where(r_sig > hi[q], hi[q], np.where(r_sig < lo[q], lo[q], r_sig))
        if not genome_centric and mn[q]:                        # _plot_commands.py:946-952
            r_sig = r_sig[::-1]
            ov = (ov[::-1] * -1) + ov[-1]
            if len(ov) < int_end - int_start:
                start_offset = int_end - int_start - len(ov) - start_offset
        for base_i, (b_start, b_end) in enumerate(zip(ov[:-1].tolist(), ov[1:].tolist())):
            position.append(int_start + base_i + start_offset + np.linspace(0, 1, b_end - b_start, endpoint=False))
            signal.append(r_sig[b_start - ov[0]:b_end - ov[0]])
            base.append(np.full(b_end - b_start, base_i, dtype=np.int64))
        sizes.append(int(ov[-1] - ov[0]))
    cat = (lambda xs, t: np.concatenate(xs).astype(t) if xs else np.empty(0, dtype=t))
    return (np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), cat(position, np.float64),
            cat(signal, np.float64), cat(base, np.int64))

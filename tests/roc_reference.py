"""TEST INFRASTRUCTURE: the three ROC entries of the engine restated in numpy (tombo_stats.py:2406-2535 and
_plot_commands.py:60-82 behind them): labels by vectorised sequence lookups and np.isin-style searches, the
ordering by np.lexsort, the counts by np.cumsum.  tests/test_roc_reference.py pins this to the fixture recorded
from the live reference; the GPU tests and tools/roc_timing.py compare the device with it beyond the fixture."""
import numpy as np


def _block_of(rec_off, n_rec):
    return np.repeat(np.arange(rec_off.shape[0] - 1), np.diff(rec_off))


def motif_labels(blk_minus, blk_seq_start, seq_off, seq_codes, rec_off, rec_pos, rec_stat, motifs, ctrl_label=None):
    """-> per motif (stats, has_mod, record index) of the kept records, in record order.  motifs: (length, mod_pos,
    mod_base code, base sets).  The rule of compute_motif_stats (ctrl_label None) or of compute_ctrl_motif_stats."""
    blk = _block_of(rec_off, rec_pos.shape[0])
    minus = blk_minus[blk] != 0
    s0, length = seq_off[blk], np.diff(seq_off)[blk]
    idx = rec_pos - blk_seq_start[blk]

    def code_at(g):
        inside = (g >= 0) & (g < length)
        if seq_codes.shape[0] == 0:
            return np.full(g.shape, 4), inside
        c = seq_codes[np.where(inside, s0 + g, 0)].astype(np.int64)
        c = np.where(inside & (c < 4), np.where(minus, 3 - c, c), 4)
        return c, inside

    out = []
    for mot_len, mod_pos, mod_base, sets in motifs:
        c, _ = code_at(idx)
        base = (c < 4) & (c == mod_base)
        match = np.ones(idx.shape[0], dtype=bool)
        for j in range(mot_len):
            o = j - (mod_pos - 1)
            c, _ = code_at(np.where(minus, idx - o, idx + o))
            match &= (c < 4) & (((int(sets[j]) >> np.minimum(c, 3)) & 1) == 1)
        if ctrl_label is None:
            keep, label = base, match
        else:
            keep, label = match, np.full(idx.shape[0], bool(ctrl_label))
        out.append((rec_stat[keep], label[keep], np.flatnonzero(keep)))
    return out


def loc_labels(blk_loc, mod_locs, unmod_locs, rec_off, rec_pos, rec_stat):
    """-> (stats, has_mod, record index): kept when the position is in either slice of the record's block"""
    in_mod, in_unmod = np.zeros(rec_pos.shape[0], dtype=bool), np.zeros(rec_pos.shape[0], dtype=bool)
    for t in range(blk_loc.shape[0]):
        a, b = rec_off[t], rec_off[t + 1]
        in_mod[a:b] = np.isin(rec_pos[a:b], mod_locs[blk_loc[t, 0]:blk_loc[t, 1]])
        in_unmod[a:b] = np.isin(rec_pos[a:b], unmod_locs[blk_loc[t, 2]:blk_loc[t, 3]])
    keep = in_mod | in_unmod
    return rec_stat[keep], in_mod[keep], np.flatnonzero(keep)


def rank_counts(stats, has_mod, ranks):
    """-> (tp_at, tp_total, n_nan): True labels among the ranks[j] + 1 first entries in (stat, has_mod) order, which
    is what sorted() gives a list of (float, bool) tuples without NaN: -0.0 == 0.0, False < True"""
    order = np.lexsort((has_mod, stats))
    tp_cumsum = np.cumsum(has_mod[order], dtype=np.int64)
    return tp_cumsum[ranks], int(has_mod.sum()), int(np.isnan(stats).sum())

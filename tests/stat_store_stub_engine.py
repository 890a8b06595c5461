"""TEST INFRASTRUCTURE: `Engine.site_aggregate` in numpy, so that the host layer of the statistics files
(aggregate_per_read_stats: grouping, layout, writing) runs on a box without a GPU: pass an instance as `engine=`.
The arithmetic is the reference's _agg_stats_worker / apply_per_read_thresh (tombo_stats.py:4084-4122, 4699-4725)
restated: stable sort by position, split per site, threshold -- plus the NaN drop of the device."""
import numpy as np

from tombo_amd import _native
from tombo_amd._native import SiteFractions


def aggregate_block(block, single_read_thresh, lower_thresh, abs_rule):
    """-> (frac, poss, cov, valid_cov) of one block's records"""
    block = block[~np.isnan(block['stat'])]
    block = block[np.argsort(block['pos'], kind='stable')]
    poss, first = np.unique(block['pos'], return_index=True)
    frac, cov, valid = np.full(poss.shape[0], np.nan), np.zeros(poss.shape[0], np.int64), np.zeros(poss.shape[0], np.int64)
    for k, st in enumerate(np.split(block['stat'], first[1:]) if poss.shape[0] else ()):   # (np.split of nothing: one empty piece)
        cov[k] = st.shape[0]
        if lower_thresh is not None:
            st = st[(st <= lower_thresh) | (st >= single_read_thresh)]
        elif abs_rule:
            st = st[np.abs(st) >= single_read_thresh]
        valid[k] = st.shape[0]
        if st.shape[0] > 0:
            frac[k] = (st >= single_read_thresh).sum() / st.shape[0]
    return frac, poss.astype(np.int64), cov, valid


class NumpyStatStoreEngine(object):
    def __init__(self):
        self.calls = []      # (number of blocks, number of records) of every call

    def site_aggregate(self, blk_start, blk_end, rec_off, records, single_read_thresh, lower_thresh=None,
                       abs_rule=False, damp_counts=None):
        bs, be, off, rec = _native._check_site_aggregate_args(blk_start, blk_end, rec_off, records)
        self.calls.append((bs.shape[0], rec.shape[0]))
        pos_off = np.concatenate([[0], np.cumsum(be - bs)]).astype(np.int64)
        n_pos = int(pos_off[-1])
        frac, damp = np.full(n_pos, np.nan), None if damp_counts is None else np.full(n_pos, np.nan)
        poss, cov, valid = (np.zeros(n_pos, dtype=np.int64) for _ in range(3))
        counts, n_stats = np.zeros(bs.shape[0], dtype=np.int64), np.zeros(bs.shape[0], dtype=np.int64)
        for t in range(bs.shape[0]):
            block = rec[off[t]:off[t + 1]]
            if np.any((block['pos'] < bs[t]) | (block['pos'] >= be[t])):
                raise _native.EngineError('tba_site_aggregate failed (-1): record position outside its block')
            f, p, c, v = aggregate_block(block, single_read_thresh, lower_thresh, abs_rule)
            a, b = int(pos_off[t]), int(pos_off[t]) + p.shape[0]
            frac[a:b], poss[a:b], cov[a:b], valid[a:b] = f, p, c, v
            counts[t], n_stats[t] = p.shape[0], c.sum()
            if damp is not None:
                with np.errstate(invalid='ignore'):
                    damp[a:b] = (np.round(f * v) + damp_counts[0]) / (v + damp_counts[0] + damp_counts[1])
        return SiteFractions(pos_off, frac, poss, cov, valid, damp, counts, n_stats, None)

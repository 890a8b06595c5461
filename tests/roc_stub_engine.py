"""TEST INFRASTRUCTURE: the ROC methods of `_native.Engine` over the numpy restatement of tests/roc_reference.py,
with the engine's own argument checks, so that the host layer (compute_*_stats, prep_accuracy_rates) runs on a box
without a GPU: pass an instance as `engine=`."""
import numpy as np

import roc_reference as ref
from tombo_amd import _native


def _split_motifs(table, sets):
    out, a = [], 0
    for length, mod_pos, mod_base in table.tolist():
        out.append((length, mod_pos, mod_base, sets[a:a + length]))
        a += length
    return out


class NumpyRocEngine(object):
    def __init__(self):
        self.calls = []      # (entry, records or entries) of every call

    def roc_motif_labels(self, blk_minus, blk_seq_start, seq_off, seq_codes, rec_off, rec_pos, rec_stat, motifs,
                         ctrl_label=None, return_index=False):
        minus, ss, s_off, seq, off, pos, stat, table, sets = _native._check_roc_motif_args(
            blk_minus, blk_seq_start, seq_off, seq_codes, rec_off, rec_pos, rec_stat, motifs)
        self.calls.append(('motif', pos.shape[0]))
        res = ref.motif_labels(minus, ss, s_off, seq, off, pos, stat, _split_motifs(table, sets), ctrl_label)
        return [r if return_index else r[:2] for r in res]

    def roc_loc_labels(self, blk_loc, mod_locs, unmod_locs, rec_off, rec_pos, rec_stat, return_index=False):
        args = _native._check_roc_loc_args(blk_loc, mod_locs, unmod_locs, rec_off, rec_pos, rec_stat)
        self.calls.append(('loc', args[4].shape[0]))
        res = ref.loc_labels(*args)
        return res if return_index else res[:2]

    def roc_rank_counts(self, stats, has_mod, ranks):
        st, hm, rk = _native._check_roc_rank_args(stats, has_mod, ranks)
        self.calls.append(('rank', st.shape[0]))
        return ref.rank_counts(st, hm.view(np.bool_), rk)

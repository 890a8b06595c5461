"""TEST INFRASTRUCTURE: numpy forms of `Engine.region_level_piles`, `Engine.segment_percentiles` and
`Engine.region_raw_signal`, so that the host layer of the region plot data (tombo_amd/plot_commands.py) runs on a box
without a GPU.  The argument checks are the binding's own (tombo_amd._native._check_*), the arithmetic is
tests/plot_reference.py, which tests/test_plot_reference.py pins to the live reference's recorded frames."""
import numpy as np

from tombo_amd import _native
import plot_reference as pr


class PlotStubEngine(object):
    def __init__(self):
        self.calls = []   # (method name, regions / segments / pairs) of every call, for the tests
        self.last_plot_kernel_ms = 0.0

    def region_level_piles(self, read_start, read_minus, read_off, means, reg_read_off, reg_reads, reg_start, reg_end,
                           q_linear=None, q_nearest=None, want_levels=True):
        rs, rm, off, m, roff, rr, st, en, ql, qn, cap = _native._check_region_level_piles_args(
            read_start, read_minus, read_off, means, reg_read_off, reg_reads, reg_start, reg_end, q_linear, q_nearest)
        self.calls.append(('region_level_piles', st.shape[0]))
        pile_off, levels = pr.level_piles(rs, rm, off, m, roff, rr, st, en)
        assert levels.shape[0] <= cap
        lin, near = pr.segment_percentiles(levels, pile_off, ql, qn)
        return (pile_off, levels if want_levels else None, None if q_linear is None else lin,
                None if q_nearest is None else near)

    def segment_percentiles(self, values, off, q_linear, q_nearest):
        v, off, ql, qn = _native._check_segment_percentiles_args(values, off, q_linear, q_nearest)
        self.calls.append(('segment_percentiles', off.shape[0] - 1))
        return pr.segment_percentiles(v, off, ql, qn)

    def region_raw_signal(self, raw, raw_off, segs, segs_off, read_start, rsrtr, minus, rna, shift, scale, lower_lim,
                          upper_lim, pair_read, pair_start, pair_end, genome_centric=True):
        args = _native._check_region_raw_signal_args(raw, raw_off, segs, segs_off, read_start, rsrtr, minus, rna, shift,
                                                     scale, lower_lim, upper_lim, pair_read, pair_start, pair_end)
        self.calls.append(('region_raw_signal', args[12].shape[0]))
        out = pr.raw_signal(*args[:-1], genome_centric=genome_centric)
        assert np.array_equal(np.diff(out[0]), args[-1])      # the binding's sample counts are the reference's
        return out

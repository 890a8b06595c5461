"""Reads that take the traceback walkers off their fast paths (helper module of test_tb_cases_reference.py and
test_gpu_tb_paths.py; no tests of its own).

The synthetic generator gives every base 8-9 events at the most and keeps the path within ~15 cells of the middle of
the band, so a read of its making only ever meets the 64-cell window of tbp_block (k_tb_par.h) and the 16-31 cell
look-back of k_main_tb_long (k_long.h).  A STUTTER -- one base whose level flickers by a sixth of a model unit, nine
samples at a time -- makes event detection cut that base into J events that the forward pass then assigns to it: a
stay run of J - 1 cells in one row of the move matrix, wherever the test wants that row.  Long enough, the run carries
the path to the edge of the band and the read fails with TBA_BEYOND_BANDWIDTH.

The tables below were found by search on the CPU oracle (a read is (bandwidth, nb, seed, where, J): the stutter follows
base `where` of synth_read(model, nb, seed)) and are kept as literals: test_tb_cases_reference.py holds every row
to what it claims, so that an edited table fails there and not silently on the GPU.
"""
import collections

import numpy as np

TBA_BEYOND_BANDWIDTH = 11
TBP_MIN_CHUNK = 64      # k_tb_par.h
LANES = {'latency': 64, 'throughput': 16}   # lanes per read of the chunk kernel of a dispatch form
TOP_OFFSETS = (1, 0, -1, -2, -15, -16, -17)

Case = collections.namedtuple('Case', 'bandwidth nb seed where J')


def dna():
    """(model, {bandwidth: params}): the DNA model and the resquiggle parameters of the four band widths"""
    from tombo_amd import tombo_stats as ts, tombo_helper as th
    samp = th.seqSampleType('DNA', False)
    model = ts.TomboModel(seq_samp_type=samp)
    base = ts.load_resquiggle_parameters(samp)
    params = {bw: base._replace(bandwidth=bw) for bw in (300, 500, 1000)}
    params[100] = base._replace(bandwidth=100, band_bound_thresh=10)     # (the default 40 fails every read at W = 100)
    return model, params


def samp_ind(nb, seed):
    """np.random.choice(nb, 1000, replace=False) under `seed` for reads of more than 1000 bases (Theil-Sen)"""
    if nb <= 1000:
        return None
    st = np.random.get_state()
    np.random.seed(seed % (1 << 32))
    si = np.random.choice(nb, 1000, replace=False)
    np.random.set_state(st)
    return si


def stutter_read(model, nb, seed, where, J, amp=2.0, noise_sd=0.6, seg=9, noise_seed=None):
    """synth_read(model, nb, seed, **DNA_SYNTH) with J segments of `seg` samples inserted after the samples of base
    `where`: alternately `amp` raw units above and below the mean of that base's own samples, plus N(0, noise_sd).
    The sequence is unchanged.  J = 0 (or where None): the plain read.  -> (seq, raw)"""
    from tombo_amd import synth
    seq, raw, starts = synth.synth_read(model, nb, seed, **synth.DNA_SYNTH)
    if not J or where is None:
        return seq, raw
    a, b = int(starts[where]), int(starts[where + 1])
    level = raw[a:b].mean()
    rng = np.random.default_rng([seed, where, J] if noise_seed is None else noise_seed)
    sign = np.where(np.arange(J) % 2 == 0, 1.0, -1.0)
    ins = np.repeat(level + amp * sign, seg) + rng.normal(0.0, noise_sd, J * seg)
    return seq, np.concatenate([raw[:b], ins, raw[b:]])


def make_read(model, case):
    """a Case as a read of tests/test_gpu_parity.run_batch: (raw, seq, stall_ints, samp_ind)"""
    seq, raw = stutter_read(model, case.nb, case.seed, case.where, case.J)
    return raw, seq, None, samp_ind(case.nb, case.seed)


def oracle_read(model, params, case):
    """the oracle's result for a Case, with what run_batch gives the oracle for the same read"""
    from test_gpu_parity import _oracle_read
    raw, seq, _, si = make_read(model, case)
    return _oracle_read(model, params, raw, seq, 5.0, 'DNA', samp_ind=si)


def chunk_tops(B, n_static, lpr):
    """tbp_chunks (k_tb_par.h) restated: (L, [hi_0, hi_1, ...]) -- chunk c is rows (hi_c - L, hi_c] and the lowest
    chunk goes down to row 1, the static rows included"""
    top_rows = max(1, B - (n_static + 16))
    L = max(TBP_MIN_CHUNK, -(-top_rows // lpr))
    n_chunks = -(-top_rows // L)
    return L, [B - c * L for c in range(n_chunks)]


def run_profile(o):
    """of an oracle result (debug=True): (events per base = np.diff(read_tb), band position leaving each row =
    read_tb[:B] - 1 - band_event_starts).  Base i is walked in row i + 1 of the move matrix: n events on it are
    n - 1 stay cells in that row."""
    d = o['dbg']
    tb = np.asarray(d['read_tb'])
    B = tb.shape[0] - 1
    return np.diff(tb), tb[:B] - 1 - np.asarray(d['band_event_starts'])[:B]


def longest_run(o):
    """(row, events) of the base with the most events"""
    per_base, _ = run_profile(o)
    i = int(np.argmax(per_base))
    return i + 1, int(per_base[i])


def top_offset(row, tops):
    """(c, row - hi_c) for the chunk top c >= 1 nearest to `row`"""
    c = min(range(1, len(tops)), key=lambda k: abs(row - tops[k]))
    return c, row - tops[c]


def _band_class(W):
    """cpl_class (k_dp.h): cells per lane of the band class"""
    return next(c for c in (4, 5, 8, 12, 16, 24, 32, 48) if 64 * c >= W)


def strip_s0(W):
    """mv_strip_s0 (k_dp.h): first cell of the centre strip, -1 without one"""
    c = _band_class(W)
    if c not in (4, 8, 16, 32):
        return -1
    unit = max(c, 16)
    s0 = ((W // 2 - 40) // unit) * unit
    return s0 if s0 >= 0 and s0 + 64 <= 64 * c else -1


def window_start(o, case, lanes):
    """tbp_block's window placement restated for the walker that walks the run row of `case` on the true path (phase A
    of its chunk at `lanes` lanes per read; chunk 0 and the serial walk place it alike away from the top of the read):
    the first cell of the 64-cell window fetched for that row -- 16 * ((guess >> 4) - 2) clamped to the row, or the
    strip's -- where the guess is the position the walker had on entering the block of 16 rows"""
    _, pos = run_profile(o)
    n_static = int(o['dbg']['mask_seq_len'])
    _, tops = chunk_tops(case.nb, n_static, lanes)
    rr, W = case.where + 1, case.bandwidth
    hi = min(t for t in tops if t >= rr)
    r0 = hi - 16 * ((hi - rr) // 16)
    assert r0 < case.nb, 'the top block of the read starts from top_pos'
    guess = W // 2 if r0 == hi else int(pos[r0])         # pos[r0]: leaving row r0 + 1
    wb = min(max((guess >> 4) - 2, 0), 4 * _band_class(W) - 4)
    s0 = strip_s0(W)
    if s0 >= 0 and r0 - 15 > n_static and s0 + 24 <= guess < s0 + 60:
        wb = s0 >> 4
    return 16 * wb


# ---- the tables -------------------------------------------------------------------------------------------------
# The run-length ladder, per band width: ((fewest, most events), read) -- the read's longest run, on base `where`, lies in
# the bucket.  10-16: inside every look-back; 17-32: past k_main_tb_long's guaranteed 16 cells; 33-47: from the lower
# half of tbp_block's window, or out of it; 48-64; >= 66: 65 stay cells leave a 64-cell window wherever it lies; >= 100.
# (W = 100: rows of 16 dwords, the window start is clamped; the band holds no longer run.  W = 1000: class 16.)
LADDER = {
    500: [
        ((10, 16), Case(500, 2000, 3, 1200, 12)),   # 13 events
        ((17, 32), Case(500, 2000, 3, 1200, 24)),   # 26 events
        ((33, 47), Case(500, 2000, 3, 1200, 38)),   # 40 events
        ((48, 64), Case(500, 2000, 3, 1200, 54)),   # 56 events
        ((66, 99), Case(500, 2000, 3, 1200, 78)),   # 80 events
        ((100, None), Case(500, 2000, 3, 1200, 110)),   # 114 events
    ],
    300: [
        ((10, 16), Case(300, 2000, 3, 1200, 12)),   # 13 events
        ((17, 32), Case(300, 2000, 3, 1200, 24)),   # 26 events
        ((33, 47), Case(300, 2000, 3, 1200, 38)),   # 40 events
        ((48, 64), Case(300, 2000, 3, 1200, 54)),   # 56 events
        ((66, 99), Case(300, 2000, 3, 1200, 78)),   # 80 events
        ((100, None), Case(300, 2000, 3, 1200, 110)),   # 114 events
    ],
    100: [
        ((10, 16), Case(100, 2000, 3, 1200, 12)),   # 13 events
        ((17, 32), Case(100, 2000, 3, 1200, 24)),   # 26 events
        ((33, 47), Case(100, 2000, 3, 1200, 38)),   # 40 events
    ],
    1000: [
        ((66, 99), Case(1000, 2000, 3, 1200, 78)),   # 80 events
        ((100, None), Case(1000, 2000, 3, 1200, 110)),   # 114 events
    ],
}
# The fine sweep, per band width: (the first read, how many) -- read k has J + k segments: runs of nearly every length
# from 17 to 66.  The end of such a run stays where it is (the band puts it on W / 2) and the position the walk enters
# the row at moves up cell by cell: every alignment to the dwords and the two halves of tbp_block's window, the answer
# from the upper half, from the lower half, and from under the window.
SWEEP = {300: (Case(300, 2000, 3, 1200, 16), 50), 500: (Case(500, 2000, 3, 1200, 16), 50)}

# Runs that end on the cell just under tbp_block's window (window_start - 1), per band width, the same for 16 and 64
# lanes per read: (read, position on leaving the row).  Every cell of the window at or below the position is a stay,
# the slow path of the row takes over at window_start - 1, and the end of the run is that very cell where the walk
# leaves the row one under window_start by a move along the row, or two under it by a diagonal move (which of the two
# a read_tb does not show: the table has both kinds, and a restart position one cell too low loses about half of them).
UNDER_WINDOW = {
    300: [(Case(300, 2000, 3, 1053, 41), 95), (Case(300, 2000, 3, 1054, 45), 95), (Case(300, 2000, 4, 1040, 35), 111),
          (Case(300, 2000, 4, 1049, 34), 111), (Case(300, 2000, 4, 1055, 36), 111), (Case(300, 2000, 5, 1055, 37), 111),
          (Case(300, 2000, 3, 1048, 35), 110), (Case(300, 2000, 3, 1049, 37), 110), (Case(300, 2000, 3, 1053, 43), 94),
          (Case(300, 2000, 3, 1054, 46), 94), (Case(300, 2000, 3, 1057, 38), 110), (Case(300, 2000, 3, 1059, 34), 110)],
    500: [(Case(500, 2000, 3, 1048, 37), 207), (Case(500, 2000, 3, 1054, 34), 207), (Case(500, 2000, 3, 1057, 37), 207),
          (Case(500, 2000, 4, 1040, 39), 207), (Case(500, 2000, 4, 1048, 34), 207), (Case(500, 2000, 5, 1053, 35), 207),
          (Case(500, 2000, 3, 1054, 36), 206), (Case(500, 2000, 3, 1059, 38), 206),
          (Case(500, 2000, 4, 1040, 40), 206), (Case(500, 2000, 4, 1043, 39), 206), (Case(500, 2000, 4, 1048, 36), 206)],
}

# Runs of >= 66 events on the bases just after the masked start, W = 500: (base - n_static, read) -- where tbp_block's
# strip turns on (rows above n_static + 15) and where the lowest chunk takes over all static rows.
AFTER_STATIC = [
    (0, Case(500, 2000, 3, 116, 80)),    # 84 events, n_static 116
    (16, Case(500, 2000, 5, 134, 80)),   # 83 events, n_static 118
    (17, Case(500, 2000, 4, 137, 80)),   # 83 events, n_static 120
]

# Runs of >= 66 events around chunk tops, per (band width, lanes per read): (which top, row - hi_c, read) with the row
# of the run = where + 1.  first: c = 1; middle: c = n_chunks // 2; last: c = n_chunks - 1, whose chunk owns the static
# rows.  Offset 0: the first row of a lane's phase A (from the W / 2 guess), of the upper lane's phase B and of the
# verifier; +1: the upper lane hands over a state straight out of the run; -16: the first row of phase B's second block.
# (A stutter near the start of a read moves n_static, and with it L and the tops: the geometry is that of the read itself.)
CHUNK_TOPS = {
    (300, 16): [
        ('first', 1, Case(300, 2000, 3, 1881, 80)),   # 85 events
        ('first', 0, Case(300, 2000, 3, 1880, 80)),   # 82 events
        ('first', -1, Case(300, 2000, 3, 1879, 80)),   # 81 events
        ('first', -2, Case(300, 2000, 3, 1878, 80)),   # 83 events
        ('first', -15, Case(300, 2000, 4, 1865, 80)),   # 81 events
        ('first', -16, Case(300, 2000, 5, 1864, 80)),   # 84 events
        ('first', -17, Case(300, 2000, 6, 1862, 80)),   # 83 events
        ('middle', 1, Case(300, 2000, 3, 1048, 80)),   # 81 events
        ('middle', 0, Case(300, 2000, 4, 1047, 80)),   # 82 events
        ('middle', -1, Case(300, 2000, 3, 1046, 80)),   # 82 events
        ('middle', -2, Case(300, 2000, 8, 1045, 80)),   # 82 events
        ('middle', -15, Case(300, 2000, 3, 1032, 80)),   # 83 events
        ('middle', -16, Case(300, 2000, 4, 1031, 80)),   # 81 events
        ('middle', -17, Case(300, 2000, 4, 1030, 80)),   # 82 events
        ('last', 1, Case(300, 2000, 6, 200, 80)),   # 81 events
        ('last', 0, Case(300, 2000, 6, 199, 80)),   # 82 events
        ('last', -1, Case(300, 2000, 9, 198, 80)),   # 83 events
        ('last', -2, Case(300, 2000, 6, 197, 80)),   # 81 events
        ('last', -15, Case(300, 2000, 6, 184, 80)),   # 80 events
        ('last', -16, Case(300, 2000, 6, 183, 80)),   # 82 events
        ('last', -17, Case(300, 2000, 6, 182, 80)),   # 83 events
    ],
    (300, 64): [
        ('first', 1, Case(300, 2000, 3, 1936, 80)),   # 71 events
        ('first', 0, Case(300, 2000, 3, 1935, 80)),   # 81 events
        ('first', -1, Case(300, 2000, 4, 1934, 80)),   # 83 events
        ('first', -2, Case(300, 2000, 3, 1933, 80)),   # 82 events
        ('first', -15, Case(300, 2000, 3, 1920, 80)),   # 82 events
        ('first', -16, Case(300, 2000, 3, 1919, 80)),   # 77 events
        ('first', -17, Case(300, 2000, 4, 1918, 80)),   # 80 events
        ('middle', 1, Case(300, 2000, 4, 1040, 80)),   # 81 events
        ('middle', 0, Case(300, 2000, 3, 1039, 80)),   # 81 events
        ('middle', -1, Case(300, 2000, 3, 1038, 80)),   # 81 events
        ('middle', -2, Case(300, 2000, 3, 1037, 80)),   # 82 events
        ('middle', -15, Case(300, 2000, 3, 1024, 80)),   # 82 events
        ('middle', -16, Case(300, 2000, 3, 1023, 80)),   # 83 events
        ('middle', -17, Case(300, 2000, 3, 1022, 80)),   # 82 events
        ('last', 1, Case(300, 2000, 3, 144, 80)),   # 85 events
        ('last', 0, Case(300, 2000, 3, 143, 80)),   # 82 events
        ('last', -1, Case(300, 2000, 4, 142, 80)),   # 80 events
        ('last', -2, Case(300, 2000, 3, 141, 80)),   # 84 events
        ('last', -15, Case(300, 2000, 3, 128, 80)),   # 82 events
        ('last', -16, Case(300, 2000, 3, 127, 80)),   # 85 events
        ('last', -17, Case(300, 2000, 3, 126, 80)),   # 83 events
    ],
    (500, 16): [
        ('first', 1, Case(500, 2000, 5, 1884, 100)),   # 108 events
        ('first', 0, Case(500, 2000, 5, 1883, 100)),   # 102 events
        ('first', -1, Case(500, 2000, 3, 1882, 100)),   # 104 events
        ('first', -2, Case(500, 2000, 3, 1881, 100)),   # 106 events
        ('first', -15, Case(500, 2000, 4, 1868, 100)),   # 102 events
        ('first', -16, Case(500, 2000, 12, 1867, 100)),   # 102 events
        ('first', -17, Case(500, 2000, 3, 1866, 100)),   # 100 events
        ('middle', 1, Case(500, 2000, 3, 1072, 100)),   # 101 events
        ('middle', 0, Case(500, 2000, 5, 1071, 100)),   # 101 events
        ('middle', -1, Case(500, 2000, 5, 1070, 100)),   # 102 events
        ('middle', -2, Case(500, 2000, 3, 1069, 100)),   # 101 events
        ('middle', -15, Case(500, 2000, 5, 1056, 100)),   # 103 events
        ('middle', -16, Case(500, 2000, 3, 1055, 100)),   # 102 events
        ('middle', -17, Case(500, 2000, 3, 1054, 100)),   # 99 events
        ('last', 1, Case(500, 2000, 3, 260, 100)),   # 102 events
        ('last', 0, Case(500, 2000, 5, 259, 100)),   # 105 events
        ('last', -1, Case(500, 2000, 3, 258, 100)),   # 101 events
        ('last', -2, Case(500, 2000, 5, 257, 100)),   # 102 events
        ('last', -15, Case(500, 2000, 4, 229, 100)),   # 102 events
        ('last', -16, Case(500, 2000, 4, 228, 100)),   # 102 events
        ('last', -17, Case(500, 2000, 5, 227, 100)),   # 102 events
    ],
    (500, 64): [
        ('first', 1, Case(500, 2000, 4, 1936, 100)),   # 102 events
        ('first', 0, Case(500, 2000, 4, 1935, 100)),   # 103 events
        ('first', -1, Case(500, 2000, 4, 1934, 100)),   # 103 events
        ('first', -2, Case(500, 2000, 3, 1933, 100)),   # 102 events
        ('first', -15, Case(500, 2000, 3, 1920, 100)),   # 102 events
        ('first', -16, Case(500, 2000, 5, 1919, 100)),   # 101 events
        ('first', -17, Case(500, 2000, 4, 1918, 100)),   # 100 events
        ('middle', 1, Case(500, 2000, 3, 1104, 100)),   # 104 events
        ('middle', 0, Case(500, 2000, 5, 1103, 100)),   # 102 events
        ('middle', -1, Case(500, 2000, 5, 1102, 100)),   # 102 events
        ('middle', -2, Case(500, 2000, 4, 1101, 100)),   # 90 events
        ('middle', -15, Case(500, 2000, 4, 1088, 100)),   # 100 events
        ('middle', -16, Case(500, 2000, 5, 1087, 100)),   # 103 events
        ('middle', -17, Case(500, 2000, 3, 1086, 100)),   # 103 events
        ('last', 1, Case(500, 2000, 3, 144, 100)),   # 103 events
        ('last', 0, Case(500, 2000, 3, 143, 100)),   # 102 events
        ('last', -1, Case(500, 2000, 4, 142, 100)),   # 100 events
        ('last', -2, Case(500, 2000, 3, 141, 100)),   # 106 events
        ('last', -15, Case(500, 2000, 3, 128, 100)),   # 102 events
        ('last', -16, Case(500, 2000, 4, 127, 100)),   # 99 events
        ('last', -17, Case(500, 2000, 3, 126, 100)),   # 102 events
    ],
}
# Failing stutters at 24 consecutive bases spanning the middle chunk top, per (band width, lanes per read):
# (the first read, the oracle's statuses) -- read k has its stutter after base where + k.  A status 11 is a phase A's on
# the true path (the chunk kernel's own) or a phase B's (handed to k_main_tb, whose band-edge exit then gives it).
BAND_EDGE = {
    (300, 16): (Case(300, 2000, 4, 1036, 150),
        [0, 0, 11, 11, 11, 11, 11, 11, 11, 0, 0, 11, 11, 11, 0, 11, 0, 0, 0, 11, 0, 0, 11, 0]),
    (300, 64): (Case(300, 2000, 3, 1028, 150),
        [0, 0, 0, 0, 0, 0, 0, 11, 0, 0, 0, 0, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11]),
    (500, 16): (Case(500, 2000, 4, 1060, 280),
        [0, 0, 11, 11, 0, 11, 11, 11, 0, 0, 11, 11, 0, 0, 11, 11, 0, 11, 11, 11, 11, 0, 0, 11]),
    (500, 64): (Case(500, 2000, 4, 1092, 240),
        [0, 11, 11, 11, 11, 0, 0, 11, 11, 11, 0, 0, 11, 0, 11, 11, 11, 11, 11, 11, 11, 0, 11, 0]),
}

# Four reads past TBA_LONG_BASES (24 576) at W = 500: plain, a run of 20-31, a run of >= 66, a failing stutter.
LONG = [
    ('plain', Case(500, 24800, 21, None, 0)),       # longest run 11
    ('run 20-31', Case(500, 24800, 22, 12000, 23)), # 20 events
    ('run >= 66', Case(500, 24800, 24, 12000, 90)), # 93 events
    ('fail', Case(500, 24800, 24, 8000, 230)),
]

# The hand-back batch of the inject build (every read at an index = 3 mod 5 gets lane 1's entry under its chunk top
# hi_2 perturbed; throughput form, W = 500): (row - hi_2 at 16 lanes per read, read)
INJECT = [
    (0, Case(500, 2000, 14, 1767, 100)),    # 103 events
    (0, Case(500, 2000, 17, 1769, 100)),    # 102 events
    (-3, Case(500, 2000, 12, 1764, 100)),   # 99 events
    (-5, Case(500, 2000, 12, 1762, 100)),   # 102 events
]

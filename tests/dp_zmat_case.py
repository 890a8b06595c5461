"""Crafted z matrices for the forward pass's kernel (k_dp<CPL, true>, csrc/k_dp.h) and their reference: shared by
test_gpu_dp_lane_argmax.py and test_gpu_dp_first_cell.py.

The kernel is driven through tba_c_banded_forward_pass_adaptive: the caller's z matrix, N_STATIC static rows with
given band starts, adaptive rows behind them.  A row's band cells are its z row wherever its band lies, so the
reference is the oracle's forward pass over the same matrix (oracle.banded_forward_pass), with the adaptive rows' band
starts placed row by row from the first index of the maximum of the oracle's own previous row (pyx:342-358).

Every value is a multiple of 1/8 of moderate size (or -inf), the penalties multiples of 1/4: all sums are exact, ties
are plentiful in the random rows and exact where a case builds one.

Where an arg-max shows.  A row's arg-max is read by the NEXT adaptive row (band start = previous start + arg-max -
W // 2 + 1, never below the previous start: an arg-max in the left half of the band leaves the start where it was)
and, of the last row, as top_pos.  So a case that places a maximum anywhere in the band is a launch of its own whose
LAST row holds it: N_ROWS - 2 shared rows, a steering row (a single peak that fixes the last row's band offset) and the
crafted row, built from the reference's row before it."""
import numpy as np

SKIP_PEN, STAY_PEN = 1.5, 2.25
N_ROWS, N_STATIC = 70, 20        # 70 rows: past one 64-row block of the kernel's level registers
N_EVENTS = 1 << 20               # the adaptive rows never reach it
CLASSES = (4, 5, 8, 12)
LOW = -1000.0                    # a cell that must not win
PEAK = 20000.0                   # the value of a crafted maximum: above anything 70 rows of |z| <= 6 add up to
STEER = 5000.0


def band(cpl):
    """the class's widest band less three cells: the last lane with cells is partial"""
    return 64 * cpl - 3


def first_argmax(row):
    """c_argmax (pyx:186-197): the first index of the maximum"""
    return int(np.argmax(row))


def reference(z, static_starts, skip_pen=SKIP_PEN, stay_pen=STAY_PEN, prefix=None):
    """-> (fwd [n + 1, W], tb int64 [n + 1, W], starts [n], top_pos).  prefix: band starts already known (the rows
    they belong to are the same in z)"""
    import oracle
    z = np.ascontiguousarray(z, dtype=np.float64)
    n, W = z.shape
    starts = np.zeros(n, np.int64)
    starts[:len(static_starts)] = static_starts
    r0 = len(static_starts)
    if prefix is not None:
        starts[:len(prefix)] = prefix
        r0 = len(prefix)
    for r in range(r0, n):
        fwd, _ = oracle.banded_forward_pass(z[:r], starts[:r], skip_pen, stay_pen)
        cur = starts[r - 1] + first_argmax(fwd[r]) - W // 2 + 1
        cur = max(cur, starts[r - 1])
        assert cur < N_EVENTS
        starts[r] = cur
    fwd, tb = oracle.banded_forward_pass(z, starts, skip_pen, stay_pen)
    return fwd, tb, starts, first_argmax(fwd[n])


def run_gpu(z, static_starts, skip_pen=SKIP_PEN, stay_pen=STAY_PEN):
    """-> (rc, fwd, tb, starts, top_pos) of tba_c_banded_forward_pass_adaptive"""
    from tombo_amd.resquiggle import get_engine
    eng = get_engine(0)
    z = np.ascontiguousarray(z, dtype=np.float64)
    n, W = z.shape
    starts = np.zeros(n, np.int64)
    starts[:len(static_starts)] = static_starts
    fwd, tb, top = np.full((n + 1, W), 7.5), np.full((n + 1, W), -9, np.int64), np.full(1, -9, np.int64)
    rc = eng._L.tba_c_banded_forward_pass_adaptive(eng._h, z, n, W, starts, len(static_starts), N_EVENTS,
                                                   skip_pen, stay_pen, fwd, tb, top)
    return rc, fwd, tb, starts, int(top[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, ref, what):
    """forward rows bit for bit, moves (unpacked from the kernel's packed rows by the entry), band starts, top_pos"""
    rc, fwd, tb, starts, top = got
    rfwd, rtb, rstarts, rtop = ref
    assert rc == 0, (what, rc)
    assert np.array_equal(starts, rstarts), (what, np.flatnonzero(starts != rstarts)[:5])
    bad = np.argwhere(bits(fwd) != bits(rfwd))
    assert bad.size == 0, (what, 'forward rows', bad[:5].tolist())
    # One cell's move is not compared: band cell 0 where its forward value is -inf (it only is under skip_pen = +inf).
    # c_banded_forward_pass writes that cell's move -- skip or diagonal, by the band offset -- without a comparison;
    # the kernel derives it like every cell's, move = candidate > stay value ? the candidate's : stay, and -inf is not
    # above the -inf that stands for cell 0's missing stay move.  No traceback reads a move of a -inf cell.
    differ = tb != rtb
    differ[:, 0] &= ~np.isneginf(rfwd[:, 0])
    bad = np.argwhere(differ)
    assert bad.size == 0, (what, 'moves', bad[:8].tolist())
    assert top == rtop, (what, top, rtop)


_base = {}


def base(cpl, skip_pen=SKIP_PEN, stay_pen=STAY_PEN, seed=0):
    """the rows every case of a class shares -> (z [N_ROWS, W], static starts, band starts of rows 0 .. N_ROWS - 2)"""
    key = (cpl, skip_pen, stay_pen, seed)
    if key not in _base:
        W = band(cpl)
        rng = np.random.default_rng(1000 * cpl + seed)
        z = rng.integers(-48, 33, (N_ROWS, W)) / 8.0
        static = np.cumsum(rng.integers(0, 4, N_STATIC)).astype(np.int64)
        _, _, starts, _ = reference(z[:N_ROWS - 1], static, skip_pen, stay_pen)
        _base[key] = (z, static, starts[:N_ROWS - 1].copy())
    return _base[key]


def tail_case(cpl, offset, build, skip_pen=SKIP_PEN, stay_pen=STAY_PEN):
    """the class's base matrix with its last two rows replaced: the steering row puts one peak where the last row's
    band then starts `offset` cells past the row before (0 .. 3: the kernel's register-renaming paths), and
    build(prev, offset) -> the last z row, from prev, the reference's forward row before it.
    -> (z, static starts, reference)"""
    z, static, pre = base(cpl, skip_pen, stay_pen)
    z = z.copy()
    W = z.shape[1]
    z[N_ROWS - 2] = LOW
    z[N_ROWS - 2, W // 2 - 1 + offset] = STEER
    fwd, _, starts, _ = reference(z[:N_ROWS - 1], static, skip_pen, stay_pen, prefix=pre)
    assert first_argmax(fwd[N_ROWS - 1]) == W // 2 - 1 + offset       # the steering peak is the row's maximum
    z[N_ROWS - 1] = build(fwd[N_ROWS - 1], offset)
    ref = reference(z, static, skip_pen, stay_pen, prefix=pre)
    assert ref[2][N_ROWS - 1] - ref[2][N_ROWS - 2] == offset
    return z, static, ref


def peaks_row(prev, offset, cells, value=PEAK, skip_pen=SKIP_PEN, stay_pen=STAY_PEN):
    """a z row whose cells `cells` all come out at exactly `value` and no other cell comes near it: the row is walked
    the way c_process_band walks it (cell b: stay from cell b - 1, diagonal from prev[b + offset - 1], skip from
    prev[b + offset]) and a wanted cell's z is what lifts the better of its stay and diagonal sources to `value`.
    Cell 0 has no z of its own at offset 0 (its only move is the skip)."""
    W = prev.shape[0]
    z = np.full(W, LOW)
    cur = np.empty(W)
    for b in range(W):
        src = b + offset - 1
        diag = prev[src] if 0 <= src < W else -np.inf
        stay = cur[b - 1] - stay_pen if b > 0 else -np.inf
        if b in cells:
            assert np.isfinite(max(stay, diag)) and not (b == 0 and offset == 0)
            z[b] = value - max(stay, diag)
        skip = prev[b + offset] - skip_pen if b + offset < W else -np.inf
        if b == 0:
            cur[0] = prev[0] - skip_pen if offset == 0 else prev[offset - 1] + z[0]
        else:
            cur[b] = max(stay + z[b], diag + z[b], skip)
        assert cur[b] == value if b in cells else cur[b] < value - 100
    return z

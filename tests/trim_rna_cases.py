"""Seeded signals and parameter sets of the trim_rna tests (tests/golden/gen_golden_trim_rna.py records the live
reference's answers for them; the tests rebuild the signals and check their SHA-256).

A signal: events of geometric dwell (6 samples or more, 15 on average) at normal levels, plus noise whose SD is
`head_sd` over the first `adapter_len` samples -- the DNA adapter: events with little spread -- and `body_sd` behind
(`ramp`: rising linearly from one to the other over the whole read instead).  Samples lie around 500 with a spread of
some 60, the range of DAC values, so the int16 rounding of a signal is a plausible raw read."""
from collections import namedtuple

import numpy as np

RNA_SEG = (12, 6, 15)        # running_stat_width, min_obs_per_base, mean_obs_per_event of the RNA parameter set
DNA_SEG = (5, 3, 5)          # ... of the DNA one
DEFAULT_TRIM = (50, 100, 0.7, 40000)   # moving_window_size, min_running_values, thresh_scale, max_raw_obs

Case = namedtuple('Case', 'name seed n adapter_len ramp seg trim')


def _trim(mw=50, mr=100, ts=0.7, mro=40000):
    return (mw, mr, ts, mro)


CASES = [
    # lengths at the defaults: the error, zero windows, one window, around the cap
    Case('n2234', 1, 2234, 600, False, RNA_SEG, DEFAULT_TRIM),
    Case('n2235', 2, 2235, 600, False, RNA_SEG, DEFAULT_TRIM),
    Case('n2249', 3, 2249, 0, False, RNA_SEG, DEFAULT_TRIM),
    Case('n2250', 4, 2250, 0, False, RNA_SEG, DEFAULT_TRIM),
    Case('n39999', 5, 39999, 9000, False, RNA_SEG, DEFAULT_TRIM),
    Case('n40000', 6, 40000, 14000, False, RNA_SEG, DEFAULT_TRIM),
    Case('n40001', 7, 40001, 4000, False, RNA_SEG, DEFAULT_TRIM),
    Case('n70000', 8, 70000, 21000, False, RNA_SEG, DEFAULT_TRIM),
    # the branches: the first window answers (no adapter), the last one does (the noise steps up over the last 50
    # events or so and thresh_scale lies between the two largest minima, 1.7399 and 1.7489 times the mean), none does
    Case('first_window', 9, 12000, 0, False, RNA_SEG, DEFAULT_TRIM),
    Case('last_window', 10, 12000, 11350, False, RNA_SEG, _trim(mr=1, ts=1.745)),
    Case('no_window', 11, 12000, 3000, False, RNA_SEG, _trim(ts=5.0)),
    # off the defaults
    Case('mw1', 12, 9000, 2500, False, RNA_SEG, _trim(mw=1, mr=3)),
    Case('mw8', 13, 9000, 2500, False, RNA_SEG, _trim(mw=8, mr=20)),
    Case('mw9', 14, 9000, 2500, False, RNA_SEG, _trim(mw=9, mr=20)),
    Case('mw128', 15, 9000, 2500, False, RNA_SEG, _trim(mw=128)),
    Case('mw130', 16, 9000, 2500, False, RNA_SEG, _trim(mw=130)),
    Case('mr1', 17, 9000, 2500, False, RNA_SEG, _trim(mr=1)),
    Case('ts0', 18, 9000, 2500, False, RNA_SEG, _trim(ts=0.0)),
    Case('cap_below', 19, 30000, 6000, False, RNA_SEG, _trim(mro=20000)),
    Case('cap_above', 20, 30000, 6000, False, RNA_SEG, _trim(mro=50000)),
    Case('cap150k', 21, 150000, 40000, False, RNA_SEG, _trim(mro=150000)),   # 9 852 means: beyond one 8192 block
    Case('dna_seg', 22, 20000, 5000, False, DNA_SEG, DEFAULT_TRIM),
    Case('wide_stat', 23, 9000, 2500, False, (40, 6, 15), DEFAULT_TRIM),     # 2 * running_stat_width > 64
    # too short for the detector at all
    Case('fewer_cpts', 24, 60, 0, False, RNA_SEG, DEFAULT_TRIM),
]
BY_NAME = dict((c.name, c) for c in CASES)


def signal(case, head_sd=1.5, body_sd=7.0):
    rng = np.random.default_rng(730000 + case.seed)
    n = case.n
    dwell = 5 + rng.geometric(1.0 / 10.0, size=n // 6 + 2)
    levels = rng.normal(500.0, 60.0, size=dwell.shape[0])
    base = np.repeat(levels, dwell)[:n]
    pos = np.arange(n)
    if case.ramp:
        sd = head_sd + (body_sd - head_sd) * pos / max(n - 1, 1)
    else:
        sd = np.where(pos < case.adapter_len, head_sd, body_sd)
    return base + rng.normal(0.0, 1.0, size=n) * sd


def dac(raw):
    """the int16 DAC rounding of a float signal"""
    return np.round(raw).astype(np.int16)

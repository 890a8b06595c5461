"""ts.trim_rna (tombo/tombo_stats.py:235-267) restated in numpy, with the change-point detector and the segment SDs
passed in: over `oracle.valid_cpts` / `oracle.new_mean_stds` it is pinned to the live reference
(tests/test_trim_rna_reference.py, tests/golden/stats_trim_rna.npz) and serves the GPU tests as the expected answer on any
input, int16 DAC samples included (where the reference's own answer depends on numpy's argsort).

Every sum is spelled so that numpy adds in the order the reference's expressions do: a row mean is
np.add.reduce of a contiguous copy of the row divided by its length (what `.mean(-1)` of the as_strided rows gives),
the mean of the means is `.mean()` of a contiguous vector.
"""
import numpy as np

FEWER_CPTS_MSG = 'Fewer changepoints found than requested'
TOO_FEW_EVENTS_MSG = 'negative dimensions are not allowed'


class TomboErrorLike(Exception):
    """stands for th.TomboError where no Tombo module is imported"""


def window_stage(sds, cpts, moving_window_size, min_running_values, thresh_scale):
    """steps 4-8: the SDs of a read's events and its change points -> the adapter end"""
    mw, mr = int(moving_window_size), int(min_running_values)
    sds = np.ascontiguousarray(sds, dtype=np.float64)
    n_means = sds.shape[0] - mw + 1
    if n_means < 0 or n_means - mr + 1 < 0:
        raise ValueError(TOO_FEW_EVENTS_MSG)
    n_runs = n_means - mr + 1
    if n_runs == 0:
        return 0
    means = np.array([np.add.reduce(sds[i:i + mw].copy()) / mw for i in range(n_means)], dtype=np.float64)
    thresh = means.mean() * thresh_scale
    mins = np.array([means[i:i + mr].min() for i in range(n_runs)])
    above = np.nonzero(mins > thresh)[0]
    return int(cpts[above[0]]) if above.shape[0] else 0


def trim_rna(raw, seg_params, trim_params, valid_cpts, new_mean_stds, tombo_error=TomboErrorLike):
    """seg_params: (running_stat_width, min_obs_per_base, mean_obs_per_event); trim_params: (moving_window_size,
    min_running_values, thresh_scale, max_raw_obs); valid_cpts(x, min_obs_per_base, width, num) -> (rc, sorted change
    points), rc 2: fewer than requested; new_mean_stds(x, cpts) -> (means, sds)"""
    width, min_obs, mean_obs = seg_params
    mw, mr, thresh_scale, max_raw_obs = trim_params
    x = np.asarray(raw)[:max_raw_obs].astype(np.float64)
    num_events = x.shape[0] // mean_obs
    rc, cpts = valid_cpts(x, min_obs, width, num_events)
    if rc == 2:
        raise tombo_error(FEWER_CPTS_MSG)
    assert rc == 0, rc
    _, sds = new_mean_stds(x, cpts)
    return window_stage(sds, cpts, mw, mr, thresh_scale)

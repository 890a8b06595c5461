"""The host layer of `tombo plot kmer` (plot_commands.kmer_dist_plot_data) through a stub engine built on the numpy
restatement: every recorded case of the live reference, every error and warning, the binding's declarations."""
import os
import re
import warnings

import numpy as np
import pytest

from tombo_amd import _native, plot_commands as pc, tombo_helper as th
import kmer_dist_cases as kc
from kmer_dist_cases import Read
from kmer_dist_stub_engine import KmerDistStubEngine


@pytest.mark.parametrize('case', kc.kmer_cases(), ids=lambda c: c['name'])
def test_recorded_case(case):
    eng = KmerDistStubEngine()
    kc.check_case(case, eng)
    assert len(eng.calls) <= 1       # one engine call does all the numbers


def _reads(rng, n_reads=3, n=300):
    return [Read(rng.standard_normal(n), ''.join('ACGT'[i] for i in rng.integers(0, 4, n)), 'r%d' % i)
            for i in range(n_reads)]


def test_exit_and_warning_texts():
    rng = np.random.default_rng(1)
    reads = _reads(rng)
    with pytest.raises(th.TomboError) as err:
        pc.kmer_dist_plot_data(reads[:1], True, 0, 1, 1, 5, engine=KmerDistStubEngine())
    assert str(err.value) == pc.KMER_DIST_NO_READS_ERROR and str(err.value).startswith('No valid reads present.\n\t\tCheck')
    with pytest.raises(th.TomboError):
        pc.kmer_dist_plot_data([Read(None, 'ACGT', 'x')], True, 0, 1, 1, 5, engine=KmerDistStubEngine())
    with pytest.raises(th.TomboError):
        pc.kmer_dist_plot_data([], True, 0, 1, 1, 5, engine=KmerDistStubEngine())
    with pytest.warns(UserWarning) as caught:
        pc.kmer_dist_plot_data(reads, True, 0, 1, 1, 5, engine=KmerDistStubEngine())
    assert [str(w.message) for w in caught] == [pc.KMER_DIST_FEW_READS_WARNING]
    assert pc.KMER_DIST_FEW_READS_WARNING.startswith('Fewer valid reads present than requested.\n\tConsider')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        pc.kmer_dist_plot_data(reads, True, 0, 1, 1, 3, engine=KmerDistStubEngine())


def test_value_errors():
    rng = np.random.default_rng(2)
    reads = _reads(rng)
    run = (lambda rds, up=0, dn=1: pc.kmer_dist_plot_data(rds, True, up, dn, 1, 3, engine=KmerDistStubEngine()))
    for up, dn in ((5, 0), (0, 5), (-1, 1), (1.5, 1)):
        with pytest.raises(ValueError, match='integer in \\[0, 4\\]'):
            run(reads, up, dn)
    with pytest.raises(ValueError, match='differ in number'):
        run(reads + [Read(np.zeros(5), 'ACGTAC', 'bad')])
    with pytest.raises(ValueError, match='outside ACGT'):
        run(reads + [Read(np.zeros(5), 'ACNTA', 'bad')])
    nan = reads[0].means.copy()
    nan[7] = np.nan
    with pytest.raises(ValueError, match='NaN level'):
        run([Read(nan, reads[0].seq, 'bad')] + reads)
    many = [Read(np.zeros(1), 'A', 'tiny')] * (2 ** 27 // 4 ** 9 + 1)
    with pytest.raises(ValueError, match='table limit of 2\\*\\*27'):
        run(many, 4, 4)


def test_binding_checks_and_declarations():
    ok = (np.zeros(4), np.zeros(4, dtype=np.uint8), np.array([0, 4], dtype=np.int64))
    _native._check_kmer_dist_args(*ok, 2, 1, 0, 3)
    for bad in ((ok[0].astype(np.float32), ok[1], ok[2], 2, 1, 0, 3), (ok[0], ok[1].astype(np.int8), ok[2], 2, 1, 0, 3),
                (ok[0], ok[1], ok[2].astype(np.int32), 2, 1, 0, 3), (ok[0], ok[1], np.array([1, 4], dtype=np.int64), 2, 1, 0, 3),
                ok + (0, 0, 0, 3), ok + (10, 0, 0, 3), ok + (2, 2, 0, 3), ok + (2, -1, 0, 3), ok + (2, 1, 0.5, 3),
                (ok[0][:3], ok[1], ok[2], 2, 1, 0, 3),
                (ok[0], ok[1], np.zeros(2 ** 27 // 4 ** 9 + 2, dtype=np.int64) + np.r_[0, [4] * (2 ** 27 // 4 ** 9 + 1)], 9, 0, 0, 3)):
        with pytest.raises(ValueError):
            _native._check_kmer_dist_args(*bad)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    hdr = open(os.path.join(root, 'include', 'tombo_amd.h')).read()
    assert len(re.findall(r'\bint tba_kmer_dist\(', hdr)) == 1
    assert len(_native.PROTOTYPES['tba_kmer_dist'][1]) == 20
    assert hasattr(_native.Engine, 'kmer_dist')
    assert 'k_kmer_dist.h' in open(os.path.join(root, 'tombo_amd', 'csrc', 'tba_engine.hip')).read()


# ---- model overlays and per-read statistic frames (host only) ----
import model_overlay_cases as mc  # noqa: E402


@pytest.mark.parametrize('case', mc.meta()['kmers_cases'], ids=lambda c: c['name'])
def test_get_reg_kmers_and_model_frames(case):
    mc.check_kmers_case(case)


@pytest.mark.parametrize('case', mc.meta()['body_cases'], ids=lambda c: c['name'])
def test_plot_bodies(case):
    mc.check_body_case(case, mc.OverlayStubEngine())


def test_model_position_check_and_its_quirk():
    std = mc.models('k4_cp1')[0]
    with pytest.raises(th.TomboError) as err:
        pc.get_reg_kmers(std, mc.intervals([0]), mc.reads_index(0), alt_ref=mc.models('k4_cp2')[1])
    assert str(err.value) == mc.meta()['kmer_pos_error'] == pc.MODEL_KMER_POS_ERROR
    # another width passes: the reference compares alt_ref.kmer_width with itself
    pc.get_reg_kmers(std, mc.intervals([0]), mc.reads_index(0), alt_ref=mc.models('k3_cp1')[1])
    regs = mc.intervals([0])
    pc.get_reg_kmers(mc.models('k1_cp0')[0], regs, mc.reads_index(0))
    assert regs[0].seq == ''          # seq[0:-0]
    assert (pc.PLOT_PVAL_MAX, pc.PLOT_LLR_MAX) == (4, 4)


def test_motif_alt_model_needs_a_model_and_no_control():
    std, alt = mc.models('k3_cp1')
    locs = [(0.0, 0.5)]
    with pytest.raises(ValueError):
        pc.motif_with_stats_plot_data(mc.reads_index(0), mc.reads_index(1), mc.intervals([0]), locs, 5, std, alt_ref=alt)
    with pytest.raises(ValueError):
        pc.motif_with_stats_plot_data(mc.reads_index(0), None, mc.intervals([0]), locs, 5, None, alt_ref=alt)


def test_llr_trim_happens_in_the_callers_array():
    m = np.array([[9.0, -9.0, np.nan, 1.0], [0.5, 7.0, -1.0, 2.0]])
    stats, order = pc.get_reg_r_stats([('r', '-', m)], engine=mc.OverlayStubEngine())
    assert m[0, :2].tolist() == [4.0, -4.0] and m[1, 1] == 4.0
    assert stats['Stats'][:4].tolist()[0] == 1.0 and stats['Position'][:4].tolist() == [0.0, 1.0, 2.0, 3.0]
    assert sorted(order['Read'].tolist()) == [0.0, 1.0] and order['Region'].tolist() == ['r', 'r']

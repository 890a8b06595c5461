"""The numpy restatement of plot_kmer_dist (tests/kmer_dist_reference.py) against the live reference's recorded
frames (tests/golden/stats_kmer_dist.npz) and against the literal dict loop on random reads, by bits."""
import numpy as np
import pytest

import kmer_dist_reference as kr
import kmer_dist_cases as kc


def frames_from_arrays(res, K, up):
    """(kmer_levels, Kmer, Signal, Read) of the arrays Engine.kmer_dist returns"""
    label, n_sel, n_exam, counts, off, values, vlabel, kmer_mean = res
    order = kr.kmer_order(counts, kmer_mean)
    levels = [kr.kmer_string(int(q), K) for q in order]
    rows = np.concatenate([np.arange(off[q], off[q + 1]) for q in order] + [np.empty(0, dtype=np.int64)]).astype(np.int64)
    return levels, [levels[i] for i, q in enumerate(order) for _ in range(counts[q])], values[rows], vlabel[rows]


@pytest.mark.parametrize('case', kc.kmer_cases(), ids=lambda c: c['name'])
def test_restatement_and_dict_loop_equal_the_recorded_reference(case):
    z = kc.fixture()[0]
    reads = kc.case_reads(case)
    read_mean, up, dn, thresh, num_reads = kc.case_args(case)
    K = up + dn + 1
    added, levels, kmers, bases, sig, rid = kr.kmer_dist_dict_loop([(r.means, r.seq) for r in reads], *kc.case_args(case))
    res = kr.kmer_dist(*kr.pack_reads([(r.means, r.seq) for r in reads if r.means is not None]), K, up, thresh,
                       num_reads, read_mean)
    assert res[1] == added
    if case['exit'] is not None:
        assert added in (0, 1)
        return
    assert (added < num_reads) == bool(case['warnings'])
    get = (lambda k: z['kmer/%s/%s' % (case['name'], k)])
    assert levels == get('levels').tolist() and list(kmers) == get('Kmer').tolist()
    assert kc.same_bits(sig, get('Signal')) and [str(x) for x in rid] == get('Read').tolist()
    lv2, kmers2, sig2, rid2 = frames_from_arrays(res, K, up)
    assert lv2 == levels and kmers2 == list(kmers)
    assert kc.same_bits(sig2, get('Signal')) and [str(x) for x in rid2.tolist()] == get('Read').tolist()


@pytest.mark.parametrize('seed', range(4))
@pytest.mark.parametrize('read_mean', [True, False])
def test_restatement_equals_the_dict_loop_on_random_reads(seed, read_mean):
    rng = np.random.default_rng(seed)
    K, up = (1, 0) if seed == 0 else (2, int(rng.integers(0, 2))) if seed < 3 else (3, 1)
    reads = []
    for n in [1, 2, 7, 20000, 300, 9000, 40][:4 + seed]:
        p = np.array([0.9, 0.04, 0.03, 0.03]) if n >= 9000 else np.full(4, 0.25)   # runs past the 8192-value block
        reads.append((rng.standard_normal(n) * 3 + 90, ''.join('ACGT'[i] for i in rng.choice(4, n, p=p))))
    thresh = 0 if seed % 2 == 0 else 1
    added, levels, kmers, bases, sig, rid = kr.kmer_dist_dict_loop(reads, read_mean, up, K - 1 - up, thresh, 5)
    res = kr.kmer_dist(*kr.pack_reads(reads), K, up, thresh, 5, read_mean)
    assert res[1] == added
    lv2, kmers2, sig2, rid2 = frames_from_arrays(res, K, up)
    assert lv2 == levels and kmers2 == list(kmers) and rid2.tolist() == list(rid)
    assert kc.same_bits(sig2, np.array(sig, dtype=np.float64))


def test_selection_rule():
    c = np.array([[3, 3], [2, 5], [0, 9], [4, 3], [3, 4]], dtype=np.int64)
    assert kr.select_reads(c, 0, 3)[0].tolist() == [1, 2, 3, 0, 0]
    assert kr.select_reads(c, 1, 9)[0].tolist() == [1, 2, 0, 3, 4] and kr.select_reads(c, 1, 9)[1:] == (4, 5)
    assert kr.select_reads(c, 2, 9)[0].tolist() == [1, 0, 0, 2, 3]      # more than 2: 2 is rejected, 3 accepted
    assert kr.select_reads(c, 3, 9)[0].tolist() == [0, 0, 0, 0, 0]
    label, n_sel, n_exam = kr.select_reads(c, 2, 2)
    assert (label.tolist(), n_sel, n_exam) == ([1, 0, 0, 2, 0], 2, 4)
    assert kr.select_reads(c, 1, 0)[1:] == (1, 1) and kr.select_reads(c[2:], 1, 0)[1:] == (0, 1)

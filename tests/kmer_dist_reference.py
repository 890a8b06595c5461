"""TEST INFRASTRUCTURE: the numbers of `tombo plot kmer` (plot_kmer_dist, tombo/_plot_commands.py:451-559) in numpy:
`kmer_dist` returns the arrays `tba_kmer_dist` / `Engine.kmer_dist` returns, `kmer_dist_dict_loop` is a literal copy
of the reference's dict loop (reads given as (means, sequence string)), for cross-checking the restatement.
tests/test_kmer_dist_reference.py pins both to the live reference's recorded frames."""
from collections import defaultdict
from itertools import repeat
from operator import itemgetter

import numpy as np

BASES = 'ACGT'


def kmer_string(index, K):
    return ''.join(BASES[(index >> (2 * (K - 1 - j))) & 3] for j in range(K))


def encode(seq):
    """str -> uint8 codes (0..3 = ACGT, 4: anything else)"""
    lut = np.full(256, 4, dtype=np.uint8)
    for i, b in enumerate(BASES):
        lut[ord(b)] = i
    return lut[np.frombuffer(seq.encode(), dtype=np.uint8)]


def pack_reads(reads):
    """[(means, seq str)] -> (means float64, codes uint8, read_off int64)"""
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for _, s in reads])
    means = np.concatenate([np.asarray(m, dtype=np.float64) for m, _ in reads]) if reads else np.empty(0)
    codes = np.concatenate([encode(s) for _, s in reads]) if reads else np.empty(0, dtype=np.uint8)
    return means.astype(np.float64), codes.astype(np.uint8), off


def read_window_keys(codes, K):
    """the k-mer index of every window of one read, -1 where a base is outside ACGT"""
    n_win = max(codes.shape[0] - K + 1, 0)
    key = np.zeros(n_win, dtype=np.int64)
    ok = np.ones(n_win, dtype=bool)
    for j in range(K):
        c = codes[j:j + n_win].astype(np.int64)
        ok &= c < 4
        key = key * 4 + (c & 3)
    return np.where(ok, key, -1)


def select_reads(counts_per_read, kmer_thresh, num_reads):
    """rule 3 / 4 of the issue over int64[n_reads, 4**K] -> (label int64[n_reads], n_sel, n_examined)"""
    n_reads, n_kmers = counts_per_read.shape
    label = np.zeros(n_reads, dtype=np.int64)
    added = examined = 0
    for r in range(n_reads):
        examined += 1
        c = counts_per_read[r]
        if kmer_thresh == 0 or (np.count_nonzero(c) == n_kmers and (kmer_thresh == 1 or int(c.min()) > kmer_thresh)):
            added += 1
            label[r] = added
        if added >= num_reads:
            break
    return label, added, examined


def kmer_dist(means, codes, read_off, kmer_width, central_pos, kmer_thresh, num_reads, read_mean):
    """-> (read_label, n_sel, n_examined, counts, off, values, value_label, kmer_mean), as Engine.kmer_dist"""
    K, n_reads, n_kmers = int(kmer_width), read_off.shape[0] - 1, 4 ** int(kmer_width)
    keys, levels = [], []
    per_read = np.zeros((n_reads, n_kmers), dtype=np.int64)
    for r in range(n_reads):
        s, e = int(read_off[r]), int(read_off[r + 1])
        key = read_window_keys(codes[s:e], K)
        lv = means[s + central_pos:s + central_pos + key.shape[0]]
        keys.append(key[key >= 0])
        levels.append(lv[key >= 0])
        per_read[r] = np.bincount(keys[-1], minlength=n_kmers)
    label, n_sel, n_exam = select_reads(per_read, kmer_thresh, num_reads)
    ent_val = [[] for _ in range(n_kmers)]
    ent_lab = [[] for _ in range(n_kmers)]
    for r in np.flatnonzero(label):
        order = np.argsort(keys[r], kind='stable')
        sk, sl = keys[r][order], levels[r][order]
        bounds = np.flatnonzero(np.diff(sk)) + 1
        for q, seg in zip(sk[np.concatenate([[0], bounds]).astype(np.int64)] if sk.shape[0] else [],
                          np.split(sl, bounds) if sk.shape[0] else []):
            seg = np.ascontiguousarray(seg)
            if read_mean:
                ent_val[q].append(np.array([np.add.reduce(seg) / seg.shape[0]]))
                ent_lab[q].append(np.array([label[r]]))
            else:
                ent_val[q].append(seg)
                ent_lab[q].append(np.full(seg.shape[0], label[r], dtype=np.int64))
    counts = np.array([sum(v.shape[0] for v in vs) for vs in ent_val], dtype=np.int64)
    off = np.zeros(n_kmers + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    values = np.concatenate([v for vs in ent_val for v in vs] + [np.empty(0)]).astype(np.float64)
    vlabel = np.concatenate([v for vs in ent_lab for v in vs] + [np.empty(0, dtype=np.int64)]).astype(np.int64)
    kmer_mean = np.full(n_kmers, np.nan)
    for q in np.flatnonzero(counts):
        run = np.ascontiguousarray(values[off[q]:off[q + 1]])
        kmer_mean[q] = np.add.reduce(run) / run.shape[0]
    return label, n_sel, n_exam, counts, off, values, vlabel, kmer_mean


def kmer_order(counts, kmer_mean):
    """the k-mers with entries ordered by (mean, k-mer string) -> their indices (index order is string order)"""
    have = np.flatnonzero(counts)
    return have[np.lexsort((have, kmer_mean[have]))]


def kmer_dist_dict_loop(reads, read_mean, upstrm_bases, dnstrm_bases, kmer_thresh, num_reads):
    """_plot_commands.py:455-514 word for word, for reads as (means or None, sequence str) in the order given
    -> (reads_added, kmer_levels, plot_kmers, plot_bases, plot_means, plot_r_ids)"""
    kmer_width = upstrm_bases + dnstrm_bases + 1
    reads_added = 0
    all_kmers = defaultdict(list)
    for r_means, r_seq in reads:
        if r_means is None:
            continue
        read_kmers = defaultdict(list)
        for kmer, event_mean in zip([r_seq[i:i + kmer_width] for i in range(len(r_seq) - kmer_width + 1)],
                                    r_means[upstrm_bases:]):
            read_kmers[kmer].append(event_mean)
        if kmer_thresh == 0 or (len(read_kmers) == 4 ** kmer_width and
                                (kmer_thresh == 1 or min(len(x) for x in read_kmers.values()) > kmer_thresh)):
            reads_added += 1
            for kmer, kmer_means in read_kmers.items():
                if read_mean:
                    all_kmers[kmer].append((np.mean(kmer_means), reads_added))
                else:
                    all_kmers[kmer].extend(zip(kmer_means, repeat(reads_added)))
        if reads_added >= num_reads:
            break
    kmer_levels = [kmer for means, kmer in sorted([
        (np.mean(list(map(itemgetter(0), means))), kmer) for kmer, means in all_kmers.items()])]
    rows = [(kmer, kmer[upstrm_bases], sig_mean, read_i) for kmer in kmer_levels for sig_mean, read_i in all_kmers[kmer]]
    cols = list(zip(*rows)) if rows else [(), (), (), ()]
    return (reads_added, kmer_levels) + tuple(cols)

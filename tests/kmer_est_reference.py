"""TEST INFRASTRUCTURE: a numpy restatement of the k-mer level extraction of the reference
(get_region_kmer_levels / extract_kmer_levels / tabulate_kmer_levels / tabulate_mod_kmer_levels,
tombo_stats.py:1242-1501, :2108-2158) in its own shape: one dict of lists per region, one Python loop per
position, the levels of a position in READ order (what a stable sort in get_reads_events gives).  It is pinned to
the live reference by tests/test_kmer_est_reference.py and is what the stand-in engine and the GPU tests are
compared with.  The region sequence and the motif search are tombo_helper's (get_region_seq, TomboMotif): they
are strings, the product does them on the host too, and the golden file pins them through this restatement."""
import math
from itertools import product

import numpy as np

from tombo_amd import tombo_helper as th


def all_kmers(K):
    return [''.join(p) for p in product('ACGT', repeat=K)]


def motif_keys(K, motif):
    return [(kmer, p - 1) for kmer in all_kmers(K) for p in motif.find_mod_poss(kmer)]


def c_mean_std(vals):
    """left-to-right sum, then left-to-right sum of squared deviations, sqrt(var / n)"""
    acc = 0.0
    for v in vals.tolist():
        acc += v
    m = acc / len(vals)
    var = 0.0
    for v in vals.tolist():
        var += (v - m) * (v - m)
    return m, math.sqrt(var / len(vals))


def pair(vals, est_mean):
    vals = np.asarray(vals, dtype=np.float64)
    with np.errstate(all='ignore'):
        return c_mean_std(vals) if est_mean else (float(np.median(vals)), float(np.std(vals)))


def position_levels(reads):
    """{genomic position: levels in read order} of the reads that have as many levels as bases"""
    events = {}
    for rd in reads:
        if rd.means is None or len(rd.means) != rd.end - rd.start:
            continue
        m = np.asarray(rd.means, dtype=np.float64)
        for g, v in zip(range(rd.start, rd.end), (m[::-1] if rd.strand == '-' else m).tolist()):
            events.setdefault(g, []).append(v)
    return events


def region_reads(reads_index, chrm, strand, reg_start, region_size):
    return [rd for rd in reads_index.get((chrm, strand), ())
            if not (rd.start >= reg_start + region_size or rd.end <= reg_start)]


def region_kmer_levels(reads, chrm, strand, reg_start, region_size, cov_thresh, upstrm, dnstrm, cs_cov_thresh,
                       est_mean, motif=None, valid_poss=None):
    """one region -> {key: [(level, sd)]}, or None where the reference returns None (or dies on len(None))"""
    reads = list(reads)
    if cs_cov_thresh is not None:
        np.random.shuffle(reads)
        total = 0
        for i, rd in enumerate(reads):
            total += max(rd.end, reg_start + region_size) - min(rd.start, reg_start)
            if total >= region_size * cs_cov_thresh:
                reads = reads[:i]
                break
    events = position_levels(reads)
    if not events:
        return None
    cov = np.array([len(events.get(g, ())) for g in range(reg_start, reg_start + region_size)])
    ok = cov > cov_thresh
    intervals, a = [], None
    for i in range(region_size):
        if ok[i] and a is None:
            a = i
        if not ok[i] and a is not None:
            intervals.append((a, i))
            a = None
    if a is not None:
        intervals.append((a, region_size))
    if not intervals:
        return None
    K = upstrm + dnstrm + 1
    out = dict((k, []) for k in (all_kmers(K) if motif is None else motif_keys(K, motif)))
    bb, ab = (upstrm, dnstrm) if strand == '+' else (dnstrm, upstrm)
    for a, b in intervals:
        seq = th.get_region_seq(reads, reg_start + a - bb, reg_start + b + ab)
        if motif is None:
            poss = [(p, None) for p in range(b - a)]
        else:
            if valid_poss is not None:
                if (chrm, strand) not in valid_poss:
                    continue
                mods = [int(v) - reg_start - a for v in valid_poss[(chrm, strand)]]
            elif strand == '+':
                mods = [m.start() + motif.mod_pos - 1 - bb for m in motif.motif_pat.finditer(seq)]
            else:
                mods = [m.start() + motif.motif_len - motif.mod_pos - bb for m in motif.rev_comp_pat.finditer(seq)]
            poss = [(mp - i + bb, i if strand == '+' else K - i - 1) for mp in mods if 0 <= mp < b - a
                    for i in range(K) if 0 <= mp - i + bb < b - a]
        for p, offset in poss:
            kmer = seq[p:p + K]
            if strand == '-':
                kmer = th.rev_comp(kmer)
            key = kmer if offset is None else (kmer, offset)
            g = p + reg_start + a
            if key in out and g in events:
                out[key].append(pair(events[g], est_mean))
    return out


def extract(reads_index, regs, region_size, cov_thresh, upstrm, dnstrm, cs_cov_thresh, est_mean=False, motif=None,
            valid_poss=None):
    """regs: the (chrm, strand, start) of iter_cov_regs -> the list of per-region dicts"""
    out = []
    for chrm, strand, reg_start in regs:
        reads = region_reads(reads_index, chrm, strand, int(reg_start), region_size)
        if not reads:
            continue
        res = region_kmer_levels(reads, chrm, strand, int(reg_start), region_size, cov_thresh, upstrm, dnstrm,
                                 cs_cov_thresh, est_mean, motif, valid_poss)
        if res is not None:
            out.append(res)
    return out


def flatten(all_regs, keys):
    """per-region dicts -> (reg_counts[n_regions, n_keys], levels, sds in region, key, position order)"""
    counts = np.array([[len(reg[k]) for k in keys] for reg in all_regs], dtype=np.int64).reshape(len(all_regs), len(keys))
    pairs = [p for reg in all_regs for k in keys for p in reg[k]]
    return (counts, np.array([p[0] for p in pairs], dtype=np.float64), np.array([p[1] for p in pairs], dtype=np.float64))


def table(reg_counts, levels, sds):
    """the flat per-region lists regrouped per key (region order inside a key) -> (off, levels, sds)"""
    n_reg, n_keys = reg_counts.shape
    starts = np.concatenate([[0], np.cumsum(reg_counts.reshape(-1))])[:-1].reshape(n_reg, n_keys)
    idx = [np.arange(starts[r, k], starts[r, k] + reg_counts[r, k]) for k in range(n_keys) for r in range(n_reg)]
    idx = np.concatenate(idx).astype(np.int64) if idx else np.empty(0, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(reg_counts.sum(axis=0))]).astype(np.int64)
    return off, levels[idx], sds[idx]


def medians(values, off):
    with np.errstate(all='ignore'):
        return np.array([np.median(values[a:b]) if b > a else np.nan
                         for a, b in zip(off[:-1].tolist(), off[1:].tolist())], dtype=np.float64)

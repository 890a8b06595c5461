"""Golden vectors of the read filters from the REFERENCE (build container only).

    python tests/golden/gen_golden_filters.py   # writes tests/golden/stats_filters.npz

(The `stats_` prefix keeps the file out of the resquiggle golden cases that tests/conftest.py lists.)

Runs the live reference's clear_filters, filter_reads_for_stuck / _coverage / _qscore / _signal_matching /
_genome_pos (tombo/_filter_reads.py) and its two parsers on a synthetic reads index.  Every case starts from a real
index file that the reference's own TomboReads writes into a temporary directory and reads back; the FAST5 files
the filters open are served from memory (tests/memh5.py) through a class put in place of `h5py.File`.  Only data is
written: the input index tuples, the per-read base lengths, FASTQ quality strings and score attributes, the seeds,
and per case the output index tuples, the messages (time stamps removed) and the error, if any.

The reference merges the indices of its directories through a set of the (chrm, strand) keys, so the order in which
it iterates the keys -- and with it the numbering of the reads in the coverage filter's draw -- changes from one
Python process to the next.  The order of a case is the order of the keys of its recorded output; the tests give the
input in that order (tests/filter_reference.py case_index).  A fresh run of this script records other orders and
other drawn reads.
"""
import contextlib
import io
import json
import os
import pickle
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_oracle  # noqa: E402
import memh5  # noqa: E402

rq, ts, th = ref_oracle.load()
if not hasattr(np, 'float'):
    np.float = float            # filter_reads_for_coverage: numpy 2 has no np.float
from tombo import _filter_reads as fr  # noqa: E402
import h5py  # noqa: E402  (the stand-in module ref_oracle installs)

CORR, BC, SUB = 'RawGenomeCorrected_000', 'Basecall_1D_000', 'BaseCalled_template'
FILES = {}      # base name -> MemGroup tree (a name that is not here: the file cannot be opened)


class FastqDataset(memh5.MemDataset):
    def __getitem__(self, key):     # the reference slices the scalar string with [:]
        return self.data.item()


class MemFile(memh5.MemGroup):
    """what `h5py.File(fn, 'r')` gives here: the tree stored under the file's base name"""

    def __init__(self, fn, mode='r'):
        memh5.MemGroup.__init__(self)
        tree = FILES[os.path.basename(fn)]
        self.items, self.attrs = tree.items, tree.attrs

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def close(self):
        pass


h5py.File = MemFile

# ---- the reads ------------------------------------------------------------------------------------------
# lens kinds: 0 a table, 1 an empty table, 2 no Events table, 3 no file
READS = []      # dict(chrm, strand, start, end, filtered, sms, mq, lens, kind, fastq_q, sms_attr)


def add(chrm, strand, start, lens, filtered=False, sms=0.9, mq=10.0, kind=0, end=None, fastq_q=None, sms_attr=None):
    lens = np.asarray(lens, dtype=np.uint32)
    READS.append(dict(chrm=chrm, strand=strand, start=int(start),
                      end=int(start + max(lens.shape[0], 1) if end is None else end), filtered=filtered, sms=sms, mq=mq,
                      lens=lens, kind=kind, fastq_q=fastq_q, sms_attr=sms_attr))


def make_reads(rng):
    geo = lambda n: rng.geometric(0.12, n) + 1                     # noqa: E731
    # chr1 +: the percentile edges of the three stuck filters
    add('chr1', '+', 100, [200] * 100)                                # p99 == 200: stays
    add('chr1', '+', 100, [201] * 100, mq=6.5)                        # p99 == 201: filtered by (99, 200)
    add('chr1', '+', 150, [8] * 51 + [5000] * 50, sms=1.3)            # median 8, max 5000: stays under (50, 8), (100, 5000)
    add('chr1', '+', 150, [8] * 50 + [9] * 51)                        # median 9
    add('chr1', '+', 160, [3] * 40 + [5001], mq=None, fastq_q='5555555555')    # max 5001
    add('chr1', '+', 170, [1] + [7] * 30, mq=None, fastq_q='++++++++')         # min 1: stays under (0, 1)
    add('chr1', '+', 170, [2] + [7] * 30, sms=None, sms_attr=0.8)     # min 2
    add('chr1', '+', 180, np.concatenate([np.arange(1, 199), [200, 203]]))     # p99 between 200 and 203 (t = 0.01)
    add('chr1', '+', 180, np.concatenate([np.arange(1, 200), [200, 203]]))     # 201 values: (n - 1) q = 198, integral
    add('chr1', '+', 200, [4], mq=12.5)                               # one base
    add('chr1', '+', 200, [4, 900], sms=None, sms_attr=1.5)           # two bases: p50 = 452.0, t = 0.5
    add('chr1', '+', 210, [], kind=1, end=260)                        # an empty Events table
    add('chr1', '+', 210, [], kind=2, end=270, sms=None)              # no Events table, no score attribute either
    add('chr1', '+', 220, [], kind=3, end=300, mq=None)               # the file cannot be opened
    add('chr1', '+', 230, geo(120), filtered=True)
    add('chr1', '+', 100, geo(100), filtered=True, mq=2.0)
    for _ in range(6):
        n = int(rng.integers(30, 160))
        lens = geo(n)
        lens[rng.random(n) < 0.03] = rng.integers(4000, 70000)
        add('chr1', '+', int(rng.integers(0, 300)), lens, sms=float(rng.choice([0.7, 1.0, 1.2])),
            mq=float(rng.choice([5.0, 7.0, 9.5])))
    # chr1 -: genome-position edges around the regions 100-200 and 400-450
    add('chr1', '-', 100, geo(100))                                   # 100..200: contained, touching both ends
    add('chr1', '-', 99, geo(101))                                    # starts one before
    add('chr1', '-', 100, geo(101), mq=6.9)                           # ends one after
    add('chr1', '-', 200, geo(50))                                    # starts at the region's end: partial only
    add('chr1', '-', 201, geo(50), filtered=True)
    add('chr1', '-', 201, geo(60))                                    # starts one after the end: outside
    add('chr1', '-', 350, geo(50))                                    # ends at 400: partial only
    add('chr1', '-', 349, geo(50), sms=1.11)                          # ends at 399: outside
    add('chr1', '-', 410, geo(30), mq=None, fastq_q='!!!!!!!!!!')
    # chr2 +: a pile for the coverage filter; chr2 -: a single read
    for _ in range(14):
        n = int(rng.integers(20, 80))
        add('chr2', '+', int(rng.integers(0, 60)), geo(n), filtered=bool(rng.random() < 0.2),
            mq=float(rng.choice([6.0, 8.0, 11.0])))
    for _ in range(4):
        add('chr2', '+', int(rng.integers(300, 500)), geo(40))
    add('chr2', '-', 5, geo(64), sms=1.05, mq=7.0)


def read_name(i):
    return 'r%03d.fast5' % i


def make_files():
    for i, r in enumerate(READS):
        if r['kind'] == 3:
            continue
        root = memh5.MemGroup()
        grp = root.create_group('/'.join(('Analyses', CORR, SUB)))
        if r['sms_attr'] is not None:
            grp.attrs['signal_match_score'] = r['sms_attr']
        if r['kind'] in (0, 1):
            ev = np.zeros(r['lens'].shape[0], dtype=[('norm_mean', 'f8'), ('start', 'u4'), ('length', 'u4')])
            ev['length'] = r['lens']
            grp.create_dataset('Events', data=ev)
        if r['fastq_q'] is not None:
            fq = '@%s\n%s\n+\n%s\n' % (read_name(i), 'A' * len(r['fastq_q']), r['fastq_q'])
            bc = root.create_group('/'.join(('Analyses', BC, SUB)))
            bc.items['Fastq'] = FastqDataset(np.bytes_(fq.encode()))
        FILES[read_name(i)] = root


def write_index(td, all_filtered=False):
    """the reference's own writer: TomboReads(for_writing) -> add_read_data -> write_index_file"""
    d = os.path.join(td, 'reads')
    os.makedirs(d, exist_ok=True)
    with contextlib.redirect_stderr(io.StringIO()):
        tr = th.TomboReads([d], CORR, for_writing=True)
        for i, r in enumerate(READS):
            tr.add_read_data(r['chrm'], r['strand'], th.readData(
                r['start'], r['end'], bool(r['filtered'] or all_filtered), 0, r['strand'], os.path.join(d + '/', read_name(i)),
                CORR + '/' + SUB, False, r['sms'], r['mq'], 'id%03d' % i))
        tr.write_index_file()
    return d


def jsonable(index):
    """{(chrm, strand): [tuple]} as stored -> [[chrm, strand, [records]]] in the file's key order"""
    return [[c, s, [[(x.item() if isinstance(x, np.generic) else x) for x in rec] for rec in recs]]
            for (c, s), recs in index.items()]


def load_pickle(d):
    with open(os.path.join(os.path.dirname(d), '.reads.' + CORR + '.tombo.index'), 'rb') as fp:
        return jsonable(pickle.load(fp))


def run_case(name, func, args, seed=None, all_filtered=False):
    with tempfile.TemporaryDirectory() as td:
        d = write_index(td, all_filtered)
        err, buf = None, io.StringIO()
        if seed is not None:
            np.random.seed(seed)
        with contextlib.redirect_stderr(buf):
            try:
                getattr(fr, func)(d, *args)
            except SystemExit:
                err = ['exit', None]
            except th.TomboError as e:
                err = ['TomboError', str(e)]
        mess = [re.sub(r'^\t?\[\d\d:\d\d:\d\d\] ', '', ln).replace(d, '<DIR>') for ln in buf.getvalue().split('\n') if ln]
        if err is not None and err[0] == 'exit':
            err[1] = mess[-1].strip()
        out = load_pickle(d)
    print('%-28s %s' % (name, mess[-2:] if err is None else err))
    return dict(name=name, func=func, args=args, seed=seed, all_filtered=all_filtered, error=err, messages=mess, out=out)


def main():
    rng = np.random.default_rng(20260211)
    make_reads(rng)
    make_files()
    # what this numpy does with an empty array (the reference's read_is_stuck turns any exception into True)
    try:
        np.percentile(np.zeros(0, dtype=np.uint32), 99)
        empty = 'no exception'
    except Exception as e:
        empty = type(e).__name__
    print('np.percentile of an empty array:', empty, '(numpy %s)' % np.__version__)

    obs_texts = [['99:200'], ['50:8', '100:5000'], ['0:1']]
    obs_parsed = [th.parse_obs_filter(t) for t in obs_texts]
    reg_texts = [['chr1:100-200', 'chr1:400-450'], ['chr1:100-200', 'chr2'], ['"chr1:1,00-2,00"', "chr2:0-1,000"]]
    reg_parsed = [th.parse_genome_regions(t) for t in reg_texts]

    cases = [run_case('clear', 'clear_filters', [CORR])]
    for k, obs in enumerate(obs_parsed):
        cases.append(run_case('stuck_%d' % k, 'filter_reads_for_stuck', [CORR, obs]))
    for frac in (0.0, 0.25, 0.999):
        for seed in (7, 1234):
            cases.append(run_case('coverage_%s_%d' % (frac, seed), 'filter_reads_for_coverage', [CORR, frac], seed=seed))
    for thresh in (7.0, 9.5):
        cases.append(run_case('qscore_%s' % thresh, 'filter_reads_for_qscore', [BC, CORR, thresh]))
    for thresh in (1.1, 0.8):
        cases.append(run_case('sigmatch_%s' % thresh, 'filter_reads_for_signal_matching', [CORR, thresh]))
    for k, regs in enumerate(reg_parsed):
        for partial in (False, True):
            cases.append(run_case('genome_pos_%d_%d' % (k, partial), 'filter_reads_for_genome_pos',
                                  [CORR, regs, partial]))
    # everything already filtered: the reference prints its error and exits
    cases.append(run_case('allfilt_stuck', 'filter_reads_for_stuck', [CORR, obs_parsed[0]], all_filtered=True))
    cases.append(run_case('allfilt_coverage', 'filter_reads_for_coverage', [CORR, 0.25], seed=7, all_filtered=True))
    cases.append(run_case('allfilt_qscore', 'filter_reads_for_qscore', [BC, CORR, 7.0], all_filtered=True))
    cases.append(run_case('allfilt_sigmatch', 'filter_reads_for_signal_matching', [CORR, 1.1], all_filtered=True))
    cases.append(run_case('allfilt_genome_pos', 'filter_reads_for_genome_pos', [CORR, reg_parsed[0], False],
                          all_filtered=True))
    # an index left without reads
    tr = object.__new__(th.TomboReads)
    try:
        tr.replace_index({('chr1', '+'): []})
        empty_err = None
    except th.TomboError as e:
        empty_err = str(e)
    assert empty_err is not None

    with tempfile.TemporaryDirectory() as td:
        d = write_index(td)
        base = load_pickle(d)
    doc = dict(corr_grp=CORR, bc_grp=BC, sub_grp=SUB, index=base, cases=cases, empty_index_error=empty_err,
               empty_percentile=empty, numpy=np.__version__,
               obs_texts=obs_texts, obs_parsed=obs_parsed, reg_texts=reg_texts, reg_parsed=reg_parsed,
               kind=[r['kind'] for r in READS], fastq_q=[r['fastq_q'] for r in READS],
               sms_attr=[r['sms_attr'] for r in READS])
    lens_off = np.concatenate([[0], np.cumsum([r['lens'].shape[0] for r in READS])]).astype(np.int64)
    path = os.path.join(HERE, 'stats_filters.npz')
    np.savez_compressed(path, doc=np.array(json.dumps(doc)), lens_off=lens_off,
                        lens=np.concatenate([r['lens'] for r in READS]).astype(np.uint32))
    print('wrote', path, os.path.getsize(path), 'bytes;', len(READS), 'reads,', len(cases), 'cases')


if __name__ == '__main__':
    main()

"""The host batch path without a device: what the read packers, the subsample / stall / scale-value
packing, the cut planner, a streamed `resquiggle_batch` call and the worker loop hand to the engine.
Needs the built library (tba_pack_reads, tba_unpack_reads and tba_batch_footprint are host-only
entries) and no GPU.  Every literal below was recorded from the tree before the host batch path was
reorganised (one read packer, one in-flight batch object); the tests pass on both."""
import numpy as np
import pytest

from tombo_amd import _native, resquiggle as rq, streaming, tombo_stats as ts, tombo_helper as th


class StubPinned(object):
    def __init__(self, shape, dtype):
        self.a = np.zeros(shape, dtype)
        self.nbytes = self.a.nbytes

    def close(self):
        self.a = None


class RecordingEngine(object):
    """stand-in for _native.Engine that computes nothing: it keeps what it was handed in `log` (shared by all
    instances) and "downloads" status 0, plausible records and boundaries"""
    log = []
    made = []
    K = 6

    def __init__(self, device=0):
        self.device, self.kmer_width = device, self.K
        self.id = len(RecordingEngine.made)
        RecordingEngine.made.append(self)
        self._stage = None

    def _rec(self, what, *a):
        RecordingEngine.log.append((what, self.id) + a)

    def ensure_model(self, std_ref):
        pass

    def set_sharing(self, n):
        self._rec('sharing', n)

    def host_stage(self):
        if self._stage is None:
            self._stage = _native.PinnedStage()
        return self._stage

    def upload_packed(self, params, opts, raw, raw_off, seq, seq_off, sv_in=None, sv_flags=None, samp_ind=None,
                      stall_ints=None, stall_off=None, wait=False):
        cp = lambda x: None if x is None else np.array(x)
        self.n = len(raw_off) - 1
        self.raw_off, self.seq_off = np.array(raw_off), np.array(seq_off)
        self.B = np.maximum(np.diff(self.seq_off) - self.K + 1, 0)
        self.ref_off = np.concatenate([[0], np.cumsum(self.B)]).astype(np.int64)
        self.seg_off = self.ref_off + np.arange(self.n + 1)
        self.n_raw_total = int(self.raw_off[-1])
        self._rec('upload', dict(raw=cp(raw), raw_off=cp(raw_off), seq=cp(seq), seq_off=cp(seq_off), sv_in=cp(sv_in),
                                 sv_flags=cp(sv_flags), samp_ind=cp(samp_ind), stall_ints=cp(stall_ints),
                                 stall_off=cp(stall_off), first_read=int(opts.subsample_first_read),
                                 skip_norm_out=bool(opts.skip_norm_out), n=self.n))

    def wait_for(self, other):
        self._rec('wait_for', other.id)

    def enqueue(self):
        self._rec('enqueue')

    def query(self):
        return False

    def sync(self):
        self._rec('sync')

    def download_async(self, results=None, segs32=None, segs64=None, norm=None):
        self._rec('download', norm is not None)
        n = self.n
        results['status'][:n] = 0
        results['norm_params_changed'][:n] = 0
        results['read_start_rel_to_raw'][:n] = 7
        results['norm_len'][:n] = np.diff(self.raw_off)
        results['shift'][:n], results['scale'][:n] = 0.5, 2.0
        results['lower_lim'][:n], results['upper_lim'][:n] = -5.0, 5.0
        results['sig_match_score'][:n] = 1.0
        segs64[:int(self.seg_off[-1])] = np.arange(int(self.seg_off[-1]))
        if norm is not None:
            norm[:self.n_raw_total] = np.arange(self.n_raw_total) % 11 - 5.0

    def held_bytes(self):
        return 0

    def device_mem(self):
        return 64 << 30, 64 << 30

    def close(self):
        pass


@pytest.fixture
def host_only(monkeypatch):
    """page-locked memory and the engine replaced, the process-wide engine tables emptied, switches unset"""
    monkeypatch.setattr(_native, 'PinnedArray', StubPinned)
    monkeypatch.setattr(_native, 'Engine', RecordingEngine)
    monkeypatch.setattr(rq, '_ENGINES', {})
    monkeypatch.setattr(rq, '_STREAM_ENGINES', {})
    monkeypatch.setattr(RecordingEngine, 'log', [])
    monkeypatch.setattr(RecordingEngine, 'made', [])
    for k in ('STREAM', 'STREAM_MIN', 'CUTS', 'CHAIN', 'TRACE', 'ZERO_COPY', 'ZERO_COPY_MIN'):
        monkeypatch.delenv('TBA_API_' + k, raising=False)
    monkeypatch.setenv('TBA_API_ZERO_COPY', '0')    # (the result pool leases real page-locked memory)
    return monkeypatch


def _model():
    samp = th.seqSampleType('DNA', False)
    return samp, ts.TomboModel(seq_samp_type=samp), ts.load_resquiggle_parameters(samp)


def _map_results(n_bases, seed=0, dtype=np.int16, per_base=9):
    """mapping results with made-up signals of 300 + `per_base` samples per base and random ACGT sequences"""
    rng = np.random.RandomState(seed)
    out = []
    for i, nb in enumerate(n_bases):
        seq = ''.join(rng.choice(list('ACGT'), nb + 5))
        raw = rng.randint(300, 700, 300 + per_base * nb).astype(dtype)
        out.append(th.resquiggleResults(
            align_info=th.alignInfo('r%d' % i, 'BaseCalled_template', 0, 0, 0, 0, nb, 0),
            genome_loc=th.genomeLocation(0, '+', 'synth'), genome_seq=seq, mean_q_score=10.0, raw_signal=raw))
    return out


# ---- 1. the packers agree -------------------------------------------------------------------------------------
def _packer_cases():
    rng = np.random.RandomState(3)
    lens = [0, 1, 7, 64, 65, 300]
    seqs = [''.join(rng.choice(list('ACGT'), int(k))) for k in rng.randint(6, 41, len(lens))]
    base = [rng.randint(-500, 500, n) for n in lens]
    wide = rng.randint(-500, 500, 128).astype(np.int16)
    sliced = [r.astype(np.int16) for r in base]
    sliced[3] = wide[::2]
    assert sliced[3].shape[0] == 64 and not sliced[3].flags.c_contiguous
    return seqs, [
        ('int16', [r.astype(np.int16) for r in base], np.int16),
        ('float32', [r.astype(np.float32) for r in base], np.float32),
        ('mixed', [r.astype(np.int16 if i % 2 else np.float64) for i, r in enumerate(base)], np.float64),
        ('sliced', sliced, np.int16)]


def test_every_read_packer_gives_the_plain_concatenation(host_only):
    seqs, cases = _packer_cases()
    codes = [ts.encode_seq(s) for s in seqs]
    want_seq = np.concatenate(codes)
    want_seq_off = np.concatenate([[0], np.cumsum([len(c) for c in codes])])
    p, o = _native.make_params(_model()[2]), _native.make_opts()

    def check(name, raw, raw_off, seq, seq_off, raws, dt):
        assert raw.dtype == np.dtype(dt), name
        np.testing.assert_array_equal(raw, np.concatenate(raws).astype(dt), err_msg=name)
        np.testing.assert_array_equal(raw_off, np.concatenate([[0], np.cumsum([len(r) for r in raws])]))
        assert seq.dtype == np.uint8 and np.asarray(raw_off).dtype == np.int64 and np.asarray(seq_off).dtype == np.int64
        np.testing.assert_array_equal(seq, want_seq)
        np.testing.assert_array_equal(seq_off, want_seq_off)
    for name, raws, dt in cases:
        for pinned in (False, True):
            b = streaming.ReadBatch.from_lists(raws, codes, pinned=pinned)
            check((name, pinned), b.raw, b.raw_off, b.seq, b.seq_off, raws, dt)
            assert b.n == len(raws) and b.samp_ind is None and b.stall_ints is None and b.stall_off is None
        # the code path of Engine.upload, captured where it hands over to upload_packed
        eng = RecordingEngine()
        _REAL_UPLOAD(eng, p, o, raws, codes)
        up = [e for e in RecordingEngine.log if e[0] == 'upload' and e[1] == eng.id][-1][2]
        check((name, 'upload'), up['raw'], up['raw_off'], up['seq'], up['seq_off'], raws, dt)
        assert up['stall_ints'] is None and up['stall_off'] is None
        # str sequences: the native packer encodes them
        raw, raw_off, seq, seq_off, keep = _native.pack_reads(raws, seqs)
        check((name, 'pack_reads'), raw, raw_off, seq, seq_off, raws, dt)
        raw, raw_off, seq, seq_off, keep = _native.pack_reads(raws, seqs, stage=_native.PinnedStage())
        check((name, 'pack_reads staged'), raw, raw_off, seq, seq_off, raws, dt)
    # one read: Engine.upload takes it as it is
    eng = RecordingEngine()
    _REAL_UPLOAD(eng, p, o, [cases[0][1][5]], [codes[5]])
    up = RecordingEngine.log[-1][2]
    assert up['raw'].dtype == np.int16 and np.array_equal(up['raw'], cases[0][1][5]) and up['raw_off'].tolist() == [0, 300]


_REAL_UPLOAD = _native.Engine.upload      # (taken at import: the fixture replaces _native.Engine)


# ---- 2. subsample rows ----------------------------------------------------------------------------------------
def test_rows_of_reads_without_a_subsample_are_minus_one_in_a_reused_staging_set(host_only):
    rng = np.random.RandomState(8)
    raws = [rng.randint(0, 100, 50).astype(np.int16) for _ in range(3)]
    seqs = ['ACGTACGTAC', 'ACGTACGTACG', 'ACGTACGTACGT']
    row_a, row_b = rng.permutation(5000)[:1000], rng.permutation(5000)[:1000]
    feeder = streaming.ReadFeeder(n_slots=1)
    try:
        b1 = feeder.pack(raws, seqs, samp_inds=[None, row_a, None])
        assert b1.samp_ind.shape == (3, 1000) and b1.samp_ind.dtype == np.int64
        assert np.array_equal(b1.samp_ind[1], row_a) and (b1.samp_ind[[0, 2]] == -1).all()
        held = b1.samp_ind
        b1.release()
        b2 = feeder.pack(raws, seqs, samp_inds=[None, None, row_b])
        assert np.shares_memory(b2.samp_ind, held)                 # the same staging set
        assert (b2.samp_ind[[0, 1]] == -1).all() and np.array_equal(b2.samp_ind[2], row_b)
        b2.release()
        assert feeder.pack(raws, seqs).samp_ind is None
    finally:
        feeder.close()
    codes = [ts.encode_seq(s) for s in seqs]
    for pinned in (False, True):
        b = streaming.ReadBatch.from_lists(raws, codes, samp_inds=[None, row_a, row_b], pinned=pinned)
        assert b.samp_ind.shape == (3, 1000) and b.samp_ind.dtype == np.int64
        assert (b.samp_ind[0] == -1).all() and np.array_equal(b.samp_ind[1], row_a) and np.array_equal(b.samp_ind[2], row_b)
        assert streaming.ReadBatch.from_lists(raws, codes, samp_inds=[None] * 3, pinned=pinned).samp_ind is None


# ---- 3. stall intervals and scale values ----------------------------------------------------------------------
def test_stall_and_scale_value_packing(host_only):
    assert _native.pack_stalls(None) == (None, None)
    st, sto = _native.pack_stalls([[], None, []])
    assert st.dtype == np.int64 and st.tolist() == [[0, 0]] and sto.dtype == np.int64 and sto.tolist() == [0, 0, 0, 0]
    st, sto = _native.pack_stalls([None, [], [(3, 9), (20, 41)], None, [(1, 2)]])
    assert st.dtype == np.int64 and st.tolist() == [[3, 9], [20, 41], [1, 2]] and sto.tolist() == [0, 0, 0, 2, 2, 3]
    raws = [np.arange(30, dtype=np.int16)] * 3
    codes = [ts.encode_seq('ACGTACGTAC')] * 3
    b = streaming.ReadBatch.from_lists(raws, codes, stalls=[[], None, []])
    assert b.stall_ints is None and b.stall_off is None
    b = streaming.ReadBatch.from_lists(raws, codes, stalls=[None, [(3, 9), (20, 41)], []])
    assert b.stall_ints.dtype == np.int64 and b.stall_ints.tolist() == [[3, 9], [20, 41]]
    assert b.stall_off.dtype == np.int64 and b.stall_off.tolist() == [0, 0, 2, 2]
    # through resquiggle_batch: the scale values, stall intervals and subsample rows one batch uploads
    samp, model, params = _model()
    mrs = _map_results([200, 1100, 180, 160])
    mrs[1] = mrs[1]._replace(scale_values=th.scaleValues(91.5, 12.25, None, None, None))
    mrs[3] = mrs[3]._replace(scale_values=th.scaleValues(88.0, 11.0, 33.0, 143.0, None), stall_ints=[(5, 60), (70, 90)])
    row = np.random.RandomState(2).permutation(1100)[:1000]
    eng = RecordingEngine()
    res = rq.resquiggle_batch(mrs, model, params, outlier_thresh=5.0, seq_samp_type=samp, engine=eng,
                              samp_inds=[None, row, None, None])
    assert len(res) == 4 and not any(isinstance(r, Exception) for r in res)
    up = [e for e in RecordingEngine.log if e[0] == 'upload'][-1][2]
    assert up['sv_flags'].dtype == np.int32 and up['sv_flags'].tolist() == [0, 1, 0, 3]
    assert up['sv_in'].tolist() == [[0.0] * 4, [91.5, 12.25, 0.0, 0.0], [0.0] * 4, [88.0, 11.0, 33.0, 143.0]]
    assert up['stall_ints'].tolist() == [[5, 60], [70, 90]] and up['stall_off'].tolist() == [0, 0, 0, 0, 2]
    assert up['samp_ind'].shape == (4, 1000) and np.array_equal(up['samp_ind'][1], row)
    assert (up['samp_ind'][[0, 2, 3]] == -1).all()
    # none of the three: nothing is uploaded for them
    rq.resquiggle_batch(_map_results([200, 300]), model, params, outlier_thresh=5.0, seq_samp_type=samp, engine=eng)
    up = [e for e in RecordingEngine.log if e[0] == 'upload'][-1][2]
    assert up['sv_in'] is None and up['sv_flags'] is None and up['stall_ints'] is None and up['samp_ind'] is None


# ---- 4. cuts --------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _recorded_cuts(monkeypatch, mrs, env, **kw):
    """the (a, b) sub-batches resquiggle_batch plans: the list handed to _stream_batches, or the one _submit_batch"""
    samp, model, params = _model()
    seen = {}

    def stream(engines, cuts, *a, **k):
        seen['cuts'], seen['engines'] = [(int(x), int(y)) for x, y in cuts], len(engines)
        raise _Stop()

    def submit(eng, a, b, *rest, **k):
        seen['cuts'], seen['engines'] = [(int(a), int(b))], 1
        raise _Stop()
    monkeypatch.setattr(rq, '_stream_batches', stream)
    monkeypatch.setattr(rq, '_submit_batch', submit)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(_Stop):
        rq.resquiggle_batch(mrs, model, params, outlier_thresh=5.0, seq_samp_type=samp, **kw)
    for k in env:
        monkeypatch.delenv(k)
    return seen['cuts'], seen['engines']


def test_sub_batch_cuts_are_the_recorded_ones(host_only):
    n_bases = [int(x) for x in np.random.RandomState(5).randint(150, 1201, 50)]
    mrs = _map_results(n_bases)
    rec = lambda env, m=mrs, **kw: _recorded_cuts(host_only, m, env, **kw)
    assert rec({}, m=mrs[:1]) == ([(0, 1)], 1)
    assert rec({}) == ([(0, 50)], 1)
    assert rec({'TBA_API_STREAM_MIN': '12'}) == (CUTS_STREAM_MIN_12, 3)
    assert rec({'TBA_API_STREAM_MIN': '12', 'TBA_API_CUTS': '5'}) == (CUTS_STREAM_MIN_12_CUTS_5, 3)
    # by memory: slow reads (100 samples per base), so that the 50 together are over a budget that holds about eight
    slow = _map_results(n_bases, per_base=100)
    assert rec({'TBA_API_STREAM': '0'}, m=slow, mem_budget=MEM_BUDGET_EIGHT_READS) == (CUTS_BY_MEMORY, 1)
    assert rec({'TBA_API_STREAM': '0'}, m=slow, mem_budget=6.0e8) == ([(0, 50)], 1)
    assert rec({'TBA_API_STREAM_MIN': '12'}, engine=RecordingEngine()) == ([(0, 50)], 1)


CUTS_STREAM_MIN_12 = [(0, 9), (9, 18), (18, 27), (27, 36), (36, 45), (45, 50)]
CUTS_STREAM_MIN_12_CUTS_5 = [(0, 10), (10, 20), (20, 30), (30, 40), (40, 50)]
# (tba_batch_footprint of the 50 slow reads: 597 692 469 bytes; the planner's estimate keeps 512 MiB for the arenas)
MEM_BUDGET_EIGHT_READS = 5.7e8
CUTS_BY_MEMORY = [(0, 7), (7, 17), (17, 23), (23, 31), (31, 39), (39, 46), (46, 50)]


# ---- 5. a streamed call's engine traffic ------------------------------------------------------------------------
@pytest.mark.parametrize('return_signal', [True, False])
def test_streamed_call_engine_traffic(host_only, return_signal):
    samp, model, params = _model()
    n_bases = [int(x) for x in np.random.RandomState(6).randint(150, 400, 40)]
    mrs = _map_results(n_bases, seed=1)
    host_only.setenv('TBA_API_STREAM_MIN', '12')
    res = rq.resquiggle_batch(mrs, model, params, outlier_thresh=5.0, seq_samp_type=samp, subsample_seed=3,
                              return_signal=return_signal)
    log = RecordingEngine.log
    assert len(RecordingEngine.made) == 3
    ups = [e for e in log if e[0] == 'upload']
    cuts = [(e[2]['first_read'], e[2]['first_read'] + e[2]['n']) for e in ups]
    assert cuts == STREAMED_40_CUTS
    assert [e[1] for e in ups] == [k % 3 for k in range(len(ups))]                       # rotation
    first_up = log.index(ups[0])
    assert sorted(e[1] for e in log[:first_up] if e == ('sharing', e[1], 3)) == [0, 1, 2]
    assert log[-6:] == _IDLE_AGAIN                                                      # back to the defaults
    waits = [e for e in log if e[0] == 'wait_for']
    if return_signal:    # sub-batch k computes after sub-batch k - 1: its engine waits for that one's
        assert [(e[1], e[2]) for e in waits] == [(k % 3, (k - 1) % 3) for k in range(1, len(ups))]
        for w in waits:  # ... between its upload and its enqueue
            i = log.index(w)
            assert log[i - 1][0] == 'upload' and log[i - 1][1] == w[1] and log[i + 1] == ('enqueue', w[1])
    else:
        assert waits == []
    assert all(e[2]['skip_norm_out'] == (not return_signal) for e in ups)
    assert [e[2] for e in log if e[0] == 'download'] == [return_signal] * len(ups)
    # one result per read, in input order
    assert len(res) == len(mrs)
    for mr, r in zip(mrs, res):
        assert r.align_info == mr.align_info and r.genome_seq == mr.genome_seq[2:-3]
        assert r.read_start_rel_to_raw == 7 and r.scale_values == th.scaleValues(0.5, 2.0, -5.0, 5.0, 5.0)
        assert r.segs.shape[0] == len(mr.genome_seq) - 5 + 1
        assert (r.raw_signal.shape[0] == mr.raw_signal.shape[0]) if return_signal else r.raw_signal is None
    for a, b in cuts:     # the stand-in's boundaries count up within a sub-batch
        got = np.concatenate([r.segs for r in res[a:b]])
        assert np.array_equal(got, np.arange(got.shape[0]))
    # a stream that raises on its second sub-batch: every engine is synced afterwards, sharing reset
    calls, real = {'n': 0}, rq._submit_batch

    def boom(*a_, **k_):
        calls['n'] += 1
        if calls['n'] == 2:
            raise _native.EngineError('injected')
        return real(*a_, **k_)
    host_only.setattr(rq, '_submit_batch', boom)
    del log[:]
    with pytest.raises(_native.EngineError, match='injected'):
        rq.resquiggle_batch(mrs, model, params, outlier_thresh=5.0, seq_samp_type=samp, subsample_seed=3,
                            return_signal=return_signal)
    assert len([e for e in log if e[0] == 'upload']) == 1
    assert log[-6:] == _IDLE_AGAIN


# how a streamed call ends, whatever happened: every engine synced, its sharing hint reset
_IDLE_AGAIN = [x for k in range(3) for x in (('sync', k), ('sharing', k, 1))]
STREAMED_40_CUTS = [(0, 8), (8, 16), (16, 24), (24, 32), (32, 40)]


# ---- 6. the worker loop, read by read -------------------------------------------------------------------------
def test_worker_loop_read_major_call_sequence(monkeypatch):
    """the scripted engine of test_abi_and_host.test_worker_loop_control_flow_without_gpu under rng_order='read_major':
    every read finishes -- its passes, then, when it failed, its passes with the save parameters -- before the next
    one starts"""
    calls, seen = [], {}
    script = {
        'a': (['ok'], []),
        'b': (['changed', 'changed', 'ok'], []),
        'c': (['changed', 'changed', 'changed', 'changed'], []),
        'd': (['fail'], ['changed', 'ok']),
        'e': (['changed', 'fail'], ['fail']),
    }

    def fake_batch(map_results, std_ref, params, outlier_thresh=None, all_raw_signals=None,
                   const_scale=None, skip_seq_scaling=False, seq_samp_type=None, engine=None, **kw):
        calls.append((params, ''.join(m.align_info for m in map_results), const_scale, skip_seq_scaling,
                      [m.scale_values for m in map_results], all_raw_signals, kw))
        out = []
        for m in map_results:
            k = (m.align_info, params)
            seen[k] = seen.get(k, 0) + 1
            what = script[m.align_info][0 if params == 'main' else 1][seen[k] - 1]
            out.append(th.TomboError('boom %s' % m.align_info) if what == 'fail' else m._replace(
                segs=[0, 1], scale_values=('sv', m.align_info, params, seen[k]), norm_params_changed=(what == 'changed')))
        return out
    monkeypatch.setattr(rq, 'resquiggle_batch', fake_batch)
    mrs = [th.resquiggleResults(align_info=r, genome_loc=None, genome_seq='ACGT', mean_q_score=1.0,
                                raw_signal='raw-' + r) for r in 'abcde']
    res, passes = rq.resquiggle_batch_iters(mrs, None, 'main', 'save', outlier_thresh=5.0, const_scale=12.0,
                                            skip_seq_scaling=True, return_passes=True, rng_order='read_major',
                                            subsample_seed=4)
    assert passes == [1, 3, 3, 1 + 2, 2 + 1]
    assert [isinstance(r, Exception) for r in res] == [False, False, False, False, True]
    assert res[2].norm_params_changed and res[2].scale_values == ('sv', 'c', 'main', 3)
    assert res[3].scale_values == ('sv', 'd', 'save', 2) and str(res[4]) == 'boom e'
    assert [c[:2] for c in calls] == READ_MAJOR_CALLS
    for c in calls:
        first = c[5] is None       # a first pass: the options, no fitted scale values, the read's own signal
        assert (c[2], c[3]) == ((12.0, True) if first else (None, False))
        assert c[5] is None or c[5] == ['raw-' + c[1]]
        assert c[6] == dict(subsample_seed=4)
    assert [c[4] for c in calls if c[1] == 'b'] == [[None], [('sv', 'b', 'main', 1)], [('sv', 'b', 'main', 2)]]
    assert [c[4] for c in calls if c[1] == 'd'] == [[None], [None], [('sv', 'd', 'save', 1)]]
    with pytest.raises(ValueError, match="rng_order is 'round_major' or 'read_major'"):
        rq.resquiggle_batch_iters(mrs, None, 'main', 'save', rng_order='other')


READ_MAJOR_CALLS = [('main', 'a'), ('main', 'b'), ('main', 'b'), ('main', 'b'), ('main', 'c'), ('main', 'c'), ('main', 'c'),
                    ('main', 'd'), ('save', 'd'), ('save', 'd'), ('main', 'e'), ('main', 'e'), ('save', 'e')]

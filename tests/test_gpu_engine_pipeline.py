"""GPU: the host side of the batch engine (tba_engine.hip) -- the bytes it says it holds are the bytes it
allocated, and the pipeline run whole, on one or two streams, equals its seven public stages run one at
a time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup(samp_name):
    from tombo_amd import tombo_stats as ts, tombo_helper as th, _native as N
    from tombo_amd._default_parameters import SIG_MATCH_THRESH
    samp = th.seqSampleType(samp_name, False)
    model = ts.TomboModel(seq_samp_type=samp)
    params = ts.load_resquiggle_parameters(samp)
    o = N.make_opts(outlier_thresh=5.0, sig_match_thresh=SIG_MATCH_THRESH[samp_name], subsample_seed=5)
    return model, params, N.make_params(params), o


def test_held_bytes_is_what_a_fresh_engine_allocated():
    """tba_engine_held_bytes on an engine that has seen one model and one batch: the model's two level
    tables and every buffer of the size table (tba_batch_footprint), each with the grow-only
    capacity bytes + bytes / 8 + 256 -- exactly, the read-order and long-read index lists included"""
    from tombo_amd import synth, tombo_stats as ts, _native as N
    model, _, p, o = _setup('DNA')
    K = model.kmer_width
    reads = [synth.synth_read(model, 300, 71000 + i, **synth.DNA_SYNTH) for i in range(5)]
    raws, seqs = [r[1] for r in reads], [ts.encode_seq(r[0]) for r in reads]
    eng = N.Engine(0)
    try:
        eng.set_model(model.level_means, model.level_sds, K, model.central_pos)
        eng.upload(p, o, raws, seqs)
        want = eng.footprint(p, o, [r.shape[0] for r in raws], [s.shape[0] for s in seqs]) + \
            2 * (9 * 4 ** K + 256)
        held = eng.held_bytes()
        print('held_bytes', held, 'footprint + model', want, 'difference', held - want)
        assert held == want
    finally:
        eng.close()


def _batches():
    from tombo_amd import synth
    dna = _setup('DNA')
    reads = []
    for i, nb in enumerate((300, 700, 450, 520, 380, 610)):
        seq, raw, _ = synth.synth_read(dna[0], nb, 72000 + i, **synth.DNA_SYNTH)
        if i == 3:      # too little signal for the running statistic: fails before event detection
            raw = raw[:4 * dna[1].running_stat_width + 1]
        reads.append((raw, seq))
    rna = _setup('RNA')
    rna_reads = []
    for i in range(4):
        seq, raw, _ = synth.synth_read(rna[0], 150, 73000 + i, **synth.RNA_SYNTH)
        rna_reads.append((raw, seq))
    return (('DNA', dna, reads), ('RNA', rna, rna_reads))


GETS = ('GET_STATUS', 'GET_N_CPTS', 'GET_VALID_CPTS', 'GET_EVENT_MEANS', 'GET_BAND_STARTS', 'GET_READ_TB',
        'GET_DP_SEGS', 'GET_SEGS', 'GET_THEIL_SEN', 'GET_PATH', 'GET_DP_FORM', 'GET_TS_FORM')


def test_full_run_equals_the_stages_run_one_at_a_time():
    """A full run with the side stream, a full run without it, and tba_batch_run_stages(k, k) for
    k = 0..6: every downloaded array and every intermediate the engine reports, bit for bit.  DNA
    (float64 samples, one read whose signal is too short to pass) and RNA."""
    from tombo_amd import tombo_stats as ts, _native as N
    for name, (model, params, p, o), reads in _batches():
        raws, seqs = [r[0] for r in reads], [ts.encode_seq(r[1]) for r in reads]
        eng = N.Engine(0)
        try:
            eng.set_model(model.level_means, model.level_sds, model.kmer_width, model.central_pos)
            results = {}
            for way in ('side', 'one_stream', 'stages'):
                eng.set_side_stream(1 if way == 'side' else 0)
                eng.upload(p, o, raws, seqs)
                if way == 'stages':
                    for k in range(N.STAGE_SEGMENT, N.STAGE_RESCALE + 1):
                        eng.run_stages(k, k)
                else:
                    eng.run()
                assert eng.last_side_stream() == (way == 'side')
                got = {k: np.array(v, copy=True) for k, v in eng.download().items()}
                got.update((g, eng.get(getattr(N, g))) for g in GETS)
                results[way] = got
            eng.set_side_stream(-1)
        finally:
            eng.close()
        st = results['side']['status'].tolist()
        assert sum(x == 0 for x in st) >= len(st) - 1, (name, st)
        if name == 'DNA':
            assert st[3] != 0, st
        for way in ('one_stream', 'stages'):
            for k, a in results['side'].items():
                b = results[way][k]
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, way, k)

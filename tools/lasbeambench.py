"""LAS beam-search decoding time at the reference's inference configuration: one utterance, F 840 (40 MFCC, context 10),
T 400, C 32, beam width 1000, at most 100 steps, length penalty 0.5.  One decode = nasr_las_beam_search (the search and
gather_tree, ending in a device synchronise) plus the read-back of the gathered ids.  Then one profiled search for its
device-timed phases: encoder, decoder GEMMs, decoder cell, attention, selection (scores, top-W, update), gather_tree,
host waits between chunks of steps; the read-back is host-timed.  Prints one JSON line.
   python tools/lasbeambench.py [--steps 10 --warmup 3]
--lm-order N times the same search three ways in one process: plain, fused with an order-N table at weight 0.3
(nasr_las_beam_set_lm; zero-mean random log-probs, the end id's column lowered by 20 so that both searches run all the
steps), and plain again, whose distance from the first plain run is the run-to-run spread; each with its profiled phases.
   python tools/lasbeambench.py --lm-order 4 [--steps 10 --warmup 3]
--from-audio times one LAS.evaluate of that batch shape given as audio (one utterance at 16 kHz whose 400 frames give
T 400) two ways, alternating in one process: the host route (Featurizer.compute, zero-pad, evaluate: the features come to
the host and go back) and evaluate_audio (the features stay in the handle's batch slot).  Host clock around each call;
both end in the read-back of the search's results.  Prints one JSON line with both medians and their spreads.
   python tools/lasbeambench.py --from-audio [--steps 10 --warmup 3]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from neuralasr_amd.engine import LasEngine      # noqa: E402
from neuralasr_amd.networks.las import LAS      # noqa: E402


def evaluate_from_audio(a):
    """one evaluate() per route and repetition, alternating; ms per call"""
    import tempfile
    from neuralasr_amd.config import Config
    sr, numcep, numcontext, C, T = 16000, 40, 10, 32, a.frames
    syms = ['<padding>', '^', '$'] + [chr(ord('a') + i) for i in range(26)] + ['_', "'", '<blank>']
    assert len(syms) == C
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, 'symbols'), 'w') as fh:
            fh.write(''.join('%s %d\n' % (s, i) for i, s in enumerate(syms)))
        cfg = os.path.join(d, 'las.config')
        with open(cfg, 'w') as fh:
            fh.write('[Parameters]\nsamplerate=%d\nnumcep=%d\nnumcontext=%d\nlabel_context=0\nbatch_size=1\nepochs=1\n'
                     'learningrate=0.0001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z ]\n'
                     'sym_file=%s\nnetwork=networks.las.LAS\n[Train]\ninput=%s\n[Test]\n'
                     '[MFCC Featurizer]\nstart_marker=^\nend_marker=$$\n'
                     % (sr, numcep, numcontext, os.path.join(d, 'model'), os.path.join(d, 'symbols'), os.path.join(d, 'none')))
        net = Config(cfg, True).load_network(fortraining=True)
    net.beam_width, net.max_decode_steps = a.width, a.max_steps
    rs = np.random.RandomState(1)
    audio = (0.1 * rs.randn(400 + (T - 1) * 160)).astype(np.float32)      # 25 ms frames every 10 ms: T frames
    labels = rs.randint(3, C - 1, size=(1, 20)).astype(np.int32)
    f = net.featurizer()

    def host_route():
        feats = f.compute([audio], rates=[sr])
        padded = np.zeros((1, max(x.shape[0] for x in feats), f.width), np.float32)
        padded[0, :feats[0].shape[0]] = feats[0]
        return net.evaluate(padded, labels, [np.asarray(feats[0].shape[0], np.int32)], [20])

    def audio_route():
        return net.evaluate_audio([audio], [sr], labels, [20])
    ms = {'host_route': [], 'evaluate_audio': []}
    for i in range(a.warmup + a.steps):
        for name, fn in (('host_route', host_route), ('evaluate_audio', audio_route)):
            t0 = time.perf_counter()
            out = fn()
            if i >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    ids = {name: fn()[0] for name, fn in (('host_route', host_route), ('evaluate_audio', audio_route))}
    res = {'workload': 'las_evaluate_from_audio', 'B': 1, 'T': T, 'F': f.width, 'C': C, 'W': a.width, 'max_steps': a.max_steps,
           'T_dec': int(out[0].shape[1]), 'repetitions': a.steps, 'warmup': a.warmup,
           'same_ids': bool(np.array_equal(ids['host_route'], ids['evaluate_audio']))}
    for name, v in ms.items():
        res[name + '_ms'] = {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    print(json.dumps(res))
    net.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--width', type=int, default=1000)
    ap.add_argument('--max-steps', type=int, default=100)
    ap.add_argument('--from-audio', action='store_true', help='time LAS.evaluate through the host route and evaluate_audio')
    ap.add_argument('--lm-order', type=int, default=0, help='also time the search fused with an n-gram table of this order')
    a = ap.parse_args()
    if a.from_audio:
        return evaluate_from_audio(a)
    F, C, B, T, W, S = 840, 32, 1, a.frames, a.width, a.max_steps
    start_id, end_id = 1, 2
    rs = np.random.RandomState(1)
    seq = np.full(B, T, np.int32)
    feats = rs.randn(B, T, F).astype(np.float32)
    e = LasEngine(F, C)
    e.set_params(LAS.initial_params(LAS.__new__(LAS), e.tensors(), seed=1))

    def timed():
        for _ in range(a.warmup):
            out = e.beam_search(feats, seq, W, S, start_id, end_id, 0.5)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = e.beam_search(feats, seq, W, S, start_id, end_id, 0.5)
        dt = (time.perf_counter() - t0) / a.steps
        e.set_profiling(True)
        t0 = time.perf_counter()
        out = e.beam_search(feats, seq, W, S, start_id, end_id, 0.5)
        t1 = time.perf_counter()
        ph = e.beam_times()
        t2 = time.perf_counter()
        ids = np.empty((B, out['steps'], W), np.int32)
        e._ck(e.lib.nasr_las_beam_get_ids(e.h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        readback = (time.perf_counter() - t2) * 1e3
        e.set_profiling(False)
        phases = {k + '_ms': v for k, v in ph.items()}
        phases['readback_ms'] = readback
        phases['profiled_total_ms'] = (t1 - t0) * 1e3
        return {'T_dec': out['steps'], 'ms_per_decode': round(dt * 1e3, 3), 'phases': {k: round(v, 3) for k, v in phases.items()}}

    res = {'workload': 'las_beam', 'B': B, 'T': T, 'F': F, 'C': C, 'W': W, 'max_steps': S}
    res.update(timed())
    if a.lm_order:
        table = rs.randn(C ** (a.lm_order - 1), C).astype(np.float32)
        table[:, end_id] -= 20.0
        e.set_lm((table, a.lm_order), 0.3)
        res['lm'] = dict(timed(), order=a.lm_order, weight=0.3, table_bytes=int(table.nbytes))
        e.set_lm(None)
        res['plain_again'] = timed()
    print(json.dumps(res))
    e.close()


if __name__ == '__main__':
    main()

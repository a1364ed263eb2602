"""LAS beam-search decoding time at the reference's inference configuration: one utterance, F 840 (40 MFCC, context 10),
T 400, C 32, beam width 1000, at most 100 steps, length penalty 0.5.  One decode = nasr_las_beam_search (the search and
gather_tree, ending in a device synchronise) plus the read-back of the gathered ids.  Then one profiled search for its
device-timed phases: encoder, decoder GEMMs, decoder cell, attention, selection (scores, top-W, update), gather_tree,
host waits between chunks of steps; the read-back is host-timed.  Prints one JSON line.
   python tools/lasbeambench.py [--steps 10 --warmup 3]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--width', type=int, default=1000)
    ap.add_argument('--max-steps', type=int, default=100)
    a = ap.parse_args()
    F, C, B, T, W, S = 840, 32, 1, a.frames, a.width, a.max_steps
    start_id, end_id = 1, 2
    rs = np.random.RandomState(1)
    seq = np.full(B, T, np.int32)
    feats = rs.randn(B, T, F).astype(np.float32)
    e = LasEngine(F, C)
    e.set_params(LAS.initial_params(LAS.__new__(LAS), e.tensors(), seed=1))
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
    phases = {k + '_ms': v for k, v in ph.items()}
    phases['readback_ms'] = readback
    phases['profiled_total_ms'] = (t1 - t0) * 1e3
    print(json.dumps({'workload': 'las_beam', 'B': B, 'T': T, 'F': F, 'C': C, 'W': W, 'max_steps': S,
                      'T_dec': out['steps'], 'ms_per_decode': round(dt * 1e3, 3),
                      'phases': {k: round(v, 3) for k, v in phases.items()}}))
    e.close()


if __name__ == '__main__':
    main()

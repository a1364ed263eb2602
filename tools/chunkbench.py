"""What latency-controlled training costs per step: the 3x500 bidirectional concat network (F 494, C 29) at
B 16, T 500, every utterance full length, timed in ONE process in four configurations that take turns:
  persistent       the whole-utterance step on the persistent kernels (skipped where the handle has none)
  per_step         the whole-utterance step on the per-step kernels (set_recurrence_mode(0)): what the chunked step is
                   compared with - it runs on the same kernels
  chunked_50_20    nasr_set_chunking(50, 20): 10 windows of 70 rows, (C+R)/C = 1.4 times the rows
  chunked_100_50   nasr_set_chunking(100, 50): 5 windows of 150 rows, 1.5 times the rows
A turn uploads the batch once and times --steps steps (compute_grads + apply_adam, one synchronise at the end) with the
host clock, then one more step under nasr_set_profiling for the phase times of nasr_get_phase_times.  --rounds turns per
configuration, interleaved, so that clock and thermal drift hit all four alike; reported: the median over the turns of the
per-step time, its min and max, the ratio to per_step's median, and the medians of the phases.
   python tools/chunkbench.py [--rounds 5 --steps 10 --warmup 3] [--out profiles/lc_train_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

F, H, L, C = 494, 500, 3, 29
CONFIGS = [('persistent', 1, (0, 0)), ('per_step', 0, (0, 0)), ('chunked_50_20', 0, (50, 20)), ('chunked_100_50', 0, (100, 50))]
PHASES = ['pack_ms', 'xproj_ms', 'rec_fwd_ms', 'proj_ctc_ms', 'proj_bwd_ms', 'rec_bwd_ms', 'wgrad_ms', 'adam_ms', 'total_ms',
          'rec_fwd_launches', 'rec_bwd_launches']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine
    from neuralasr_amd.networks.hipnetwork import _glorot_init
    from oracle import nasr_oracle as O
    spec = O.ModelSpec(F, H, L, True, 'concat', C)
    feats, seq_len, labels, label_len = O.synth_batch(spec, a.batch, a.frames, seed=3, var_len=False, Lmin=20, Lmax=60)
    feats = feats.astype(np.float32)
    e = Engine(F, H, L, True, 'concat', C, learning_rate=1e-4)
    e.set_params(_glorot_init(e.tensors(), 1))
    kind = e.recurrence_mode
    configs = [c for c in CONFIGS if c[1] == 0 or kind != 'per-step']
    ms = {name: [] for name, _, _ in configs}
    phases = {name: [] for name, _, _ in configs}
    losses = {}

    def turn(name, persistent, chunk, steps, record):
        e.set_chunking(*chunk)
        try:
            e.set_recurrence_mode(persistent)
        except _lib.NasrError:
            return
        e.upload_batch(feats, seq_len, labels, label_len)
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            e.compute_grads()
            e.apply_adam(1.0)
        e.synchronize()
        per = (time.perf_counter() - t0) * 1e3 / steps
        e.set_profiling(True)
        e.compute_grads()
        e.apply_adam(1.0)
        e.synchronize()
        pt = e.phase_times()
        e.set_profiling(False)
        if record:
            ms[name].append(per)
            phases[name].append([float(pt[k]) for k in PHASES])
            losses[name] = float(e.get_loss())

    for name, persistent, chunk in configs:
        turn(name, persistent, chunk, a.warmup, False)
    for _ in range(a.rounds):
        for name, persistent, chunk in configs:
            turn(name, persistent, chunk, a.steps, True)
    e.close()
    base = float(np.median(ms['per_step']))
    res = {'network': '3x500 bidirectional concat, F %d, C %d' % (F, C), 'B': a.batch, 'T': a.frames,
           'recurrence_kind_of_the_handle': kind, 'rounds': a.rounds, 'steps_per_turn': a.steps, 'configs': {}}
    for name, _, chunk in configs:
        v = ms[name]
        ph = np.median(np.asarray(phases[name]), axis=0)
        res['configs'][name] = {'chunking': list(chunk), 'step_ms': {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3),
                                                                    'max': round(max(v), 3)},
                                'ratio_to_per_step': round(float(np.median(v)) / base, 3), 'last_loss': losses[name],
                                'phases_median': {k: round(float(x), 3) for k, x in zip(PHASES, ph)}}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()

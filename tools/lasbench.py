"""LAS training-step time at the reference's configuration (config/8000sr_40mfcc_10context.config): B 8, F 840 (40 MFCC,
context 10), T 400, U 80, C 32, scheduled sampling 0.1.  One step = nasr_compute_grads + nasr_apply_adam on a resident
batch.  Then one profiled step for its phases: encoder forward, decoder forward (with the sequence loss), decoder BPTT,
encoder BPTT, weight gradients, Adam.  Prints one JSON line.   python tools/lasbench.py [--steps 10 --warmup 3]"""
import argparse
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
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--label-len', type=int, default=80)
    a = ap.parse_args()
    F, C, B, T, U = 840, 32, a.batch, a.frames, a.label_len
    rs = np.random.RandomState(1)
    seq = np.full(B, T, np.int32)
    feats = rs.randn(B, T, F).astype(np.float32)
    labels = rs.randint(0, C, size=(B, U)).astype(np.int32)
    ll = np.full(B, U, np.int32)
    e = LasEngine(F, C, sampling_probability=0.1)
    e.set_params(LAS.initial_params(LAS.__new__(LAS), e.tensors(), seed=1))
    e.upload_batch(feats, seq, labels, ll)
    for _ in range(a.warmup):
        e.compute_grads()
        e.apply_adam(1.0)
    e.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        e.compute_grads()
        e.apply_adam(1.0)
    e.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    loss = e.get_loss()
    e.set_profiling(True)
    e.compute_grads()
    e.apply_adam(1.0)
    e.synchronize()
    pt = e.phase_times()
    phases = {'encoder_fwd_ms': pt['rec_fwd_ms'], 'decoder_fwd_ms': pt['proj_ctc_ms'], 'decoder_bptt_ms': pt['proj_bwd_ms'],
              'encoder_bptt_ms': pt['rec_bwd_ms'], 'weight_grads_ms': pt['wgrad_ms'], 'adam_ms': pt['adam_ms'],
              'total_ms': pt['total_ms']}
    print(json.dumps({'workload': 'las', 'B': B, 'T': T, 'U': U, 'F': F, 'C': C, 'params': e.param_count,
                      'ms_per_step': round(dt * 1e3, 3), 'phases': {k: round(v, 3) for k, v in phases.items()},
                      'loss': loss}))
    e.close()


if __name__ == '__main__':
    main()

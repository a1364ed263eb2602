"""WaveNet training-step time at the reference's size: B 16, T 500, F 546, C 29, the full 3 x (1,2,4,8,16) model.
One step = nasr_compute_grads + nasr_apply_adam on a resident batch (what bench.py times for the LSTM workloads).
Prints one JSON line: ms/step and frames/s.   python tools/wavenet_step.py [--steps 20 --warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from neuralasr_amd.engine import WaveNetEngine      # noqa: E402
from neuralasr_amd.networks.wavenet import WaveNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--frames', type=int, default=500)
    a = ap.parse_args()
    F, C, B, T = 546, 29, a.batch, a.frames
    rs = np.random.RandomState(1)
    seq = np.full(B, T, np.int32)
    feats = rs.randn(B, T, F).astype(np.float32)
    ll = np.full(B, 40, np.int32)
    labels = rs.randint(0, C - 1, size=(B, 40)).astype(np.int32)
    e = WaveNetEngine(F, C)
    e.set_params(WaveNet.initial_params(WaveNet.__new__(WaveNet), e.tensors(), seed=1))
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
    print(json.dumps({'workload': 'wavenet', 'B': B, 'T': T, 'F': F, 'C': C, 'params': e.param_count,
                      'ms_per_step': round(dt * 1e3, 3), 'frames_per_s': round(B * T / dt, 1), 'loss': loss}))
    e.close()


if __name__ == '__main__':
    main()

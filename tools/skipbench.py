"""What frame_skip buys, measured: for s in 1, 2, 3
  step   compute_grads + apply_adam on bench.py's flagship workload - the 3x500 BiLSTM (F 546, C 29), B 16, input T 500,
         bench.py's own synthetic batch and initial parameters - with the batch resident: ms per step (median of --repeats
         timed runs of --steps steps, each run between two synchronises, after --warmup steps) and INPUT frames per second,
         the project's metric (audio frames, whatever the network sees of them)
  feed   Engine.stream_feed of a 50-frame chunk (input frames) on the 3x500 LstmCTCNet, S in {1, 16} streams: host ms per
         feed, features in host memory to logits in host memory (median / min / max over --steps feeds after --warmup)
The s = 1 lines are the library without the key; bench.py measures that step too, and stays the yardstick.  The tool reads
nothing but the library and bench.py's workload definitions.
   python tools/skipbench.py [--steps 20 --warmup 5 --repeats 5] [--out profiles/skipbench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SKIPS = (1, 2, 3)
B, T, TC = 16, 500, 50


def bench_step(a, s):
    import bench
    from neuralasr_amd.engine import Engine
    spec, name = bench.workload_spec('bilstm3x500')
    e = Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes,
               learning_rate=1e-4)
    e.set_params(bench.init_params(e.tensors(), seed=1))
    e.set_frame_skip(s)
    e.upload_batch(*bench.synth_batch(spec, B, T, seed=1234))
    frames = e.resident_frames()
    for _ in range(a.warmup):
        e.compute_grads()
        e.apply_adam(1.0)
    e.synchronize()
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            e.compute_grads()
            e.apply_adam(1.0)
        e.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3 / a.steps)
    loss = e.get_loss()
    assert np.isfinite(loss) and not e.step_void()
    ms = float(np.median(runs))
    res = {'what': 'step', 'workload': name, 'frame_skip': s, 'B': B, 'input_T': T, 'network_T': e.logit_frames(T),
           'recurrence_mode': e.recurrence_mode, 'ms_per_step': round(ms, 3), 'ms_min': round(min(runs), 3),
           'ms_max': round(max(runs), 3), 'input_frames_per_s': round(frames / ms * 1e3, 1)}
    e.close()
    return res


def bench_feed(a, s, S):
    import bench
    from neuralasr_amd.engine import Engine
    spec, name = bench.workload_spec('lstm3')
    e = Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes)
    e.set_params(bench.init_params(e.tensors(), seed=1))
    e.set_frame_skip(s)
    rs = np.random.RandomState(7)
    chunks = [rs.randn(S, TC, spec.feature_size).astype(np.float32) for _ in range(4)]
    n = [TC] * S
    e.stream_open(S)
    ms = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        out = e.stream_feed(chunks[i % 4], n)
        if i >= a.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert np.isfinite(out).all()
    kept = int(e.stream_frames()[0])
    e.stream_close()
    e.close()
    return {'what': 'feed', 'workload': name, 'frame_skip': s, 'S': S, 'input_rows_per_feed': TC, 'logit_rows_per_feed': out.shape[0],
            'kept_rows_in_all': kept, 'host_ms_per_feed': round(float(np.median(ms)), 3), 'ms_min': round(min(ms), 3),
            'ms_max': round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the result lines to this JSON file')
    a = ap.parse_args()
    lines = [bench_step(a, s) for s in SKIPS]
    lines += [bench_feed(a, s, S) for S in (1, 16) for s in SKIPS]
    for ln in lines:
        print('SKIPBENCH ' + json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(lines, f, indent=1)


if __name__ == '__main__':
    main()

"""What parameter averaging costs in the optimiser phase: the PH_ADAM time (adam_ms of the handle's phase
timings: the norm's kernels when clipping is on, the Adam sweep, the repack of the operand images) of the flagship 3x500
bidirectional concat network (F 546, C 29) at batch 16, T 500, with averaging off and on.  One handle, one resident batch;
the two configurations take turns (--rounds turns of --steps steps each, after --warmup steps), so that clock and thermal
drift hit both alike.  Reported per configuration: the median over all timed steps, and the smallest and largest of the
turns' medians.  On a library without nasr_set_ema (the parent commit) only "off" is timed.
   python tools/emabench.py [--rounds 5 --steps 20 --warmup 5] [--decay 0.999] [--out profiles/ema_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import bench
    from neuralasr_amd.engine import Engine
    spec, name = bench.workload_spec('bilstm3x500')
    feats, seq_len, labels, label_len = bench.synth_batch(spec, a.batch, a.frames)
    eng = Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes,
                 learning_rate=1e-4)
    eng.set_params(bench.init_params(eng.tensors()))
    eng.upload_batch(feats, seq_len, labels, label_len)
    configs = ['off', 'on'] if hasattr(eng, 'set_ema') else ['off']

    def step():
        eng.compute_grads()
        eng.apply_adam(1.0)
        return eng.phase_times()['adam_ms']          # (synchronises)

    for _ in range(a.warmup):
        step()
    eng.set_profiling(True)
    ms = {c: [] for c in configs}
    for _ in range(a.rounds):
        for c in configs:
            if len(configs) > 1:
                eng.set_ema(a.decay if c == 'on' else 0.0)
            step()                                    # the first step behind a switch is not timed
            ms[c].append([step() for _ in range(a.steps)])
    n = eng.param_count
    out = {'workload': name, 'batch': a.batch, 'frames': a.frames, 'params': int(n), 'rounds': a.rounds, 'steps': a.steps,
           'sweep_bytes_per_param': {'off': 28, 'on': 36}}
    for c in configs:
        turns = [float(np.median(t)) for t in ms[c]]
        out['adam_ms_' + c] = {'median': float(np.median(np.concatenate(ms[c]))), 'min_turn': min(turns), 'max_turn': max(turns)}
    if len(configs) > 1:
        out['on_over_off'] = out['adam_ms_on']['median'] / out['adam_ms_off']['median']
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)
    eng.close()


if __name__ == '__main__':
    main()

"""Forced alignment beside the loss lattice on the same batch.  The bench's network and batch - 3x500 BiLSTM,
concat merge, B 16, T 500, labels 40..80, C 29 - whose back-pointers stay in LDS, and the same at T 1000, where they go
through the global workspace.  Per shape, one child process under `rocprofv3 --kernel-trace --stats` alternates
loss_resident and align_resident on the resident batch; the kernels' device times come from its kernel statistics:
ctc_align_kernel (walk + traceback, one launch), its ctc_logz_kernel share, and the loss pass's ctc_alpha_beta_kernel, the
yardstick - the alignment does two compares and an add per state where that one does two exp and a log, so a walk slower
than it wants another look.  The child also clocks the calls on the host (align_resident and forward_resident both end in
a read-back and a synchronise; their difference is what the alignment adds to a forward pass), and runs the same launch
on the same frames with labels of 24 ids (two states per lane): the walk's arithmetic at its least, which brackets the share
of the way back.
   python tools/alignbench.py [--steps 20 --warmup 3] [--out profiles/align_bench.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SHAPES = {'lds': 500, 'global': 1000}


def worker(a):
    from bench import synth_batch, workload_spec
    from neuralasr_amd.engine import Engine
    from neuralasr_amd.networks.hipnetwork import _glorot_init
    spec, name = workload_spec('bilstm3x500')
    B, T = 16, SHAPES[a.worker]
    e = Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes)
    e.set_params(_glorot_init(e.tensors(), 1))
    feats, seq_len, labels, label_len = synth_batch(spec, B, T, seed=1234)
    e.upload_batch(feats, seq_len, labels, label_len)
    assert e.align_in_lds(int(seq_len.max()), labels.shape[1]) == (a.worker == 'lds')
    ms = {'align_resident': [], 'forward_resident': [], 'loss_resident': []}
    calls = {'align_resident': lambda: e.align_resident(B, T), 'forward_resident': lambda: e.forward_resident(B, T),
             'loss_resident': lambda: e.loss_resident(B)}
    for i in range(a.warmup + a.steps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            out = fn()
            if i >= a.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            if k == 'align_resident':
                path, score = out
            elif k == 'loss_resident':
                nll = out[1]
    # the same launch with two states per lane (labels up to 31 ids, random logits): the way back and the fixed costs are
    # what they were, the walk's arithmetic is at its least - an upper bound on what is not the walk
    rs = np.random.RandomState(3)
    lg = rs.randn(T, B, spec.num_classes).astype(np.float32)
    short = rs.randint(1, spec.num_classes - 1, size=(B, 24)).astype(np.int32)
    for _ in range(a.warmup + a.steps):
        e.align_logits(lg, [T] * B, short, [24] * B)
    res = {'workload': name, 'B': B, 'T': T, 'labels': [int(label_len.min()), int(label_len.max())], 'C': spec.num_classes,
           'backpointers': a.worker, 'recurrence_mode': e.recurrence_mode, 'steps': a.steps, 'warmup': a.warmup,
           'mean_path_logprob': float(np.mean(score)), 'mean_nll': float(np.mean(nll)),
           'host_ms': {k: {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
                       for k, v in ms.items()}}
    print('ALIGNBENCH ' + json.dumps(res), flush=True)
    e.close()


def kernel_stats(d):
    out = {}
    for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                for key in ('ctc_align_kernel', 'ctc_alpha_beta_kernel', 'ctc_logz_kernel'):
                    if key in row['Name']:
                        inst = row['Name'].split('(')[0].split('nasr::')[-1]
                        out[inst] = {'calls': int(row['Calls']), 'avg_us': round(float(row['AverageNs']) / 1e3, 2),
                                     'min_us': round(float(row['MinNs']) / 1e3, 2), 'max_us': round(float(row['MaxNs']) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'align_bench.json'))
    ap.add_argument('--worker', choices=sorted(SHAPES), help='(internal) the measured process of one shape')
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    doc = {'tool': 'tools/alignbench.py', 'method': 'rocprofv3 --kernel-trace --stats around one child per shape; host clock inside it',
           'shapes': {}}
    for shape in ('lds', 'global'):
        with tempfile.TemporaryDirectory() as d:
            cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
                   os.path.abspath(__file__), '--worker', shape, '--steps', str(a.steps), '--warmup', str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
            line = [l for l in r.stdout.splitlines() if l.startswith('ALIGNBENCH ')]
            if r.returncode != 0 or not line:
                raise SystemExit('the %s child failed (%d):\n%s\n%s' % (shape, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            res = json.loads(line[0][len('ALIGNBENCH '):])
            res['kernels'] = kernel_stats(d)
        al = [v for k, v in res['kernels'].items() if k.startswith('ctc_align_kernel')]
        ab = [v for k, v in res['kernels'].items() if k.startswith('ctc_alpha_beta_kernel')]
        if al and ab:
            # (the instantiation with the most states per lane is the resident batch's; <2, ..> is the short-label launch)
            res['align_over_alpha_beta'] = round(max(v['avg_us'] for v in al) / ab[0]['avg_us'], 3)
        doc['shapes'][shape] = res
    with open(a.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')
    print(json.dumps(doc))


if __name__ == '__main__':
    main()

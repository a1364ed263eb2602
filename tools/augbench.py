#!/usr/bin/env python3
"""The PH_PACK phase (nasr_set_profiling: the kernels slot_commit runs - context expansion, operand scales, layer 0's
transposed input) of a batch uploaded in the centre form, without masks and with SpecAugment masks, in
one run on one handle, the two alternating: the headline shape of bench.py - 3x500 BiLSTM, B 16, T 500, numcep 26,
numcontext 10 - with 2 time masks (up to 40 frames) and 2 frequency masks (up to 7 columns) per utterance.  The unmasked
upload launches expand_context_kernel, the masked one expand_context_masked_kernel; everything else in the phase is the same.

    python tools/augbench.py [--reps 200] [--warmup 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

from neuralasr_amd.augment import Augmenter            # noqa: E402
from neuralasr_amd.engine import BatchAug, Engine      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--numcep', type=int, default=26)
    ap.add_argument('--numcontext', type=int, default=10)
    a = ap.parse_args()
    B, T, ncep, ctx = a.batch, a.frames, a.numcep, a.numcontext
    rs = np.random.RandomState(0)
    centre = rs.randn(B, T, ncep).astype(np.float32)
    feats = np.empty((B, T, 2 * ctx + 1, ncep), np.float32)
    pad = np.float32(-0.25)
    for w in range(2 * ctx + 1):                          # include_context with one pad value
        ts = np.arange(T) + w - ctx
        ok = (ts >= 0) & (ts < T)
        feats[:, :, w] = pad
        feats[:, ok, w] = centre[:, ts[ok]]
    feats = feats.reshape(B, T, -1)
    seq = [T] * B
    labels = rs.randint(0, 28, size=(B, 60)).astype(np.int32)
    ll = [60] * B
    from types import SimpleNamespace
    aug = Augmenter(SimpleNamespace(samplerate=16000, numcep=ncep, feature_size=feats.shape[2], spec_time_masks=2,
                                    spec_time_width=40, spec_time_ratio=1.0, spec_freq_masks=2, spec_freq_width=7,
                                    speed_perturb=(), augment_seed=0))
    tm, fm = aug.masks(1, seq)
    masks = BatchAug(ncep, tm, fm)
    e = Engine(feats.shape[2], 500, 3, True, 'concat', 29)
    e.set_profiling(True)
    times = {'plain': [], 'masked': []}
    for i in range(a.warmup + a.reps):
        for name, m in (('plain', None), ('masked', masks)) if i % 2 == 0 else (('masked', masks), ('plain', None)):
            assert e.upload_batch_context(feats, seq, labels, ll, ctx, ncep, aug=m)
            ms = e.phase_times()['pack_ms']
            if i >= a.warmup:
                times[name].append(ms * 1e3)
    e.close()

    def stats(v):
        v = np.sort(np.asarray(v))
        return {'median_us': round(float(np.median(v)), 2), 'mean_us': round(float(v.mean()), 2),
                'p10_us': round(float(v[len(v) // 10]), 2), 'p90_us': round(float(v[len(v) * 9 // 10]), 2),
                'min_us': round(float(v[0]), 2)}
    half = a.reps // 2
    print(json.dumps({'B': B, 'T': T, 'numcep': ncep, 'numcontext': ctx, 'reps': a.reps,
                      'masked_frames': int(tm[:, :, 1].sum()), 'masked_columns': int(fm[:, :, 1].sum()),
                      'pack_plain': stats(times['plain']), 'pack_masked': stats(times['masked']),
                      # the spread of two runs of the same thing: the two halves of each series
                      'pack_plain_halves_median_us': [round(float(np.median(times['plain'][:half])), 2),
                                                      round(float(np.median(times['plain'][half:])), 2)],
                      'pack_masked_halves_median_us': [round(float(np.median(times['masked'][:half])), 2),
                                                       round(float(np.median(times['masked'][half:])), 2)]}))


if __name__ == '__main__':
    main()

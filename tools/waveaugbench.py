#!/usr/bin/env python3
"""The front end's kernel phase (nasr_featurize_times) of the headline audio batch - 16 utterances of 5 s at 16 kHz, numcep
26, numcontext 10 - uploaded into a model handle without waveform augmentation, with noise, and with a 4000-tap RIR plus
noise, the three alternating in one run on one handle; and the kernel phase of nasr_augment_audio alone
(the three kernels of wave_aug.hip, nothing else) for the two augmented variants.

    python tools/waveaugbench.py [--reps 100] [--warmup 10] [--taps 4000] [--out profiles/wave_aug_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mfccbench import synth                                    # noqa: E402
from neuralasr_amd.augment import prepare_rir                   # noqa: E402
from neuralasr_amd.engine import Engine, WaveAug               # noqa: E402
from neuralasr_amd.features import Featurizer                  # noqa: E402


def stats(v):
    v = np.sort(np.asarray(v))
    half = len(v) // 2
    return {'median_us': round(float(np.median(v)), 1), 'p10_us': round(float(v[len(v) // 10]), 1),
            'p90_us': round(float(v[len(v) * 9 // 10]), 1), 'min_us': round(float(v[0]), 1)}, half


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--seconds', type=float, default=5.0)
    ap.add_argument('--taps', type=int, default=4000)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    sr, B, n = 16000, a.batch, int(a.seconds * 16000)
    audios = [synth(n, sr, i) for i in range(B)]
    rs = np.random.RandomState(0)
    f = Featurizer(sr, 26, 10)
    f.set_noise([(0.1 * rs.randn(3 * sr)).astype(np.float32), (0.1 * rs.randn(7 * sr + 13)).astype(np.float32)])
    f.set_rirs([prepare_rir(rs.randn(a.taps) * np.exp(-np.arange(a.taps) / (0.2 * a.taps)))])
    noise = dict(noise=[i % 2 for i in range(B)], noise_off=[(977 * i) % sr for i in range(B)], snr_db=[5.0 + i for i in range(B)])
    variants = {'none': None, 'noise': WaveAug(None, **noise), 'rir+noise': WaveAug([0] * B, **noise)}
    e = Engine(f.width, 64, 1, True, 'concat', 29)
    labels, ll = np.ones((B, 4), np.int32), [4] * B
    front = {k: [] for k in variants}
    alone = {k: [] for k in variants if k != 'none'}
    names = list(variants)
    for i in range(a.warmup + a.reps):
        order = names[i % 3:] + names[:i % 3]                   # the variants alternate, none of them always first
        for name in order:
            e.upload_batch_audio(f, audios, labels, ll, None, wave=variants[name])
            ms = f.times()[1]
            if i >= a.warmup:
                front[name].append(ms * 1e3)
        for name in alone:
            f.augment_audio(audios, None, variants[name])
            if i >= a.warmup:
                alone[name].append(f.times()[1] * 1e3)
    e.close()
    f.close()
    out = {'B': B, 'seconds': a.seconds, 'samplerate': sr, 'numcep': 26, 'numcontext': 10, 'rir_taps': a.taps, 'reps': a.reps,
           'fir_gfma': round(B * n * a.taps / 1e9, 3)}
    for group, series in (('front_end_kernels', front), ('wave_kernels_alone', alone)):
        out[group] = {}
        for name, v in series.items():
            s, half = stats(v)
            s['halves_median_us'] = [round(float(np.median(v[:half])), 1), round(float(np.median(v[half:])), 1)]
            out[group][name] = s
    fir_us = out['wave_kernels_alone']['rir+noise']['median_us'] - out['wave_kernels_alone']['noise']['median_us']
    out['fir_over_copy_us'] = round(fir_us, 1)
    out['fir_tfma_per_s'] = round(out['fir_gfma'] / fir_us * 1e3, 2) if fir_us > 0 else None
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()

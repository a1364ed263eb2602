"""MFCC front-end throughput and error: a batch of synthetic int16 utterances (default 64 x 10 s at 16 kHz, the
16000sr_26mfcc config: numcep 26, numcontext 10) through nasr_featurize, split into host-to-device copies, kernels and
device-to-host copies (device events), and through the fp64 NumPy restatement of tests/mfcc_ref.py on the same batch.
Prints one JSON line.   python tools/mfccbench.py [--utts 64 --seconds 10 --sr 16000 --numcep 26 --numcontext 10]
With --features logfbank and --deltas 1|2 the batch goes through the log-mel filterbank and the delta kernels instead
(the restatement is then tests/feat_ref.py); the line carries "features", "deltas" and "frame_width".
With --native-sr R the utterances are made at R Hz and resampled to --sr on the GPU first (nasr_featurize_rates); the
line then also carries a "resample" field: nasr_resample's phases alone, and the fp64 restatement of
tests/resample_ref.py timed on a few utterances and scaled to the batch.
With --to-batch the line also carries a "to_batch" field: the same batch made resident on a BiLSTM handle by
Engine.upload_batch_audio (features written into the batch slot on the device) and, in the same run, by the route through
the host (Featurizer.compute, zero-pad, Engine.upload_batch_context): wall time of each up to the end of the upload's
device work, and the audio call's device-timed copies and kernels.
With --normalization causal [--norm-min-frames M] the batch goes through the causal normaliser (the
restatement is then tests/causal_ref.py) and the line carries a "normalization" field: the kernels' time of the causal and
of the whole-utterance front end on the same batch, rep by rep in turn in the same run - the spectral kernel is the same
launch in both, so their difference is the normalisers'."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import causal_ref as CR                             # noqa: E402
import feat_ref as FR                               # noqa: E402
import resample_ref as RR                           # noqa: E402
from neuralasr_amd.features import Featurizer       # noqa: E402


def synth(n, sr, seed):
    """int16-quantised harmonics of a wandering pitch, syllable-rate envelope, noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 110 + 40 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6))
    phase = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(np.sin(h * phase + rng.uniform(0, 6)) / h ** 1.2 for h in range(1, 30) if h * 160 <= sr / 2)
    x = x * (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t)) / 3 + 0.05 * rng.standard_normal(n)
    return (np.clip(np.round(x * 0.3 * 32767), -32768, 32767).astype(np.int16).astype(np.float32) / np.float32(32768))


def batch_routes(a, fz, audios, rates):
    """the batch made resident on a model handle: through the host, and straight from audio"""
    from neuralasr_amd.engine import Engine
    e = Engine(fz.width, 128, 1, True, 'stack_reshape', 30)
    labels, ll = np.ones((len(audios), 1), np.int32), [1] * len(audios)

    def host_route():
        feats = fz.compute(audios, rates=rates)
        T = max(f.shape[0] for f in feats)
        x = np.zeros((len(feats), T, fz.width), np.float32)
        for b, f in enumerate(feats):
            x[b, :f.shape[0]] = f
        seq = [f.shape[0] for f in feats]
        if not e.upload_batch_context(x, seq, labels, ll, fz.numcontext, fz.frame_width):
            e.upload_batch(x, seq, labels, ll)
        e.synchronize()

    def audio_route():
        e.upload_batch_audio(fz, audios, labels, ll, rates)
        e.synchronize()
    out = {}
    for name, fn in (('host_route', host_route), ('audio_route', audio_route)):
        fn()                                              # warm-up: slot buffers
        wall = h2d = k = 0.0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            wall += time.perf_counter() - t0
            if name == 'audio_route':
                t = fz.times()
                h2d += t[0]; k += t[1]
        out[name + '_ms'] = round(wall / a.reps * 1e3, 3)
        if name == 'audio_route':
            out['audio_h2d_ms'] = round(h2d / a.reps, 3)
            out['audio_kernel_ms'] = round(k / a.reps, 3)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--sr', type=int, default=16000)
    ap.add_argument('--numcep', type=int, default=26)
    ap.add_argument('--numcontext', type=int, default=10)
    ap.add_argument('--features', choices=('mfcc', 'logfbank'), default='mfcc', help='logfbank: --numcep log-mel filters')
    ap.add_argument('--deltas', type=int, choices=(0, 1, 2), default=0, help='append delta (and delta-delta) columns')
    ap.add_argument('--normalization', choices=('utterance', 'causal'), default='utterance')
    ap.add_argument('--norm-min-frames', type=int, default=50, help='M of the causal rule')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--ref-utts', type=int, default=8, help='utterances the fp64 restatement is timed and checked on')
    ap.add_argument('--native-sr', type=int, default=None, help='make the audio at this rate and resample it to --sr')
    ap.add_argument('--to-batch', action='store_true', help='also time the batch into a model handle, both routes')
    a = ap.parse_args()
    native = a.native_sr or a.sr
    n = int(a.seconds * native)
    audios = [synth(n, native, s) for s in range(a.utts)]
    rates = None if a.native_sr is None else [native] * a.utts
    fz = Featurizer(a.sr, a.numcep, a.numcontext, max_samples=(n if rates is None else n + int(a.seconds * a.sr) + 1) * a.utts,
                    kind=a.features, deltas=a.deltas, normalization=a.normalization,
                    norm_min_frames=a.norm_min_frames if a.normalization == 'causal' else None)
    feats = fz.compute(audios, rates=rates)               # warm-up: code objects, buffers
    normalization = None
    if a.normalization == 'causal':
        whole = Featurizer(a.sr, a.numcep, a.numcontext, max_samples=fz.max_samples, kind=a.features)
        whole.compute(audios, rates=rates)
        k_causal, k_whole = [], []
        for _ in range(a.reps):
            fz.compute(audios, rates=rates)
            k_causal.append(fz.times()[1])
            whole.compute(audios, rates=rates)
            k_whole.append(whole.times()[1])
        whole.close()
        normalization = {'norm_min_frames': a.norm_min_frames, 'frames_per_utt': fz.frames(int(a.seconds * a.sr)),
                         'causal_kernel_ms': round(float(np.median(k_causal)), 4),
                         'utterance_kernel_ms': round(float(np.median(k_whole)), 4),
                         'causal_minus_utterance_ms': round(float(np.median(k_causal) - np.median(k_whole)), 4)}
    t_h2d = t_k = t_d2h = wall = 0.0
    for _ in range(a.reps):
        t0 = time.perf_counter()
        feats = fz.compute(audios, rates=rates)
        wall += time.perf_counter() - t0
        h2d, k, d2h = fz.times()
        t_h2d += h2d; t_k += k; t_d2h += d2h
    frames = sum(f.shape[0] for f in feats)
    audio_s = a.utts * a.seconds
    m = a.reps
    nref = min(a.ref_utts, a.utts)
    resample = None
    at_sr = audios
    if rates is not None:
        fz.resample(audios, rates)                        # warm-up
        r_h2d = r_k = r_d2h = r_wall = 0.0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            at_sr = fz.resample(audios, rates)
            r_wall += time.perf_counter() - t0
            h2d, k, d2h = fz.times()
            r_h2d += h2d; r_k += k; r_d2h += d2h
        nrs = min(2, a.utts)
        table = RR.table()
        t0 = time.perf_counter()
        restated = [RR.resample(x, native, a.sr, win=table) for x in audios[:nrs]]
        t_rs = (time.perf_counter() - t0) * a.utts / nrs
        resample = {'native_sr': native, 'h2d_ms': round(r_h2d / m, 3), 'kernel_ms': round(r_k / m, 3),
                    'd2h_ms': round(r_d2h / m, 3), 'call_ms': round(r_wall / m * 1e3, 3),
                    'outputs': int(sum(x.size for x in at_sr)),
                    'ref_fp64_s_batch': round(t_rs, 3), 'ref_checked_utts': nrs,
                    'bitwise_vs_ref': all(x.tobytes() == y.tobytes() for x, y in zip(at_sr, restated))}
    to_batch = batch_routes(a, fz, audios, rates) if a.to_batch else None
    t0 = time.perf_counter()
    if a.normalization == 'causal':
        ref = [CR.features(x, a.sr, a.numcontext, a.numcep, a.norm_min_frames, a.features)[0] for x in at_sr[:nref]]
    else:
        ref = [FR.features(x, a.sr, a.numcontext, a.numcep, a.features, a.deltas)[0] for x in at_sr[:nref]]
    t_ref = (time.perf_counter() - t0) * a.utts / nref
    err = np.concatenate([np.abs(f.astype(np.float64) - r).ravel() for f, r in zip(feats, ref)])
    fz.close()
    print(json.dumps({
        'utts': a.utts, 'seconds_each': a.seconds, 'sr': a.sr, 'numcep': a.numcep, 'numcontext': a.numcontext,
        'features': a.features, 'deltas': a.deltas, 'frame_width': fz.frame_width,
        'frames': frames, 'out_mb': round(frames * feats[0].shape[1] * 4 / 2 ** 20, 1),
        'h2d_ms': round(t_h2d / m, 3), 'kernel_ms': round(t_k / m, 3), 'd2h_ms': round(t_d2h / m, 3),
        'call_ms': round(wall / m * 1e3, 3),
        'audio_s_per_s_call': round(audio_s / (wall / m)), 'audio_s_per_s_kernels': round(audio_s / (t_k / m * 1e-3)),
        'frames_per_s_call': round(frames / (wall / m)), 'frames_per_s_kernels': round(frames / (t_k / m * 1e-3)),
        'ref_fp64_s_batch': round(t_ref, 3), 'ref_checked_utts': nref,
        'max_abs_err': float(err.max()), 'mean_abs_err': float(err.mean()),
        **({} if normalization is None else {'normalization': normalization}),
        **({} if resample is None else {'resample': resample}),
        **({} if to_batch is None else {'to_batch': to_batch})}))


if __name__ == '__main__':
    main()

"""Generates tests/golden/frontend_parent.json: SHA-256 digests of what the feature front end gives on every route out of it
(tests/test_gpu_frontend_parent_bits.py runs the same cases and compares).  Run it on an MI355X with the commit BEFORE a
change to the front end's kernels or their launchers (csrc/mfcc.hip), to the featurizer handle (csrc/nasr_fz.hip) or to the
resampling and waveform-augmentation kernels it drives is built (`python tests/golden/make_frontend_parent_golden.py`); a
change that claims to keep every bit is then measured against what that commit computed.  A mismatch is fixed in the code,
never by running this again.

Only data is written.  Feature arrays and logits are digested as their float32 bytes, the (mean, std) pairs as their
float64 bytes.  Only the public calls of Featurizer and Engine are used; every input comes from a fixed numpy seed: Gaussian
noise of sd 0.1 (about +-0.3) at 8 kHz, so a frame is 200 samples and a step 80, and T frames are 200 + 80 (T - 1) samples.
`python make_frontend_parent_golden.py OUT ID...` runs only the cases named and merges them into OUT."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'frontend_parent.json')

SR, FLEN, FSTEP = 8000, 200, 80
H, C = 8, 5

CONFIGS = {
    'A': dict(numcep=13, numcontext=2),
    'B': dict(numcep=13, numcontext=0),
    'C': dict(numcep=26, numcontext=1, kind='logfbank', deltas=2),
    'D': dict(numcep=13, numcontext=2, normalization='causal', norm_min_frames=5),
    'E': dict(numcep=5, numcontext=3, normalization='causal'),                      # the default norm_min_frames, 50
}

# in samples: one frame, one frame, two frames; then T frames: fewer than E's numcontext and at or below A's and D's (2, 3),
# around the two norm_min_frames (4, 5, 6 and 49, 50, 51), the chunk edges of causal_prefix and of the NORM_THREADS-strided
# writer loops (256, 257, 513)
SAMPLES = [1, FLEN, FLEN + 1] + [FLEN + FSTEP * (T - 1) for T in (2, 3, 4, 5, 6, 49, 50, 51, 256, 257, 513)]
ZEROS = FLEN + FSTEP * 6                                   # one utterance of exact zeros: sd = 1 under the causal rule

CASES = ([dict(id='feat-' + k, kind='feat', cfg=k) for k in 'ABCDE']
         + [dict(id='resample-mixed', kind='resample', cfg='A', rates=[8000, 16000, 11025, 44100]),
            dict(id='resample-none', kind='resample', cfg='A', rates=[8000, 8000, 8000, 8000]),
            dict(id='waveaug', kind='waveaug', cfg='A'),
            dict(id='slot-A', kind='slot', cfg='A'),
            dict(id='slot-D', kind='slot', cfg='D'),
            dict(id='stream-D', kind='stream', cfg='D')])


def case_id(c):
    return c['id']


def digest(x, dtype=np.float32):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=dtype).tobytes()).hexdigest()


def noise(rs, n):
    return (0.1 * rs.randn(n)).astype(np.float32)


def featurizer(key):
    from neuralasr_amd.features import Featurizer
    return Featurizer(SR, nfilt=128, **CONFIGS[key])


def net(F):
    from neuralasr_amd.engine import Engine
    e = Engine(F, H, 1, False, 'none', C, learning_rate=1e-3)
    e.set_params((0.2 * np.random.RandomState(21).randn(e.param_count)).astype(np.float32))
    return e


def abs_sum(arrays):
    return float(sum(np.abs(np.asarray(a, np.float64)).sum() for a in arrays))


def run_feat(case, f):
    rs = np.random.RandomState(101)
    audios = [noise(rs, n) for n in SAMPLES]
    audios.insert(5, np.zeros(ZEROS, np.float32))
    feats, stats = f.compute(audios, return_stats=True)
    return dict(frames=[int(len(x)) for x in feats], feats=[digest(x) for x in feats], stats=digest(stats, np.float64),
                abs_sum=abs_sum(feats))


def run_resample(case, f):
    rs = np.random.RandomState(102)
    audios = [noise(rs, n) for n in (1000, 2000, 1501, 5000)]
    res = f.resample(audios, case['rates'])
    feats, stats = f.compute(audios, return_stats=True, rates=case['rates'])
    return dict(samples=[int(x.size) for x in res], resampled=[digest(x) for x in res], frames=[int(len(x)) for x in feats],
                feats=[digest(x) for x in feats], stats=digest(stats, np.float64), abs_sum=abs_sum(res) + abs_sum(feats))


def run_waveaug(case, f):
    """RIR only (300 taps), noise only at 0 dB (the clip longer than the utterance), both at 20 dB (1 tap, the clip shorter
    than the utterance: it wraps), neither"""
    from neuralasr_amd.engine import WaveAug
    rs = np.random.RandomState(103)
    f.set_rirs([np.array([0.8], np.float32), (rs.randn(300) * np.exp(-np.arange(300) / 40.0) * 0.3).astype(np.float32)])
    f.set_noise([noise(rs, 4000), noise(rs, 700)])
    audios = [noise(rs, n) for n in (2000, 1800, 2500, 1200)]
    wave = WaveAug([1, -1, 0, -1], [-1, 0, 1, -1], [0, 7, 3, 0], [0.0, 0.0, 20.0, 0.0])
    out = f.augment_audio(audios, None, wave)
    return dict(samples=[int(x.size) for x in out], audio=[digest(x) for x in out], abs_sum=abs_sum(out))


def run_slot(case, f):
    """the batch-slot form of the normaliser: B = 3, a 1-frame utterance last"""
    rs = np.random.RandomState(104)
    audios = [noise(rs, FLEN + FSTEP * 8), noise(rs, FLEN + FSTEP * 3 + 17), noise(rs, FLEN)]
    e = net(f.width)
    seq, T = e.upload_batch_audio(f, audios, np.array([[1], [2], [3]], np.int32), [1, 1, 1])
    logits = e.forward_resident(3, T)
    e.close()
    return dict(seq_len=[int(x) for x in seq], T=int(T), logits=digest(logits), abs_sum=abs_sum([logits]))


def run_stream(case, f):
    """two slots, 3000 samples each in pieces of 100, 700 and 2200: slot 0 ends with `last` on its final piece, slot 1 with
    an empty `last` feed"""
    rs = np.random.RandomState(105)
    audios = [noise(rs, 3000), noise(rs, 3000)]
    e = net(f.width)
    e.stream_open(2)
    e.stream_attach_audio(f)
    got, rows_all, pos = [[], []], [], 0
    feeds = [(k, [False, False]) for k in (100, 700)] + [(2200, [True, False]), (0, [False, True])]
    for k, last in feeds:
        chunks = [a[pos:pos + k] if k else None for a in audios]
        pos += k
        logits, rows = e.stream_feed_audio(chunks, last)
        rows_all.append([int(r) for r in rows])
        for b in range(2):
            got[b].append(logits[:rows[b], b].copy())
    e.stream_close()
    e.close()
    out = [np.concatenate(g) for g in got]
    return dict(rows=rows_all, logits=[digest(x) for x in out], abs_sum=abs_sum(out))


RUN = dict(feat=run_feat, resample=run_resample, waveaug=run_waveaug, slot=run_slot, stream=run_stream)


def run_case(case):
    """Runs the case on a fresh featurizer: the record that goes into the JSON"""
    f = featurizer(case['cfg'])
    try:
        return RUN[case['kind']](case, f)
    finally:
        f.close()


def main():
    sys.path.insert(0, ROOT)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    only = sys.argv[2:]
    doc = {}
    if only and os.path.exists(out):
        with open(out) as f:
            doc = json.load(f)
    doc['_note'] = ('SHA-256 of the features, statistics, resampled and augmented samples and of the logits of batches and '
                    'stream feeds given as audio, taken on an MI355X from the commit before the front end was split into '
                    'kernels (csrc/mfcc.hip) and handle (csrc/nasr_fz.hip).  tests/golden/make_frontend_parent_golden.py')
    for c in CASES:
        if only and case_id(c) not in only:
            continue
        rec = run_case(c)
        doc[case_id(c)] = rec
        print(case_id(c), {k: (v if not isinstance(v, str) else v[:16]) for k, v in rec.items()
                           if not (isinstance(v, list) and v and isinstance(v[0], str))}, flush=True)
        with open(out, 'w') as f:                     # after every case: what ran is kept whatever the next one does
            json.dump(doc, f, indent=1)
            f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()

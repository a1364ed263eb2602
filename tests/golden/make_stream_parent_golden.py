"""Generates tests/golden/stream_parent.json: SHA-256 digests of what the stream sessions give, feed by feed, for the
cases below (tests/test_gpu_stream_parent_bits.py runs the same cases and compares).  Run it on an MI355X with the commit
BEFORE a change to the session code (csrc/nasr_stream.hip), its state kernels (csrc/lstm.hip) or the chunk's pass
(csrc/nasr_pass.hip) is built (`python tests/golden/make_stream_parent_golden.py`); a change that claims to keep every
bit is then measured against what that commit computed.  A mismatch is fixed in the code, never by running this again.

Only data is written.  After every feed: digests of the rows each slot emitted (logits[:rows[b], b] only: the other rows
are unspecified), of stream_state() and of stream_frames() (floats as float32(x + 0.0) bytes, so the sign of an exact
zero does not count; int arrays as int32), and the row counts in plain.  Only Engine's and Featurizer's public calls are
used; every input comes from a fixed numpy seed."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'stream_parent.json')

F, C = 13, 5
SR, NUMCEP, NUMCONTEXT, NORM_MIN = 8000, 13, 2, 3     # the front end of tests/test_gpu_stream_audio.py, its smallest M
FLEN, FSTEP = 200, 80                                 # 25 ms and 10 ms at 8 kHz


def cycle(S, k):
    return [(b + k) % 4 for b in range(S)]


# A step is ('feed', n, Tc, last) - frames: n[b] rows inside a chunk of Tc, samples: n[b] samples (Tc unused) - or
# ('reset', slots) or ('params', seed): set_params between two feeds.
SAMPLES = [
    ('feed', [100, 0], None, None),                   # fewer than NORM_MIN complete frames: Tc = 0, no pass
    ('feed', [437, 0], None, None),                   # slot 1 idle
    ('feed', [333, 800], None, None),
    ('feed', [630, 901], None, None),                 # slot 0 now has all of its 1500 samples
    ('feed', [0, 0], None, [1, 0]),                   # `last` on slot 0 with no samples: the held rows leave
    ('reset', [0]),
    ('feed', [700, 0], None, None),                   # slot 0 reused for a second utterance
    ('feed', [513, 0], None, [1, 1]),                 # slot 1 finishes without samples
]
CASES = [
    dict(id='frames-H70x2-S3', kind='frames', H=70, L=2, S=3, R=0, steps=[
        ('feed', [4, 1, 0], 4, None),
        ('feed', [0, 3, 2], 3, None),
        ('feed', [5, 5, 5], 6, None),                 # the chunk is longer than every slot's rows
        ('feed', [0, 0, 0], 2, None),                 # runs, nothing moves
        ('reset', [1]),
        ('feed', [2, 2, 2], 2, None)]),
    dict(id='frames-H32-S17', kind='frames', H=32, L=1, S=17, R=0, steps=[   # two M tiles, 15 padded slots
        ('feed', cycle(17, 0), 3, None),
        ('feed', cycle(17, 1), 3, None)]),
    dict(id='frames-rebuild-H32x2-S2', kind='frames', H=32, L=2, S=2, R=0, persistent=True, steps=[
        ('feed', [6, 6], 6, None),
        ('params', 12),                               # the session rebuilds the per-step operand images itself
        ('feed', [8, 3], 8, None)]),
    dict(id='samples-S2', kind='samples', H=16, L=2, S=2, R=0, steps=SAMPLES),
    dict(id='lookahead-H70x2-S3-R3', kind='frames', H=70, L=2, S=3, R=3, steps=[
        ('feed', [2, 1, 0], 2, None),                 # every slot only holds: no pass
        ('feed', [1, 4, 0], 4, None),                 # slot 0 gets fewer rows than it holds, emits nothing; slot 1 emits 2 of 5
        ('feed', [5, 0, 2], 5, None),
        ('feed', [0, 0, 0], 0, [1, 0, 1]),            # slot 2's whole utterance is shorter than R
        ('reset', [0]),
        ('feed', [4, 0, 0], 4, None)]),
    dict(id='lookahead-H32-S17-R1', kind='frames', H=32, L=1, S=17, R=1, steps=[
        ('feed', cycle(17, 0), 3, None),
        ('feed', cycle(17, 1), 3, None)]),
    dict(id='lookahead-samples-S2-R4', kind='samples', H=16, L=2, S=2, R=4, steps=SAMPLES),
]


def case_id(c):
    return c['id']


def digest(x):
    """SHA-256 over the bytes of x: floats as float32(x + 0.0), everything else as int32"""
    a = np.asarray(x)
    if a.dtype.kind == 'f':
        a = a.astype(np.float32) + np.float32(0.0)
    else:
        a = a.astype(np.int32)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def audio(n, seed):
    """n samples of three drifting tones under noise, quantised to int16 (float32 x / 32768)"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / SR
    x = sum(np.sin(2 * np.pi * f * t * (1 + 0.1 * np.sin(2 * np.pi * 3 * t)) + rs.uniform(0, 6)) / (k + 1)
            for k, f in enumerate((180.0, 730.0, 2100.0)))
    x = 0.15 * x + 0.03 * rs.randn(n)
    return (np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16).astype(np.float32) / np.float32(32768))


def params(e, seed):
    return (0.2 * np.random.RandomState(seed).randn(e.param_count)).astype(np.float32)


def run_case(case):
    """Runs the case on a fresh engine: {'mode': the recurrence mode reached, 'feeds': [a record per feed]}"""
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine
    from neuralasr_amd.features import Featurizer
    S, R, samples = case['S'], case['R'], case['kind'] == 'samples'
    fz = Featurizer(SR, NUMCEP, NUMCONTEXT, normalization='causal', norm_min_frames=NORM_MIN) if samples else None
    e = Engine(fz.width if samples else F, case['H'], case['L'], R > 0, 'concat' if R > 0 else 'none', C, learning_rate=1e-3)
    if case.get('persistent'):
        try:
            e.set_recurrence_mode(True)
        except _lib.NasrError:
            pass                                      # no resident kind on this device: `mode` says so
    e.set_params(params(e, 11))
    if R > 0:
        e.stream_open_lookahead(S, R)
    else:
        e.stream_open(S)
    if samples:
        e.stream_attach_audio(fz)
    rs = np.random.RandomState(len(case['id']) + 100 * S)
    utt = [audio(4000, 20 + b) for b in range(S)]     # the samples each slot takes its pieces from, in order
    sent = [0] * S
    feeds = []
    for step in case['steps']:
        if step[0] == 'reset':
            e.stream_reset(step[1])
            continue
        if step[0] == 'params':
            e.set_params(params(e, step[1]))
            continue
        _, n, Tc, last = step
        if samples:
            chunks = [utt[b][sent[b]:sent[b] + n[b]] if n[b] else None for b in range(S)]
            sent = [sent[b] + n[b] for b in range(S)]
            logits, rows = e.stream_feed_audio(chunks, last)
        else:
            feats = rs.randn(S, Tc, F).astype(np.float32)        # the rows past n[b] are not zeroed: nothing may read them
            if R > 0:
                logits, rows = e.stream_feed_lookahead(feats, n, last)
            else:
                logits, rows = e.stream_feed(feats, n), np.asarray(n, np.int32)
        emitted = np.concatenate([logits[:rows[b], b].ravel() for b in range(S)])
        feeds.append({'rows': [int(x) for x in rows], 'frames': [int(x) for x in e.stream_frames()],
                      'T_out': int(logits.shape[0]), 'logits': digest(emitted), 'state': digest(e.stream_state()),
                      'frames_digest': digest(e.stream_frames()), 'rows_digest': digest(rows),
                      'logits_abs_sum': float(np.abs(emitted.astype(np.float64)).sum())})
    rec = {'mode': e.recurrence_mode, 'feeds': feeds}
    e.close()
    if fz is not None:
        fz.close()
    return rec


def main():
    sys.path.insert(0, ROOT)
    doc = {'_note': 'SHA-256 of what every feed of a stream session emitted, of stream_state() and of stream_frames(), taken on '
                    'an MI355X from the commit before the four feed routes became one.  tests/golden/make_stream_parent_golden.py'}
    for c in CASES:
        rec = run_case(c)
        doc[case_id(c)] = rec
        print(case_id(c), rec['mode'], flush=True)
        for f in rec['feeds']:
            print('   rows', f['rows'], 'frames', f['frames'], 'T', f['T_out'], 'sum|logits|', f['logits_abs_sum'], f['logits'][:16],
                  f['state'][:16], flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()

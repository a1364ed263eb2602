"""GPU: frame_skip (nasr_set_frame_skip).  The batch funnel's output is a copy, so a handle with skip s
given the input X must compute THE BITS of a handle with skip 1 given the host-made rows of the kept frames
(tests/frame_skip_ref.py: include_context, rows [::s], zeros from the network length on, the full form, the network lengths,
T' = ceil(T/s)).  No tolerance anywhere.  The two sides of a comparison run on ONE handle, the skip switched in between and
the parameters put back: which kernels run the recurrence is settled per handle at create (test_gpu_audio_batch.py says
why), and every comparison checks that they stayed the same.  Shapes: numcep 13, numcontext 1 (F 39), H 24, 2 layers, C 7."""
import ctypes
import os

import numpy as np
import pytest

import frame_skip_ref as R
from test_gpu_mfcc import speech_like

pytestmark = pytest.mark.gpu

NUMCEP, NC, F, H, C = 13, 1, 39, 24, 7
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')

NETS = {'concat': (2, True, 'concat'), 'lstm': (2, False, 'none'), 'stack_reshape': (1, True, 'stack_reshape')}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def init(e, seed=3):
    """seeded parameters and a fresh optimiser: also puts a handle that has taken a step back where it started"""
    rs = np.random.RandomState(seed)
    e.set_params((0.2 * rs.randn(e.param_count)).astype(np.float32))
    zero = np.zeros(e.param_count, np.float32)
    e.set_adam_state(zero, zero, 0)
    return e


def make(kind):
    from neuralasr_amd.engine import Engine
    layers, bidi, merge = NETS[kind]
    return init(Engine(F, H, layers, bidi, merge, C, learning_rate=1e-3))


@pytest.fixture(scope='module')
def nets():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = make(kind)
        return made[kind]
    yield get
    for e in made.values():
        e.close()


def kernels(e):
    return e.recurrence_mode, e.persist_stats()


class Batch:
    """utterances of centre frames (seeded), pad values, labels without repeats (so label_len frames are enough)"""

    def __init__(self, lens, label_lens, T, seed, pads=True):
        rng = np.random.default_rng(seed)
        self.B, self.T, self.lens = len(lens), T, list(lens)
        self.utts = [rng.standard_normal((n, NUMCEP)).astype(np.float32) for n in lens]
        self.pads = [float(np.float32(p)) for p in rng.uniform(-0.9, 0.9, self.B)] if pads else [0.0] * self.B
        self.label_len = list(label_lens)
        self.labels = np.zeros((self.B, max(label_lens)), np.int32)
        for b, n in enumerate(label_lens):
            self.labels[b, :n] = (np.arange(n) + b) % (C - 1)            # neighbours differ: C - 1 >= 2 labels
        self.feats, _ = R.input_batch(self.utts, NC, NUMCEP, T, self.pads)

    def kept(self, s, utts=None):
        return R.kept_batch(self.utts if utts is None else utts, NC, NUMCEP, self.T, s, self.pads)


def batch_a(seed=11):
    return Batch([41, 40, 39, 7, 1], [4, 3, 2, 1, 1], 41, seed)


def batch_b(seed=12):
    return Batch([12] * 16, [2] * 16, 12, seed)


def upload_skip(e, b, form, aug=None):
    """the caller's batch, input frames and input lengths, in the given form"""
    if form == 'centre':
        assert e.upload_batch_context(b.feats, b.lens, b.labels, b.label_len, NC, NUMCEP, aug=aug)
    else:
        assert aug is None
        e.upload_batch(b.feats, b.lens, b.labels, b.label_len)
    return b.T


def upload_ref(e, b, s, utts=None):
    """the host-made rows of the kept frames, the full form, the network lengths"""
    feats, lens = b.kept(s, utts)
    e.upload_batch(feats, lens, b.labels, b.label_len)
    return feats.shape[1]


def observe(e, B, T):
    out = {'logits': e.forward_resident(B, T)}
    out['loss_fwd'], out['nll'] = e.loss_resident(B)
    e.compute_grads()
    out['loss'] = e.get_loss()
    out['grads'] = e.get_grads()
    return out


def assert_same(got, want, note=''):
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = np.asarray(got[k], np.float32), np.asarray(want[k], np.float32)
        assert same(g, w), '%s differs: shapes %s %s, %d elements, max |difference| %g %s' % (
            k, g.shape, w.shape, int(np.sum(bits(g) != bits(w))) if g.shape == w.shape else -1,
            float(np.abs(g.astype(np.float64) - w).max()) if g.shape == w.shape else float('nan'), note)


def both(e, b, s, form, aug=None, ref_utts=None, watch=observe):
    """(what the skip-s side gives, what the skip-1 side gives), on handle e, which ends at skip 1"""
    before = kernels(e)
    e.set_frame_skip(s)
    assert e.frame_skip == s
    T = upload_skip(e, b, form, aug)
    assert e.logit_frames(T) == R.net_len(T, s) * (2 if e.cfg.merge == 1 else 1)
    got = watch(e, b.B, T)
    e.set_frame_skip(1)
    Tn = upload_ref(e, b, s, ref_utts)
    want = watch(e, b.B, Tn)
    assert kernels(e) == before, 'the recurrence changed kernels between the two sides'
    return got, want


CASES = [('A', 2), ('A', 3), ('A', 4), ('B', 3)]


# ---- 1. logits, loss and every gradient tensor
@pytest.mark.parametrize('form', ['centre', 'full'])
@pytest.mark.parametrize('which,s', CASES, ids=['A-s2', 'A-s3', 'A-s4', 'B-s3'])
@pytest.mark.parametrize('kind', list(NETS))
def test_step_bits_equal_the_skip1_handle_on_kept_rows(nets, kind, which, s, form):
    e = nets(kind)
    b = batch_a() if which == 'A' else batch_b()
    got, want = both(e, b, s, form)
    assert got['logits'].shape[0] == e.logit_frames(R.net_len(b.T, s))      # (skip 1 again: the network's frames)
    assert_same(got, want, '(%s, batch %s, s = %d, %s form)' % (kind, which, s, form))
    assert np.isfinite(got['grads']).all() and np.abs(got['grads']).max() > 0


def test_what_the_resident_calls_report(nets):
    """input B, T and input frames stay the caller's; rows are the network's; batch A is compacted, batch B is not"""
    e = nets('concat')
    a, b = batch_a(), batch_b()
    e.set_frame_skip(3)
    try:
        upload_skip(e, a, 'centre')
        rb, rt = ctypes.c_int(), ctypes.c_int()
        e._ck(e.lib.nasr_resident_shape(e.h, ctypes.byref(rb), ctypes.byref(rt)))
        assert (rb.value, rt.value) == (5, 41)
        assert e.resident_frames() == sum(a.lens)
        assert e.resident_rows() == sum(R.net_len(n, 3) for n in a.lens)     # compacted: the network's frames
        upload_skip(e, b, 'full')
        assert e.resident_frames() == 16 * 12 and e.resident_rows() == R.net_len(12, 3) * 16
    finally:
        e.set_frame_skip(1)


def test_step_bits_on_the_per_step_recurrence(nets):
    e = nets('concat')
    was = e.recurrence_mode
    e.set_recurrence_mode(False)
    try:
        assert e.recurrence_mode == 'per-step'
        got, want = both(e, batch_a(), 2, 'centre')
        assert_same(got, want, '(per-step recurrence)')
    finally:
        if was != 'per-step':
            e.set_recurrence_mode(True)


# ---- 2. SpecAugment masks, in input frames
@pytest.mark.parametrize('s', [2, 3, 4])
def test_masked_batch_bits(nets, s):
    """utterance 0's first time mask covers frames 6 and 7: 6 is kept at s = 2 and 3 and 7 is not; at s = 4 its second one
    covers 20 (kept) and 21, 22 (not).  The reference masks the centre frames on the host, then stacks and slices."""
    from neuralasr_amd.engine import BatchAug
    e = nets('concat')
    b = batch_a()
    tm = np.asarray([[(6, 2), (20, 3)], [(9, 2), (30, 1)], [(0, 3), (38, 1)], [(2, 2), (0, 0)], [(0, 1), (0, 0)]], np.int32)
    fm = np.asarray([[(3, 4)], [(0, 2)], [(11, 2)], [(5, 0)], [(6, 3)]], np.int32)
    got, want = both(e, b, s, 'centre', aug=BatchAug(NUMCEP, tm, fm), ref_utts=R.masked(b.utts, NUMCEP, tm, fm))
    assert_same(got, want, '(masked, s = %d)' % s)
    # (and the masks did something: the unmasked batch gives other logits)
    e.set_frame_skip(s)
    upload_skip(e, b, 'centre')
    plain = e.forward_resident(b.B, b.T)
    e.set_frame_skip(1)
    assert not same(plain, got['logits'])


# ---- 3. from audio
def test_audio_batch_bits(nets):
    """nasr_upload_batch_audio under skip 3 against the featurizer's own rows [::3] on the skip-1 handle: bits, of
    everything test_gpu_audio_batch.py compares"""
    from neuralasr_amd.features import Featurizer
    e = nets('concat')
    f = Featurizer(8000, NUMCEP, NC)
    s = 3
    try:
        audios = [speech_like(n, 8000, 40 + i) for i, n in enumerate((2900, 1700, 96))]
        labels = np.asarray([[1, 2, 3], [4, 0, 0], [2, 0, 0]], np.int32)
        label_len = [3, 1, 1]

        def watch(B, T):
            out = observe(e, B, T)
            out['greedy'] = np.asarray([len(h) for h in e.greedy_decode_resident(B, T)], np.float32)
            e.compute_grads()
            e.apply_adam(1.0)
            out['params'] = e.get_params()
            return out
        before = kernels(e)
        init(e)
        e.set_frame_skip(s)
        seq, T = e.upload_batch_audio(f, audios, labels, label_len)
        rows = f.compute(audios)
        assert [int(t) for t in seq] == [r.shape[0] for r in rows] and T == max(seq)       # input frames, as ever
        assert e.resident_frames() == int(sum(seq))
        got = watch(3, T)
        e.set_frame_skip(1)
        init(e)
        kept = [r[::s] for r in rows]
        e.upload_batch(R.padded(kept, R.net_len(T, s)), [k.shape[0] for k in kept], labels, label_len)
        want = watch(3, R.net_len(T, s))
        assert kernels(e) == before
        assert_same(got, want, '(from audio)')
    finally:
        e.set_frame_skip(1)
        init(e)
        f.close()


# ---- 4. two optimiser steps; a staged batch
def test_two_adam_steps_and_a_staged_batch(nets):
    e = nets('concat')
    a, a2, s = batch_a(), batch_a(seed=21), 2

    def steps(upload):
        init(e)
        for b in (a, a2):
            upload(b)
            e.compute_grads()
            e.apply_adam(1.0)
        m, v, step = e.get_adam_state()
        assert step == 2
        return {'params': e.get_params(), 'm': m, 'v': v}

    def staged(b):
        ticket = e.stage_batch(b.feats, b.lens, b.labels, b.label_len, NC, NUMCEP)
        assert ticket is not None
        e.commit_batch(ticket)
    before = kernels(e)
    try:
        e.set_frame_skip(s)
        got = steps(lambda b: upload_skip(e, b, 'centre'))
        got_staged = steps(staged)
        e.set_frame_skip(1)
        want = steps(lambda b: upload_ref(e, b, s))
        assert kernels(e) == before
        assert_same(got, want, '(two steps)')
        assert_same(got_staged, want, '(two steps, staged)')
        assert not same(want['params'], init(e).get_params())
    finally:
        e.set_frame_skip(1)
        init(e)


# ---- 5. chunked training counts network frames
def test_chunked_training_bits(nets):
    e = nets('concat')
    e.set_chunking(4, 2)
    try:
        got, want = both(e, batch_a(), 2, 'centre')
        assert_same(got, want, '(chunked 4 + 2)')
    finally:
        e.set_chunking(0)
    whole, _ = both(e, batch_a(), 2, 'centre')
    assert not same(whole['logits'], got['logits'])          # (the windows were really run)


# ---- 6. greedy decode and forced alignment
@pytest.mark.parametrize('s', [2, 3, 4])
def test_greedy_and_alignment(nets, s):
    e = nets('concat')
    a = batch_a()

    def watch(e_, B, T):
        ids, lens = np.zeros((B, e_.logit_frames(T)), np.int32), np.zeros(B, np.int32)
        e_._ck(e_.lib.nasr_greedy_decode_resident(e_.h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        path, score = e_.align_resident(B, T)
        return {'ids': ids, 'lens': lens, 'path': path, 'score': score}
    got, want = both(e, a, s, 'centre', watch=watch)
    Tn = R.net_len(a.T, s)
    assert got['ids'].shape == got['path'].shape == (a.B, Tn)          # nasr_logit_frames(T) columns
    for k in ('ids', 'lens', 'path'):
        assert np.array_equal(got[k], want[k]), k
    assert got['score'].tobytes() == want['score'].tobytes()
    for b, n in enumerate(a.lens):                                      # the path ends where the network's frames do
        assert (got['path'][b, :R.net_len(n, s)] >= 0).all() and (got['path'][b, R.net_len(n, s):] == -1).all()


# ---- 7. stream sessions
STREAM_S = 3
SPLITS = [[5, 1, 7, 0, 10], [0, 4, 4, 2, 0]]          # an utterance of 23 rows, one of 10


def stream_rows(seed=31):
    rng = np.random.default_rng(seed)
    return [R.stack(rng.standard_normal((n, NUMCEP)).astype(np.float32), NC, NUMCEP) for n in (23, 10)]


def end_session(e):
    """a test's way out: the session closed if one is still open (a failed assertion left it), the skip back at 1"""
    from neuralasr_amd._lib import NasrError
    try:
        e.stream_close()
    except NasrError:
        pass
    e.set_frame_skip(1)


def chunk_of(parts, Tc):
    feats = np.zeros((len(parts), Tc, F), np.float32)
    for b, p in enumerate(parts):
        feats[b, :len(p)] = p
    return feats


def test_stream_session_bits(nets):
    from neuralasr_amd.engine import stream_keep
    e = nets('lstm')
    rows = stream_rows()
    extra = stream_rows(seed=32)[1][:4]                # what slot 1 gets after its reset
    feeds = [[SPLITS[0][k], SPLITS[1][k]] for k in range(5)]
    e.set_frame_skip(STREAM_S)
    try:
        e.stream_open(2)
        pos, phase, total, seen = [0, 0], [0, 0], [0, 0], []
        for n in feeds:
            Tc = max(n)
            parts = [rows[b][pos[b]:pos[b] + n[b]] for b in range(2)]
            logits = e.stream_feed(chunk_of(parts, Tc), n)
            assert logits.shape == (R.net_len(Tc, STREAM_S), 2, C)
            kept = []
            for b in range(2):
                idx, phase[b] = R.feed_kept(phase[b], n[b], STREAM_S)
                assert stream_keep((pos[b]) % STREAM_S, n[b], STREAM_S)[1] == len(idx)
                kept.append(parts[b][idx])
                pos[b] += n[b]
                total[b] += len(idx)
            assert e.stream_frames().tolist() == total             # rows reported = the host's bookkeeping
            seen.append((logits, kept))
        assert total == [R.net_len(23, STREAM_S), R.net_len(10, STREAM_S)]
        # slot 1 ended at phase 10 % 3 = 1; reset, it starts at phase 0 again: rows 0 and 3 of the next four are kept
        e.stream_reset([1])
        assert e.stream_frames().tolist() == [total[0], 0]
        logits = e.stream_feed(chunk_of([extra[:0], extra], 4), [0, 4])
        assert e.stream_frames().tolist() == [total[0], 2]
        seen.append((logits, [extra[:0], extra[[0, 3]]]))
        e.stream_close()
        # the skip-1 session, fed each feed's kept rows in a chunk of as many rows as the skip-3 chunk had
        e.set_frame_skip(1)
        e.stream_open(2)
        for i, (logits, kept) in enumerate(seen):
            if i == 5:
                e.stream_reset([1])
            ref = e.stream_feed(chunk_of(kept, logits.shape[0]), [len(k) for k in kept])
            assert ref.shape == logits.shape
            for b in range(2):
                assert logits[:len(kept[b]), b].tobytes() == ref[:len(kept[b]), b].tobytes(), 'feed %d slot %d' % (i, b)
        e.stream_close()
    finally:
        end_session(e)


def test_lookahead_session_bits(nets):
    e = nets('concat')
    rows = stream_rows()
    feeds = [[SPLITS[0][k], SPLITS[1][k]] for k in range(5)]
    e.set_frame_skip(STREAM_S)
    try:
        e.stream_open_lookahead(2, 2)
        pos, phase, pending, total, seen = [0, 0], [0, 0], [0, 0], [0, 0], []
        for k, n in enumerate(feeds):
            last = [k == 4, k == 4]
            parts = [rows[b][pos[b]:pos[b] + n[b]] for b in range(2)]
            want_rows, want_Te = e.stream_lookahead_rows(n, last)
            logits, got_rows = e.stream_feed_lookahead(chunk_of(parts, max(n)), n, last)
            kept = []
            for b in range(2):
                idx, phase[b] = R.feed_kept(phase[b], n[b], STREAM_S)
                kept.append(parts[b][idx])
                pos[b] += n[b]
                pending[b] += len(idx)
                emit = pending[b] if last[b] else max(0, pending[b] - 2)       # R = 2 network frames are held back
                assert got_rows[b] == want_rows[b] == emit
                pending[b] -= emit
                total[b] += emit
            assert logits.shape[0] == want_Te == max(got_rows)
            assert e.stream_frames().tolist() == total
            seen.append((logits, got_rows, kept, last))
        assert total == [R.net_len(23, STREAM_S), R.net_len(10, STREAM_S)]
        e.stream_close()
        e.set_frame_skip(1)
        e.stream_open_lookahead(2, 2)
        for i, (logits, got_rows, kept, last) in enumerate(seen):
            n = [len(k) for k in kept]
            ref, ref_rows = e.stream_feed_lookahead(chunk_of(kept, max(n)), n, last)
            assert ref_rows.tolist() == got_rows.tolist() and ref.shape == logits.shape
            for b in range(2):
                assert logits[:got_rows[b], b].tobytes() == ref[:got_rows[b], b].tobytes(), 'feed %d slot %d' % (i, b)
        e.stream_close()
    finally:
        end_session(e)


def test_stream_from_audio_bits(nets):
    """feed_audio under normalization=causal and skip 3: the logits are those of feed() given that front end's rows, the
    kept ones (DESIGN.md §16's bit-for-bit claim is the standard), whatever pieces the samples arrive in"""
    from neuralasr_amd.features import Featurizer
    e = nets('lstm')
    f = Featurizer(8000, NUMCEP, NC, normalization='causal', norm_min_frames=3)
    audio = [speech_like(3100, 8000, 51), speech_like(1500, 8000, 52)]
    offline = [f.compute([a])[0] for a in audio]
    pieces = [[433, 80, 1, 900, 0, 1686], [0, 700, 0, 800, 0, 0]]
    e.set_frame_skip(STREAM_S)
    try:
        e.stream_open(2)
        e.stream_attach_audio(f)
        sent, total, seen = [0, 0], [0, 0], []
        for k in range(6):
            sizes = [pieces[0][k], pieces[1][k]]
            last = [k == 5, k == 3]
            chunks = [audio[b][sent[b]:sent[b] + sizes[b]] if sizes[b] else None for b in range(2)]
            want_rows, Tc = e.stream_audio_rows(sizes, last)
            logits, rows = e.stream_feed_audio(chunks, last)
            assert np.array_equal(rows, want_rows) and logits.shape == (Tc, 2, C) and Tc == int(rows.max())
            for b in range(2):
                sent[b] += sizes[b]
                total[b] += int(rows[b])
            assert e.stream_frames().tolist() == total
            seen.append((logits, rows))
        assert sent == [3100, 1500]
        assert total == [R.net_len(len(o), STREAM_S) for o in offline]       # every kept row came out, and no other
        e.stream_close()
        e.set_frame_skip(1)
        e.stream_open(2)
        pos = [0, 0]
        for i, (logits, rows) in enumerate(seen):
            if not logits.shape[0]:
                continue
            parts = [offline[b][::STREAM_S][pos[b]:pos[b] + rows[b]] for b in range(2)]
            ref = e.stream_feed(chunk_of(parts, logits.shape[0]), rows)
            for b in range(2):
                assert logits[:rows[b], b].tobytes() == ref[:rows[b], b].tobytes(), 'feed %d slot %d' % (i, b)
                pos[b] += int(rows[b])
        e.stream_close()
    finally:
        end_session(e)
        f.close()


# ---- 8. refusals
def test_refusals(nets):
    from neuralasr_amd._lib import InfeasibleLabelError, NasrError
    from neuralasr_amd.engine import LasEngine, WaveNetEngine
    e = nets('lstm')
    for bad in (0, 9):
        with pytest.raises(NasrError, match=r'frame_skip = %d: must be in \[1,8\]' % bad):
            e.set_frame_skip(bad)
    assert e.frame_skip == 1
    for other in (WaveNetEngine(F, C, num_blocks=1, rates=(1, 2)), LasEngine(F, C)):
        try:
            with pytest.raises(NasrError, match='a WaveNet or LAS handle takes every frame'):
                other.set_frame_skip(2)
            other.set_frame_skip(1)
            assert other.frame_skip == 1
        finally:
            other.close()
    e.stream_open(1)
    try:
        with pytest.raises(NasrError, match='a stream session is open'):
            e.set_frame_skip(2)
        assert e.frame_skip == 1
    finally:
        e.stream_close()
    a = batch_a()
    try:
        e.set_frame_skip(2)
        ticket = e.stage_batch(a.feats, a.lens, a.labels, a.label_len, NC, NUMCEP)
        e.set_frame_skip(3)
        with pytest.raises(NasrError, match=r'staged under another nasr_set_frame_skip \(2\).*\(3\): stage it again'):
            e.commit_batch(ticket)
        # utterance 3 has 7 input frames: 3 labels fit those, not its 2 network frames at s = 4
        e.set_frame_skip(4)
        labels = np.zeros((5, 4), np.int32)
        labels[:, :4] = [0, 1, 2, 3]
        with pytest.raises(InfeasibleLabelError, match=r'required: 3, available: 2 network frames: 7 input frames under '
                                                       r'frame_skip 4\) in sequence 3'):
            e.upload_batch(a.feats, a.lens, labels, [4, 3, 2, 3, 1])
        e.set_frame_skip(1)
        e.upload_batch(a.feats, a.lens, labels, [4, 3, 2, 3, 1])            # (the input frames are enough)
    finally:
        e.set_frame_skip(1)


def config_with(tmp_path, **extra):
    out = []
    for ln in open(os.path.join(SAMPLES, 'toy.config')).read().splitlines():
        if ln.startswith('output='):
            ln = 'output=' + SAMPLES
        elif ln.startswith('model_dir='):
            ln = 'model_dir=' + str(tmp_path / 'model')
        out.append(ln)
        if ln.strip() == '[Parameters]':
            out += ['%s=%s' % kv for kv in extra.items()]
    p = tmp_path / 'toy.config'
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_checkpoint_remembers_the_skip(tmp_path):
    from neuralasr_amd.config import Config
    net = Config(config_with(tmp_path, frame_skip=2), True).load_network(fortraining=True)
    try:
        assert net.engine.frame_skip == 2
        net.save_checkpoint()
    finally:
        net.engine.close()
    with pytest.raises(ValueError, match='trained with frame_skip = 2, the config says frame_skip = 3'):
        Config(config_with(tmp_path, frame_skip=3), True).load_network(fortraining=False)
    with pytest.raises(ValueError, match='trained with frame_skip = 2, the config says frame_skip = 1'):
        Config(config_with(tmp_path), True).load_network(fortraining=False)
    again = Config(config_with(tmp_path, frame_skip=2), True).load_network(fortraining=False)
    assert again.engine.frame_skip == 2
    again.engine.close()


# ---- 9. s = 1 set explicitly
@pytest.mark.parametrize('kind', ['concat', 'stack_reshape'])
def test_skip_one_is_the_handle_that_never_heard_of_it(kind):
    e = make(kind)
    try:
        a = batch_a()

        def run():
            assert e.upload_batch_context(a.feats, a.lens, a.labels, a.label_len, NC, NUMCEP)
            return observe(e, a.B, a.T)
        never = run()
        state = kernels(e)
        e.set_frame_skip(1)
        set_once = run()
        e.set_frame_skip(2)
        e.set_frame_skip(1)
        back = run()
        assert kernels(e) == state
        assert_same(set_once, never, '(set_frame_skip(1))')
        assert_same(back, never, '(2, then 1 again)')
    finally:
        e.close()

"""GPU: a stream session that takes samples (nasr_stream_attach_audio / _audio_rows / _feed_audio).  The
property: whatever pieces the samples arrive in, the rows each feed reports are nasr_stream_audio_rows', and its logits
are, BIT FOR BIT, those of nasr_stream_feed on a second handle given the offline causal features (nasr_featurize with
norm = 1 of the whole utterance) sliced by those same row counts.  A tiny unidirectional net (2 layers, H 16, C 5), 8 kHz,
13 cepstra, numcontext 2, norm_min_frames 3."""
import logging

import numpy as np
import pytest

import mfcc_ref as R
from test_gpu_mfcc import speech_like

pytestmark = pytest.mark.gpu

SR, NUMCEP, NC, M, C = 8000, 13, 2, 3, 5
FLEN, FSTEP = R.frame_params(SR)


def make_fz(nc=NC, M_=M, **kw):
    from neuralasr_amd.features import Featurizer
    return Featurizer(SR, NUMCEP, nc, normalization='causal', norm_min_frames=M_, **kw)


def make_net(F, seed=3):
    from neuralasr_amd.engine import Engine
    e = Engine(F, 16, 2, False, 'none', C, learning_rate=1e-3)
    rs = np.random.RandomState(seed)
    e.set_params((0.2 * rs.randn(e.param_count)).astype(np.float32))
    return e


class Pair:
    """the session under test (fed samples) and the second handle (fed the offline features), S slots each"""

    def __init__(self, S, nc=NC, M_=M):
        self.S = S
        self.f = make_fz(nc, M_)
        self.a, self.b = make_net(self.f.width), make_net(self.f.width)
        self.a.stream_open(S)
        self.a.stream_attach_audio(self.f)
        self.b.stream_open(S)
        self.feats = [None] * S              # the offline rows of the utterance each slot is in
        self.pos = [0] * S                   # rows of it consumed
        self.audio, self.sent = [None] * S, [0] * S

    def start(self, slot, audio):
        self.audio[slot], self.sent[slot], self.pos[slot] = audio, 0, 0
        self.feats[slot] = self.f.compute([audio])[0]

    def feed(self, sizes, last=None):
        """slot b gets its next sizes[b] samples; checks the reported rows and the logits; returns the rows"""
        S = self.S
        chunks = []
        for b, k in enumerate(sizes):
            chunks.append(None if k == 0 else self.audio[b][self.sent[b]:self.sent[b] + k])
            assert k == 0 or chunks[-1].size == k
        want_rows, Tc = self.a.stream_audio_rows(sizes, last)
        logits, rows = self.a.stream_feed_audio(chunks, last)
        assert np.array_equal(rows, want_rows) and logits.shape == (Tc, S, C) and Tc == (int(rows.max()) if S else 0)
        for b, k in enumerate(sizes):
            self.sent[b] += k
        if Tc:
            feats = np.zeros((S, Tc, self.f.width), np.float32)
            for b in range(S):
                feats[b, :rows[b]] = self.feats[b][self.pos[b]:self.pos[b] + rows[b]]
                assert rows[b] == 0 or self.pos[b] + rows[b] <= len(self.feats[b])
            ref = self.b.stream_feed(feats, rows)
            for b in range(S):
                assert logits[:rows[b], b].tobytes() == ref[:rows[b], b].tobytes(), 'slot %d' % b
                self.pos[b] += int(rows[b])
        return rows

    def reset(self, slot):
        self.a.stream_reset([slot])
        self.b.stream_reset([slot])

    def close(self):
        for o in (self.a, self.b, self.f):
            o.close()


def pieces(n, k):
    return [k] * (n // k) + ([n % k] if n % k else [])


def test_three_slots_fed_in_different_pieces_and_a_reused_slot():
    """slot 0 in 37-sample pieces, slot 1 in irregular pieces with idle feeds, slot 2 whole with `last`; slot 2 is then
    reset and takes a second utterance while the others continue (every feed is checked inside Pair.feed)"""
    p = Pair(3)
    utt = [speech_like(2500, SR, 1), speech_like(3100, SR, 2), speech_like(1700, SR, 3)]
    second = speech_like(1300, SR, 4)
    for b in range(3):
        p.start(b, utt[b])
    plan0 = pieces(2500, 37)
    rng = np.random.default_rng(5)
    plan1, left = [], 3100
    while left:
        k = int(min(left, rng.choice([0, 0, 1, 79, 80, 81, 199, 200, 201, 433])))
        plan1.append(k)
        left -= k
    total = [0, 0, 0]
    i = 0
    fresh_rows = None
    while i < max(len(plan0), len(plan1)):
        k0 = plan0[i] if i < len(plan0) else 0
        k1 = plan1[i] if i < len(plan1) else 0
        last = [i == len(plan0) - 1, i == len(plan1) - 1, i == 0]
        k2 = 1700 if i == 0 else 0
        if i == 3:                                           # slot 2 finished in feed 0: reset it, start its second utterance
            assert p.a.stream_frames()[2] == R.num_frames(1700, SR)
            p.reset(2)
            assert p.a.stream_frames()[2] == 0
            p.start(2, second)
        if i == 4:
            k2, last[2] = 1300, True
        rows = p.feed([k0, k1, k2], last)
        if i == 4:
            fresh_rows = int(rows[2])
        for b in range(3):
            total[b] += int(rows[b])
        i += 1
    assert total == [R.num_frames(2500, SR), R.num_frames(3100, SR), R.num_frames(1700, SR) + R.num_frames(1300, SR)]
    assert fresh_rows == R.num_frames(1300, SR)
    assert p.a.stream_frames().tolist() == [R.num_frames(2500, SR), R.num_frames(3100, SR), R.num_frames(1300, SR)]
    p.close()


def test_a_reused_slot_equals_a_fresh_session():
    first, second = speech_like(1500, SR, 7), speech_like(2100, SR, 8)
    out = []
    for reuse in (True, False):
        f = make_fz()
        e = make_net(f.width)
        e.stream_open(1)
        e.stream_attach_audio(f)
        if reuse:
            for k in pieces(1500, 400):
                e.stream_feed_audio([first[:k]], None)       # (an utterance left unfinished: the reset clears it all)
            e.stream_reset([0])
        got, n = [], 0
        for k in pieces(2100, 333):
            lg, rows = e.stream_feed_audio([second[n:n + k]], [n + k == 2100])
            n += k
            got.append(lg[:rows[0], 0])
        out.append(np.concatenate(got))
        e.close()
        f.close()
    assert out[0].shape == (R.num_frames(2100, SR), C) and out[0].tobytes() == out[1].tobytes()


def test_thirty_seconds_in_tenth_of_a_second_feeds():
    """S = 1, 300 feeds of 800 samples: the rows sum to T (nothing is dropped, nothing grows) and every feed's logits are
    the second handle's bit for bit; numcontext 0 and M = 1 here, the other path through the ring"""
    p = Pair(1, nc=0, M_=1)
    a = speech_like(30 * SR, SR, 9)
    p.start(0, a)
    total = 0
    plan = pieces(a.size, 800)
    for i, k in enumerate(plan):
        total += int(p.feed([k], [i == len(plan) - 1])[0])
    assert total == R.num_frames(a.size, SR) == len(p.feats[0])
    p.close()


def test_an_empty_last_feed_and_tc_zero_keep_the_resident_batch():
    p = Pair(2)
    e = p.a
    rs = np.random.RandomState(1)
    feats = rs.randn(2, 6, p.f.width).astype(np.float32)
    want = e.forward(feats, [6, 4])
    frames = e.resident_frames()
    a = speech_like(FLEN + 2 * FSTEP + 30, SR, 11)           # 3 complete frames = M; numcontext 2 holds two rows back
    p.start(0, a)
    p.start(1, a)
    assert p.feed([100, 0]).tolist() == [0, 0]              # Tc = 0: fewer than M frames
    assert p.feed([FLEN + FSTEP - 100, 0]).tolist() == [0, 0]
    assert e.resident_frames() == frames
    assert e.forward_resident(2, 6).tobytes() == want.tobytes()
    rows = p.feed([FSTEP + 30, a.size])                      # slot 0: its third frame; slot 1: all at once, not finished
    assert rows.tolist() == [1, 1]
    rows = p.feed([0, 0], [True, True])                      # finishing with no samples: the padded frame and the held rows
    assert rows.tolist() == [R.num_frames(a.size, SR) - 1] * 2
    assert p.pos == [R.num_frames(a.size, SR)] * 2
    p.close()


def refused(call, code, *words):
    from neuralasr_amd import _lib
    with pytest.raises(_lib.NasrError) as err:
        call()
    assert err.value.code == code, str(err.value)
    for w in words:
        assert w in str(err.value), str(err.value)


def test_refusals():
    from neuralasr_amd import _lib
    from neuralasr_amd.features import Featurizer
    STATE, ARG = _lib.NASR_ERR_STATE, _lib.NASR_ERR_ARG
    f = make_fz()
    whole = Featurizer(SR, NUMCEP, NC)
    narrow = make_fz(nc=0)
    e, other = make_net(f.width), make_net(f.width)
    a = speech_like(1000, SR, 1)
    refused(lambda: e.stream_attach_audio(f), STATE, 'no open stream session')
    e.stream_open(2)
    refused(lambda: e.stream_feed_audio([a, None]), STATE, 'nasr_stream_attach_audio first')
    refused(lambda: e.stream_audio_rows([5, 0]), STATE, 'nasr_stream_attach_audio first')
    refused(lambda: e.stream_attach_audio(other), STATE, 'not a featurizer handle')
    refused(lambda: e.stream_attach_audio(whole), STATE, 'norm', 'causal')
    refused(lambda: e.stream_attach_audio(narrow), ARG, 'feature_size')
    e.stream_attach_audio(f)
    refused(lambda: e.stream_attach_audio(f), STATE, 'takes samples already')
    # `last` on a slot that has received no sample at all: named, nothing changed
    refused(lambda: e.stream_feed_audio([a, None], [False, True]), ARG, 'slot 1', 'no sample')
    refused(lambda: e.stream_audio_rows([a.size, 0], [False, True]), ARG, 'slot 1')
    assert e.stream_audio_rows([a.size, 0])[0].tolist() == [1 + (a.size - FLEN) // FSTEP - NC, 0]
    lg, rows = e.stream_feed_audio([a, None], [True, False])
    assert rows.tolist() == [R.num_frames(a.size, SR), 0] and e.stream_frames().tolist() == [R.num_frames(a.size, SR), 0]
    # a finished slot waits for its reset; the other slot goes on meanwhile
    refused(lambda: e.stream_feed_audio([a[:10], None]), STATE, 'slot 0', 'nasr_stream_reset')
    refused(lambda: e.stream_feed_audio([None, None], [True, False]), STATE, 'slot 0')
    lg, rows = e.stream_feed_audio([None, a[:500]])
    assert rows.tolist() == [0, max(0, 1 + (500 - FLEN) // FSTEP - NC)]
    e.stream_reset([0])
    lg, rows = e.stream_feed_audio([a[:300], None])
    assert rows.tolist() == [0, 0]
    # too small a logits buffer: NASR_ERR_ARG before anything runs
    import ctypes
    fp, i64 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    off = np.array([0, 700, 700], np.int64)
    got, Tc = np.zeros(2, np.int32), ctypes.c_int(0)
    small = np.zeros((1, 2, C), np.float32)
    rc = e.lib.nasr_stream_feed_audio(e.h, a.ctypes.data_as(fp), off.ctypes.data_as(i64), None,
                                      got.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(Tc),
                                      small.ctypes.data_as(fp), 1)
    assert rc == ARG and Tc.value > 1 and b'logits_out holds 1' in e.lib.nasr_last_error(e.h)
    assert e.stream_audio_rows([700, 0])[1] == Tc.value                       # nothing changed
    f2 = make_fz(max_samples=1000)
    e2 = make_net(f2.width)
    e2.stream_open(1)
    e2.stream_attach_audio(f2)
    with pytest.raises(ValueError, match='max_samples'):
        e2.stream_feed_audio([np.zeros(1001, np.float32)])
    for o in (e, other, e2, f, f2, whole, narrow):
        o.close()


def test_recognizer_feed_audio_and_decode_wav(tmp_path, caplog):
    """StreamingRecognizer.feed_audio on a network whose config says normalization=causal: the hypotheses are those of
    feed() on the offline causal features sliced by the rows each feed emitted; finish() completes an utterance that no
    `last` ended.  Then decode_wav --stream feeds the file's samples: Partial lines, and the final text is the last."""
    from neuralasr_amd import decode_wav
    from neuralasr_amd.config import Config
    from neuralasr_amd.features import read_wav_native
    from tests.test_gpu_align_network import corpus_config
    cfg_path, _ = corpus_config(tmp_path, 'lstm_ctc_net.LstmCTCNet')
    text = cfg_path.read_text().replace('[Train]', 'normalization=causal\nnorm_min_frames=5\n[Train]', 1)
    cfg_path.write_text(text)
    config = Config(str(cfg_path), True)
    assert (config.normalization, config.norm_min_frames) == ('causal', 5)
    network = config.load_network(fortraining=True)
    network.save_checkpoint()
    fz = network.featurizer()
    assert (fz.cfg.norm, fz.cfg.norm_min_frames) == (1, 5)
    audios = [read_wav_native(str(tmp_path / ('utt%d.wav' % i)))[0] for i in (0, 3)]
    feats = [np.asarray(x, np.float32) for x in fz.compute(audios)]
    step = 16 * FSTEP
    rec = network.stream(2)
    real, seen = network.engine.stream_feed_audio, []

    def spy(chunks, last=None):
        out = real(chunks, last)
        seen.append(out[1].copy())
        return out
    network.engine.stream_feed_audio = spy
    hyps = []
    for t in range(0, max(a.size for a in audios), step):
        hyps.append(rec.feed_audio([a[t:t + step] if t < a.size else None for a in audios],
                                   [t < audios[0].size <= t + step, False]))       # slot 0 ends with `last`, slot 1 does not
    final = [rec.finish(0), rec.finish(1)]                       # slot 1: finish() sends the empty `last` feed itself
    del network.engine.stream_feed_audio
    assert [int(sum(r[b] for r in seen)) for b in range(2)] == [len(x) for x in feats]
    rec.close()
    ref = network.stream(2)
    pos, k = [0, 0], 0
    for rows in seen[:len(hyps)]:
        want = ref.feed([feats[b][pos[b]:pos[b] + rows[b]] if rows[b] else None for b in range(2)])
        pos = [pos[b] + int(rows[b]) for b in range(2)]
        assert hyps[k] == want, k
        k += 1
    for rows in seen[len(hyps):]:
        ref.feed([feats[b][pos[b]:pos[b] + rows[b]] if rows[b] else None for b in range(2)])
        pos = [pos[b] + int(rows[b]) for b in range(2)]
    assert pos == [len(x) for x in feats]
    for b in range(2):
        got = ref.finish(b)
        assert got[0] == final[b][0] and np.float32(got[1]).tobytes() == np.float32(final[b][1]).tobytes()
    ref.close()
    network.engine.close()
    fz.close()

    with caplog.at_level(logging.INFO):
        text = decode_wav.main([str(cfg_path), str(tmp_path / 'utt4.wav'), '--stream', '--chunk-frames', '16'])
    lines = [r.getMessage() for r in caplog.records]
    partials = [m[len('Partial: '):] for m in lines if m.startswith('Partial: ')]
    decoded = [m[len('Decoded: '):] for m in lines if m.startswith('Decoded: ')]
    assert partials and decoded == [partials[-1]] and text == partials[-1]

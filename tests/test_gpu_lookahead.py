"""Look-ahead streaming of the bidirectional (concat) networks on the GPU (nasr_stream_open_lookahead / _lookahead_rows /
_feed_lookahead) through Engine, against the fp64 restatement of the rule in tests/lookahead_ref.py: every
feed's emitted logits and the forward state saved after it.  Tolerance: max-abs 1e-4 for both, the project's own figure
(tests/test_gpu_stream.py); the reference's chain is as long as the session's, so it is not widened.
No utterance exceeds 40 frames; the shapes are the smallest at which each branch of the window path can go wrong."""
import ctypes
import logging

import numpy as np
import pytest

from oracle import nasr_oracle as O
from tests import lookahead_ref as LR

pytestmark = pytest.mark.gpu

TOL = 1e-4


def make_engine(spec, lr=1e-3):
    from neuralasr_amd.engine import Engine
    return Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes,
                  forget_bias=spec.forget_bias, learning_rate=lr, pre=spec.pre, post=spec.post, relu_clip=spec.relu_clip,
                  dropout=spec.dropout)


def rand_params(spec, seed):
    rs = np.random.RandomState(seed)
    return [p + 0.05 * rs.randn(*p.shape) for p in O.init_params(spec, seed=seed)]     # non-zero biases too


def utterances(spec, lengths, seed):
    rs = np.random.RandomState(seed)
    return [rs.randn(n, spec.feature_size).astype(np.float32) for n in lengths]


def oracle_logits(spec, params, utt):
    return O.network_forward(spec, params, utt[None].astype(np.float64), [len(utt)])[0][:, 0]


class RefSlot:
    """one slot of the session in fp64: lookahead_ref's rule, feed by feed"""

    def __init__(self, spec, params, R):
        self.spec, self.params, self.R = spec, params, R
        self.reset()

    def reset(self):
        self.state = LR.zero_state(self.spec)
        self.held = np.zeros((0, self.spec.feature_size))
        self.emitted = 0

    def feed(self, rows, last):
        pend = np.concatenate([self.held, np.asarray(rows, np.float64).reshape(-1, self.spec.feature_size)])
        E, keep = LR.emitted(len(self.held), len(pend) - len(self.held), self.R, last)
        lg = np.zeros((0, self.spec.num_classes))
        if E:
            lg, self.state = LR.run_window(self.spec, self.params, pend, self.state, E)
        self.held = pend[E:]
        self.emitted += E
        assert len(self.held) == keep
        return lg


class Session:
    """an engine with an open look-ahead session and its fp64 twin; feed() checks every feed"""

    def __init__(self, spec, seed, S, R, engine=None, params=None):
        self.spec, self.S, self.R = spec, S, R
        self.params = params if params is not None else rand_params(spec, seed)
        self.e = engine or make_engine(spec)
        self.e.set_params(O.flatten(self.params))
        self.e.stream_open_lookahead(S, R)
        self.refs = [RefSlot(spec, self.params, R) for _ in range(S)]
        self.got = [[] for _ in range(S)]      # the emitted logits per slot, as the GPU gave them

    def feed(self, rows, last=None, Tc=None):
        """rows[b]: float32 [n_b, F] or None.  Returns the emitted row counts."""
        S, F, C = self.S, self.spec.feature_size, self.spec.num_classes
        n = [0 if r is None else len(r) for r in rows]
        Tc = max(n) if Tc is None else Tc
        feats = np.zeros((S, Tc, F), np.float32)
        for b in range(S):
            if n[b]:
                feats[b, :n[b]] = rows[b]
        want_rows, Te = self.e.stream_lookahead_rows(n, last)
        logits, got_rows = self.e.stream_feed_lookahead(feats, n, last)
        assert np.array_equal(got_rows, want_rows) and logits.shape == (Te, S, C) and Te == int(got_rows.max())
        state = self.e.stream_state()
        assert state.shape == (self.spec.num_layers, S, 2, self.spec.hidden) and state.dtype == np.float32
        for b in range(S):
            lg = self.refs[b].feed(np.zeros((0, F)) if rows[b] is None else rows[b], bool(last is not None and last[b]))
            assert got_rows[b] == len(lg), 'slot %d' % b
            np.testing.assert_allclose(logits[:got_rows[b], b], lg, atol=TOL, rtol=0, err_msg='slot %d' % b)
            np.testing.assert_allclose(state[:, b], self.refs[b].state, atol=TOL, rtol=0, err_msg='slot %d' % b)
            self.got[b].append(logits[:got_rows[b], b].copy())
        assert self.e.stream_frames().tolist() == [r.emitted for r in self.refs]
        return got_rows

    def reset(self, slot):
        self.e.stream_reset([slot])
        self.refs[slot].reset()
        self.got[slot] = []

    def close(self):
        self.e.close()


def test_single_stream_feeds_of_1_3_4_5_9():
    """1 layer, H 24, S 1, R 4, 22 frames as feeds of 1, 3, 4, 5 and 9 rows: the first two emit nothing (no pass runs),
    and a final empty `last` feed flushes the 4 held rows"""
    spec = O.ModelSpec(10, 24, 1, True, 'concat', 4)
    s = Session(spec, 3, 1, 4)
    assert np.array_equal(s.e.stream_state(), np.zeros((1, 1, 2, 24), np.float32))
    utt = utterances(spec, [22], 1)[0]
    pos, emitted = 0, []
    for n in (1, 3, 4, 5, 9):
        emitted.append(int(s.feed([utt[pos:pos + n]])[0]))
        pos += n
    emitted.append(int(s.feed([None], [True])[0]))
    assert emitted == [0, 0, 4, 5, 9, 4] and s.e.stream_frames().tolist() == [22]
    s.close()


@pytest.mark.parametrize('T', [1, 5])
def test_an_utterance_shorter_than_the_lookahead_is_the_whole_network(T):
    """an utterance of 1 frame, and one of 5 < R = 8 frames fed as 2 + 3 with `last`: nothing leaves before `last`, and
    then the logits are the whole-utterance oracle's"""
    spec = O.ModelSpec(10, 24, 2, True, 'concat', 4)
    s = Session(spec, 4, 1, 8)
    utt = utterances(spec, [T], 2)[0]
    if T > 1:
        assert s.feed([utt[:2]])[0] == 0
    assert s.feed([utt[2:] if T > 1 else utt], [True])[0] == T
    np.testing.assert_allclose(np.concatenate(s.got[0]), oracle_logits(spec, s.params, utt), atol=TOL, rtol=0)
    s.close()


@pytest.mark.parametrize('R', [1, 9])
def test_three_layers_padded_units_ragged_slots_and_a_reused_slot(R):
    """3 layers, H 70 (Hp 128), S 3 with utterances of 25, 19 and 7 frames, one slot idle in every feed; with R = 9 slots
    0 and 1 hold everything (E = 0) in the feed in which slot 2 finishes; slot 2 is then reset and reused for a second
    utterance of 11 frames while the others continue"""
    spec = O.ModelSpec(13, 70, 3, True, 'concat', 5)
    s = Session(spec, 5, 3, R)
    u = utterances(spec, [25, 19, 7], 3)
    second = utterances(spec, [11], 4)[0]
    rows = s.feed([u[0][:6], None, u[2][:3]])
    assert rows.tolist() == ([5, 0, 2] if R == 1 else [0, 0, 0])
    rows = s.feed([u[0][6:8], u[1][:6], u[2][3:]], [False, False, True])
    assert rows.tolist() == ([2, 5, 5] if R == 1 else [0, 0, 7])
    assert s.e.stream_frames()[2] == 7
    np.testing.assert_allclose(np.concatenate(s.got[2]), np.concatenate([LR.run_session(spec, s.params, u[2], [3, 4], R)[0][k]
                                                                         for k in range(2)]), atol=TOL, rtol=0)
    before = s.e.stream_state()
    s.reset(2)
    after = s.e.stream_state()
    assert not after[:, 2].any() and np.array_equal(np.delete(after, 2, 1), np.delete(before, 2, 1))
    assert s.e.stream_frames()[2] == 0
    s.feed([None, u[1][6:11], second[:6]])
    s.feed([u[0][8:14], u[1][11:12], None])
    s.feed([u[0][14:19], None, second[6:]], [False, False, True])
    s.feed([u[0][19:], u[1][12:], None], [True, True, False])
    assert s.e.stream_frames().tolist() == [25, 19, 11]
    for b, n in enumerate((25, 19, 11)):
        assert sum(len(g) for g in s.got[b]) == n
    s.close()


@pytest.mark.parametrize('S', [17, 33])
def test_m_tiles_and_padded_slots(S):
    """a second and a third M tile of the step kernels, padded slots in the state images: utterances of 1 .. 7 frames in
    feeds of at most 3 rows (Tc = 3), R = 2, then one flush of every slot"""
    spec = O.ModelSpec(12, 20, 1, True, 'concat', 6)
    s = Session(spec, 6, S, 2)
    u = utterances(spec, [1 + (5 * b) % 7 for b in range(S)], 6)
    for t in (0, 3, 6):
        s.feed([x[t:t + 3] if t < len(x) else None for x in u], Tc=3)
    s.feed([None] * S, [True] * S)
    assert s.e.stream_frames().tolist() == [len(x) for x in u]
    s.close()


def test_dense_stages():
    """a DeepSpeech spec with dropout 0: dense stages in front of and behind the two bidirectional layers"""
    spec = O.ModelSpec(14, 24, 2, True, 'concat', 7, pre=(20,), post=12, relu_clip=2.0, dropout=(0.0, 0.0))
    s = Session(spec, 7, 2, 3)
    drop0 = s.e.dropout_state()
    u = utterances(spec, [13, 8], 7)
    s.feed([u[0][:5], u[1][:5]])
    s.feed([u[0][5:10], u[1][5:]], [False, True])
    s.feed([u[0][10:], None], [True, False])
    assert s.e.dropout_state() == drop0                    # a feed is no pass of the dropout counter
    np.testing.assert_allclose(np.concatenate(s.got[1])[:2], LR.run_session(spec, s.params, u[1], [5, 3], 3)[0][0], atol=TOL, rtol=0)
    s.close()


def test_one_last_feed_against_forward():
    """the whole utterance in one `last` feed: nasr_forward's logits of the same utterance (another summation split in the
    bulk GEMMs: 1e-4, not bits), and the oracle's"""
    spec = O.ModelSpec(13, 32, 2, True, 'concat', 5)
    s = Session(spec, 8, 2, 6)
    u = utterances(spec, [23, 40], 8)
    assert s.feed(u, [True, True]).tolist() == [23, 40]
    for b in range(2):
        got = np.concatenate(s.got[b])
        np.testing.assert_allclose(got, s.e.forward(u[b][None], [len(u[b])])[:, 0], atol=TOL, rtol=0)
        np.testing.assert_allclose(got, oracle_logits(spec, s.params, u[b]), atol=TOL, rtol=0)
    s.close()


def session_bits(e, u, R):
    """a fixed sequence of feeds on a fresh session of e: every emitted logit row and the final state, as bytes"""
    e.stream_open_lookahead(2, R)
    F = u[0].shape[1]
    out = []
    for t, last in ((0, None), (5, None), (10, None), (15, [True, True])):
        n = [max(0, min(5, len(x) - t)) if last is None else max(0, len(x) - t) for x in u]
        feats = np.zeros((2, max(n), F), np.float32)
        for b in range(2):
            feats[b, :n[b]] = u[b][t:t + n[b]]
        logits, rows = e.stream_feed_lookahead(feats, n, last)
        out += [logits[:rows[b], b].tobytes() for b in range(2)]
    out.append(e.stream_state().tobytes())
    assert e.stream_frames().tolist() == [len(x) for x in u]
    e.stream_close()
    return b''.join(out)


def test_same_feeds_same_bits_whatever_the_recurrence_mode():
    """two identical sessions give identical bits, on one handle and on two; and the same bits with the handle's batches on
    the persistent kernels (where this device offers them) and on the per-step ones"""
    from neuralasr_amd import _lib
    spec = O.ModelSpec(13, 32, 2, True, 'concat', 5)
    params = O.flatten(rand_params(spec, 11))
    u = utterances(spec, [21, 17], 11)
    e, e2 = make_engine(spec), make_engine(spec)
    e.set_params(params)
    e2.set_params(params)
    runs = {'second handle': session_bits(e2, u, 3)}
    for persistent in (False, True):
        try:
            e.set_recurrence_mode(persistent)
        except _lib.NasrError:
            assert persistent                              # no resident kind on this device: one mode to test
            continue
        mode = e.recurrence_mode
        e.set_params(params)
        runs[mode] = session_bits(e, u, 3)
        runs[mode + ' again'] = session_bits(e, u, 3)
        assert e.recurrence_mode == mode and e.persist_stats() == (0, 0)
    assert len(set(runs.values())) == 1, sorted(runs)
    e.close()
    e2.close()


def test_a_session_leaves_the_handle_alone():
    """parameters and Adam state keep their bits across feeds; nasr_compute_grads on the re-uploaded batch gives the bits
    it gave before; and the handle trains on as a twin that never streamed.  (The gradient buffer itself cannot be read
    behind a feed: every upload, a window's included, makes nasr_get_grads answer "without gradients" until gradients
    are computed again - what a feed could have left in it shows in the recomputed bits and the twin's step.)"""
    spec = O.ModelSpec(13, 32, 2, True, 'concat', 5)
    feats, seq_len, labels, label_len = O.synth_batch(spec, 4, 21, seed=9, var_len=True, Lmin=1, Lmax=4)
    s = Session(spec, 9, 2, 4)
    e, twin = s.e, make_engine(spec)
    twin.set_params(O.flatten(s.params))
    for x in (e, twin):
        x.train_step(feats, seq_len, labels, label_len)      # Adam state that is not zero
        x.upload_batch(feats, seq_len, labels, label_len)
        x.compute_grads()
    s.params = O.unflatten(spec, e.get_params().astype(np.float64))
    for r in s.refs:
        r.params = s.params
    grads, loss = e.get_grads().copy(), e.get_loss()
    assert grads.tobytes() == twin.get_grads().tobytes()
    p0, (m0, v0, step0) = e.get_params(), e.get_adam_state()
    mode, stats = e.recurrence_mode, e.persist_stats()
    u = utterances(spec, [16, 9], 9)
    s.feed([u[0][:8], u[1]], [False, True])
    s.feed([u[0][8:], None], [True, False])
    assert e.get_params().tobytes() == p0.tobytes()
    with pytest.raises(Exception) as err:
        e.get_grads()
    assert 'without gradients' in str(err.value)
    m1, v1, step1 = e.get_adam_state()
    assert m1.tobytes() == m0.tobytes() and v1.tobytes() == v0.tobytes() and step1 == step0
    assert (e.recurrence_mode, e.persist_stats()) == (mode, stats)
    with pytest.raises(Exception) as err:                    # the window replaced the resident batch and is itself none
        e.compute_grads()
    assert 'no resident batch' in str(err.value)
    e.upload_batch(feats, seq_len, labels, label_len)
    e.compute_grads()
    assert e.get_grads().tobytes() == grads.tobytes() and e.get_loss() == loss
    assert e.train_step(feats, seq_len, labels, label_len) == twin.train_step(feats, seq_len, labels, label_len)
    assert e.get_params().tobytes() == twin.get_params().tobytes()
    twin.close()
    s.close()


def test_audio_route_equals_the_frames_route():
    """normalization=causal, utterances of 0.4 s and 0.31 s at 8 kHz in pieces of 333 and of 800 samples: feed_audio's
    rows are stream_audio_rows', and its logits are, bit for bit, those of stream_feed_lookahead on a second handle given
    the Featurizer's rows of the whole utterance in the per-feed row counts of the front end (include/nasr.h at
    nasr_stream_audio_rows: none before norm_min_frames frames are complete, numcontext frames held back until `last`)"""
    import mfcc_ref as MR
    from neuralasr_amd.engine import Engine
    from neuralasr_amd.features import Featurizer
    from test_gpu_mfcc import speech_like
    SR, C, R, NC, M = 8000, 5, 3, 2, 3
    flen, fstep = MR.frame_params(SR)
    audio = [speech_like(3200, SR, 1), speech_like(2500, SR, 2)]

    def front_end_rows(n, finished):
        if finished:
            return MR.num_frames(n, SR)
        fc = 0 if n < flen else 1 + (n - flen) // fstep
        return 0 if fc < M else max(0, fc - NC)
    for piece in (333, 800):
        fz = Featurizer(SR, 13, NC, normalization='causal', norm_min_frames=M)
        rows_all = [np.asarray(x, np.float32) for x in fz.compute(audio)]
        a, b = (Engine(fz.width, 16, 2, True, 'concat', C, learning_rate=1e-3) for _ in range(2))
        flat = (0.2 * np.random.RandomState(3).randn(a.param_count)).astype(np.float32)
        for e in (a, b):
            e.set_params(flat)
            e.stream_open_lookahead(2, R)
        a.stream_attach_audio(fz)
        pos, quiet = [0, 0], 0
        for t in range(0, 3200, piece):
            chunks = [x[t:t + piece] if t < x.size else None for x in audio]
            last = [t < x.size <= t + piece for x in audio]
            want_rows, Te = a.stream_audio_rows([0 if c is None else c.size for c in chunks], last)
            logits, rows = a.stream_feed_audio(chunks, last)
            assert np.array_equal(rows, want_rows) and logits.shape == (Te, 2, C)
            n = [front_end_rows(min(t + piece, x.size), t + piece >= x.size) - pos[s] for s, x in enumerate(audio)]
            feats = np.zeros((2, max(n), fz.width), np.float32)
            for s in range(2):
                feats[s, :n[s]] = rows_all[s][pos[s]:pos[s] + n[s]]
                pos[s] += n[s]
            ref, ref_rows = b.stream_feed_lookahead(feats, n, last)
            assert np.array_equal(ref_rows, rows)
            for s in range(2):
                assert logits[:rows[s], s].tobytes() == ref[:rows[s], s].tobytes(), 'slot %d at %d' % (s, t)
            quiet += int(rows.max() == 0)
        assert pos == [len(x) for x in rows_all] and a.stream_frames().tolist() == pos == b.stream_frames().tolist()
        assert a.stream_state().tobytes() == b.stream_state().tobytes()
        assert quiet >= (1 if piece == 333 else 0)             # the small pieces begin with feeds that emit nothing
        for o in (a, b, fz):
            o.close()


def refused(call, code, *words):
    from neuralasr_amd import _lib
    with pytest.raises(_lib.NasrError) as err:
        call()
    assert err.value.code == code, str(err.value)
    for w in words:
        assert w in str(err.value), str(err.value)


def test_refusals():
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine, LasEngine, WaveNetEngine
    from neuralasr_amd.features import Featurizer
    STATE, ARG = _lib.NASR_ERR_STATE, _lib.NASR_ERR_ARG
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    e = Engine(8, 16, 1, False, 'none', 5)
    refused(lambda: e.stream_open_lookahead(1, 4), STATE, 'nasr_stream_open_lookahead', 'use nasr_stream_open')
    # a plain session refuses the look-ahead calls
    e.stream_open(1)
    refused(lambda: e.stream_feed_lookahead(np.zeros((1, 2, 8), np.float32), [2]), STATE, 'no look-ahead')
    e.close()
    e = Engine(8, 16, 1, True, 'stack_reshape', 5)
    refused(lambda: e.stream_open_lookahead(1, 4), STATE, 'NASR_MERGE_STACK_RESHAPE', 'point in time')
    refused(lambda: e.stream_open(1), STATE, 'nasr_stream_open', 'bidirectional')
    e.close()
    e = Engine(8, 16, 1, True, 'concat', 5, pre=(12,), post=0, relu_clip=2.0, dropout=(0.1,))
    refused(lambda: e.stream_open_lookahead(1, 4), STATE, 'dropout')
    e.close()
    for e in (WaveNetEngine(39, 29), LasEngine(39, 29)):
        refused(lambda: e._ck(e.lib.nasr_stream_open_lookahead(e.h, 1, 4)), STATE, 'nasr_stream_open_lookahead', 'WaveNet or LAS',
                'cannot stream')
        e.close()
    f = Featurizer(16000, 13, 2)
    assert f.lib.nasr_stream_open_lookahead(f.h, 1, 4) == STATE
    msg = f.lib.nasr_last_error(f.h).decode()
    assert 'nasr_stream_open_lookahead' in msg and 'featurizer handle has no model' in msg
    f.close()

    spec = O.ModelSpec(10, 16, 1, True, 'concat', 4)
    e = make_engine(spec)
    e.set_params(O.flatten(rand_params(spec, 1)))
    refused(lambda: e.stream_open(1), STATE, 'nasr_stream_open', 'a bidirectional network cannot stream')     # word for word
    x = np.ones((2, 3, 10), np.float32)
    n33, got, Te = np.array([3, 3], np.int32), np.zeros(2, np.int32), ctypes.c_int(0)
    lg = np.zeros((3, 2, 4), np.float32)

    def raw_feed():     # (Engine's own methods count the slots first: the library's answer without a session needs the bare call)
        e._ck(e.lib.nasr_stream_feed_lookahead(e.h, x.ctypes.data_as(fp), n33.ctypes.data_as(ip), None, 3, got.ctypes.data_as(ip),
                                               ctypes.byref(Te), lg.ctypes.data_as(fp), 3))

    def raw_rows():
        e._ck(e.lib.nasr_stream_lookahead_rows(e.h, n33.ctypes.data_as(ip), None, got.ctypes.data_as(ip), ctypes.byref(Te)))
    refused(raw_feed, STATE, 'no open stream session')
    refused(raw_rows, STATE, 'no open stream session')
    for S, R, word in ((0, 4, '[1,64]'), (65, 4, '[1,64]'), (2, 0, '[1,1024]'), (2, 1025, '[1,1024]')):
        refused(lambda: e.stream_open_lookahead(S, R), ARG, word)
    e.stream_open_lookahead(2, 2)
    refused(lambda: e.stream_open_lookahead(2, 2), STATE, 'open already')
    refused(lambda: e.stream_open(2), STATE, 'bidirectional')
    refused(lambda: e.stream_feed(x, [3, 3]), STATE, 'nasr_stream_feed_lookahead')
    # bad feeds: nothing changes, the resident batch stays what it was
    feats, seq_len, _, _ = O.synth_batch(spec, 3, 7, seed=1, var_len=True, Lmin=1, Lmax=2)
    want = e.forward(feats, seq_len)
    refused(lambda: e.stream_feed_lookahead(x, [-1, 3]), ARG, 'n_frames[0]')
    refused(lambda: e.stream_feed_lookahead(x, [3, 4]), ARG, 'n_frames[1]')
    n, got, Te = np.array([3, 3], np.int32), np.zeros(2, np.int32), ctypes.c_int(0)
    fin = np.array([1, 0], np.uint8)
    small = np.zeros((2, 2, 4), np.float32)
    rc = e.lib.nasr_stream_feed_lookahead(e.h, x.ctypes.data_as(fp), n.ctypes.data_as(ip), fin.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                          3, got.ctypes.data_as(ip), ctypes.byref(Te), small.ctypes.data_as(fp), 2)
    assert rc == ARG and b'logits_out holds 2' in e.lib.nasr_last_error(e.h)
    assert e.stream_frames().tolist() == [0, 0] and e.stream_lookahead_rows([3, 3], [True, False])[0].tolist() == [3, 1]
    assert e.resident_frames() == int(np.sum(seq_len))
    out = np.empty_like(want)
    e._ck(e.lib.nasr_forward_resident(e.h, out.ctypes.data_as(fp)))
    assert out.tobytes() == want.tobytes()
    # a feed in which every slot only holds keeps the resident batch too
    assert e.stream_feed_lookahead(x[:, :2], [2, 1])[1].tolist() == [0, 0]
    e._ck(e.lib.nasr_forward_resident(e.h, out.ctypes.data_as(fp)))
    assert out.tobytes() == want.tobytes()
    # set_state only while no slot holds rows
    state = e.stream_state()
    refused(lambda: e.set_stream_state(state), STATE, 'holds', 'slot 0')
    # after `last` the slot waits for its reset
    assert e.stream_feed_lookahead(x[:, :0], [0, 0], [True, False])[1].tolist() == [2, 0]
    refused(lambda: e.stream_feed_lookahead(x, [1, 0]), STATE, 'slot 0', 'has had `last`')
    refused(lambda: e.stream_feed_lookahead(x[:, :0], [0, 0], [True, False]), STATE, 'slot 0', 'has had `last`')
    refused(lambda: e.stream_lookahead_rows([1, 0]), STATE, 'has had `last`')
    assert e.stream_frames().tolist() == [2, 0]
    e.stream_reset()
    assert e.stream_frames().tolist() == [0, 0] and not e.stream_state().any()
    e.set_stream_state(state)                              # nothing held now
    assert np.array_equal(e.stream_state(), state)
    assert e.stream_feed_lookahead(x, [3, 0])[1].tolist() == [1, 0]
    e.stream_close()
    refused(raw_feed, STATE, 'no open stream session')
    e.close()


def test_recognizer_and_decode_wav_end_to_end(tmp_path, caplog, monkeypatch):
    """StreamingRecognizer on BiLstm3x500CTCNet shrunk to H 24, look-ahead 8: partial hypotheses while the audio arrives,
    finish() flushes the held rows, and the final hypothesis is the host beam search on the session's own concatenated
    logits (exact).  A bidirectional network without the key refuses by naming it.  Then decode_wav --stream
    --lookahead-frames 8 on the frames route and, with normalization=causal, on the samples route."""
    from neuralasr_amd import decode_wav
    from neuralasr_amd.config import Config
    from neuralasr_amd.features import read_wav_native
    from neuralasr_amd.networks.bilstm_ctc_net import BiLstm3x500CTCNet
    from tests.test_gpu_align_network import corpus_config
    monkeypatch.setattr(BiLstm3x500CTCNet, 'num_hidden', 24)
    cfg_path, config = corpus_config(tmp_path, 'bilstm_ctc_net.BiLstm3x500CTCNet')
    assert config.stream_lookahead == 0
    network = config.load_network(fortraining=True)          # fresh variables
    network.save_checkpoint()
    with pytest.raises(ValueError, match='stream_lookahead'):
        network.stream(2)
    audios, rates = zip(*[read_wav_native(str(tmp_path / ('utt%d.wav' % i))) for i in (0, 3)])
    feats = [np.asarray(f, np.float32) for f in network.featurizer().compute(list(audios), rates=list(rates))]
    rec = network.stream(2, lookahead=8)
    real_feed, seen = network.engine.stream_feed_lookahead, []

    def spy(f, n, last=None):
        out = real_feed(f, n, last)
        seen.append(out)
        return out
    network.engine.stream_feed_lookahead = spy
    T = [len(f) for f in feats]
    hyps = [rec.feed([f[t:t + 20] if t < len(f) else None for f in feats]) for t in range(0, max(T), 20)]
    assert len(seen) == len(hyps) >= 3 and all(len(h) == 2 for h in hyps)    # a partial hypothesis per slot after every feed
    assert [rec.hypothesis(b)[0] for b in range(2)] == hyps[-1]
    assert network.engine.stream_frames().tolist() == [t - 8 for t in T]
    for b in range(2):
        got = rec.finish(b)                                   # flushes slot b with an empty `last` feed, then resets it
        lg = np.concatenate([out[:rows[b], b] for out, rows in seen])
        assert lg.shape == (T[b], network.num_classes)
        ids, logp = network.engine.beam_search(lg[:, None, :], [T[b]], network.beam_width, merge_repeated=True)
        assert got[0] == ids[0] and np.float32(got[1]).tobytes() == np.float32(logp[0]).tobytes()
    del network.engine.stream_feed_lookahead
    assert network.engine.stream_frames().tolist() == [0, 0]
    rec.close()
    network.engine.close()
    network.featurizer().close()

    def run(argv):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            text = decode_wav.main(argv)
        lines = [r.getMessage() for r in caplog.records]
        partials = [m[len('Partial: '):] for m in lines if m.startswith('Partial: ')]
        decoded = [m[len('Decoded: '):] for m in lines if m.startswith('Decoded: ')]
        # (finish() flushes the rows held for their look-ahead: the decoded text may go beyond the last partial line)
        assert len(partials) >= 2 and decoded == [text]
    wav =str(tmp_path / 'utt4.wav')
    run([str(cfg_path), wav, '--stream', '--chunk-frames', '16', '--lookahead-frames', '8'])
    # the samples route, the look-ahead from the config key this time overridden by the option
    cfg_path.write_text(cfg_path.read_text().replace('[Train]', 'normalization=causal\nnorm_min_frames=5\nstream_lookahead=3\n[Train]', 1))
    assert Config(str(cfg_path), True).stream_lookahead == 3
    run([str(cfg_path), wav, '--stream', '--chunk-frames', '16', '--lookahead-frames', '8'])
    run([str(cfg_path), wav, '--stream', '--chunk-frames', '16'])

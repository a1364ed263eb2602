"""Streaming recognition on the GPU (nasr_stream_*): utterances fed chunk by chunk through a stream session
against the fp64 oracle ON THE WHOLE UTTERANCES (oracle.nasr_oracle.network_forward) and, for the saved (c, h), the fp64
restatement of tests/stream_ref.py.  Tolerances: logits max-abs 1e-4, the project's own (BASELINE.md §6,
tests/test_gpu_parity.py); the states the same 1e-4 max-abs - the oracle's chain is as long as the stream's, so neither
grows with the number of hand-overs.  Different chunkings are NOT compared bit for bit: the bulk GEMMs split their sums by
the row count.  Shapes are the smallest at which each branch of the state path can go wrong."""
import ctypes
import logging

import numpy as np
import pytest

from oracle import nasr_oracle as O
from tests import stream_ref as R

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


def feed(e, utts, pos, n, Tc=None):
    """one feed: slot b gets frames [pos[b], pos[b] + n[b]) of utts[b] inside a zero-padded [S, Tc, F] chunk; returns the
    real logit rows per slot and advances pos"""
    S, Tc = len(utts), Tc or int(max(n))
    feats = np.zeros((S, Tc, utts[0].shape[1]), np.float32)
    for b in range(S):
        feats[b, :n[b]] = utts[b][pos[b]:pos[b] + n[b]]
        pos[b] += n[b]
    out = e.stream_feed(feats, n)
    assert out.shape == (Tc, S, e.num_classes)
    return [out[:n[b], b].copy() for b in range(S)]


def run_stream(e, utts, chunks, Tc=None):
    """every slot fed in lockstep: chunk k gives each slot its next min(chunks[k], what is left) frames.  Returns the
    concatenated logits per slot."""
    S = len(utts)
    pos, got = [0] * S, [[] for _ in range(S)]
    for c in chunks:
        n = [min(c, len(utts[b]) - pos[b]) for b in range(S)]
        if max(n) == 0:
            break
        for b, lg in enumerate(feed(e, utts, pos, n, Tc)):
            got[b].append(lg)
    assert pos == [len(u) for u in utts]
    return [np.concatenate(g) for g in got]


def check(spec, params, e, utts, got):
    """logits against the oracle on the whole utterances, saved state against the fp64 restatement, frame counts"""
    for b, u in enumerate(utts):
        np.testing.assert_allclose(got[b], oracle_logits(spec, params, u), atol=TOL, rtol=0, err_msg='slot %d' % b)
    state = e.stream_state()
    assert state.shape == (spec.num_layers, len(utts), 2, spec.hidden) and state.dtype == np.float32
    for b, u in enumerate(utts):
        np.testing.assert_allclose(state[:, b], R.state_after(spec, params, u), atol=TOL, rtol=0, err_msg='slot %d' % b)
    assert e.stream_frames().tolist() == [len(u) for u in utts]


def open_stream(spec, seed, S):
    params = rand_params(spec, seed)
    e = make_engine(spec)
    e.set_params(O.flatten(params))
    e.stream_open(S)
    return e, params


def test_single_short_stream():
    """one stream, 12 frames as chunks of 1, 1, 3, 7: the first-step state path on every chunk, a one-frame chunk"""
    spec = O.ModelSpec(10, 16, 1, False, 'none', 4)
    e, params = open_stream(spec, 3, 1)
    assert np.array_equal(e.stream_state(), np.zeros((1, 1, 2, 16), np.float32))
    utts = utterances(spec, [12], 1)
    check(spec, params, e, utts, run_stream(e, utts, [1, 1, 3, 7]))
    e.close()


def test_three_layers_ragged_slots_and_a_reused_slot():
    """S = 4 utterances of 25, 19, 7 and 1 frames in chunks of Tc = 6, every slot with its own n_frames per feed, 0 while
    the others run; slot 2 is finished, reset and reused for a second utterance"""
    spec = O.ModelSpec(13, 32, 3, False, 'none', 5)
    e, params = open_stream(spec, 3, 4)
    utts = utterances(spec, [25, 19, 7, 1], 2)
    second = utterances(spec, [11], 3)[0]
    plan = [[6, 0, 3, 1],      # slot 1 idle while the others run; slot 3's whole utterance
            [2, 6, 4, 0],      # slot 2's utterance ends here
            [0, 5, 0, 0],      # one slot alone
            [6, 1, 0, 0]]
    pos, got = [0] * 4, [[] for _ in range(4)]
    for n in plan:
        for b, lg in enumerate(feed(e, utts, pos, n, Tc=6)):
            got[b].append(lg)
    assert e.stream_frames().tolist() == [14, 12, 7, 1]
    state = e.stream_state()
    np.testing.assert_allclose(state[:, 2], R.state_after(spec, params, utts[2]), atol=TOL, rtol=0)
    np.testing.assert_allclose(state[:, 0], R.state_after(spec, params, utts[0][:14]), atol=TOL, rtol=0)
    e.stream_reset([2])                                   # a new utterance starts in slot 2, the others go on
    assert e.stream_frames().tolist() == [14, 12, 0, 1]
    after = e.stream_state()
    assert not after[:, 2].any() and np.array_equal(np.delete(after, 2, 1), np.delete(state, 2, 1))
    utts2 = [utts[0], utts[1], second, utts[3]]
    pos[2], got2 = 0, []
    for n in ([5, 6, 6, 0], [6, 1, 5, 0]):
        lgs = feed(e, utts2, pos, n, Tc=6)
        for b in (0, 1):
            got[b].append(lgs[b])
        got2.append(lgs[2])
    assert pos == [25, 19, 11, 1]
    np.testing.assert_allclose(np.concatenate(got2), oracle_logits(spec, params, second), atol=TOL, rtol=0)
    np.testing.assert_allclose(np.concatenate(got[2]), oracle_logits(spec, params, utts[2]), atol=TOL, rtol=0)
    check(spec, params, e, utts2, [np.concatenate(got[0]), np.concatenate(got[1]), np.concatenate(got2), np.concatenate(got[3])])
    e.stream_reset()
    assert not e.stream_state().any() and e.stream_frames().tolist() == [0, 0, 0, 0]
    e.close()


def test_long_chain():
    """133 frames in chunks of 10: 14 hand-overs of the state"""
    spec = O.ModelSpec(11, 24, 2, False, 'none', 6)
    e, params = open_stream(spec, 3, 1)
    utts = utterances(spec, [133], 4)
    check(spec, params, e, utts, run_stream(e, utts, [10] * 14))
    e.close()


@pytest.mark.parametrize('H,L', [(70, 1), (500, 1), (530, 1), (1000, 2)], ids=['H70', 'H500-NQ8', 'H530-generic', 'H1000x2'])
def test_padded_hidden_sizes(H, L):
    """9 frames in chunks of 4, 4, 1 at hidden sizes below their padded Hp (128, 512, 576, 1024): padded units of the
    state image, the NQ = 8 and the generic instantiation of the step kernel, two layers"""
    spec = O.ModelSpec(12, H, L, False, 'none', 6)
    e, params = open_stream(spec, 5, 3)
    utts = utterances(spec, [9, 6, 9], 5)
    check(spec, params, e, utts, run_stream(e, utts, [4, 4, 1]))
    e.close()


@pytest.mark.parametrize('S', [17, 33, 64])
def test_m_tiles(S):
    """two, three and four M tiles of the step kernel, padded slots in the state image (17, 33), Tc = 3"""
    spec = O.ModelSpec(12, 20, 1, False, 'none', 6)
    e, params = open_stream(spec, 6, S)
    utts = utterances(spec, [1 + (5 * b) % 7 for b in range(S)], 6)
    check(spec, params, e, utts, run_stream(e, utts, [3, 3, 3], Tc=3))
    e.close()


def test_dense_stages():
    spec = O.ModelSpec(14, 24, 2, False, 'none', 7, pre=(20,), post=12, relu_clip=2.0)
    e, params = open_stream(spec, 7, 2)
    drop0 = e.dropout_state()
    utts = utterances(spec, [13, 8], 7)
    check(spec, params, e, utts, run_stream(e, utts, [5, 5, 3]))
    assert e.dropout_state() == drop0                      # a feed is no pass of the dropout counter
    e.close()


def test_state_round_trip_and_determinism():
    """get_state after two chunks is the fp64 state; set into a second handle, the remaining chunks give the first
    handle's logits bit for bit; the same feeds on a fresh session give identical bits"""
    spec = O.ModelSpec(13, 32, 3, False, 'none', 5)
    utts = utterances(spec, [23, 17], 8)
    e1, params = open_stream(spec, 8, 2)
    head = run_stream(e1, [u[:10] for u in utts], [4, 6])
    state = e1.stream_state()
    for b in range(2):
        np.testing.assert_allclose(state[:, b], R.state_after(spec, params, utts[b][:10]), atol=TOL, rtol=0)
    tail1 = run_stream(e1, [u[10:] for u in utts], [5, 5, 5])
    e2, _ = open_stream(spec, 8, 2)
    e2.set_stream_state(state)
    assert np.array_equal(e2.stream_state(), state)
    tail2 = run_stream(e2, [u[10:] for u in utts], [5, 5, 5])
    for a, b in zip(tail1, tail2):
        assert a.tobytes() == b.tobytes()
    assert e1.stream_state().tobytes() == e2.stream_state().tobytes()
    # the same sequence of feeds on a fresh session of the second handle, from the start
    e2.stream_close()
    e2.stream_open(2)
    again = [np.concatenate(p) for p in zip(run_stream(e2, [u[:10] for u in utts], [4, 6]),
                                            run_stream(e2, [u[10:] for u in utts], [5, 5, 5]))]
    for b in range(2):
        assert again[b].tobytes() == np.concatenate([head[b], tail1[b]]).tobytes()
    assert e2.stream_state().tobytes() == e1.stream_state().tobytes()
    with pytest.raises(Exception) as err:
        e2.set_stream_state(state[:, :1])
    assert 'floats' in str(err.value)
    e1.close()
    e2.close()


def test_a_session_leaves_the_handle_alone():
    """after feeds, forward and loss_and_grads of a batch return the bits of a handle that never streamed; the recurrence
    mode and the abort counters are what they were; a training step between two feeds is allowed, and the stream goes on
    with the new parameters from the state it had"""
    spec = O.ModelSpec(13, 32, 3, False, 'none', 5)
    feats, seq_len, labels, label_len = O.synth_batch(spec, 4, 21, seed=9, var_len=True, Lmin=1, Lmax=4)
    utts = utterances(spec, [16, 9], 9)
    e, params = open_stream(spec, 9, 2)
    ref = make_engine(spec)
    ref.set_params(O.flatten(params))
    mode, stats = e.recurrence_mode, e.persist_stats()
    assert (mode, stats) == (ref.recurrence_mode, ref.persist_stats())
    want_fwd, want_lg = ref.forward(feats, seq_len), ref.loss_and_grads(feats, seq_len, labels, label_len)
    pos = [0, 0]
    first = feed(e, utts, pos, [8, 9])
    got_fwd, got_lg = e.forward(feats, seq_len), e.loss_and_grads(feats, seq_len, labels, label_len)
    assert got_fwd.tobytes() == want_fwd.tobytes()
    assert got_lg[0] == want_lg[0] and got_lg[1].tobytes() == want_lg[1].tobytes() and got_lg[2].tobytes() == want_lg[2].tobytes()
    assert (e.recurrence_mode, e.persist_stats()) == (mode, stats)
    for b in range(2):
        np.testing.assert_allclose(first[b], oracle_logits(spec, params, utts[b])[:len(first[b])], atol=TOL, rtol=0)
    state = e.stream_state()
    for b, k in enumerate((8, 9)):
        np.testing.assert_allclose(state[:, b], R.state_after(spec, params, utts[b][:k]), atol=TOL, rtol=0)
    # a training step between two feeds: the state is carried, the parameters are the new ones
    assert e.train_step(feats, seq_len, labels, label_len) == ref.train_step(feats, seq_len, labels, label_len)
    assert e.stream_state().tobytes() == state.tobytes()
    new = O.unflatten(spec, e.get_params().astype(np.float64))
    assert e.get_params().tobytes() == ref.get_params().tobytes() and np.abs(O.flatten(new) - O.flatten(params)).max() > 1e-4
    rest = feed(e, utts, pos, [8, 0])[0]
    want_rest, want_state = R.run_chunk(spec, new, utts[0][8:], state[:, 0])
    np.testing.assert_allclose(rest, want_rest, atol=TOL, rtol=0)
    np.testing.assert_allclose(e.stream_state()[:, 0], want_state, atol=TOL, rtol=0)
    assert (e.recurrence_mode, e.persist_stats()) == (mode, stats) and e.stream_frames().tolist() == [16, 9]
    # the chunk replaced the resident batch and is itself none
    with pytest.raises(Exception) as err:
        e.compute_grads()
    assert 'no resident batch' in str(err.value)
    # ... and the handle goes on training as the one that never streamed
    assert e.train_step(feats, seq_len, labels, label_len) == ref.train_step(feats, seq_len, labels, label_len)
    assert e.get_params().tobytes() == ref.get_params().tobytes()
    e.stream_close()
    e.close()
    ref.close()


def test_feeds_do_not_depend_on_the_recurrence_mode():
    """A feed runs the per-step kernels whatever kind runs the handle's batches: with the persistent kind in use (where
    this device offers it) and with the per-step kernels the same feeds give the same bits, also after the parameters
    changed between two feeds (the session then rebuilds the per-step operand images itself)."""
    from neuralasr_amd import _lib
    spec = O.ModelSpec(13, 32, 2, False, 'none', 5)
    pa, pb = rand_params(spec, 11), rand_params(spec, 12)
    utts = utterances(spec, [14, 9], 11)
    e = make_engine(spec)
    runs = {}
    for persistent in (False, True):
        try:
            e.set_recurrence_mode(persistent)
        except _lib.NasrError:
            assert persistent                              # no resident kind on this device: one mode to test
            continue
        mode = e.recurrence_mode
        assert (mode == 'per-step') == (not persistent)
        e.set_params(O.flatten(pa))
        e.stream_open(2)
        pos = [0, 0]
        first = feed(e, utts, pos, [6, 6])
        state = e.stream_state()
        e.set_params(O.flatten(pb))                        # new parameters, the state carried
        rest = feed(e, utts, pos, [8, 3])
        for b in range(2):
            np.testing.assert_allclose(first[b], oracle_logits(spec, pa, utts[b])[:6], atol=TOL, rtol=0)
            want, want_state = R.run_chunk(spec, pb, utts[b][6:], state[:, b])
            np.testing.assert_allclose(rest[b], want, atol=TOL, rtol=0)
            np.testing.assert_allclose(e.stream_state()[:, b], want_state, atol=TOL, rtol=0)
        assert e.recurrence_mode == mode and e.persist_stats() == (0, 0)
        runs[mode] = np.concatenate(first + rest).tobytes() + e.stream_state().tobytes()
        e.stream_close()
    assert len(set(runs.values())) == 1, sorted(runs)
    e.close()


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
    for e in (Engine(8, 16, 1, True, 'stack_reshape', 5), Engine(8, 16, 2, True, 'concat', 5)):
        refused(lambda: e.stream_open(1), STATE, 'nasr_stream_open', 'bidirectional')
        e.close()
    e = Engine(8, 16, 1, False, 'none', 5, pre=(12,), post=0, relu_clip=2.0, dropout=(0.1,))
    refused(lambda: e.stream_open(1), STATE, 'nasr_stream_open', 'dropout')
    e.close()
    for e, word in ((WaveNetEngine(39, 29), 'WaveNet or LAS'), (LasEngine(39, 29), 'WaveNet or LAS')):
        refused(lambda: e.stream_open(1), STATE, 'nasr_stream_open', word, 'cannot stream')
        e.close()
    f = Featurizer(16000, 13, 2)
    assert f.lib.nasr_stream_open(f.h, 1) == STATE
    msg = f.lib.nasr_last_error(f.h).decode()
    assert 'nasr_stream_open' in msg and 'featurizer handle has no model' in msg
    f.close()

    spec = O.ModelSpec(10, 16, 1, False, 'none', 4)
    e = make_engine(spec)
    e.set_params(O.flatten(rand_params(spec, 1)))
    x = np.zeros((2, 3, 10), np.float32)
    for call in (lambda: e.stream_feed(x, [3, 3]), lambda: e.stream_reset(), lambda: e.stream_close(),
                 lambda: e._ck(e.lib.nasr_stream_get_state(e.h, None, 0)), lambda: e._ck(e.lib.nasr_stream_set_state(e.h, None, 0)),
                 lambda: e._ck(e.lib.nasr_stream_frames(e.h, None))):
        refused(call, STATE, 'no open stream session')
    refused(lambda: e.stream_open(0), ARG, '[1,64]')
    refused(lambda: e.stream_open(65), ARG, '[1,64]')
    e.stream_open(2)
    refused(lambda: e.stream_open(2), STATE, 'open already')
    # bad chunks: NASR_ERR_ARG, and the resident batch stays what it was
    feats, seq_len, _, _ = O.synth_batch(spec, 3, 7, seed=1, var_len=True, Lmin=1, Lmax=2)
    want = e.forward(feats, seq_len)
    assert e.resident_frames() == int(np.sum(seq_len))
    refused(lambda: e.stream_feed(x, [-1, 3]), ARG, 'n_frames[0]')
    refused(lambda: e.stream_feed(x, [3, 4]), ARG, 'n_frames[1]')
    refused(lambda: e._ck(e.lib.nasr_stream_feed(e.h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                 np.zeros(2, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 0,
                                                 x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))), ARG, 'Tc >= 1')
    refused(lambda: e.stream_reset([2]), ARG, 'slot 2')
    refused(lambda: e.stream_reset([-1]), ARG, 'slot -1')
    assert e.resident_frames() == int(np.sum(seq_len)) and e.stream_frames().tolist() == [0, 0]
    out = np.empty_like(want)
    e._ck(e.lib.nasr_forward_resident(e.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    assert out.tobytes() == want.tobytes()
    assert not e.stream_state().any()
    e.stream_feed(x, [0, 0])                               # every slot idle: allowed, nothing moves
    assert not e.stream_state().any() and e.stream_frames().tolist() == [0, 0]
    e.stream_close()
    refused(lambda: e.stream_feed(x, [3, 3]), STATE, 'no open stream session')
    e.close()


def test_recognizer_and_decode_wav_end_to_end(tmp_path, caplog):
    """A StreamingRecognizer on the LstmCTCNet of a small synthetic corpus: its final hypothesis is the whole-utterance
    beam search on the logits the stream itself produced (exact), its logits are Engine.forward's of the whole utterance
    within 1e-4 (the hypothesis is NOT compared with the offline one: the logits differ in the last bits).  Then
    decode_wav --stream on one of the files: Partial lines, and the final text is the last of them."""
    from neuralasr_amd import decode_wav
    from neuralasr_amd.features import read_wav_native
    from tests.test_gpu_align_network import corpus_config
    cfg_path, config = corpus_config(tmp_path, 'lstm_ctc_net.LstmCTCNet')
    network = config.load_network(fortraining=True)          # fresh variables
    network.save_checkpoint()
    audios, rates = zip(*[read_wav_native(str(tmp_path / ('utt%d.wav' % i))) for i in (0, 3)])
    feats = [np.asarray(f, np.float32) for f in network.featurizer().compute(list(audios), rates=list(rates))]
    rec = network.stream(2)
    real_feed, seen = network.engine.stream_feed, []

    def spy(f, n):
        out = real_feed(f, n)
        seen.append((out, np.asarray(n).copy()))
        return out
    network.engine.stream_feed = spy
    T = [len(f) for f in feats]
    for t in range(0, max(T), 20):
        rec.feed([f[t:t + 20] if t < len(f) else None for f in feats])
    del network.engine.stream_feed
    assert network.engine.stream_frames().tolist() == T
    for b in range(2):
        lg = np.concatenate([out[:n[b], b] for out, n in seen])
        assert lg.shape == (T[b], network.num_classes)
        whole = network.engine.forward(feats[b][None], [T[b]])[:, 0]
        np.testing.assert_allclose(lg, whole, atol=TOL, rtol=0)
        ids, logp = network.engine.beam_search(lg[:, None, :], [T[b]], network.beam_width, merge_repeated=True)
        got = rec.finish(b)
        assert got[0] == ids[0] and np.float32(got[1]).tobytes() == np.float32(logp[0]).tobytes()
    assert network.engine.stream_frames().tolist() == [0, 0]
    rec.close()
    network.engine.close()
    network.featurizer().close()

    with caplog.at_level(logging.INFO):
        text = decode_wav.main([str(cfg_path), str(tmp_path / 'utt4.wav'), '--stream', '--chunk-frames', '16'])
    lines = [r.getMessage() for r in caplog.records]
    partials = [m[len('Partial: '):] for m in lines if m.startswith('Partial: ')]
    decoded = [m[len('Decoded: '):] for m in lines if m.startswith('Decoded: ')]
    assert partials and decoded == [partials[-1]] and text == partials[-1]

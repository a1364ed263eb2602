"""The host side of streaming recognition without a GPU: StreamingRecognizer over a fake engine that
returns scripted logits (padding, idle slots, one beam per slot, finish resets one slot only), decode_wav's --stream
arguments and log lines, and the float64 restatement the GPU tests take their states from (tests/stream_ref.py) against
the oracle."""
import logging

import numpy as np
import pytest

from neuralasr_amd import decode_wav
from neuralasr_amd.stream import StreamingRecognizer
from oracle import nasr_oracle as O
from tests import stream_ref as R
from tests.test_beam_lm import lib_beam_lm

F, C = 5, 6


class FakeEngine:
    """stream_feed hands out the next n_frames[b] rows of slot b's script and NaN everywhere else"""

    def __init__(self, scripts):
        self.scripts = [np.asarray(s, np.float32) for s in scripts]
        self.pos = [0] * len(scripts)
        self.opened, self.closed, self.feeds, self.resets = None, 0, [], []

    def stream_open(self, slots):
        assert self.opened is None
        self.opened = slots

    def stream_close(self):
        self.closed += 1

    def stream_reset(self, slots=None):
        self.resets.append(None if slots is None else list(slots))
        for b in (range(len(self.pos)) if slots is None else slots):
            self.pos[b] = 0

    def stream_feed(self, feats, n_frames):
        feats, n = np.asarray(feats), np.asarray(n_frames)
        self.feeds.append((feats.copy(), n.copy()))
        S, Tc, _ = feats.shape
        assert S == self.opened and n.shape == (S,) and Tc == n.max() and Tc >= 1
        out = np.full((Tc, S, C), np.nan, np.float32)
        for b in range(S):
            out[:n[b], b] = self.scripts[b][self.pos[b]:self.pos[b] + n[b]]
            self.pos[b] += int(n[b])
        return out


class FakeSymbols:
    def convert_to_str(self, ids):
        return ''.join('abcde'[i] for i in ids)


class FakeConfig:
    feature_size, lm_weight, lm_bonus, symbols = F, 0.0, 0.0, FakeSymbols()


class FakeNetwork:
    num_classes, beam_width, decoder, config = C, 8, 'beam', FakeConfig()

    def __init__(self, scripts):
        self.engine = FakeEngine(scripts)
        self.settled = 0

    def _settle(self):
        self.settled += 1

    def language_model(self):
        return None

    def stream(self, slots=1):
        return StreamingRecognizer(self, slots)


def script(T, seed):
    x = np.random.RandomState(seed).randn(T, C) * 3
    x[:, C - 1] -= 1.0                      # little blank: hypotheses of several ids
    return x.astype(np.float32)


def whole(logits, width=8):
    got, lp, _, _ = lib_beam_lm(logits[:, None, :], [len(logits)], width, True, None, None, 1, 0, 0.0, 0.0)
    return got[0], float(lp[0])


def test_padding_idle_slots_independent_beams_and_finish():
    scripts = [script(9, 1), np.concatenate([script(4, 2), script(6, 3)]), script(5, 4)]
    net = FakeNetwork(scripts)
    rec = net.stream(3)
    assert net.settled == 1 and net.engine.opened == 3
    rs = np.random.RandomState(0)
    x = [rs.randn(len(s), F).astype(np.float32) for s in scripts]

    h = rec.feed([x[0][:4], x[1][:1], None])                       # ragged: padded to 4 frames, slot 2 idle
    feats, n = net.engine.feeds[-1]
    assert feats.shape == (3, 4, F) and n.tolist() == [4, 1, 0]
    assert np.array_equal(feats[0], x[0][:4]) and np.array_equal(feats[1, :1], x[1][:1])
    assert not feats[1, 1:].any() and not feats[2].any()
    assert h[0] == whole(scripts[0][:4])[0] and h[1] == whole(scripts[1][:1])[0] and h[2] == []

    assert rec.feed([None, None, None]) == h and len(net.engine.feeds) == 1       # nothing to run
    h = rec.feed([None, x[1][1:4], x[2][:5]])                      # slot 0 idle: its hypothesis stays
    assert net.engine.feeds[-1][1].tolist() == [0, 3, 5]
    assert h[0] == whole(scripts[0][:4])[0] and h[1] == whole(scripts[1][:4])[0] and h[2] == whole(scripts[2])[0]

    ids, logp = rec.finish(1)                                      # the first utterance of slot 1 is over
    assert (ids, np.float32(logp)) == (whole(scripts[1][:4])[0], np.float32(whole(scripts[1][:4])[1]))
    assert net.engine.resets == [[1]]                              # ... and only that slot starts anew
    assert rec.hypothesis(1) == ([], 0.0) and rec.hypothesis(0)[0] == h[0] and rec.hypothesis(2)[0] == h[2]
    net.engine.pos[1] = 4                                          # (the script's second utterance starts here)
    h = rec.feed([x[0][4:9], x[1][4:10], None])
    assert h[0] == whole(scripts[0])[0] and h[1] == whole(scripts[1][4:])[0]
    assert rec.finish(0)[0] == whole(scripts[0])[0] and net.engine.resets == [[1], [0]]

    with pytest.raises(ValueError):
        rec.feed([None, None])                                     # one entry per slot
    with pytest.raises(ValueError):
        rec.feed([np.zeros((2, F + 1), np.float32), None, None])   # the configured feature width
    rec.close()
    rec.close()
    assert net.engine.closed == 1


def test_greedy_decoder_streams_with_a_beam_of_one():
    net = FakeNetwork([script(7, 5)])
    net.decoder = 'greedy'
    rec = net.stream(1)
    rec.feed([np.zeros((7, F), np.float32)])
    assert rec.finish(0)[0] == whole(net.engine.scripts[0], width=1)[0]


def test_decode_wav_stream_arguments():
    a = decode_wav.parse_args(['cfg', 'x.wav'])
    assert (a.config, a.input, a.stream, a.chunk_frames) == ('cfg', 'x.wav', False, 50)
    a = decode_wav.parse_args(['cfg', 'x.wav', '--stream'])
    assert a.stream and a.chunk_frames == 50
    a = decode_wav.parse_args(['cfg', 'x.wav', '--stream', '--chunk-frames', '7'])
    assert a.stream and a.chunk_frames == 7
    for bad in (['cfg', 'x.wav', '--chunk-frames', '0'], ['cfg', 'x.wav', '--chunk-frames', 'many'], ['cfg']):
        with pytest.raises(SystemExit):
            decode_wav.parse_args(bad)


def test_decode_stream_logs_partials_then_the_decoded_line(caplog):
    s = script(23, 6)
    net = FakeNetwork([s])
    feats = np.zeros((23, F), np.float32)
    with caplog.at_level(logging.INFO):
        text = decode_wav.decode_stream(net.config, net, feats, 5)
    assert [n.tolist() for _, n in net.engine.feeds] == [[5]] * 4 + [[3]]
    lines = [r.getMessage() for r in caplog.records]
    partials = [m[len('Partial: '):] for m in lines if m.startswith('Partial: ')]
    # one line per chunk whose hypothesis changed
    want, last = [], None
    for t in range(5, 28, 5):
        ids = whole(s[:min(t, 23)])[0]
        if ids != last:
            want.append(FakeSymbols().convert_to_str(ids))
            last = ids
    assert partials == want and len(partials) >= 2
    assert lines[-1] == 'Decoded: ' + partials[-1] and text == partials[-1]
    assert net.engine.resets == [[0]] and net.engine.closed == 1
    with pytest.raises(ValueError):
        decode_wav.decode_stream(net.config, FakeNetwork([s]), feats, 0)


SPECS = [O.ModelSpec(13, 32, 3, False, 'none', 5),
         O.ModelSpec(9, 16, 2, False, 'none', 6, pre=(20,), post=12, relu_clip=2.0)]


@pytest.mark.parametrize('spec', SPECS, ids=['plain', 'dense'])
def test_the_restatement_in_chunks_is_the_oracle_on_the_whole_utterance(spec):
    rs = np.random.RandomState(2)
    params = [p + 0.05 * rs.randn(*p.shape) for p in O.init_params(spec, seed=3)]
    x = rs.randn(17, spec.feature_size)
    want = O.network_forward(spec, params, x[None], [17])[0][:, 0]
    state, got = R.zero_state(spec), []
    for a, b in ((0, 1), (1, 1), (1, 8), (8, 16), (16, 17)):          # (an empty chunk among them)
        lg, state = R.run_chunk(spec, params, x[a:b], state)
        got.append(lg)
    np.testing.assert_allclose(np.concatenate(got), want, atol=1e-12)
    np.testing.assert_allclose(state, R.state_after(spec, params, x), atol=1e-12)
    assert state.shape == (spec.num_layers, 2, spec.hidden)

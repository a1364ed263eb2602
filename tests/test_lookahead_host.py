"""tests/lookahead_ref.py (the fp64 restatement of a look-ahead session) against the oracle and against the
rule's own arithmetic.  CPU only."""
import numpy as np
import pytest

from oracle import nasr_oracle as O
from tests import lookahead_ref as LR

PLAIN = O.ModelSpec(7, 6, 2, True, 'concat', 5)
DENSE = O.ModelSpec(7, 6, 1, True, 'concat', 5, pre=(9, 8), post=10, relu_clip=20.0, dropout=(0.0, 0.0, 0.0))


def rand_params(spec, seed):
    rs = np.random.RandomState(seed)
    return [p + 0.05 * rs.randn(*p.shape) for p in O.init_params(spec, seed=seed)]


def utterance(spec, n, seed):
    return np.random.RandomState(seed).randn(n, spec.feature_size)


def oracle_logits(spec, params, utt):
    return O.network_forward(spec, params, utt[None], [len(utt)])[0][:, 0]


@pytest.mark.parametrize('spec', [PLAIN, DENSE], ids=['plain', 'dense'])
def test_one_window_over_the_utterance_is_the_whole_network(spec):
    params, utt = rand_params(spec, 3), utterance(spec, 13, 1)
    for R in (1, 4, 50):
        logits, states = LR.run_session(spec, params, utt, [len(utt)], R)
        assert len(logits) == 1 and logits[0].shape == (13, spec.num_classes)
        np.testing.assert_allclose(logits[0], oracle_logits(spec, params, utt), atol=1e-10, rtol=0)


@pytest.mark.parametrize('feeds', [[13], [1, 5, 7], [4, 0, 4, 5, 0]])
def test_a_lookahead_as_long_as_the_utterance_emits_only_at_last(feeds):
    spec, params, utt = PLAIN, rand_params(PLAIN, 4), utterance(PLAIN, 13, 2)
    for R in (13, 20):
        logits, states = LR.run_session(spec, params, utt, feeds, R)
        assert [len(lg) for lg in logits[:-1]] == [0] * (len(feeds) - 1)
        for st in states[:-1]:
            assert not st.any()
        np.testing.assert_allclose(logits[-1], oracle_logits(spec, params, utt), atol=1e-10, rtol=0)


def test_the_forward_state_of_layer_0_does_not_depend_on_the_feeds():
    """layer 0's forward direction reads the features (behind the row-wise dense stages) alone; the layers above read
    the backward direction too, whose context the feeds decide"""
    for spec in (PLAIN, DENSE):
        params, utt = rand_params(spec, 5), utterance(spec, 17, 3)
        ref = LR.run_session(spec, params, utt, [17], 3)[1][-1]
        for feeds, R in (([5, 5, 7], 3), ([1] * 17, 2), ([9, 0, 8], 6), ([2, 15], 1)):
            st = LR.run_session(spec, params, utt, feeds, R)[1][-1]
            np.testing.assert_allclose(st[0], ref[0], atol=1e-12, rtol=0)
    # ... and the split does change what the layers above see
    a = np.concatenate(LR.run_session(PLAIN, rand_params(PLAIN, 5), utterance(PLAIN, 17, 3), [5, 5, 7], 3)[0])
    b = np.concatenate(LR.run_session(PLAIN, rand_params(PLAIN, 5), utterance(PLAIN, 17, 3), [17], 3)[0])
    assert a.shape == b.shape and np.abs(a - b).max() > 1e-6


def test_a_partial_state_is_the_state_after_the_last_emitted_row():
    """after a feed, layer 0's saved state is that of a plain forward run over the rows emitted so far"""
    spec, params, utt = PLAIN, rand_params(PLAIN, 6), utterance(PLAIN, 12, 4)
    logits, states = LR.run_session(spec, params, utt, [6, 6], 4, last=False)
    assert [len(lg) for lg in logits] == [2, 6]
    whole = LR.run_session(spec, params, utt[:8], [8], 1)[1][-1]
    np.testing.assert_allclose(states[-1][0], whole[0], atol=1e-12, rtol=0)


def test_emitted_row_counts():
    """E = P with last, else max(0, P - R); P - E rows stay held: n < R, n = 0, and an empty utterance"""
    assert LR.emitted(0, 3, 4, False) == (0, 3)
    assert LR.emitted(3, 3, 4, False) == (2, 4)
    assert LR.emitted(4, 0, 4, False) == (0, 4)
    assert LR.emitted(4, 1, 4, False) == (1, 4)
    assert LR.emitted(4, 9, 4, False) == (9, 4)
    assert LR.emitted(4, 0, 4, True) == (4, 0)
    assert LR.emitted(0, 0, 4, True) == (0, 0)
    assert LR.emitted(2, 5, 4, True) == (7, 0)
    spec, params = PLAIN, rand_params(PLAIN, 7)
    logits, _ = LR.run_session(spec, params, utterance(spec, 22, 5), [1, 3, 4, 5, 9, 0], 4)
    assert [len(lg) for lg in logits] == [0, 0, 4, 5, 9, 4]
    logits, _ = LR.run_session(spec, params, utterance(spec, 22, 5), [3, 0, 2, 0], 4, last=False)
    assert [len(lg) for lg in logits] == [0, 0, 1, 0]
    logits, states = LR.run_session(spec, params, np.zeros((0, spec.feature_size)), [0], 4)
    assert [len(lg) for lg in logits] == [0] and not states[0].any()


# ------------------------------------------------------------------------------------------- config key, command line
def _config(tmp_path, extra=''):
    from neuralasr_amd.config import Config
    p = tmp_path / 'c.config'
    p.write_text('[Parameters]\nsamplerate=8000\nnumcep=13\nnumcontext=2\nlabel_context=0\nbatch_size=2\nepochs=1\n'
                 'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
                 'network=networks.bilstm_ctc_net.BiLstm3x500CTCNet\n%s[Train]\n[Test]\ninput=%s\n[MFCC Featurizer]\n'
                 % (tmp_path / 'model', extra, tmp_path / 'test.scp'))
    return Config(str(p))


def test_config_key(tmp_path, caplog):
    import logging
    from neuralasr_amd.config import log
    assert _config(tmp_path).stream_lookahead == 0
    c = _config(tmp_path, 'stream_lookahead=20\n')
    assert c.stream_lookahead == 20
    with caplog.at_level(logging.INFO, logger=log.name):
        c.print_config()
    assert 'stream_lookahead=20' in caplog.text
    for bad in ('-1', '1025', 'some'):
        with pytest.raises(ValueError, match='stream_lookahead'):
            _config(tmp_path, 'stream_lookahead=%s\n' % bad)


def test_decode_wav_options():
    from neuralasr_amd import decode_wav
    a = decode_wav.parse_args(['c', 'w', '--stream', '--lookahead-frames', '8'])
    assert a.stream and a.lookahead_frames == 8 and a.chunk_frames == 50
    assert decode_wav.parse_args(['c', 'w', '--stream']).lookahead_frames is None
    with pytest.raises(SystemExit):
        decode_wav.parse_args(['c', 'w', '--stream', '--lookahead-frames', '0'])


def test_a_bidirectional_network_names_the_key_it_needs():
    """HipNetwork.stream() without a look-ahead on a bidirectional network: the message names stream_lookahead (no engine
    call is made before it)"""
    from types import SimpleNamespace
    from neuralasr_amd.networks.hipnetwork import HipNetwork
    net = SimpleNamespace(engine=SimpleNamespace(cfg=SimpleNamespace(bidirectional=1)), config=SimpleNamespace(stream_lookahead=0))
    with pytest.raises(ValueError, match='stream_lookahead'):
        HipNetwork.stream(net, 1)
    with pytest.raises(ValueError, match='stream_lookahead'):
        HipNetwork.stream(net, 1, lookahead=0)

"""GPU: forced alignment through the handles and networks: align = align_logits on the handle's own logits,
from audio = from host-made features, an alignment between upload and compute_grads changes nothing of the step, a LAS
handle refuses, and `python -m neuralasr_amd.align` on a synthesised WAV, transcript and fresh checkpoint."""
import ctypes
import logging
import os

import numpy as np
import pytest

import ctc_align_ref as R
from test_gpu_audio_batch import host_feats, init, same
from test_gpu_mfcc import speech_like

pytestmark = pytest.mark.gpu

C, F_IN, H = 7, 13, 16
SCORE_RTOL, SCORE_ATOL = 3e-5, 1e-5
KINDS = ['bilstm-stack_reshape', 'bilstm-concat', 'lstm', 'wavenet']


def make_engine(kind, F=F_IN):
    from neuralasr_amd.engine import Engine, WaveNetEngine
    if kind == 'wavenet':
        return init(WaveNetEngine(F, C, num_blocks=1, rates=(1, 2), learning_rate=1e-3), seed=4)
    if kind == 'lstm':
        return init(Engine(F, H, 1, False, 'none', C, learning_rate=1e-3))
    return init(Engine(F, H, 1, True, kind.split('-')[1], C, learning_rate=1e-3))


def small_batch(seed=0, B=3, T=40):
    rs = np.random.RandomState(seed)
    seq = [T, T - 11, 9][:B]
    feats = rs.randn(B, T, F_IN).astype(np.float32)
    for b, n in enumerate(seq):
        feats[b, n:] = 0
    label_len = [6, 4, 3][:B]
    labels = rs.randint(1, C - 1, size=(B, 6)).astype(np.int32)
    labels[0, 2] = labels[0, 1]                                   # a repeat
    return feats, seq, labels, label_len


@pytest.mark.parametrize('kind', KINDS)
def test_align_is_align_logits_on_the_handles_own_logits(kind):
    e = make_engine(kind)
    feats, seq, labels, ll = small_batch()
    B, T = feats.shape[:2]
    path, score = e.align(feats, seq, labels, ll)
    Tp = e.logit_frames(T)
    assert Tp == (2 * T if kind == 'bilstm-stack_reshape' else T) and path.shape == (B, Tp)
    logits = e.forward_resident(B, T)
    p2, s2 = e.align_logits(logits, seq, labels, ll)
    assert np.array_equal(path, p2) and np.array_equal(score.view(np.uint64), s2.view(np.uint64))
    # the resident batch is still the uploaded one, and the resident call gives the same
    p3, s3 = e.align_resident(B, T)
    assert np.array_equal(path, p3) and np.array_equal(score.view(np.uint64), s3.view(np.uint64))
    _, nll = e.loss_resident(B)
    for b in range(B):
        lab = labels[b, :ll[b]]
        assert R.is_valid_path(path[b, :seq[b]], lab, C - 1) and np.all(path[b, seq[b]:] == -1)
        want = R.path_score(logits[:seq[b], b], lab, path[b, :seq[b]])
        assert abs(score[b] - want) <= SCORE_ATOL + SCORE_RTOL * abs(want)
        assert score[b] <= -nll[b] + SCORE_ATOL + SCORE_RTOL * abs(nll[b])      # one path is no more probable than all of them
    e.close()


@pytest.mark.parametrize('kind', KINDS)
def test_alignment_leaves_the_step_alone(kind):
    """upload, [align_resident,] compute_grads: the same loss and gradient bits with and without the alignment"""
    e = make_engine(kind)
    feats, seq, labels, ll = small_batch(seed=1)

    def step(with_alignment):
        init(e, seed=4 if kind == 'wavenet' else 3)      # (a WaveNet's gradient pass normalises with the batch's statistics)
        e.upload_batch(feats, seq, labels, ll)
        if with_alignment:
            e.align_resident(feats.shape[0], feats.shape[1])
        e.compute_grads()
        return e.get_loss(), e.get_grads()
    loss_a, grads_a = step(False)
    loss_b, grads_b = step(True)
    assert same(loss_a, loss_b) and same(grads_a, grads_b)
    e.close()


def test_from_audio_equals_from_features():
    from neuralasr_amd.engine import Engine
    from neuralasr_amd.features import Featurizer
    sr = 8000
    f = Featurizer(sr, 13, 1)
    audios = [speech_like(int(sr * s), sr, 50 + i) for i, s in enumerate((0.45, 0.3, 0.12))]
    rs = np.random.RandomState(5)
    labels = rs.randint(1, C - 1, size=(3, 5)).astype(np.int32)
    ll = [5, 3, 2]
    e = init(Engine(f.width, H, 1, True, 'concat', C, learning_rate=1e-3))
    seq, T = e.upload_batch_audio(f, audios, labels, ll)
    pa, sa = e.align_resident(3, T)
    feats, hseq, hT = host_feats(f, audios, None)
    assert hT == T and [int(t) for t in seq] == hseq
    ph, sh = e.align(feats, hseq, labels, ll)
    assert np.array_equal(pa, ph)
    assert np.allclose(sa, sh, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    e.close()
    f.close()


def test_a_las_handle_refuses():
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import LasEngine
    e = LasEngine(F_IN, C, seed=5, learning_rate=1e-3)
    feats, seq, labels, ll = small_batch()
    for call in (lambda: e.align(feats, seq, labels, ll), lambda: e.align_resident(3, 40),
                 lambda: e.align_logits(np.zeros((4, 1, C), np.float32), [4], [[1]], [1])):
        with pytest.raises(NotImplementedError):
            call()
    path, score = np.zeros((1, 4), np.int32), np.zeros(1)
    ip = ctypes.POINTER(ctypes.c_int32)
    rc = e.lib.nasr_ctc_align_resident(e.h, path.ctypes.data_as(ip), score.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == _lib.NASR_ERR_STATE and b'LAS' in e.lib.nasr_last_error(e.h)
    e.close()


def corpus_config(tmp_path, net):
    """five synthesised WAVs with transcripts, the symbol table of their characters, and a config for network `net`"""
    from neuralasr_amd.audio_dataset import prepare_symbols
    from neuralasr_amd.config import Config
    from neuralasr_amd.features import write_wav16
    sr = 8000
    texts = ['hello world', 'a cat a dog', 'old road', 'we all do', 'low cell']
    rows = []
    for i, text in enumerate(texts):
        wav, txt = tmp_path / ('utt%d.wav' % i), tmp_path / ('utt%d.txt' % i)
        write_wav16(wav, speech_like(int(sr * (0.5 + 0.1 * i)), sr, 100 + i), sr)
        txt.write_text(text + '\n')
        rows.append('%s,%s,%d' % (wav, txt, os.path.getsize(wav)))
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    cfg_path = tmp_path / 'a.config'
    cfg_path.write_text(
        '[Parameters]\nsamplerate=%d\nnumcep=13\nnumcontext=1\nlabel_context=0\nbatch_size=2\nepochs=1\n'
        'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
        'sym_file=%s\nnetwork=networks.%s\n'
        '[Train]\ninput=%s/train.scp\n[Test]\ninput=%s/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\nstart_marker=^\nend_marker=$$\n'
        % (sr, tmp_path / 'model', tmp_path / 'symbols', net, tmp_path, tmp_path, tmp_path / 'data.csv', tmp_path))
    prepare_symbols(Config(str(cfg_path), True))
    return cfg_path, Config(str(cfg_path), True)


def test_network_align_audio_equals_align(tmp_path):
    """HipNetwork.align on host-made features and align_audio on the same audio, B 3: the same spans per utterance (label
    order, sliced by labels_len), the same scores"""
    from neuralasr_amd.align import text_ids
    from neuralasr_amd.features import read_wav_native
    cfg_path, config = corpus_config(tmp_path, 'lstm_ctc_net.LstmCTCNet')
    network = config.load_network(fortraining=True)
    texts = ['hello_world', 'a_cat', 'old_road']
    ids = [text_ids(config, t) for t in texts]
    ll = [len(i) for i in ids]
    labels = np.zeros((3, max(ll)), np.int32)
    for b, i in enumerate(ids):
        labels[b, :ll[b]] = i
    audios, rates = zip(*[read_wav_native(str(tmp_path / ('utt%d.wav' % i))) for i in (2, 0, 1)])
    from_audio = network.align_audio(list(audios), list(rates), labels, ll)
    feats, seq, _ = host_feats(network.featurizer(), list(audios), list(rates))
    from_feats = network.align(feats, labels, seq, ll)
    assert len(from_audio) == len(from_feats) == 3
    for b in range(3):
        (sa, spa), (sf, spf) = from_audio[b], from_feats[b]
        assert spa == spf and [sid for sid, _, _ in spa] == [int(x) for x in ids[b]]
        assert all(0 <= a <= z < seq[b] for _, a, z in spa) and [a for _, a, _ in spa] == sorted(a for _, a, _ in spa)
        assert abs(sa - sf) <= SCORE_ATOL + SCORE_RTOL * abs(sf) and sa < 0
    with pytest.raises(ValueError):
        network.engine.align_resident(2, feats.shape[1])     # not the resident batch's B
    network.engine.close()
    network.featurizer().close()


@pytest.mark.parametrize('net', ['bilstm_ctc_net.BiLstmCTCNet', 'lstm_ctc_net.LstmCTCNet'])
def test_command_line(tmp_path, caplog, monkeypatch, net):
    """one line per symbol of the transcript, in order, with non-decreasing positions: seconds for the unidirectional net,
    logit-frame indices (and the reason) for the literal BiLstmCTCNet, whose stack_reshape frames have no time"""
    from neuralasr_amd import align
    cfg_path, config = corpus_config(tmp_path, net)
    network = config.load_network(fortraining=True)          # fresh variables
    network.save_checkpoint()
    network.engine.close()

    (tmp_path / 'new.txt').write_text('Hello, road!\n')      # every character is in the table
    with caplog.at_level(logging.INFO):
        lines, score = align.main([str(cfg_path), str(tmp_path / 'utt0.wav'), str(tmp_path / 'new.txt')])
    logged = [r.getMessage() for r in caplog.records]
    assert [l.split()[0] for l in lines] == ['^'] + list('hello_road') + ['$']
    assert ['Aligned: ' + l for l in lines] == [m for m in logged if m.startswith('Aligned: ')]
    assert any(m.startswith('Score: ') for m in logged) and np.isfinite(score) and score < 0
    timed = net.endswith('LstmCTCNet') and not net.endswith('BiLstmCTCNet')
    starts = [float(l.split()[1]) for l in lines]
    ends = [float(l.split()[2]) for l in lines]
    assert starts == sorted(starts) and all(a <= b for a, b in zip(starts, ends))
    if timed:
        assert all('.' in l.split()[1] and '.' in l.split()[2] for l in lines)
        assert ends[-1] <= 0.5 + 0.02                        # seconds inside the half-second file
        assert not any('stack_reshape' in m for m in logged)
    else:
        assert all(l.split()[1].isdigit() and l.split()[2].isdigit() for l in lines)
        assert any('stack_reshape' in m and 'logit-frame indices' in m for m in logged)

    if timed:
        # a network that takes features only: the host-made features of the same file give the same lines
        from neuralasr_amd.networks.lstm_ctc_net import LstmCTCNet
        monkeypatch.setattr(LstmCTCNet, 'takes_audio', False)
        lines2, score2 = align.main([str(cfg_path), str(tmp_path / 'utt0.wav'), str(tmp_path / 'new.txt')])
        assert lines2 == lines and abs(score2 - score) <= SCORE_ATOL + SCORE_RTOL * abs(score)

    (tmp_path / 'bad.txt').write_text('hex\n')               # no transcript has an x
    with pytest.raises(ValueError) as err:
        align.main([str(cfg_path), str(tmp_path / 'utt0.wav'), str(tmp_path / 'bad.txt')])
    assert "'x'" in str(err.value)
